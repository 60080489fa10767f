// Mixture-of-experts routing with sigmoid scores, expert groups and a selection bias (DeepSeek-V3 / R1, and with
// n_group = 1 and no bias any sigmoid top-k gate), in moe.hip's routing layout: a token's row is held by L
// neighbouring lanes, L the power of two >= Ne below 64 and the whole wave (VPL = 2 or 4 values per lane, expert
// lane + 64 i) above, so a row never straddles a wave and every reduction is an xor shuffle below L.
//
//   route_sigmoid_fwd  per row, in fp32:
//     s_e = 1 / (1 + expf(-x_e));  c_e = s_e + bias_e                     (the selection score)
//     n_group > 1: a group is Gs = Ne / n_group neighbouring lanes of one value index (Gs a power of two, 2 .. 64);
//       its score is the sum of its two largest c; topk_group rounds of an argmax over (score, group), the lower
//       group first among equal scores, keep that many groups and the experts of the others become ineligible
//     idx [T, k]: k rounds of moe.hip's (value, expert) argmax over the eligible c, descending c, the lower expert
//       first among equal values
//     gate [T, k] = scale * s_j / (sum_j s_j + 1e-20) with renorm, scale * s_j without: the UNBIASED sigmoids
//     part [blocks, Ne]: per-block sums over tokens of q_e = s_e / sum_e' s_e', folded as moe_route_fwd folds
//   route_sigmoid_bwd  dlogits from dgate and the optional dprobs; s is recomputed from the logits, the selected
//     s_j come from their owning lanes by one shuffle each.  The bias only selects: it has no gradient.
//   bias_update        bias[e] += rate * sign(mean(load) - load[e]), load[e] = 0 (auxiliary-loss-free balancing).
//
// Shuffles per row: the pair (largest, second largest) of a group merges in 2 log2 Gs shuffles per value index (the
// merge is exact, so it is the argmax / mask / second max of the definition without its third shuffle), a group
// round needs only the offsets Gs .. L / 2 (the lanes of a group already agree), an expert round 2 log2 L and one
// more to fetch the winner's s.  No LDS but the final fold, no float atomics: the same bits on every run.
#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 8;

__device__ __forceinline__ float row_sum(float v, int L) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    if (o < L) v += __shfl_xor(v, o, 64);
  return v;
}

int sigmoid_lanes(int Ne) {  // moe.hip's route_lanes
  int L = 2;
  while (L < Ne && L < 64) L <<= 1;
  return L;
}

// Round j of the top-k: the best (value, expert) of the row among the values whose bit of `out` is clear; the
// winner's bit is set.  v[i] belongs to expert sub + 64 i.
template <int VPL>
__device__ __forceinline__ int argmax_round(const float (&v)[VPL], unsigned& out, int sub, int L) {
  float bv = -INFINITY;
  int be = INT32_MAX;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    if (!((out >> i) & 1u) && (be == INT32_MAX || v[i] > bv)) {  // ascending e: a tie keeps the lower
      bv = v[i];
      be = sub + 64 * i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    if (o < L) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oe = __shfl_xor(be, o, 64);
      const bool mine = be != INT32_MAX && (oe == INT32_MAX || bv > ov || (bv == ov && be < oe));
      bv = mine ? bv : ov;
      be = mine ? be : oe;
    }
  }
#pragma unroll
  for (int i = 0; i < VPL; ++i)
    if (sub + 64 * i == be) out |= 1u << i;
  return be;
}

// s of expert e (uniform over the row, any int) from the lane that holds it; lanes are always in range.
template <int VPL>
__device__ __forceinline__ float fetch_s(const float (&s)[VPL], int e, int lane, int L) {
  float mine = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i)
    if ((e >> 6) == i) mine = s[i];
  return __shfl(mine, (lane & ~(L - 1)) | (e & (L - 1)), 64);
}

// ---------------------------------------------------------------- forward
template <typename T, int VPL>
__global__ void __launch_bounds__(kThreads)
    moe_route_sigmoid_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ bias,
                                 int32_t* __restrict__ idx, float* __restrict__ gate, float* __restrict__ part,
                                 int64_t tokens, int Ne, int k, int L, int n_group, int gshift, int topk_group,
                                 int renorm, float scale) {
  __shared__ float fold[kWaves][VPL][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (L - 1);  // the lane's place in its row
  const int per = 64 / L;          // tokens per wave
  const int Gs = 1 << gshift;
  const int64_t ngroups = (tokens + per - 1) / per;
  float acc[VPL], b[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int e = sub + 64 * i;
    acc[i] = 0.f;
    b[i] = (bias != nullptr && e < Ne) ? bias[e] : 0.f;
  }
  for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < ngroups; g += (int64_t)gridDim.x * kWaves) {
    const int64_t t = g * per + lane / L;
    const bool live = t < tokens;
    float s[VPL], c[VPL], z = 0.f;
    unsigned out = 0;  // bit i: value i is not (or no longer) eligible
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int e = sub + 64 * i;
      // a lane past the row (or a token past the end) holds s = 0 and is never eligible
      const float x = (live && e < Ne) ? Io<T>::load(logits + t * Ne + e) : -INFINITY;
      s[i] = 1.f / (1.f + expf(-x));
      c[i] = s[i] + b[i];
      z += s[i];
      if (e >= Ne) out |= 1u << i;
    }
    z = row_sum(z, L);
    const float rz = 1.f / z;
#pragma unroll
    for (int i = 0; i < VPL; ++i) acc[i] += live ? s[i] * rz : 0.f;
    if (n_group > 1) {
      // a group's score: the pair (largest, second largest) of its Gs lanes, merged exactly, then one addition
      float gs[VPL];
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        float m1 = ((out >> i) & 1u) ? -INFINITY : c[i], m2 = -INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          if (o < Gs) {
            const float o1 = __shfl_xor(m1, o, 64), o2 = __shfl_xor(m2, o, 64);
            m2 = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
            m1 = fmaxf(m1, o1);
          }
        }
        gs[i] = m1 + m2;
      }
      // topk_group rounds over (score, group); the lanes of a group hold the same pair, so only the offsets from
      // Gs up exchange anything.  A group past the row (Ne < 64 VPL) never stands.
      unsigned kept = 0;
#pragma unroll
      for (int r = 0; r < kMaxK; ++r) {
        if (r < topk_group) {
          float bv = -INFINITY;
          int bg = INT32_MAX;
#pragma unroll
          for (int i = 0; i < VPL; ++i) {
            const int gi = (sub + 64 * i) >> gshift;
            if (gi < n_group && !((kept >> i) & 1u) && (bg == INT32_MAX || gs[i] > bv)) {  // ascending group
              bv = gs[i];
              bg = gi;
            }
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            if (o < L && o >= Gs) {
              const float ov = __shfl_xor(bv, o, 64);
              const int og = __shfl_xor(bg, o, 64);
              const bool mine = bg != INT32_MAX && (og == INT32_MAX || bv > ov || (bv == ov && bg < og));
              bv = mine ? bv : ov;
              bg = mine ? bg : og;
            }
          }
          // topk_group <= n_group: a round always finds a group, bg in [0, n_group)
#pragma unroll
          for (int i = 0; i < VPL; ++i)
            if (((sub + 64 * i) >> gshift) == bg) kept |= 1u << i;
        }
      }
      out |= ~kept;
    }
    // top-k over the eligible c (k <= topk_group * Gs: a round always finds one, be in [0, Ne)); the weights are
    // the winners' unbiased s
    float ss[kMaxK];
    int se[kMaxK];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      ss[j] = 0.f;
      se[j] = 0;
      if (j < k) {
        se[j] = argmax_round<VPL>(c, out, sub, L);
        ss[j] = fetch_s<VPL>(s, se[j], lane, L);
        sum += ss[j];
      }
    }
    sum += 1e-20f;
    if (live && sub == 0) {
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        if (j < k) {
          idx[t * k + j] = se[j];
          gate[t * k + j] = (renorm ? ss[j] / sum : ss[j]) * scale;
        }
      }
    }
  }
  // this block's partial row of probs_sum: the waves in wave order, the lanes that share an expert in lane order
#pragma unroll
  for (int i = 0; i < VPL; ++i) fold[wave][i][lane] = acc[i];
  __syncthreads();
  for (int e = threadIdx.x; e < Ne; e += kThreads) {
    const int i = e >> 6, l0 = e & 63;  // L == 64 when Ne > 64, so l0 is the lane; below, l0 = e < L
    float r = 0.f;
    for (int w = 0; w < kWaves; ++w)
      for (int l = l0; l < 64; l += L) r += fold[w][i][l];
    part[(size_t)blockIdx.x * Ne + e] = r;
  }
}

// ---------------------------------------------------------------- backward
//   renorm: ds_j = scale / S (dg_j - sum_i n_i dg_i), n_j = s_j / S, S = sum_j s_j + 1e-20;  else ds_j = scale dg_j
//   dprobs: ds_e += (dp_e - sum_e' q_e' dp_e') / Z, Z = sum_e s_e, q = s / Z
//   dlogit_e = ds_e s_e (1 - s_e)
template <typename T, int VPL>
__global__ void __launch_bounds__(kThreads)
    moe_route_sigmoid_bwd_kernel(const T* __restrict__ logits, const int32_t* __restrict__ idx,
                                 const float* __restrict__ dgate, const float* __restrict__ dprobs,
                                 T* __restrict__ dlogits, int64_t tokens, int Ne, int k, int L, int renorm,
                                 float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (L - 1);
  const int per = 64 / L;
  const int64_t ngroups = (tokens + per - 1) / per;
  float dp[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int e = sub + 64 * i;
    dp[i] = (dprobs != nullptr && e < Ne) ? dprobs[e] : 0.f;
  }
  for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < ngroups; g += (int64_t)gridDim.x * kWaves) {
    const int64_t t = g * per + lane / L;
    const bool live = t < tokens;
    float s[VPL], ds[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int e = sub + 64 * i;
      const float x = (live && e < Ne) ? Io<T>::load(logits + t * Ne + e) : -INFINITY;
      s[i] = 1.f / (1.f + expf(-x));
      ds[i] = 0.f;
    }
    if (dprobs != nullptr) {  // uniform: every lane of the wave takes part in the shuffles
      float z = 0.f, d = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        z += s[i];
        d += s[i] * dp[i];
      }
      z = row_sum(z, L);
      d = row_sum(d, L);
      const float rz = 1.f / z;
      d *= rz;  // <dprobs, q>
#pragma unroll
      for (int i = 0; i < VPL; ++i) ds[i] = (dp[i] - d) * rz;
    }
    // the selected experts: every lane of the wave runs the shuffles, an idle token or an expert outside [0, Ne)
    // contributes nothing
    float sj[kMaxK], dj[kMaxK], sum = 0.f;
    int ej[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      sj[j] = dj[j] = 0.f;
      ej[j] = -1;
      if (j < k) {
        const int e = live ? idx[t * k + j] : -1;
        const float v = fetch_s<VPL>(s, e, lane, L);
        if (e >= 0 && e < Ne) {
          ej[j] = e;
          sj[j] = v;
          dj[j] = dgate[t * k + j];
        }
        sum += sj[j];
      }
    }
    sum += 1e-20f;
    float dot = 0.f, coef = scale;
    if (renorm) {
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) dot += sj[j] / sum * dj[j];
      coef = scale / sum;
    }
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
#pragma unroll
      for (int i = 0; i < VPL; ++i)
        if (ej[j] == sub + 64 * i) ds[i] += coef * (dj[j] - dot);
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int e = sub + 64 * i;
        if (e < Ne) Io<T>::store(dlogits + t * Ne + e, ds[i] * s[i] * (1.f - s[i]));
      }
    }
  }
}

// ---------------------------------------------------------------- bias update
// One block, thread e.  sign(mean(load) - load[e]) is the sign of sum(load) - Ne load[e]: integers, exact.
__global__ void __launch_bounds__(kThreads) moe_bias_update_kernel(float* __restrict__ bias, int32_t* __restrict__ load,
                                                                   int Ne, float rate) {
  __shared__ int32_t l[kThreads];
  const int e = threadIdx.x;
  l[e] = e < Ne ? load[e] : 0;
  __syncthreads();
  int64_t total = 0;
  for (int i = 0; i < Ne; ++i) total += l[i];
  if (e < Ne) {
    const int64_t d = total - (int64_t)Ne * l[e];
    bias[e] += rate * (d > 0 ? 1.f : (d < 0 ? -1.f : 0.f));
    load[e] = 0;
  }
}

int log2_exact(int v) {  // v a power of two
  int r = 0;
  while ((1 << r) < v) ++r;
  return r;
}

}  // namespace

// ---------------------------------------------------------------- launchers
bool moe_route_sigmoid_supported(int Ne, int k, int n_group, int topk_group) {
  if (!moe_route_supported(Ne, k) || n_group < 1 || Ne % n_group != 0) return false;
  if (n_group == 1) return topk_group == 1;
  const int Gs = Ne / n_group;
  return Gs >= 2 && Gs <= 64 && (Gs & (Gs - 1)) == 0 && topk_group >= 1 && topk_group <= kMaxK &&
         topk_group <= n_group && topk_group * Gs >= k;
}

template <typename T>
void moe_route_sigmoid_fwd(const T* logits, const float* bias, int32_t* idx, float* gate, float* part, int nparts,
                           int64_t tokens, int Ne, int k, int n_group, int topk_group, bool renorm, float scale,
                           hipStream_t s) {
  const int L = sigmoid_lanes(Ne);
  const int gshift = n_group > 1 ? log2_exact(Ne / n_group) : 0;
  const dim3 grid((unsigned)nparts), block(kThreads);
  const int rn = renorm ? 1 : 0;
  if (Ne <= 64) {
    hipLaunchKernelGGL((moe_route_sigmoid_fwd_kernel<T, 1>), grid, block, 0, s, logits, bias, idx, gate, part, tokens,
                       Ne, k, L, n_group, gshift, topk_group, rn, scale);
  } else if (Ne <= 128) {
    hipLaunchKernelGGL((moe_route_sigmoid_fwd_kernel<T, 2>), grid, block, 0, s, logits, bias, idx, gate, part, tokens,
                       Ne, k, L, n_group, gshift, topk_group, rn, scale);
  } else {
    hipLaunchKernelGGL((moe_route_sigmoid_fwd_kernel<T, 4>), grid, block, 0, s, logits, bias, idx, gate, part, tokens,
                       Ne, k, L, n_group, gshift, topk_group, rn, scale);
  }
}

template <typename T>
void moe_route_sigmoid_bwd(const T* logits, const int32_t* idx, const float* dgate, const float* dprobs, T* dlogits,
                           int64_t tokens, int Ne, int k, bool renorm, float scale, hipStream_t s) {
  if (tokens == 0) return;
  const int L = sigmoid_lanes(Ne);
  const dim3 grid((unsigned)moe_route_parts(tokens, Ne)), block(kThreads);
  const int rn = renorm ? 1 : 0;
  if (Ne <= 64) {
    hipLaunchKernelGGL((moe_route_sigmoid_bwd_kernel<T, 1>), grid, block, 0, s, logits, idx, dgate, dprobs, dlogits,
                       tokens, Ne, k, L, rn, scale);
  } else if (Ne <= 128) {
    hipLaunchKernelGGL((moe_route_sigmoid_bwd_kernel<T, 2>), grid, block, 0, s, logits, idx, dgate, dprobs, dlogits,
                       tokens, Ne, k, L, rn, scale);
  } else {
    hipLaunchKernelGGL((moe_route_sigmoid_bwd_kernel<T, 4>), grid, block, 0, s, logits, idx, dgate, dprobs, dlogits,
                       tokens, Ne, k, L, rn, scale);
  }
}

void moe_bias_update(float* bias, int32_t* load, int Ne, float rate, hipStream_t s) {
  hipLaunchKernelGGL(moe_bias_update_kernel, dim3(1), dim3(kThreads), 0, s, bias, load, Ne, rate);
}

#define MOE_SIGMOID_INSTANTIATE(T)                                                                                    \
  template void moe_route_sigmoid_fwd<T>(const T*, const float*, int32_t*, float*, float*, int, int64_t, int, int,    \
                                         int, int, bool, float, hipStream_t);                                         \
  template void moe_route_sigmoid_bwd<T>(const T*, const int32_t*, const float*, const float*, T*, int64_t, int, int, \
                                         bool, float, hipStream_t);
MOE_SIGMOID_INSTANTIATE(float)
MOE_SIGMOID_INSTANTIATE(bf16_t)
#undef MOE_SIGMOID_INSTANTIATE

}  // namespace mipipe
