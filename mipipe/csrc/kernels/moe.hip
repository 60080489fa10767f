// Mixture-of-experts routing: the top-k gate, the assignment of tokens to
// expert slots, the two permutations (dispatch, combine) and their backwards.
//
//   T tokens, Ne experts (2 .. 256), k experts per token (1 .. min(8, Ne)), C
//   slots per expert; a = t * k + j is token t's j-th choice.
//
//   route_fwd   idx [T, k]: the k largest logits of a row, descending, the lower
//               expert first among equal values; gate [T, k]: softmax over those
//               k; part [blocks, Ne]: per-block sums over tokens of the full-row
//               softmax (the caller folds them with reduce_parts).
//   route_bwd   dlogits from dgate and the optional dprobs (the gradient of the
//               summed full-row softmax).
//   assign      slot [T, k] = e * C + pos or -1, src [Ne * C] = a or -1, counts
//               [Ne]; pos counts the earlier entries of the same expert in
//               choice-major order (j first, then t).
//   assign_sorted  the dropless layout for the grouped GEMMs (gemm_grouped.hip):
//               expert e owns rows [offsets[e], offsets[e + 1]), offsets[e + 1] =
//               offsets[e] + ceil128(counts[e]); slot = offsets[e] + pos; src [R];
//               tile_expert [R / 128] = the expert of a 128-row tile or -1.
//   gather_slots   xe[s] = x[src[s] / k]            (dispatch forward)
//   gather_tokens  y[t] = res[t] + sum_j w[t, j] ye[slot[t, j]]
//                                                   (combine forward, dispatch backward)
//   combine_bwd    dye[s] = gate[a] dy[t], dgate[a] = <dy[t], ye[s]>
//
// All memory-bound.  fp32 arithmetic, one rounding at a store; no float atomics:
// the only atomics are integer LDS counters of the histogram, whose result does
// not depend on their order.  Every index read from memory (an expert, a slot, a
// source) is range-checked before it addresses anything.
//
// Routing layout: a token's row is held by L neighbouring lanes, L the power of
// two >= Ne below 64 and the whole wave (VPL = 2 or 4 values per lane, expert
// lane + 64 i) above, so a row never straddles a wave and the row reductions are
// xor shuffles below L, as in qknorm.hip.
//
// Row kernels (the gathers): a row of E values is 16-byte vectors shared by TPR
// neighbouring threads (a power of two <= 256), 256 / TPR rows per block.
#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 8;
constexpr int kRouteGrid = 1024;    // partial rows of probs_sum: at most this many
constexpr int kAssignChunk = 1024;  // entries per block of the assignment: 4 rounds of 256
constexpr int kRowGrid = 16384;

__device__ __forceinline__ float group_max(float v, int L) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    if (o < L) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float group_sum(float v, int L) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    if (o < L) v += __shfl_xor(v, o, 64);
  return v;
}

// Lanes per token row for Ne experts: the power of two >= Ne, at least 2, at most 64.
int route_lanes(int Ne) {
  int L = 2;
  while (L < Ne && L < 64) L <<= 1;
  return L;
}

int route_groups(int64_t T, int L) {  // wave-sized groups of 64 / L tokens
  const int per = 64 / L;
  return (int)((T + per - 1) / per);
}

// ---------------------------------------------------------------- route forward
template <typename T, int VPL>
__global__ void __launch_bounds__(kThreads) moe_route_fwd_kernel(const T* __restrict__ logits, int32_t* __restrict__ idx,
                                                                 float* __restrict__ gate, float* __restrict__ part,
                                                                 int64_t tokens, int Ne, int k, int L) {
  __shared__ float fold[kWaves][VPL][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (L - 1);  // the lane's place in its row
  const int per = 64 / L;          // tokens per wave
  const int64_t ngroups = (tokens + per - 1) / per;
  float acc[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) acc[i] = 0.f;
  for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < ngroups; g += (int64_t)gridDim.x * kWaves) {
    const int64_t t = g * per + lane / L;
    const bool live = t < tokens;
    float v[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int e = sub + 64 * i;
      // a lane past the row (or a token past the end) holds -inf and is never eligible below; an idle token's
      // lane 0 holds 0 so that its softmax stays finite
      v[i] = (live && e < Ne) ? Io<T>::load(logits + t * Ne + e) : ((!live && e == 0) ? 0.f : -INFINITY);
    }
    float m = v[0];
#pragma unroll
    for (int i = 1; i < VPL; ++i) m = fmaxf(m, v[i]);
    m = group_max(m, L);
    // the full-row softmax, summed over this wave's tokens
    float p[VPL], z = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      p[i] = expf(v[i] - m);
      z += p[i];
    }
    z = group_sum(z, L);
    const float rz = 1.f / z;
#pragma unroll
    for (int i = 0; i < VPL; ++i) acc[i] += live ? p[i] * rz : 0.f;
    // top-k: k rounds of an argmax over the values not yet taken; (value, expert) orders by the larger value,
    // then the lower expert
    unsigned taken = 0;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if (sub + 64 * i >= Ne) taken |= 1u << i;
    float sv[kMaxK];
    int se[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      sv[j] = -INFINITY;
      se[j] = 0;
      if (j < k) {
        float bv = -INFINITY;
        int be = INT32_MAX;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const int e = sub + 64 * i;
          if (!((taken >> i) & 1u) && (be == INT32_MAX || v[i] > bv)) {  // ascending e: a tie keeps the lower
            bv = v[i];
            be = e;
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
        // k <= Ne: a round always finds an eligible expert of a live token, be in [0, Ne)
#pragma unroll
        for (int i = 0; i < VPL; ++i)
          if (sub + 64 * i == be) taken |= 1u << i;
        sv[j] = bv;
        se[j] = be;
      }
    }
    // gate: the softmax over the k selected values (sv[0] is the row's maximum, finite)
    const float top = sv[0];
    float gz = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      sv[j] = j < k ? expf(sv[j] - top) : 0.f;
      gz += sv[j];
    }
    const float rg = 1.f / gz;
    if (live && sub == 0) {
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        if (j < k) {
          idx[t * k + j] = se[j];
          gate[t * k + j] = sv[j] * rg;
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
    float s = 0.f;
    for (int w = 0; w < kWaves; ++w)
      for (int l = l0; l < 64; l += L) s += fold[w][i][l];
    part[(size_t)blockIdx.x * Ne + e] = s;
  }
}

// ---------------------------------------------------------------- route backward
template <typename T, int VPL>
__global__ void __launch_bounds__(kThreads) moe_route_bwd_kernel(const T* __restrict__ logits,
                                                                 const int32_t* __restrict__ idx,
                                                                 const float* __restrict__ gate,
                                                                 const float* __restrict__ dgate,
                                                                 const float* __restrict__ dprobs,
                                                                 T* __restrict__ dlogits, int64_t tokens, int Ne, int k,
                                                                 int L) {
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
    float dl[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) dl[i] = 0.f;
    if (dprobs != nullptr) {  // uniform: every lane of the wave takes part in the shuffles
      float v[VPL];
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int e = sub + 64 * i;
        v[i] = (live && e < Ne) ? Io<T>::load(logits + t * Ne + e) : ((!live && e == 0) ? 0.f : -INFINITY);
      }
      float m = v[0];
#pragma unroll
      for (int i = 1; i < VPL; ++i) m = fmaxf(m, v[i]);
      m = group_max(m, L);
      float z = 0.f, d = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        v[i] = expf(v[i] - m);
        z += v[i];
        d += v[i] * dp[i];
      }
      z = group_sum(z, L);
      d = group_sum(d, L);
      const float rz = 1.f / z;
      d *= rz;  // <dprobs, p>
#pragma unroll
      for (int i = 0; i < VPL; ++i) dl[i] = v[i] * rz * (dp[i] - d);
    }
    if (live) {
      float gj[kMaxK], dj[kMaxK], s = 0.f;
      int ej[kMaxK];
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        gj[j] = dj[j] = 0.f;
        ej[j] = -1;
        if (j < k) {
          gj[j] = gate[t * k + j];
          dj[j] = dgate[t * k + j];
          ej[j] = idx[t * k + j];
          s += gj[j] * dj[j];
        }
      }
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
#pragma unroll
        for (int i = 0; i < VPL; ++i)
          if (ej[j] == sub + 64 * i) dl[i] += gj[j] * (dj[j] - s);
      }
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int e = sub + 64 * i;
        if (e < Ne) Io<T>::store(dlogits + t * Ne + e, dl[i]);
      }
    }
  }
}

// ---------------------------------------------------------------- assign
// Entry q = j * T + t of the choice-major order holds expert idx[t * k + j]; an expert outside [0, Ne) counts
// nowhere and its slot is -1.
__device__ __forceinline__ int assign_expert(const int32_t* __restrict__ idx, int64_t q, int64_t tokens, int k, int Ne,
                                             int64_t* a_out) {
  const int64_t j = q / tokens, t = q - j * tokens;
  const int64_t a = t * k + j;
  *a_out = a;
  const int e = idx[a];
  return (e >= 0 && e < Ne) ? e : -1;
}

// Block b's histogram of its kAssignChunk entries into hist[b][Ne]; also src = -1 everywhere.
__global__ void __launch_bounds__(kThreads) moe_assign_count_kernel(const int32_t* __restrict__ idx,
                                                                    int32_t* __restrict__ hist,
                                                                    int32_t* __restrict__ src, int64_t tokens, int k,
                                                                    int Ne, int64_t nslots) {
  __shared__ int32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t n = tokens * k;
  const int64_t q0 = (int64_t)blockIdx.x * kAssignChunk;
  for (int r = 0; r < kAssignChunk / kThreads; ++r) {
    const int64_t q = q0 + r * kThreads + threadIdx.x;
    if (q < n) {
      int64_t a;
      const int e = assign_expert(idx, q, tokens, k, Ne, &a);
      if (e >= 0) atomicAdd(&h[e], 1);  // integer, in LDS: the sum does not depend on the order
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < Ne) hist[(size_t)blockIdx.x * Ne + threadIdx.x] = h[threadIdx.x];
  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < nslots; s += (int64_t)gridDim.x * kThreads)
    src[s] = -1;
}

// One block, thread e: hist[b][e] becomes the number of entries of expert e in the blocks before b; counts[e] the
// total.
__global__ void __launch_bounds__(kThreads) moe_assign_scan_kernel(int32_t* __restrict__ hist,
                                                                   int32_t* __restrict__ counts, int nblocks, int Ne) {
  const int e = threadIdx.x;
  if (e >= Ne) return;
  int32_t run = 0;
  for (int b = 0; b < nblocks; ++b) {
    const int32_t c = hist[(size_t)b * Ne + e];
    hist[(size_t)b * Ne + e] = run;
    run += c;
  }
  counts[e] = run;
}

// Ranks: a lane's place among the wave's earlier lanes of the same expert from ballots over the expert's 8 bits,
// the waves of a round one after the other over running[] in LDS, the rounds in order.
//
// kSorted (moe_assign_sorted): expert e's rows start at offsets[e] instead of e * C, nothing is dropped, and C is the
// number of rows of src (a bound the counts cannot exceed; it only guards the store).
template <bool kSorted>
__global__ void __launch_bounds__(kThreads) moe_assign_rank_kernel(const int32_t* __restrict__ idx,
                                                                   const int32_t* __restrict__ base,
                                                                   const int32_t* __restrict__ offsets,
                                                                   int32_t* __restrict__ slot,
                                                                   int32_t* __restrict__ src, int64_t tokens, int k,
                                                                   int Ne, int C) {
  __shared__ int32_t running[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  running[threadIdx.x] = (int)threadIdx.x < Ne ? base[(size_t)blockIdx.x * Ne + threadIdx.x] +
                                                     (kSorted ? offsets[threadIdx.x] : 0)
                                               : 0;
  __syncthreads();
  const int64_t n = tokens * k;
  const int64_t q0 = (int64_t)blockIdx.x * kAssignChunk;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int r = 0; r < kAssignChunk / kThreads; ++r) {
    const int64_t q = q0 + r * kThreads + threadIdx.x;
    int64_t a = 0;
    const int e = q < n ? assign_expert(idx, q, tokens, k, Ne, &a) : -1;
    unsigned long long peers = __ballot(e >= 0);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bal = __ballot((e >> b) & 1);
      peers &= ((e >> b) & 1) ? bal : ~bal;
    }
    const int rank = __popcll(peers & below), cnt = __popcll(peers);
    for (int w = 0; w < kWaves; ++w) {
      if (wave == w && e >= 0) {
        const int pos = running[e] + rank;
        if (pos < C) {
          const int s = kSorted ? pos : e * C + pos;  // < Ne * C < 2^31 (the launcher checks)
          slot[a] = s;
          src[s] = (int32_t)a;
        } else {
          slot[a] = -1;
        }
        if (rank == cnt - 1) running[e] = pos + 1;  // the expert's last lane of this wave: after every peer's read
      }
      __syncthreads();
    }
    if (q < n && e < 0) slot[a] = -1;
  }
}

// The sorted layout's scan: as moe_assign_scan_kernel, and from the totals offsets[e + 1] = offsets[e] +
// ceil128(counts[e]) and the expert of every 128-row tile (-1 past offsets[Ne]).
__global__ void __launch_bounds__(kThreads) moe_assign_sorted_scan_kernel(int32_t* __restrict__ hist,
                                                                          int32_t* __restrict__ counts,
                                                                          int32_t* __restrict__ offsets,
                                                                          int32_t* __restrict__ tile_expert,
                                                                          int nblocks, int Ne, int ntiles) {
  __shared__ int32_t first[257];  // first tile of expert e; first[Ne] the live tiles
  const int e = threadIdx.x;
  int32_t run = 0;
  if (e < Ne) {
    for (int b = 0; b < nblocks; ++b) {
      const int32_t c = hist[(size_t)b * Ne + e];
      hist[(size_t)b * Ne + e] = run;
      run += c;
    }
    counts[e] = run;
  }
  first[e + 1] = (run + 127) >> 7;
  __syncthreads();
  if (e == 0) {
    int32_t t = 0;
    first[0] = 0;
    for (int i = 1; i <= Ne; ++i) {
      t += first[i];
      first[i] = t;
    }
  }
  __syncthreads();
  if (e <= Ne) offsets[e] = first[e] * 128;
  if (e == 0 && Ne == 256) offsets[256] = first[256] * 128;
  if (e < Ne) {
    const int hi = min(first[e + 1], ntiles);
    for (int t = first[e]; t < hi; ++t) tile_expert[t] = e;
  }
  for (int t = first[Ne] + e; t < ntiles; t += kThreads) tile_expert[t] = -1;
}

// ---------------------------------------------------------------- row kernels
int row_tpr(int64_t vpr, int cap) {  // threads per row: the power of two >= vpr, at most cap
  int t = 1;
  while (t < vpr && t < cap) t <<= 1;
  return t;
}

unsigned row_grid(int64_t rows, int tpr) {
  const int64_t rpb = kThreads / tpr;
  const int64_t g = (rows + rpb - 1) / rpb;
  return (unsigned)(g < 1 ? 1 : (g < kRowGrid ? g : kRowGrid));
}

// xe[s, :] = x[src[s] / k, :], zeros for an empty slot (or a source outside [0, T k)): 16-byte copies.
__global__ void __launch_bounds__(kThreads) moe_gather_slots_kernel(const uint4* __restrict__ x,
                                                                    const int32_t* __restrict__ src,
                                                                    uint4* __restrict__ xe, int64_t nslots,
                                                                    int64_t tokens, int k, int vpr, int tpr) {
  const int rpb = kThreads / tpr;
  const int rl = threadIdx.x / tpr, c0 = threadIdx.x - rl * tpr;
  const int64_t nk = tokens * k;
  for (int64_t s = (int64_t)blockIdx.x * rpb + rl; s < nslots; s += (int64_t)gridDim.x * rpb) {
    const int a = src[s];
    const bool full = a >= 0 && a < nk;
    const uint4* in = x + (int64_t)(full ? a / k : 0) * vpr;
    uint4* out = xe + s * vpr;
    for (int c = c0; c < vpr; c += tpr) out[c] = full ? in[c] : make_uint4(0u, 0u, 0u, 0u);
  }
}

template <typename T>
struct Vec;
template <>
struct Vec<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const u16x8 r = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f(r[i]);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* v) {
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (__bf16)v[i];
    *reinterpret_cast<bf16x8*>(p) = r;
  }
};
template <>
struct Vec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// y[t, :] = res[t, :] + sum_j w[t, j] ye[slot[t, j], :] in j order; w == nullptr: weights of 1.
template <typename T>
__global__ void __launch_bounds__(kThreads) moe_gather_tokens_kernel(const T* __restrict__ ye,
                                                                     const int32_t* __restrict__ slot,
                                                                     const float* __restrict__ w,
                                                                     const T* __restrict__ res, T* __restrict__ y,
                                                                     int64_t tokens, int k, int64_t nslots, int E,
                                                                     int tpr) {
  constexpr int N = Vec<T>::N;
  const int vpr = E / N;
  const int rpb = kThreads / tpr;
  const int rl = threadIdx.x / tpr, c0 = threadIdx.x - rl * tpr;
  for (int64_t t = (int64_t)blockIdx.x * rpb + rl; t < tokens; t += (int64_t)gridDim.x * rpb) {
    int sj[kMaxK];
    float wj[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
      sj[j] = -1;
      wj[j] = 0.f;
      if (j < k) {
        const int s = slot[t * k + j];
        sj[j] = (s >= 0 && s < nslots) ? s : -1;
        wj[j] = w != nullptr ? w[t * k + j] : 1.f;
      }
    }
    for (int c = c0; c < vpr; c += tpr) {
      float acc[N], r[N];
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] = r[i] = 0.f;
      // the residual is loaded ahead of the gathered rows (its latency overlaps theirs) and added after them
      if (res != nullptr) Vec<T>::load(res + t * E + c * N, r);
#pragma unroll
      for (int j = 0; j < kMaxK; ++j) {
        if (sj[j] >= 0) {
          float v[N];
          Vec<T>::load(ye + (int64_t)sj[j] * E + c * N, v);
#pragma unroll
          for (int i = 0; i < N; ++i) acc[i] += wj[j] * v[i];
        }
      }
      if (res != nullptr) {
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] += r[i];
      }
      Vec<T>::store(y + t * E + c * N, acc);
    }
  }
}

// One pass over the slots, a row per tpr <= 64 neighbouring lanes: dye[s, :] = gate[a] dy[t, :] and dgate[a] =
// <dy[t, :], ye[s, :]>; an empty slot gets zeros and writes no dgate.
template <typename T>
__global__ void __launch_bounds__(kThreads) moe_combine_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ ye,
                                                                   const float* __restrict__ gate,
                                                                   const int32_t* __restrict__ src,
                                                                   T* __restrict__ dye, float* __restrict__ dgate,
                                                                   int64_t nslots, int64_t tokens, int k, int E,
                                                                   int tpr) {
  constexpr int N = Vec<T>::N;
  const int vpr = E / N;
  const int rpb = kThreads / tpr;
  const int rl = threadIdx.x / tpr, c0 = threadIdx.x - rl * tpr;
  const int64_t nk = tokens * k;
  const int64_t ngroups = (nslots + rpb - 1) / rpb;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {  // block-uniform: every lane reaches the shuffles
    const int64_t s = g * rpb + rl;
    int a = -1;
    if (s < nslots) {
      a = src[s];
      if (a >= nk) a = -1;
    }
    const int64_t t = a >= 0 ? a / k : 0;
    const float ga = a >= 0 ? gate[a] : 0.f;
    float dot = 0.f;
    if (s < nslots) {
      for (int c = c0; c < vpr; c += tpr) {
        float o[N];
        if (a >= 0) {
          float d[N], v[N];
          Vec<T>::load(dy + t * E + c * N, d);
          Vec<T>::load(ye + s * E + c * N, v);
#pragma unroll
          for (int i = 0; i < N; ++i) {
            dot += d[i] * v[i];
            o[i] = ga * d[i];
          }
        } else {
#pragma unroll
          for (int i = 0; i < N; ++i) o[i] = 0.f;
        }
        Vec<T>::store(dye + s * E + c * N, o);
      }
    }
    dot = group_sum(dot, tpr);
    if (a >= 0 && c0 == 0) dgate[a] = dot;
  }
}

}  // namespace

// ---------------------------------------------------------------- launchers
bool moe_route_supported(int Ne, int k) { return Ne >= 2 && Ne <= 256 && k >= 1 && k <= kMaxK && k <= Ne; }

int moe_route_parts(int64_t tokens, int Ne) {
  const int64_t groups = route_groups(tokens, route_lanes(Ne));
  const int64_t g = (groups + kWaves - 1) / kWaves;
  return (int)(g < 1 ? 1 : (g < kRouteGrid ? g : kRouteGrid));
}

template <typename T>
void moe_route_fwd(const T* logits, int32_t* idx, float* gate, float* part, int nparts, int64_t tokens, int Ne, int k,
                   hipStream_t s) {
  const int L = route_lanes(Ne);
  const dim3 grid((unsigned)nparts), block(kThreads);
  if (Ne <= 64) {
    hipLaunchKernelGGL((moe_route_fwd_kernel<T, 1>), grid, block, 0, s, logits, idx, gate, part, tokens, Ne, k, L);
  } else if (Ne <= 128) {
    hipLaunchKernelGGL((moe_route_fwd_kernel<T, 2>), grid, block, 0, s, logits, idx, gate, part, tokens, Ne, k, L);
  } else {
    hipLaunchKernelGGL((moe_route_fwd_kernel<T, 4>), grid, block, 0, s, logits, idx, gate, part, tokens, Ne, k, L);
  }
}

template <typename T>
void moe_route_bwd(const T* logits, const int32_t* idx, const float* gate, const float* dgate, const float* dprobs,
                   T* dlogits, int64_t tokens, int Ne, int k, hipStream_t s) {
  if (tokens == 0) return;
  const int L = route_lanes(Ne);
  const dim3 grid((unsigned)moe_route_parts(tokens, Ne)), block(kThreads);
  if (Ne <= 64) {
    hipLaunchKernelGGL((moe_route_bwd_kernel<T, 1>), grid, block, 0, s, logits, idx, gate, dgate, dprobs, dlogits,
                       tokens, Ne, k, L);
  } else if (Ne <= 128) {
    hipLaunchKernelGGL((moe_route_bwd_kernel<T, 2>), grid, block, 0, s, logits, idx, gate, dgate, dprobs, dlogits,
                       tokens, Ne, k, L);
  } else {
    hipLaunchKernelGGL((moe_route_bwd_kernel<T, 4>), grid, block, 0, s, logits, idx, gate, dgate, dprobs, dlogits,
                       tokens, Ne, k, L);
  }
}

int moe_assign_blocks(int64_t tokens, int k) {
  const int64_t n = tokens * k;
  const int64_t b = (n + kAssignChunk - 1) / kAssignChunk;
  return (int)(b < 1 ? 1 : b);
}

void moe_assign(const int32_t* idx, int32_t* slot, int32_t* src, int32_t* counts, int32_t* ws, int64_t tokens, int k,
                int Ne, int C, hipStream_t s) {
  const int nb = moe_assign_blocks(tokens, k);
  const dim3 grid((unsigned)nb), block(kThreads);
  hipLaunchKernelGGL(moe_assign_count_kernel, grid, block, 0, s, idx, ws, src, tokens, k, Ne, (int64_t)Ne * C);
  hipLaunchKernelGGL(moe_assign_scan_kernel, dim3(1), block, 0, s, ws, counts, nb, Ne);
  hipLaunchKernelGGL(moe_assign_rank_kernel<false>, grid, block, 0, s, idx, ws, (const int32_t*)nullptr, slot, src,
                     tokens, k, Ne, C);
}

void moe_assign_sorted(const int32_t* idx, int32_t* slot, int32_t* src, int32_t* counts, int32_t* offsets,
                       int32_t* tile_expert, int32_t* ws, int64_t tokens, int k, int Ne, int rows, hipStream_t s) {
  const int nb = moe_assign_blocks(tokens, k);
  const dim3 grid((unsigned)nb), block(kThreads);
  hipLaunchKernelGGL(moe_assign_count_kernel, grid, block, 0, s, idx, ws, src, tokens, k, Ne, (int64_t)rows);
  hipLaunchKernelGGL(moe_assign_sorted_scan_kernel, dim3(1), block, 0, s, ws, counts, offsets, tile_expert, nb, Ne,
                     rows / 128);
  hipLaunchKernelGGL(moe_assign_rank_kernel<true>, grid, block, 0, s, idx, ws, offsets, slot, src, tokens, k, Ne,
                     rows);
}

template <typename T>
void moe_gather_slots(const T* x, const int32_t* src, T* xe, int64_t nslots, int64_t tokens, int k, int E,
                      hipStream_t s) {
  if (nslots == 0) return;
  const int vpr = E / (int)(16 / sizeof(T));
  const int tpr = row_tpr(vpr, kThreads);
  hipLaunchKernelGGL(moe_gather_slots_kernel, dim3(row_grid(nslots, tpr)), dim3(kThreads), 0, s,
                     reinterpret_cast<const uint4*>(x), src, reinterpret_cast<uint4*>(xe), nslots, tokens, k, vpr,
                     tpr);
}

template <typename T>
void moe_gather_tokens(const T* ye, const int32_t* slot, const float* w, const T* res, T* y, int64_t tokens, int k,
                       int64_t nslots, int E, hipStream_t s) {
  if (tokens == 0) return;
  const int tpr = row_tpr(E / (int)(16 / sizeof(T)), kThreads);
  hipLaunchKernelGGL((moe_gather_tokens_kernel<T>), dim3(row_grid(tokens, tpr)), dim3(kThreads), 0, s, ye, slot, w,
                     res, y, tokens, k, nslots, E, tpr);
}

template <typename T>
void moe_combine_bwd(const T* dy, const T* ye, const float* gate, const int32_t* src, T* dye, float* dgate,
                     int64_t nslots, int64_t tokens, int k, int E, hipStream_t s) {
  if (nslots == 0) return;
  const int tpr = row_tpr(E / (int)(16 / sizeof(T)), 64);
  hipLaunchKernelGGL((moe_combine_bwd_kernel<T>), dim3(row_grid(nslots, tpr)), dim3(kThreads), 0, s, dy, ye, gate, src,
                     dye, dgate, nslots, tokens, k, E, tpr);
}

#define MOE_INSTANTIATE(T)                                                                                             \
  template void moe_route_fwd<T>(const T*, int32_t*, float*, float*, int, int64_t, int, int, hipStream_t);             \
  template void moe_route_bwd<T>(const T*, const int32_t*, const float*, const float*, const float*, T*, int64_t, int, \
                                 int, hipStream_t);                                                                    \
  template void moe_gather_slots<T>(const T*, const int32_t*, T*, int64_t, int64_t, int, int, hipStream_t);            \
  template void moe_gather_tokens<T>(const T*, const int32_t*, const float*, const T*, T*, int64_t, int, int64_t, int, \
                                     hipStream_t);                                                                     \
  template void moe_combine_bwd<T>(const T*, const T*, const float*, const int32_t*, T*, float*, int64_t, int64_t,     \
                                   int, int, hipStream_t);
MOE_INSTANTIATE(float)
MOE_INSTANTIATE(bf16_t)
#undef MOE_INSTANTIATE

}  // namespace mipipe
