// QK-norm: per-head RMSNorm of the Q and K heads of the packed projection,
// fused with the rotary rotation (Qwen3, OLMo-2, Gemma-3).
//
//   x [B, S, n_q + n_k + n_v, D]: the first n_q heads are Q, the next n_k are K,
//   the last n_v (V) pass through -- rope_heads' layout (llama.hip).
//
//   fwd, per (token, head) row of a Q or K head:
//       rstd = rsqrt(mean(x^2) + eps),  n = x rstd w        (w = wq | wk, [D])
//       y = rotate(n) at position pos0 + s                   (rope_kernel's pairs
//       (i, i + D/2) and fp32 host tables; dropped when ROPE is false)
//     fp32 throughout, rounded once at the store; V is copied, or untouched
//     when out aliases x.  rstd [tokens, n_q + n_k] is written for a backward.
//   bwd:  g = inverse-rotate(dout),  xhat = x rstd,  gy = g w,  c = mean(gy xhat)
//       dx = rstd (gy - xhat c),   dV = dout,   dw[d] = sum over rows of g xhat
//
// Memory-bound, rope_kernel's item mapping: one lane owns the 8 + 8 elements
// (i .. i + 7, i + D/2 .. i + D/2 + 7) of a row, so a row is L = D / 16
// neighbouring lanes (1 .. 16, a power of two: rows never straddle a wave) and
// the row sums are xor shuffles below L.  The items of a token are a multiple
// of L and so is the grid stride: a lane keeps its column slot i in every
// iteration, which lets it hold both weights' 16 values (fwd) and both weight
// gradients' 16 partial sums (bwd) in registers for the whole kernel.
//
// dwq / dwk: the block's four waves add their lanes' sums in LDS in wave order,
// the lanes that share a column slot are then added in lane order, each block
// writes one fp32 partial row per weight and reduce_parts sums them -- no
// float atomics, the same bits every run.
#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

constexpr int kThreads = 256;
constexpr int kFwdGrid = 2048;  // rope_kernel's cap

int64_t grid_for(int64_t nitems, int cap) {
  const int64_t g = (nitems + kThreads - 1) / kThreads;
  return g < cap ? (g < 1 ? 1 : g) : cap;
}

// Sum over the L lanes of a row (L a power of two <= 16, the same in every lane).
__device__ __forceinline__ float row_sum(float v, int L) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1)
    if (o < L) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T>
__device__ __forceinline__ void copy8(const T* src, T* dst) {
  if (sizeof(T) == 2) {
    *reinterpret_cast<u16x8*>(dst) = *reinterpret_cast<const u16x8*>(src);
  } else {
    const float4* q = reinterpret_cast<const float4*>(src);
    float4* o = reinterpret_cast<float4*>(dst);
    const float4 v0 = q[0], v1 = q[1];
    o[0] = v0;
    o[1] = v1;
  }
}

// Items per token: n_norm * L row items, then -- only when V is copied --
// n_v * D / 8 vectors of the last n_v heads.
template <typename T, bool ROPE>
__global__ void __launch_bounds__(kThreads) qknorm_fwd_kernel(
    const T* x, const T* __restrict__ wq, const T* __restrict__ wk, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, T* out, float* __restrict__ rstd_out, int64_t tokens, int S, int n_q, int n_k,
    int n_v, int D, int pos0, float eps, int copy_v) {
  const int half = D >> 1;
  const int L = D >> 4;
  const int n_norm = n_q + n_k;
  const int norm_items = n_norm * L;
  const int per_tok = norm_items + (copy_v ? n_v * (D >> 3) : 0);
  const int64_t nitems = tokens * per_tok;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t tok_elems = (int64_t)(n_norm + n_v) * D;
  const float inv_d = 1.f / (float)D;
  const int i = (int)(threadIdx.x & (L - 1)) * 8;  // the lane's column slot in every iteration
  float wqa[8], wqb[8], wka[8], wkb[8];
  Io<T>::load8(wq + i, wqa);
  Io<T>::load8(wq + half + i, wqb);
  Io<T>::load8(wk + i, wka);
  Io<T>::load8(wk + half + i, wkb);
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < nitems; t += stride) {
    const int64_t tok = t / per_tok;
    const int j = (int)(t - tok * per_tok);
    if (j < norm_items) {  // whole rows: the L lanes of a row take this branch together
      const int h = j / L;
      const int64_t e = tok * tok_elems + (int64_t)h * D + i;
      float a[8], b[8], oa[8], ob[8];
      Io<T>::load8(x + e, a);
      Io<T>::load8(x + e + half, b);
      float s2 = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s2 += a[k] * a[k] + b[k] * b[k];
      const float rstd = rsqrtf(row_sum(s2, L) * inv_d + eps);
      if (rstd_out != nullptr && i == 0) rstd_out[tok * n_norm + h] = rstd;
      const bool is_q = h < n_q;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        a[k] = a[k] * rstd * (is_q ? wqa[k] : wka[k]);
        b[k] = b[k] * rstd * (is_q ? wqb[k] : wkb[k]);
      }
      if (ROPE) {
        const int64_t te = (int64_t)(pos0 + (int)(tok % S)) * half + i;
        float c[8], s[8];
        Io<float>::load8(cos_t + te, c);
        Io<float>::load8(sin_t + te, s);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          oa[k] = a[k] * c[k] - b[k] * s[k];
          ob[k] = b[k] * c[k] + a[k] * s[k];
        }
        Io<T>::store8(out + e, oa);
        Io<T>::store8(out + e + half, ob);
      } else {
        Io<T>::store8(out + e, a);
        Io<T>::store8(out + e + half, b);
      }
    } else {
      const int64_t e = tok * tok_elems + (int64_t)n_norm * D + (int64_t)(j - norm_items) * 8;
      copy8<T>(x + e, out + e);
    }
  }
}

// The backward is always out of place (dx is a fresh tensor), so the V vectors
// of dout are always copied.  part_q / part_k: [gridDim.x, D] fp32.
template <typename T, bool ROPE>
__global__ void __launch_bounds__(kThreads) qknorm_bwd_kernel(
    const T* __restrict__ dout, const T* __restrict__ x, const float* __restrict__ rstd_in, const T* __restrict__ wq,
    const T* __restrict__ wk, const float* __restrict__ cos_t, const float* __restrict__ sin_t, T* __restrict__ dx,
    float* __restrict__ part_q, float* __restrict__ part_k, int64_t tokens, int S, int n_q, int n_k, int n_v, int D,
    int pos0) {
  static_assert(kThreads == 256, "the fold below sums 4 waves");
  __shared__ float fold[32][64];
  const int half = D >> 1;
  const int L = D >> 4;
  const int n_norm = n_q + n_k;
  const int norm_items = n_norm * L;
  const int per_tok = norm_items + n_v * (D >> 3);
  const int64_t nitems = tokens * per_tok;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t tok_elems = (int64_t)(n_norm + n_v) * D;
  const float inv_d = 1.f / (float)D;
  const int i = (int)(threadIdx.x & (L - 1)) * 8;
  float wqa[8], wqb[8], wka[8], wkb[8];
  Io<T>::load8(wq + i, wqa);
  Io<T>::load8(wq + half + i, wqb);
  Io<T>::load8(wk + i, wka);
  Io<T>::load8(wk + half + i, wkb);
  float dq[16], dk[16];  // this lane's columns i .. i + 7 ([0, 8)) and half + i .. ([8, 16)) of dwq / dwk
#pragma unroll
  for (int k = 0; k < 16; ++k) dq[k] = dk[k] = 0.f;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < nitems; t += stride) {
    const int64_t tok = t / per_tok;
    const int j = (int)(t - tok * per_tok);
    if (j < norm_items) {
      const int h = j / L;
      const int64_t e = tok * tok_elems + (int64_t)h * D + i;
      float ga[8], gb[8], xa[8], xb[8];
      Io<T>::load8(dout + e, ga);
      Io<T>::load8(dout + e + half, gb);
      Io<T>::load8(x + e, xa);
      Io<T>::load8(x + e + half, xb);
      const float rstd = rstd_in[tok * n_norm + h];
      if (ROPE) {
        const int64_t te = (int64_t)(pos0 + (int)(tok % S)) * half + i;
        float c[8], s[8];
        Io<float>::load8(cos_t + te, c);
        Io<float>::load8(sin_t + te, s);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float da = ga[k], db = gb[k];
          ga[k] = da * c[k] + db * s[k];
          gb[k] = db * c[k] - da * s[k];
        }
      }
      const bool is_q = h < n_q;
      float cs = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        xa[k] *= rstd;  // xhat
        xb[k] *= rstd;
        const float pa = ga[k] * xa[k], pb = gb[k] * xb[k];
        dq[k] += is_q ? pa : 0.f;
        dq[8 + k] += is_q ? pb : 0.f;
        dk[k] += is_q ? 0.f : pa;
        dk[8 + k] += is_q ? 0.f : pb;
        ga[k] *= is_q ? wqa[k] : wka[k];  // gy
        gb[k] *= is_q ? wqb[k] : wkb[k];
        cs += ga[k] * xa[k] + gb[k] * xb[k];
      }
      const float c = row_sum(cs, L) * inv_d;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ga[k] = rstd * (ga[k] - xa[k] * c);
        gb[k] = rstd * (gb[k] - xb[k] * c);
      }
      Io<T>::store8(dx + e, ga);
      Io<T>::store8(dx + e + half, gb);
    } else {
      const int64_t e = tok * tok_elems + (int64_t)n_norm * D + (int64_t)(j - norm_items) * 8;
      copy8<T>(dout + e, dx + e);
    }
  }
  // every lane is back here (no barrier above).  The four waves add their sums into fold[value][lane] one wave at
  // a time (wave order), then one thread per column adds the 64 / L lanes that share its column slot (lane order).
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int src = 0; src < kThreads / 64; ++src) {
    if (wave == src) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (src == 0) {
          fold[k][lane] = dq[k];
          fold[16 + k][lane] = dk[k];
        } else {
          fold[k][lane] += dq[k];
          fold[16 + k][lane] += dk[k];
        }
      }
    }
    __syncthreads();
  }
  for (int c = threadIdx.x; c < 2 * D; c += kThreads) {
    const int which = c >= D ? 1 : 0, col = c - which * D;
    const int upper = col >= half ? 1 : 0, in_half = col - upper * half;
    const float* row = fold[which * 16 + upper * 8 + (in_half & 7)];
    float v = 0.f;
    for (int l = in_half >> 3; l < 64; l += L) v += row[l];
    (which ? part_k : part_q)[(size_t)blockIdx.x * D + col] = v;
  }
}

}  // namespace

bool qknorm_supported(int D) { return D == 16 || D == 32 || D == 64 || D == 128 || D == 256; }

int qknorm_bwd_parts(int64_t tokens, int n_q, int n_k, int n_v, int D) {
  // 1024 blocks of 4 waves: 16 waves per CU in flight, and at most 2 x 1024 partial rows to sum
  const int64_t nitems = tokens * ((int64_t)(n_q + n_k) * (D / 16) + (int64_t)n_v * (D / 8));
  return (int)grid_for(nitems, 1024);
}

template <typename T>
void qknorm_rope_fwd(const T* x, const T* wq, const T* wk, const float* cos_t, const float* sin_t, T* out, float* rstd,
                     int64_t tokens, int S, int n_q, int n_k, int n_v, int D, int pos0, float eps, hipStream_t s) {
  const bool copy_v = out != x;
  const int64_t nitems = tokens * ((int64_t)(n_q + n_k) * (D / 16) + (copy_v ? (int64_t)n_v * (D / 8) : 0));
  if (nitems == 0) return;
  const dim3 grid((unsigned)grid_for(nitems, kFwdGrid)), block(kThreads);
  if (cos_t != nullptr) {
    hipLaunchKernelGGL((qknorm_fwd_kernel<T, true>), grid, block, 0, s, x, wq, wk, cos_t, sin_t, out, rstd, tokens, S,
                       n_q, n_k, n_v, D, pos0, eps, copy_v ? 1 : 0);
  } else {
    hipLaunchKernelGGL((qknorm_fwd_kernel<T, false>), grid, block, 0, s, x, wq, wk, cos_t, sin_t, out, rstd, tokens, S,
                       n_q, n_k, n_v, D, pos0, eps, copy_v ? 1 : 0);
  }
}

template <typename T>
void qknorm_rope_bwd(const T* dout, const T* x, const float* rstd, const T* wq, const T* wk, const float* cos_t,
                     const float* sin_t, T* dx, float* part_q, float* part_k, int nparts, int64_t tokens, int S,
                     int n_q, int n_k, int n_v, int D, int pos0, hipStream_t s) {
  const dim3 grid((unsigned)nparts), block(kThreads);
  if (cos_t != nullptr) {
    hipLaunchKernelGGL((qknorm_bwd_kernel<T, true>), grid, block, 0, s, dout, x, rstd, wq, wk, cos_t, sin_t, dx, part_q,
                       part_k, tokens, S, n_q, n_k, n_v, D, pos0);
  } else {
    hipLaunchKernelGGL((qknorm_bwd_kernel<T, false>), grid, block, 0, s, dout, x, rstd, wq, wk, cos_t, sin_t, dx,
                       part_q, part_k, tokens, S, n_q, n_k, n_v, D, pos0);
  }
}

template void qknorm_rope_fwd<float>(const float*, const float*, const float*, const float*, const float*, float*,
                                     float*, int64_t, int, int, int, int, int, int, float, hipStream_t);
template void qknorm_rope_fwd<bf16_t>(const bf16_t*, const bf16_t*, const bf16_t*, const float*, const float*, bf16_t*,
                                      float*, int64_t, int, int, int, int, int, int, float, hipStream_t);
template void qknorm_rope_bwd<float>(const float*, const float*, const float*, const float*, const float*, const float*,
                                     const float*, float*, float*, float*, int, int64_t, int, int, int, int, int, int,
                                     hipStream_t);
template void qknorm_rope_bwd<bf16_t>(const bf16_t*, const bf16_t*, const float*, const bf16_t*, const bf16_t*,
                                      const float*, const float*, bf16_t*, float*, float*, int, int64_t, int, int, int,
                                      int, int, int, hipStream_t);

}  // namespace mipipe
