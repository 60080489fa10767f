// The LLaMA-style block's two element-wise kernels: the gated SiLU of the MLP
// (SwiGLU) and rotary position embeddings on the packed QKV projection.
//
// GeGLU (the Gemma-2 MLP's gate) is the same kernel body with the tanh-GELU in
// place of SiLU.  All are memory-bound: 16-byte vectors, grid-stride over 64-bit item
// indices, two items in flight per thread, fp32 arithmetic.
//
//   SwiGLU fwd:  h = silu(g) * u            gu [rows, 2F] = [g | u] per row
//          bwd:  dg = dh u s (1 + g (1 - s)),  du = dh silu(g),  s = sigmoid(g)
//                written as ONE dgu [rows, 2F] (it feeds W1's dgrad / wgrad
//                GEMMs without a concatenation)
//   GeGLU fwd:  h = gelu_tanh(g) * u = g s u,  s = 0.5 (1 + tanh(a)) = 1 / (1 + exp(-2a)),
//               a = sqrt(2/pi) (g + 0.044715 g^3)   (no 1 + tanh: it cancels for g << 0)
//          bwd:  dg = dh u (s + g s (1 - s) 2 sqrt(2/pi) (1 + 3 * 0.044715 g^2)),  du = dh g s
//   RoPE:  (a, b) = (q_i, q_{i + D/2}) -> (a c - b s, b c + a s) on Q and K of
//          qkv [B, S, 3, H, D] at position pos0 + s; cos / sin come from fp32
//          host-built tables [>= pos0 + S, D/2] (no device trigonometry); V is
//          copied, or untouched when out aliases qkv.  The backward is the
//          same kernel with sin negated (`inverse`) on dqkv.  The kernel takes
//          "rotate the first n_rot heads of a token, pass the last n_copy
//          through": (2H, H) is the layout above, (H + Hkv, Hkv) the
//          grouped-query projection [B, S, H + 2 Hkv, D].
//   GQA dK/dV reduce:  sums the per-query-head partials of each K/V head's
//          group into the packed dqkv (gqa_reduce_dkv_kernel).
#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

constexpr int kThreads = 256;

int64_t grid_for(int64_t nitems) {
  int64_t g = (nitems + kThreads - 1) / kThreads;
  return g < 2048 ? (g < 1 ? 1 : g) : 2048;
}

// sigmoid and silu of one gate value.  A gate of -inf gives s = 0 and the
// limits silu = 0, silu' = 0 (g * s would be -inf * 0).
__device__ __forceinline__ void silu_parts(float g, float& s, float& silu) {
  s = __builtin_amdgcn_rcpf(1.f + __expf(-g));
  silu = g == -INFINITY ? 0.f : g * s;
}

template <typename T, bool BWD>
__global__ void __launch_bounds__(kThreads) swiglu_kernel(const T* __restrict__ gu, const T* __restrict__ dh,
                                                          T* __restrict__ out, int64_t rows, int F) {
  const int fvec = F >> 3;
  const int64_t nitems = rows * fvec;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t t0 = blockIdx.x * (int64_t)kThreads + threadIdx.x; t0 < nitems; t0 += 2 * stride) {
    float g[2][8], u[2][8], d[2][8];
    int64_t row[2];
    int c[2];
    bool on[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t t = t0 + j * stride;
      on[j] = t < nitems;
      if (on[j]) {
        row[j] = t / fvec;
        c[j] = (int)(t - row[j] * fvec) * 8;
        const T* src = gu + row[j] * 2 * F + c[j];
        Io<T>::load8(src, g[j]);
        Io<T>::load8(src + F, u[j]);
        if (BWD) Io<T>::load8(dh + row[j] * F + c[j], d[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (!on[j]) continue;
      if (!BWD) {
        float h[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float s, silu;
          silu_parts(g[j][i], s, silu);
          h[i] = silu * u[j][i];
        }
        Io<T>::store8(out + row[j] * F + c[j], h);
      } else {
        float dg[8], du[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float s, silu;
          silu_parts(g[j][i], s, silu);
          const float grad = g[j][i] == -INFINITY ? 0.f : s * (1.f + g[j][i] * (1.f - s));
          dg[i] = d[j][i] * u[j][i] * grad;
          du[i] = d[j][i] * silu;
        }
        T* dst = out + row[j] * 2 * F + c[j];
        Io<T>::store8(dst, dg);
        Io<T>::store8(dst + F, du);
      }
    }
  }
}

// The tanh-GELU's s = 0.5 (1 + tanh(a)) in its cancellation-free form, gelu = g s
// and gelu' of one gate value.  exp overflowing to inf gives s = 0, gelu = 0 and
// gelu' = 0; where s (1 - s) is 0 the polynomial factor, which may be inf, is
// not multiplied in.  A gate of -inf gives the limits 0 and 0 (g * s would be
// -inf * 0), +inf gives gelu = inf, gelu' = 1.
__device__ __forceinline__ void gelu_tanh_parts(float g, float& act, float& grad) {
  constexpr float k0 = 0.7978845608028654f, k1 = 0.044715f;  // sqrt(2 / pi)
  const float g2 = g * g;
  const float a = k0 * g * (1.f + k1 * g2);
  const float s = __builtin_amdgcn_rcpf(1.f + __expf(-2.f * a));
  const float t = s * (1.f - s);
  act = s == 0.f ? 0.f : g * s;
  grad = t == 0.f ? s : s + g * t * (2.f * k0 * (1.f + 3.f * k1 * g2));
}

// swiglu_kernel with the tanh-GELU as the gate: a sibling, so that kernel stays as it is compiled.
template <typename T, bool BWD>
__global__ void __launch_bounds__(kThreads) geglu_kernel(const T* __restrict__ gu, const T* __restrict__ dh,
                                                         T* __restrict__ out, int64_t rows, int F) {
  const int fvec = F >> 3;
  const int64_t nitems = rows * fvec;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t t0 = blockIdx.x * (int64_t)kThreads + threadIdx.x; t0 < nitems; t0 += 2 * stride) {
    float g[2][8], u[2][8], d[2][8];
    int64_t row[2];
    int c[2];
    bool on[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t t = t0 + j * stride;
      on[j] = t < nitems;
      if (on[j]) {
        row[j] = t / fvec;
        c[j] = (int)(t - row[j] * fvec) * 8;
        const T* src = gu + row[j] * 2 * F + c[j];
        Io<T>::load8(src, g[j]);
        Io<T>::load8(src + F, u[j]);
        if (BWD) Io<T>::load8(dh + row[j] * F + c[j], d[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (!on[j]) continue;
      if (!BWD) {
        float h[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float act, grad;
          gelu_tanh_parts(g[j][i], act, grad);
          h[i] = act * u[j][i];
        }
        Io<T>::store8(out + row[j] * F + c[j], h);
      } else {
        float dg[8], du[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float act, grad;
          gelu_tanh_parts(g[j][i], act, grad);
          dg[i] = d[j][i] * u[j][i] * grad;
          du[i] = d[j][i] * act;
        }
        T* dst = out + row[j] * 2 * F + c[j];
        Io<T>::store8(dst, dg);
        Io<T>::store8(dst + F, du);
      }
    }
  }
}

// Items per token: n_rot * D / 16 rotations (8 pairs each: elements i .. i + 7
// and i + D/2 .. i + D/2 + 7 of one of the first n_rot heads), then -- only when
// the rest is copied -- n_copy * D / 8 vectors of the last n_copy heads.
template <typename T>
__global__ void __launch_bounds__(kThreads) rope_kernel(const T* qkv, const float* __restrict__ cos_t,
                                                        const float* __restrict__ sin_t, T* out, int64_t tokens, int S,
                                                        int n_rot, int n_copy, int D, int pos0, float sign, int copy_v) {
  const int half = D >> 1;
  const int hvec = half >> 3;        // rotation items per head
  const int rot = n_rot * hvec;      // rotation items per token
  const int per_tok = rot + (copy_v ? n_copy * (D >> 3) : 0);
  const int64_t nitems = tokens * per_tok;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t tok_elems = (int64_t)(n_rot + n_copy) * D;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < nitems; t += stride) {
    const int64_t tok = t / per_tok;
    const int j = (int)(t - tok * per_tok);
    if (j < rot) {
      const int h = j / hvec, i = (j - h * hvec) * 8;
      const int64_t e = tok * tok_elems + (int64_t)h * D + i;
      const int64_t te = (int64_t)(pos0 + (int)(tok % S)) * half + i;
      float a[8], b[8], c[8], s[8], oa[8], ob[8];
      Io<T>::load8(qkv + e, a);
      Io<T>::load8(qkv + e + half, b);
      Io<float>::load8(cos_t + te, c);
      Io<float>::load8(sin_t + te, s);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float sn = s[k] * sign;
        oa[k] = a[k] * c[k] - b[k] * sn;
        ob[k] = b[k] * c[k] + a[k] * sn;
      }
      Io<T>::store8(out + e, oa);
      Io<T>::store8(out + e + half, ob);
    } else {
      const int64_t e = tok * tok_elems + (int64_t)n_rot * D + (int64_t)(j - rot) * 8;
      if (sizeof(T) == 2) {
        *reinterpret_cast<u16x8*>(out + e) = *reinterpret_cast<const u16x8*>(qkv + e);
      } else {
        const float4* q = reinterpret_cast<const float4*>(qkv + e);
        float4* o = reinterpret_cast<float4*>(out + e);
        const float4 v0 = q[0], v1 = q[1];
        o[0] = v0;
        o[1] = v1;
      }
    }
  }
}

// Grouped-query attention: the dK / dV kernels leave one partial per QUERY head
// in dkv [tokens, 2, H, D]; item (token, which, kv head, 8 features) adds the
// G = H / Hkv partials of its group in fp32 (in head order), rounds once and
// stores into head H + which * Hkv + kv of dqkv [tokens, H + 2 Hkv, D].  The Q
// heads of dqkv (the dQ kernel's output) are not touched.  Two partials are in
// flight per thread; 64-bit item and element indices.
template <typename T>
__global__ void __launch_bounds__(kThreads) gqa_reduce_dkv_kernel(const T* __restrict__ dkv, T* __restrict__ dqkv,
                                                                  int64_t tokens, int H, int Hkv, int D) {
  const int G = H / Hkv;
  const int dvec = D >> 3;
  const int per_tok = 2 * Hkv * dvec;
  const int64_t nitems = tokens * per_tok;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t src_tok = (int64_t)2 * H * D, dst_tok = (int64_t)(H + 2 * Hkv) * D;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < nitems; t += stride) {
    const int64_t tok = t / per_tok;
    const int j = (int)(t - tok * per_tok);
    const int hk = j / dvec, i = (j - hk * dvec) * 8;  // hk = which * Hkv + kv head
    const int which = hk / Hkv, kv = hk - which * Hkv;
    const T* src = dkv + tok * src_tok + ((int64_t)which * H + (int64_t)kv * G) * D + i;
    float acc[8], x[8], y[8];
    Io<T>::load8(src, acc);
    int g = 1;
    for (; g + 1 < G; g += 2) {
      Io<T>::load8(src + (int64_t)g * D, x);
      Io<T>::load8(src + (int64_t)(g + 1) * D, y);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = (acc[k] + x[k]) + y[k];
    }
    if (g < G) {
      Io<T>::load8(src + (int64_t)g * D, x);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += x[k];
    }
    Io<T>::store8(dqkv + tok * dst_tok + (int64_t)(H + hk) * D + i, acc);
  }
}

}  // namespace

template <typename T>
void swiglu_fwd(const T* gu, T* h, int64_t rows, int F, hipStream_t s) {
  const int64_t nitems = rows * (F / 8);
  if (nitems == 0) return;
  hipLaunchKernelGGL((swiglu_kernel<T, false>), dim3((unsigned)grid_for((nitems + 1) / 2)), dim3(kThreads), 0, s, gu,
                     (const T*)nullptr, h, rows, F);
}

template <typename T>
void swiglu_bwd(const T* dh, const T* gu, T* dgu, int64_t rows, int F, hipStream_t s) {
  const int64_t nitems = rows * (F / 8);
  if (nitems == 0) return;
  hipLaunchKernelGGL((swiglu_kernel<T, true>), dim3((unsigned)grid_for((nitems + 1) / 2)), dim3(kThreads), 0, s, gu,
                     dh, dgu, rows, F);
}

template <typename T>
void geglu_fwd(const T* gu, T* h, int64_t rows, int F, hipStream_t s) {
  const int64_t nitems = rows * (F / 8);
  if (nitems == 0) return;
  hipLaunchKernelGGL((geglu_kernel<T, false>), dim3((unsigned)grid_for((nitems + 1) / 2)), dim3(kThreads), 0, s, gu,
                     (const T*)nullptr, h, rows, F);
}

template <typename T>
void geglu_bwd(const T* dh, const T* gu, T* dgu, int64_t rows, int F, hipStream_t s) {
  const int64_t nitems = rows * (F / 8);
  if (nitems == 0) return;
  hipLaunchKernelGGL((geglu_kernel<T, true>), dim3((unsigned)grid_for((nitems + 1) / 2)), dim3(kThreads), 0, s, gu,
                     dh, dgu, rows, F);
}

template <typename T>
void rope_heads(const T* x, const float* cos_t, const float* sin_t, T* out, int64_t B, int S, int n_rot, int n_copy,
                int D, int pos0, bool inverse, hipStream_t s) {
  const bool copy_v = out != x;
  const int64_t nitems = B * S * ((int64_t)n_rot * (D / 16) + (copy_v ? (int64_t)n_copy * (D / 8) : 0));
  if (nitems == 0) return;
  hipLaunchKernelGGL((rope_kernel<T>), dim3((unsigned)grid_for(nitems)), dim3(kThreads), 0, s, x, cos_t, sin_t, out,
                     B * S, S, n_rot, n_copy, D, pos0, inverse ? -1.f : 1.f, copy_v ? 1 : 0);
}

template <typename T>
void rope_packed(const T* qkv, const float* cos_t, const float* sin_t, T* out, int64_t B, int S, int H, int D, int pos0,
                 bool inverse, hipStream_t s) {
  rope_heads<T>(qkv, cos_t, sin_t, out, B, S, 2 * H, H, D, pos0, inverse, s);
}

template <typename T>
void gqa_reduce_dkv(const T* dkv, T* dqkv, int64_t tokens, int H, int Hkv, int D, hipStream_t s) {
  const int64_t nitems = tokens * 2 * Hkv * (D / 8);
  if (nitems == 0) return;
  hipLaunchKernelGGL((gqa_reduce_dkv_kernel<T>), dim3((unsigned)grid_for(nitems)), dim3(kThreads), 0, s, dkv, dqkv,
                     tokens, H, Hkv, D);
}

template void swiglu_fwd<float>(const float*, float*, int64_t, int, hipStream_t);
template void swiglu_fwd<bf16_t>(const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
template void swiglu_bwd<float>(const float*, const float*, float*, int64_t, int, hipStream_t);
template void swiglu_bwd<bf16_t>(const bf16_t*, const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
template void geglu_fwd<float>(const float*, float*, int64_t, int, hipStream_t);
template void geglu_fwd<bf16_t>(const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
template void geglu_bwd<float>(const float*, const float*, float*, int64_t, int, hipStream_t);
template void geglu_bwd<bf16_t>(const bf16_t*, const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
template void rope_packed<float>(const float*, const float*, const float*, float*, int64_t, int, int, int, int, bool, hipStream_t);
template void rope_packed<bf16_t>(const bf16_t*, const float*, const float*, bf16_t*, int64_t, int, int, int, int, bool, hipStream_t);
template void rope_heads<float>(const float*, const float*, const float*, float*, int64_t, int, int, int, int, int, bool, hipStream_t);
template void rope_heads<bf16_t>(const bf16_t*, const float*, const float*, bf16_t*, int64_t, int, int, int, int, int, bool, hipStream_t);
template void gqa_reduce_dkv<float>(const float*, float*, int64_t, int, int, int, hipStream_t);
template void gqa_reduce_dkv<bf16_t>(const bf16_t*, bf16_t*, int64_t, int, int, int, hipStream_t);

}  // namespace mipipe
