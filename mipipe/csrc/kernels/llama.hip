// The LLaMA-style block's two element-wise kernels: the gated SiLU of the MLP
// (SwiGLU) and rotary position embeddings on the packed QKV projection.
//
// Both are memory-bound: 16-byte vectors, grid-stride over 64-bit item
// indices, two items in flight per thread, fp32 arithmetic.
//
//   SwiGLU fwd:  h = silu(g) * u            gu [rows, 2F] = [g | u] per row
//          bwd:  dg = dh u s (1 + g (1 - s)),  du = dh silu(g),  s = sigmoid(g)
//                written as ONE dgu [rows, 2F] (it feeds W1's dgrad / wgrad
//                GEMMs without a concatenation)
//   RoPE:  (a, b) = (q_i, q_{i + D/2}) -> (a c - b s, b c + a s) on Q and K of
//          qkv [B, S, 3, H, D] at position pos0 + s; cos / sin come from fp32
//          host-built tables [>= pos0 + S, D/2] (no device trigonometry); V is
//          copied, or untouched when out aliases qkv.  The backward is the
//          same kernel with sin negated (`inverse`) on dqkv.
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

// Items per token: H * D / 16 rotations of Q, as many of K (8 pairs each:
// elements i .. i + 7 and i + D/2 .. i + D/2 + 7 of one head), then -- only
// when V is copied -- H * D / 8 vectors of V.
template <typename T>
__global__ void __launch_bounds__(kThreads) rope_kernel(const T* qkv, const float* __restrict__ cos_t,
                                                        const float* __restrict__ sin_t, T* out, int64_t tokens, int S,
                                                        int H, int D, int pos0, float sign, int copy_v) {
  const int half = D >> 1;
  const int hvec = half >> 3;        // rotation items per head
  const int rot = H * hvec;          // per Q (and per K) of one token
  const int per_tok = 2 * rot * (copy_v ? 2 : 1);
  const int64_t nitems = tokens * per_tok;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t tok_elems = (int64_t)3 * H * D;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < nitems; t += stride) {
    const int64_t tok = t / per_tok;
    const int j = (int)(t - tok * per_tok);
    if (j < 2 * rot) {
      const int which = j / rot, r = j - which * rot;
      const int h = r / hvec, i = (r - h * hvec) * 8;
      const int64_t e = tok * tok_elems + ((int64_t)which * H + h) * D + i;
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
      const int64_t e = tok * tok_elems + (int64_t)2 * H * D + (int64_t)(j - 2 * rot) * 8;
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
void rope_packed(const T* qkv, const float* cos_t, const float* sin_t, T* out, int64_t B, int S, int H, int D, int pos0,
                 bool inverse, hipStream_t s) {
  const bool copy_v = out != qkv;
  const int64_t nitems = B * S * (int64_t)(2 * H * (D / 16)) * (copy_v ? 2 : 1);
  if (nitems == 0) return;
  hipLaunchKernelGGL((rope_kernel<T>), dim3((unsigned)grid_for(nitems)), dim3(kThreads), 0, s, qkv, cos_t, sin_t, out,
                     B * S, S, H, D, pos0, inverse ? -1.f : 1.f, copy_v ? 1 : 0);
}

template void swiglu_fwd<float>(const float*, float*, int64_t, int, hipStream_t);
template void swiglu_fwd<bf16_t>(const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
template void swiglu_bwd<float>(const float*, const float*, float*, int64_t, int, hipStream_t);
template void swiglu_bwd<bf16_t>(const bf16_t*, const bf16_t*, bf16_t*, int64_t, int, hipStream_t);
template void rope_packed<float>(const float*, const float*, const float*, float*, int64_t, int, int, int, int, bool, hipStream_t);
template void rope_packed<bf16_t>(const bf16_t*, const float*, const float*, bf16_t*, int64_t, int, int, int, int, bool, hipStream_t);

}  // namespace mipipe
