// Fused residual + dropout + RMSNorm, forward and backward (the LLaMA-style
// block's norm; same contract as layernorm.hip, without mean and beta).
//
//   z = residual + dropout(x)          (residual optional, dropout optional)
//   y = z * rsqrt(mean(z^2) + eps) * gamma
//
// One pass over HBM each way, the row held in registers (16-byte vectors),
// statistics in fp32, ONE row reduction in the forward (LayerNorm needs two)
// and one in the backward.  The dispatch is LayerNorm's, so the two kernels
// meet the same widths the same way: rows up to 2048 wide run one wave per row
// (shuffles only), wider rows one row per 256-thread group with 2 / 4 / 8
// vectors per thread.  The dropout mask is never stored: backward regenerates
// it from the same Philox (seed, offset).
//
// The sandwich norm of the Gemma-2 block (rmsnorm_residual_fwd) is a variant of
// the same forward kernels: y = residual + x * rsqrt(mean(x^2) + eps) * gamma,
// the statistics from x alone.  Its backward is the one below on (dy, x, rstd)
// with p = 0; the residual's gradient is dy itself.
//
//   xhat = z rstd, gy = dy gamma, b = mean(gy xhat)
//   dz = rstd (gy - xhat b) [+ addend],  dx = dz mask / (1 - p),  dgamma = sum_rows dy xhat
//
// dgamma: per-workgroup partial rows, reduced by reduce_parts -- no float
// atomics, so results are reproducible.
#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

constexpr int kThreads = 256;

// Sum over the 256-thread block (layernorm.hip's): one barrier, the caller's
// scratch is written once per launch.
__device__ __forceinline__ float block_sum_once(float a, float* scratch) {
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = a;
  __syncthreads();
  return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

// 8 elements kept as loaded (bf16: 4 registers instead of 8), converted on use.
template <typename T> struct Raw8;
template <> struct Raw8<float> {
  float v[8];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
  }
  __device__ __forceinline__ void load(const float* p) { Io<float>::load8(p, v); }
  __device__ __forceinline__ float get(int i) const { return v[i]; }
};
template <> struct Raw8<bf16_t> {
  u16x8 v;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0;
  }
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const u16x8*>(p); }
  __device__ __forceinline__ float get(int i) const { return bf2f(v[i]); }
};

// POST (the sandwich norm, y = res + x rstd gamma): the statistics come from x
// alone and the residual, loaded with x and kept as loaded, is added after the
// scale; no dropout, no z, and rstd only where the caller wants it.
template <typename T, int MAXV, bool POST>
__global__ void __launch_bounds__(kThreads) rms_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ res, const T* __restrict__ gamma, T* __restrict__ y,
    T* __restrict__ z, float* __restrict__ rstd_out, int cols, float eps, float p, uint32_t threshold, uint64_t seed,
    uint64_t offset) {
  static_assert(kThreads == 256, "block_sum_once folds 4 waves");
  __shared__ float scratch[kThreads / 64];
  const int row = blockIdx.x;
  const size_t base = (size_t)row * cols;
  const int nvec = cols >> 3;
  const float scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float v[MAXV][8];
  float s2 = 0.f;
  Raw8<T> rr[POST ? MAXV : 1];
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int vi = threadIdx.x + k * kThreads;
    if (vi < nvec) {
      const size_t e = base + (size_t)vi * 8;
      Io<T>::load8(x + e, v[k]);
      if constexpr (POST) rr[k].load(res + e);
      if (!POST && p > 0.f) {
        const uint32_t keep = dropout_keep8(seed, offset, e, threshold);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[k][i] = ((keep >> i) & 1) ? v[k][i] * scale : 0.f;
      }
      if (!POST && res != nullptr) {
        float r[8];
        Io<T>::load8(res + e, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[k][i] += r[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s2 += v[k][i] * v[k][i];
    }
  }
  const float rstd = rsqrtf(block_sum_once(s2, scratch) / (float)cols + eps);
  if (threadIdx.x == 0 && (!POST || rstd_out != nullptr)) rstd_out[row] = rstd;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int vi = threadIdx.x + k * kThreads;
    if (vi < nvec) {
      const size_t e = base + (size_t)vi * 8;
      if (!POST && z != nullptr) Io<T>::store8(z + e, v[k]);
      float g[8], o[8];
      Io<T>::load8(gamma + vi * 8, g);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = v[k][i] * rstd * g[i];
      if constexpr (POST) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] += rr[k].get(i);
      }
      Io<T>::store8(y + e, o);
    }
  }
}

// Row reduction over one 256-thread row group of a G-group block (every thread
// of the block calls it: the barrier is block-wide).  Callers alternate two
// scratch buffers by row parity, so one barrier per row is enough: a buffer is
// written again two rows later, behind the next row's barrier, which a thread
// reaches only after reading this row's sum.
__device__ __forceinline__ float group_sum(float a, float (*scratch)[4], int grp, int t) {
  a = wave_sum(a);
  if ((t & 63) == 0) scratch[grp][t >> 6] = a;
  __syncthreads();
  return scratch[grp][0] + scratch[grp][1] + scratch[grp][2] + scratch[grp][3];
}

// G row groups of 256 threads per block, each on its own row, the block's rows
// strided over the grid; the groups' dgamma partials are folded through LDS so
// a block writes ONE partial row.
template <typename T, int MAXV, int G>
__global__ void __launch_bounds__(kThreads * G) rms_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ z, const float* __restrict__ rstd_in, const T* __restrict__ gamma,
    T* __restrict__ dz, T* __restrict__ dx, float* __restrict__ dgamma_part, int rows, int cols, float p,
    uint32_t threshold, uint64_t seed, uint64_t offset, const T* __restrict__ addend) {
  __shared__ float scratch[2][G][4];
  __shared__ float fold[G > 1 ? MAXV * 8 * kThreads : 1];
  const int grp = threadIdx.x / kThreads, t = threadIdx.x % kThreads;
  const int nvec = cols >> 3;
  const float scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const float inv_n = 1.f / (float)cols;

  float g[MAXV][8], dg[MAXV][8];
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int vi = t + k * kThreads;
#pragma unroll
    for (int i = 0; i < 8; ++i) dg[k][i] = g[k][i] = 0.f;
    if (vi < nvec) Io<T>::load8(gamma + vi * 8, g[k]);
  }

  const int stride = gridDim.x * G;
  const int iters = (rows + stride - 1) / stride;  // uniform over the block (barriers inside)
  auto row_of = [&](int it) { return it * stride + blockIdx.x * G + grp; };
  const bool has_add = addend != nullptr;
  struct RowBuf {
    Raw8<T> z[MAXV], d[MAXV], a[MAXV];
    float rstd;
  };
  auto load_row = [&](int row, RowBuf& r) {
    const bool valid = row < rows;
    r.rstd = valid ? rstd_in[row] : 0.f;
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int vi = t + k * kThreads;
      r.z[k].zero();
      r.d[k].zero();
      r.a[k].zero();
      if (vi < nvec && valid) {
        const size_t e = (size_t)row * cols + (size_t)vi * 8;
        r.z[k].load(z + e);
        r.d[k].load(dy + e);
        if (has_add) r.a[k].load(addend + e);
      }
    }
  };
  auto process = [&](int it, const RowBuf& r) {
    const int row = row_of(it);
    float xh[MAXV][8], gy[MAXV][8];
    float b = 0.f;  // sum(g*dy*xhat)
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float dv = r.d[k].get(i);
        xh[k][i] = r.z[k].get(i) * r.rstd;
        gy[k][i] = dv * g[k][i];
        dg[k][i] += dv * xh[k][i];
        b += gy[k][i] * xh[k][i];
      }
    }
    b = group_sum(b, scratch[it & 1], grp, t) * inv_n;
    if (row < rows) {
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {
        const int vi = t + k * kThreads;
        if (vi < nvec) {
          const size_t e = (size_t)row * cols + (size_t)vi * 8;
          float o[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] = r.rstd * (gy[k][i] - xh[k][i] * b) + r.a[k].get(i);
          Io<T>::store8(dz + e, o);
          if (dx != nullptr) {
            const uint32_t keep = dropout_keep8(seed, offset, e, threshold);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = ((keep >> i) & 1) ? o[i] * scale : 0.f;
            Io<T>::store8(dx + e, o);
          }
        }
      }
    }
  };
  if constexpr (MAXV <= 2) {
    // two rows in flight per group while one is reduced and stored (two named
    // buffers: a copy between buffers would wait for the loads in flight)
    RowBuf b0, b1;
    load_row(row_of(0), b0);
    load_row(row_of(1), b1);
    for (int it = 0; it < iters; it += 2) {
      process(it, b0);
      if (it + 2 < iters) load_row(row_of(it + 2), b0);
      if (it + 1 < iters) {
        process(it + 1, b1);
        if (it + 3 < iters) load_row(row_of(it + 3), b1);
      }
    }
  } else {  // wider rows: one row at a time
    RowBuf b0;
    for (int it = 0; it < iters; ++it) {
      load_row(row_of(it), b0);
      process(it, b0);
    }
  }
  if constexpr (G > 1) {
    // groups 1..G-1 hand their partials to group 0 through LDS, one at a time
#pragma unroll
    for (int src = 1; src < G; ++src) {
      if (grp == src) {
#pragma unroll
        for (int k = 0; k < MAXV; ++k)
#pragma unroll
          for (int i = 0; i < 8; ++i) fold[(k * 8 + i) * kThreads + t] = dg[k][i];
      }
      __syncthreads();
      if (grp == 0) {
#pragma unroll
        for (int k = 0; k < MAXV; ++k)
#pragma unroll
          for (int i = 0; i < 8; ++i) dg[k][i] += fold[(k * 8 + i) * kThreads + t];
      }
      __syncthreads();
    }
  }
  if (grp == 0) {
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int vi = t + k * kThreads;
      if (vi < nvec) Io<float>::store8(dgamma_part + (size_t)blockIdx.x * cols + vi * 8, dg[k]);
    }
  }
}

// ---- wave-per-row variants for rows up to 2048 wide ---------------------------
// One wave per row, kRowWaves rows per block, reductions by wave shuffles only
// (no LDS, no barriers in the row loop).  Lane l holds 16-byte vectors l,
// l + 64, l + 128, l + 192 of its row.
constexpr int kRowWaves = 8;
constexpr int kRowNV = 4;

template <typename T, bool POST>
__global__ void __launch_bounds__(64 * kRowWaves) rms_fwd_rows_kernel(
    const T* __restrict__ x, const T* __restrict__ res, const T* __restrict__ gamma, T* __restrict__ y,
    T* __restrict__ z, float* __restrict__ rstd_out, int rows, int cols, float eps, float p, uint32_t threshold,
    uint64_t seed, uint64_t offset) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (row >= rows) return;  // whole waves: no barriers below
  const size_t base = (size_t)row * cols;
  const int nvec = cols >> 3;
  const float scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  float v[kRowNV][8];
  float s2 = 0.f;
  Raw8<T> rr[POST ? kRowNV : 1];
#pragma unroll
  for (int k = 0; k < kRowNV; ++k) {
    const int vi = lane + 64 * k;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[k][i] = 0.f;
    if (vi < nvec) {
      const size_t e = base + (size_t)vi * 8;
      Io<T>::load8(x + e, v[k]);
      if constexpr (POST) rr[k].load(res + e);
      if (!POST && p > 0.f) {
        const uint32_t keep = dropout_keep8(seed, offset, e, threshold);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[k][i] = ((keep >> i) & 1) ? v[k][i] * scale : 0.f;
      }
      if (!POST && res != nullptr) {
        float r[8];
        Io<T>::load8(res + e, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[k][i] += r[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s2 += v[k][i] * v[k][i];
    }
  }
  const float rstd = rsqrtf(wave_sum(s2) / (float)cols + eps);
  if (lane == 0 && (!POST || rstd_out != nullptr)) rstd_out[row] = rstd;
#pragma unroll
  for (int k = 0; k < kRowNV; ++k) {
    const int vi = lane + 64 * k;
    if (vi < nvec) {
      const size_t e = base + (size_t)vi * 8;
      if (!POST && z != nullptr) Io<T>::store8(z + e, v[k]);
      float g[8], o[8];
      Io<T>::load8(gamma + vi * 8, g);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = v[k][i] * rstd * g[i];
      if constexpr (POST) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] += rr[k].get(i);
      }
      Io<T>::store8(y + e, o);
    }
  }
}

// Backward: gridDim.x = nparts blocks, waves stride over the rows; each lane
// keeps its columns' dgamma sums, folded over the block's waves through LDS in
// wave order (deterministic) into the block's partial row.
template <typename T>
__global__ void __launch_bounds__(64 * kRowWaves) rms_bwd_rows_kernel(
    const T* __restrict__ dy, const T* __restrict__ z, const float* __restrict__ rstd_in, const T* __restrict__ gamma,
    T* __restrict__ dz, T* __restrict__ dx, float* __restrict__ dgamma_part, int rows, int cols, float p,
    uint32_t threshold, uint64_t seed, uint64_t offset, const T* __restrict__ addend) {
  __shared__ float fold[kRowNV * 8 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = cols >> 3;
  const float scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const float inv_n = 1.f / (float)cols;
  float dg[kRowNV][8];
#pragma unroll
  for (int k = 0; k < kRowNV; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) dg[k][i] = 0.f;
  const int stride = gridDim.x * kRowWaves;
  for (int row = blockIdx.x * kRowWaves + wave; row < rows; row += stride) {
    const size_t base = (size_t)row * cols;
    const float rstd = rstd_in[row];
    float xh[kRowNV][8], gy[kRowNV][8];
    Raw8<T> ad[kRowNV];
    float b = 0.f;
#pragma unroll
    for (int k = 0; k < kRowNV; ++k) {
      const int vi = lane + 64 * k;
      float zz[8], d[8], g[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) zz[i] = d[i] = g[i] = 0.f;
      ad[k].zero();
      if (vi < nvec) {
        const size_t e = base + (size_t)vi * 8;
        Io<T>::load8(z + e, zz);
        Io<T>::load8(dy + e, d);
        Io<T>::load8(gamma + vi * 8, g);
        if (addend != nullptr) ad[k].load(addend + e);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        xh[k][i] = zz[i] * rstd;
        gy[k][i] = d[i] * g[i];
        dg[k][i] += d[i] * xh[k][i];
        b += gy[k][i] * xh[k][i];
      }
    }
    b = wave_sum(b) * inv_n;
#pragma unroll
    for (int k = 0; k < kRowNV; ++k) {
      const int vi = lane + 64 * k;
      if (vi < nvec) {
        const size_t e = base + (size_t)vi * 8;
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = rstd * (gy[k][i] - xh[k][i] * b) + ad[k].get(i);
        Io<T>::store8(dz + e, o);
        if (dx != nullptr) {
          const uint32_t keep = dropout_keep8(seed, offset, e, threshold);
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] = ((keep >> i) & 1) ? o[i] * scale : 0.f;
          Io<T>::store8(dx + e, o);
        }
      }
    }
  }
  // fold the waves' partials into wave 0, one wave at a time (fixed order)
  for (int src = 1; src < kRowWaves; ++src) {
    if (wave == src) {
#pragma unroll
      for (int k = 0; k < kRowNV; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) fold[(k * 8 + i) * 64 + lane] = dg[k][i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int k = 0; k < kRowNV; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) dg[k][i] += fold[(k * 8 + i) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < kRowNV; ++k) {
      const int vi = lane + 64 * k;
      if (vi < nvec) Io<float>::store8(dgamma_part + (size_t)blockIdx.x * cols + vi * 8, dg[k]);
    }
  }
}

bool rms_rows_variant(int cols) { return cols <= 64 * kRowNV * 8; }

template <typename T, int MAXV, bool POST>
void launch_fwd(const RmsArgs<T>& a, hipStream_t s) {
  hipLaunchKernelGGL((rms_fwd_kernel<T, MAXV, POST>), dim3(a.rows), dim3(kThreads), 0, s, a.x, a.res, a.gamma, a.y, a.z,
                     a.rstd, a.cols, a.eps, a.p, dropout_threshold(a.p), a.seed, a.offset);
}

template <typename T, int MAXV>
void launch_bwd(const RmsBwdArgs<T>& a, hipStream_t s) {
  // one partial row per block (a.nparts blocks, see rms_bwd_parts)
  constexpr int G = MAXV <= 2 ? 2 : 1;
  hipLaunchKernelGGL((rms_bwd_kernel<T, MAXV, G>), dim3(a.nparts), dim3(kThreads * G), 0, s, a.dy, a.z, a.rstd,
                     a.gamma, a.dz, a.dx, a.dgamma_part, a.rows, a.cols, a.p, dropout_threshold(a.p), a.seed,
                     a.offset, a.addend);
}

}  // namespace

int rms_max_vec(int cols) {
  const int per = kThreads * 8;
  if (cols <= 0 || cols % 8 != 0) return -1;
  if (cols <= 2 * per) return 2;  // rows up to 2048 wide take the wave-per-row kernels
  if (cols <= 4 * per) return 4;
  if (cols <= 8 * per) return 8;
  return -1;
}

int rms_bwd_parts(int rows, int cols) {
  // blocks of 2 x 256 threads for rows up to 4096 wide (2048 waves in flight
  // at 256 blocks), single-group blocks of 256 beyond
  const int cap = rms_max_vec(cols) <= 2 ? 256 : 512;
  return rows < cap ? (rows < 1 ? 1 : rows) : cap;
}

template <typename T, bool POST>
void rmsnorm_fwd_impl(const RmsArgs<T>& a, hipStream_t s) {
  if (a.rows <= 0) return;
  if (rms_rows_variant(a.cols)) {
    hipLaunchKernelGGL((rms_fwd_rows_kernel<T, POST>), dim3((a.rows + kRowWaves - 1) / kRowWaves), dim3(64 * kRowWaves), 0,
                       s, a.x, a.res, a.gamma, a.y, a.z, a.rstd, a.rows, a.cols, a.eps, a.p, dropout_threshold(a.p),
                       a.seed, a.offset);
    return;
  }
  switch (rms_max_vec(a.cols)) {
    case 2: launch_fwd<T, 2, POST>(a, s); break;
    case 4: launch_fwd<T, 4, POST>(a, s); break;
    case 8: launch_fwd<T, 8, POST>(a, s); break;
    default: break;
  }
}

template <typename T>
void rmsnorm_fwd(const RmsArgs<T>& a, hipStream_t s) {
  rmsnorm_fwd_impl<T, false>(a, s);
}

// y = res + x rstd gamma: a.res is required, a.rstd may be null, a.p and a.z are not used.
template <typename T>
void rmsnorm_residual_fwd(const RmsArgs<T>& a, hipStream_t s) {
  rmsnorm_fwd_impl<T, true>(a, s);
}

template <typename T>
void rmsnorm_bwd(const RmsBwdArgs<T>& a, hipStream_t s) {
  if (a.rows <= 0) return;
  if (rms_rows_variant(a.cols)) {
    hipLaunchKernelGGL((rms_bwd_rows_kernel<T>), dim3(a.nparts), dim3(64 * kRowWaves), 0, s, a.dy, a.z, a.rstd,
                       a.gamma, a.dz, a.dx, a.dgamma_part, a.rows, a.cols, a.p, dropout_threshold(a.p), a.seed,
                       a.offset, a.addend);
  } else {
    switch (rms_max_vec(a.cols)) {
      case 2: launch_bwd<T, 2>(a, s); break;
      case 4: launch_bwd<T, 4>(a, s); break;
      case 8: launch_bwd<T, 8>(a, s); break;
      default: return;
    }
  }
  reduce_parts(a.dgamma_part, nullptr, a.nparts, a.cols, a.dgamma, nullptr, a.out_f32, a.accumulate, s);
}

template void rmsnorm_fwd<float>(const RmsArgs<float>&, hipStream_t);
template void rmsnorm_fwd<bf16_t>(const RmsArgs<bf16_t>&, hipStream_t);
template void rmsnorm_residual_fwd<float>(const RmsArgs<float>&, hipStream_t);
template void rmsnorm_residual_fwd<bf16_t>(const RmsArgs<bf16_t>&, hipStream_t);
template void rmsnorm_bwd<float>(const RmsBwdArgs<float>&, hipStream_t);
template void rmsnorm_bwd<bf16_t>(const RmsBwdArgs<bf16_t>&, hipStream_t);

}  // namespace mipipe
