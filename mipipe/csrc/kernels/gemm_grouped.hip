// Grouped bf16 MFMA GEMMs for the dropless mixture-of-experts path (gfx950).
//
// The rows of all experts live in one [R, *] buffer, sorted by expert, every
// expert's segment padded to whole 128-row tiles (ops/moe.py moe_assign_sorted).
// Which expert a tile belongs to, and where an expert's rows start, is read
// from device memory, so one launch serves every expert and no shape depends
// on the routing:
//
//   forward  Y [R, N]   = X  . W_e^T      e = tile_expert[row tile]; W_e [N, K] K-contiguous
//   dgrad    dX[R, K]   = dY . W_e        W_e read as [N, K] N-strided (transposing LDS read)
//   wgrad    dW_e[N, K] (+)= dY_e^T X_e   rows [offsets[e], offsets[e + 1]); fp32 output
//
// The weights (and the wgrad outputs) of the experts are separate allocations:
// the kernels take a device table of Ne pointers.  A tile whose expert is -1
// (the tiles past offsets[Ne]) stores zeros.  An expert without rows stores
// zeros (store mode) or leaves its output alone (accumulate mode).
//
// Structure: gemm.hip's 128x128x64 register-staged kernel -- 4 waves (2 x 2,
// 64x64 per wave as 4x4 v_mfma_f32_16x16x32_bf16 tiles), two 32 KiB LDS
// buffers, the next K-tile's global loads in flight under the MFMAs -- with
// the same swizzled LDS images and fragment readers (kept as copies here:
// gemm.hip stays as it is).  Results leave through LDS as 16-byte row stores.
#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kTileBytes = BM * BK * 2;    // 16 KiB per operand tile (BM == BN)
constexpr int kBufBytes = 2 * kTileBytes;  // A + B
constexpr int kSmemBytes = 2 * kBufBytes;  // double buffered = 64 KiB (the limit without an attribute); reused by the epilogues

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// ---- LDS images (as in gemm.hip) ---------------------------------------------
// K-contiguous tile [128 rows (i)][64 k]: 128-byte rows, 16-byte chunk c of
// row r stored at chunk c ^ ((r >> 1) & 7).
__device__ __forceinline__ int kc_off(int r, int c16) { return r * 128 + ((c16 ^ ((r >> 1) & 7)) << 4); }

// I-contiguous tile [64 rows (k)][128 i]: 256-byte rows, 8-byte chunk c of row
// r stored at chunk c ^ (4 * rk(r)), rk(r) = (r & 3) | (((r >> 3) & 1) << 2).
__device__ __forceinline__ int ic_rk(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }
__device__ __forceinline__ int ic_off(int r, int c8) { return r * 256 + ((c8 ^ (ic_rk(r) << 2)) << 3); }

template <bool KC>
struct Stager {
  u32x4 v[4];
  // Loads the tile whose first element is (i0, k0) of an operand of leading dimension ld.
  __device__ __forceinline__ void load(const bf16_t* __restrict__ base, int64_t ld, int i0, int k0, int tid) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int id = tid + u * kThreads;
      const bf16_t* p;
      if (KC) {
        const int r = id >> 3, c = id & 7;
        p = base + (int64_t)(i0 + r) * ld + k0 + c * 8;
      } else {
        const int r = id >> 4, c = id & 15;
        p = base + (int64_t)(k0 + r) * ld + i0 + c * 8;
      }
      v[u] = *reinterpret_cast<const u32x4*>(p);
    }
  }
  __device__ __forceinline__ void store(char* tile, int tid) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int id = tid + u * kThreads;
      int off;
      if (KC) {
        off = kc_off(id >> 3, id & 7);
      } else {
        off = ic_off(id >> 4, (id & 15) * 2);
      }
      *reinterpret_cast<u32x4*>(tile + off) = v[u];
    }
  }
};

// Fragment of the 16x16x32 operand for rows/cols [ib, ib+16) and k-step s:
// lane l holds element (i = ib + (l & 15), k = 32 s + 8 (l >> 4) + j), j = 0..7.
template <bool KC>
__device__ __forceinline__ bf16x8 read_frag(const char* tile, int ib, int s, int lane) {
  if (KC) {
    const int r = ib + (lane & 15);
    const int c = 4 * s + (lane >> 4);
    return *reinterpret_cast<const bf16x8*>(tile + kc_off(r, c));
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const int r0 = 32 * s + 8 * g + q;
    const int c8 = (ib >> 2) + p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + ic_off(r0, c8)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + ic_off(r0 + 4, c8)));
    const s16x8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, both);
  }
}

// Bijective XCD-aware remap + grouped ordering: the blocks of 8 neighbouring row tiles (mostly one expert's) and one
// column tile run next to each other on one XCD, so they share the expert's weight panel in its L2.
__device__ __forceinline__ void tile_coords(int tiles_m, int tiles_n, int& tm, int& tn, int G = 8) {
  const int nwg = tiles_m * tiles_n;
  const int bid = blockIdx.x;
  int wg = bid;
  if (nwg > 8) {
    const int xcd = bid & 7, local = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
  }
  const int group = wg / (G * tiles_n);
  const int first_m = group * G;
  const int gsize = min(tiles_m - first_m, G);
  const int in_group = wg % (G * tiles_n);
  tm = first_m + in_group % gsize;
  tn = in_group / gsize;
}

// acc += A-tile . B-tile over nk K-tiles; A's tile starts at (am0, ak0), B's at (bn0, bk0).  nk >= 1.  Ends on a
// barrier: LDS is free for the epilogue.
template <bool A_KC, bool B_KC>
__device__ __forceinline__ void main_loop(char* smem, const bf16_t* __restrict__ A, int64_t lda, int am0, int ak0,
                                          const bf16_t* __restrict__ B, int64_t ldb, int bn0, int bk0, int nk,
                                          f32x4 (&acc)[4][4], int tid, int lane, int wm, int wn) {
  Stager<A_KC> sa;
  Stager<B_KC> sb;
  sa.load(A, lda, am0, ak0, tid);
  sb.load(B, ldb, bn0, bk0, tid);
  sa.store(smem, tid);
  sb.store(smem + kTileBytes, tid);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * kBufBytes;
    const bool more = kt + 1 < nk;
    if (more) {
      sa.load(A, lda, am0, ak0 + (kt + 1) * BK, tid);
      sb.load(B, ldb, bn0, bk0 + (kt + 1) * BK, tid);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) af[t] = read_frag<A_KC>(cur, wm * 64 + 16 * t, s, lane);
#pragma unroll
      for (int t = 0; t < 4; ++t) bfr[t] = read_frag<B_KC>(cur + kTileBytes, wn * 64 + 16 * t, s, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      char* nxt = smem + ((kt + 1) & 1) * kBufBytes;
      sa.store(nxt, tid);
      sb.store(nxt + kTileBytes, tid);
    }
    __syncthreads();
  }
}

// ---- epilogues ------------------------------------------------------------------
// The accumulator layout: acc[i][j][r] is element (row = wm * 64 + 16 i + 4 (lane >> 4) + r,
// col = wn * 64 + 16 j + (lane & 15)) of the 128x128 tile.

constexpr int kStageLdBf = BN + 8;  // bf16 staging rows of 272 bytes: 16-byte aligned, 4 banks apart
constexpr int kStageLdF = BN + 4;   // fp32 staging rows of 528 bytes

// The tile as bf16, rounded once, out through LDS in 16-byte row stores.
__device__ __forceinline__ void store_bf16(char* smem, const f32x4 (&acc)[4][4], bf16_t* __restrict__ C, int64_t ldc,
                                           int m0, int n0, int tid, int lane, int wm, int wn) {
  bf16_t* stg = reinterpret_cast<bf16_t*>(smem);
  const int quad = lane >> 4, col_in = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        stg[(wm * 64 + 16 * i + 4 * quad + r) * kStageLdBf + wn * 64 + 16 * j + col_in] = f2bf(acc[i][j][r]);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int id = tid + u * kThreads;
    const int row = id >> 4, c = id & 15;
    const u32x4 v = *reinterpret_cast<const u32x4*>(stg + row * kStageLdBf + c * 8);
    *reinterpret_cast<u32x4*>(C + (int64_t)(m0 + row) * ldc + n0 + c * 8) = v;
  }
}

__device__ __forceinline__ void store_zero_bf16(bf16_t* __restrict__ C, int64_t ldc, int m0, int n0, int tid) {
  const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int id = tid + u * kThreads;
    const int row = id >> 4, c = id & 15;
    *reinterpret_cast<u32x4*>(C + (int64_t)(m0 + row) * ldc + n0 + c * 8) = z;
  }
}

// The tile as fp32, stored or added to C, in two passes of 64 rows (the rows of the waves with wm == pass).
template <bool ACCUM>
__device__ __forceinline__ void store_f32(char* smem, const f32x4 (&acc)[4][4], float* __restrict__ C, int64_t ldc,
                                          int m0, int n0, int tid, int lane, int wm, int wn) {
  float* stg = reinterpret_cast<float*>(smem);
  const int quad = lane >> 4, col_in = lane & 15;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (wm == pass) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            stg[(16 * i + 4 * quad + r) * kStageLdF + wn * 64 + 16 * j + col_in] = acc[i][j][r];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int id = tid + u * kThreads;
      const int row = id >> 5, c = id & 31;
      f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * kStageLdF + c * 4);
      float* p = C + (int64_t)(m0 + pass * 64 + row) * ldc + n0 + c * 4;
      if (ACCUM) v += *reinterpret_cast<const f32x4*>(p);
      *reinterpret_cast<f32x4*>(p) = v;
    }
    __syncthreads();
  }
}

// ---- kernels -----------------------------------------------------------------------
// Forward (B_KC) and dgrad (!B_KC): C[R, Nout] = A[R, Kred] . op(W_e), one block per (row tile, column tile).
//   B_KC:  W_e is [Nout, Kred], K-contiguous (ldw = Kred)
//   !B_KC: W_e is [Kred, Nout], read through the transposing LDS read (ldw = Nout)
template <bool B_KC>
__global__ void __launch_bounds__(kThreads) grouped_rows_kernel(const bf16_t* __restrict__ A,
                                                                const int64_t* __restrict__ wptr,
                                                                const int32_t* __restrict__ tile_expert,
                                                                bf16_t* __restrict__ C, int R, int Nout, int Kred,
                                                                int Ne) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  int tm, tn;
  tile_coords(R / BM, Nout / BN, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int e = tile_expert[tm];  // uniform over the block
  if (e < 0 || e >= Ne) {
    store_zero_bf16(C, Nout, m0, n0, tid);
    return;
  }
  const bf16_t* W = reinterpret_cast<const bf16_t*>(wptr[e]);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  main_loop<true, B_KC>(smem, A, Kred, m0, 0, W, B_KC ? Kred : Nout, n0, 0, Kred / BK, acc, tid, lane, wm, wn);
  store_bf16(smem, acc, C, Nout, m0, n0, tid, lane, wm, wn);
}

// Wgrad: dW_e[N, K] (+)= dY[rows_e, N]^T . X[rows_e, K], rows_e = [offsets[e], offsets[e + 1]).  Grid
// (N / 128 * K / 128, Ne).  The output of expert e is optr[e], or obase + e * N * K without a table.
template <bool ACCUM>
__global__ void __launch_bounds__(kThreads) grouped_wgrad_kernel(const bf16_t* __restrict__ dY,
                                                                 const bf16_t* __restrict__ X,
                                                                 const int32_t* __restrict__ offsets,
                                                                 const int64_t* __restrict__ optr,
                                                                 float* __restrict__ obase, int R, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  const int e = blockIdx.y;
  const int tiles_n = K / BN;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const int lo = max(offsets[e], 0), hi = min(offsets[e + 1], R);
  const int nk = hi > lo ? (hi - lo) / BK : 0;  // whole tiles of 128 rows: no tail
  if (ACCUM && nk == 0) return;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nk > 0) main_loop<false, false>(smem, dY, N, m0, lo, X, K, n0, lo, nk, acc, tid, lane, wm, wn);

  float* C = optr != nullptr ? reinterpret_cast<float*>(optr[e]) : obase + (int64_t)e * N * K;
  store_f32<ACCUM>(smem, acc, C, K, m0, n0, tid, lane, wm, wn);
}

}  // namespace

bool grouped_gemm_supported(int64_t R, int64_t Nout, int64_t Kred) {
  return R > 0 && R % BM == 0 && Nout > 0 && Nout % BN == 0 && Kred > 0 && Kred % BK == 0 && R < (1ll << 31) &&
         Nout < (1ll << 31) && Kred < (1ll << 31) && (R / BM) * (Nout / BN) < (1ll << 31);
}

void grouped_gemm_rows(const bf16_t* A, const int64_t* wptr, const int32_t* tile_expert, bf16_t* C, int64_t R,
                       int64_t Nout, int64_t Kred, int Ne, bool w_kc, hipStream_t s) {
  const dim3 grid((unsigned)((R / BM) * (Nout / BN))), block(kThreads);
  if (w_kc) {
    hipLaunchKernelGGL(grouped_rows_kernel<true>, grid, block, kSmemBytes, s, A, wptr, tile_expert, C, (int)R,
                       (int)Nout, (int)Kred, Ne);
  } else {
    hipLaunchKernelGGL(grouped_rows_kernel<false>, grid, block, kSmemBytes, s, A, wptr, tile_expert, C, (int)R,
                       (int)Nout, (int)Kred, Ne);
  }
}

void grouped_gemm_wgrad(const bf16_t* dY, const bf16_t* X, const int32_t* offsets, const int64_t* optr, float* obase,
                        int64_t R, int64_t N, int64_t K, int Ne, bool accumulate, hipStream_t s) {
  const dim3 grid((unsigned)((N / BM) * (K / BN)), (unsigned)Ne), block(kThreads);
  if (accumulate) {
    hipLaunchKernelGGL(grouped_wgrad_kernel<true>, grid, block, kSmemBytes, s, dY, X, offsets, optr, obase, (int)R,
                       (int)N, (int)K);
  } else {
    hipLaunchKernelGGL(grouped_wgrad_kernel<false>, grid, block, kSmemBytes, s, dY, X, offsets, optr, obase, (int)R,
                       (int)N, (int)K);
  }
}

}  // namespace mipipe
