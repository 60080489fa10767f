// bf16 MFMA GEMM for gfx950 with fused epilogues.
//
//   C[M, N] = A[M, K] . B[K, N]      (bf16 operands, fp32 accumulation)
//
// Every Transformer linear runs on this one kernel template, in three
// operand layouts:
//   forward  Y  = X  . W^T   A = X  [T, K] (K-contiguous)  B = W  [N, K] (K-contiguous)
//   dgrad    dX = dY . W     A = dY [T, N] (K-contiguous)  B = W  [N, K] read as [K, N] (N-contiguous)
//   wgrad    dW += dY^T . X  A = dY read as [K=T, M] (M-contiguous), B = X [K=T, N] (N-contiguous)
// Operand tiles are staged into LDS in their memory layout (16-byte loads,
// coalesced); K-contiguous fragments are read with ds_read_b128 and K-strided
// ones with the gfx950 transposing read ds_read_b64_tr_b16, so no layout ever
// needs a transpose pass in HBM.  Both LDS images are XOR-swizzled so the
// lane groups of a read hit distinct banks (T2/T10).
//
// Main kernel (big::gemm256_kernel): 256x256x64 block tile, 8 waves (2 M x 4 N,
// 128x64 per wave as 8x4 v_mfma_f32_16x16x32_bf16 tiles), operand tiles staged
// by LDS-DMA (global_load_lds_dwordx4, SADDR form with loop-invariant per-lane
// offsets) into two 64 KiB buffers, and either a ping-pong main loop (the two
// wave groups one barrier interval apart: one group's 16-MFMA cluster runs
// while the other reads its fragments) or one barrier per K-tile.  Edge tiles
// (M, N any multiple of 8) are clamped on load and masked on store; K may be
// split into segments living in different buffers (deferred weight gradients).
// Block ids are remapped so consecutive tiles of an 8-row group share an XCD's
// L2 (T1, bijective form).  Grids that would leave CUs idle get a 256x128 block
// or, with a long K, split-K: 2-8 blocks per tile writing fp32 partials that
// one reduction adds.  A 128x128 register-staged kernel serves small
// exact-multiple grids.  Which of these a call gets is one table: gemm_plan.
// Epilogues (all results leave through LDS as 16-byte row stores, staged_store):
//   kEpiStoreBf16 -- + bias, activation (ReLU/GELU), dropout (Philox mask in
//                    the "column-quad" layout shared with the elementwise
//                    backward), optional pre-activation aux output, optional
//                    bf16 addend `res` (a fan-out's other gradient: the
//                    autograd add kernel folded into the dgrad), bf16 store;
//   kEpiAccumF32  -- C(fp32) += acc  (weight gradients straight into main_grad);
//   kEpiStoreF32  -- fp32 store (first write of a step, split-K partials).
#include <algorithm>
#include <stdexcept>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kTileBytes = BM * BK * 2;  // 16 KiB per operand tile (BM == BN)
constexpr int kBufBytes = 2 * kTileBytes;  // A + B
constexpr int kSmemBytes = 2 * kBufBytes;  // double buffered = 64 KiB

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// ---- LDS images --------------------------------------------------------------
// K-contiguous tile [128 rows (i)][64 k]: 128-byte rows, 16-byte chunk c of
// row r stored at chunk c ^ ((r >> 1) & 7).
__device__ __forceinline__ int kc_off(int r, int c16) { return r * 128 + ((c16 ^ ((r >> 1) & 7)) << 4); }

// I-contiguous tile [64 rows (k)][128 i]: 256-byte rows, 8-byte chunk c of row
// r stored at chunk c ^ (4 * rk(r)), rk(r) = (r & 3) | (((r >> 3) & 1) << 2).
__device__ __forceinline__ int ic_rk(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }
__device__ __forceinline__ int ic_off(int r, int c8) { return r * 256 + ((c8 ^ (ic_rk(r) << 2)) << 3); }

// ---- global -> registers -> LDS staging ------------------------------------------
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

template <bool KC>
struct Stager {
  u32x4 v[4];  // native vector: HIP's uint4 struct copies become memcpys that pin the array in scratch
  // Loads the tile whose first element is (i0, k0) of an operand of leading
  // dimension ld.
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

// ---- LDS -> fragment ---------------------------------------------------------------
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

// act'(s) for the activation-backward epilogue (GemmArgs::dact): ReLU's from its
// output, GELU's from the pre-activation, or s itself (kActSavedGrad: the forward
// stored GELU'(pre) -- one multiply, like ReLU's sign test).
__device__ __forceinline__ float dact_f(int dact, float s) {
  return dact == kActRelu ? (s > 0.f ? 1.f : 0.f) : (dact == kActSavedGrad ? s : gelu_grad_f(s));
}

// Bijective XCD-aware remap + grouped (8 tile-rows) ordering.
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

template <bool A_KC, bool B_KC, int EPI, int ACT>
__global__ void __launch_bounds__(kThreads) gemm_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  int tm, tn;
  tile_coords(g.M / BM, g.N / BN, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const bf16_t* A = reinterpret_cast<const bf16_t*>(g.A);
  const bf16_t* B = reinterpret_cast<const bf16_t*>(g.B);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Stager<A_KC> sa;
  Stager<B_KC> sb;
  const int nk = g.K / BK;

  sa.load(A, g.lda, m0, 0, tid);
  sb.load(B, g.ldb, n0, 0, tid);
  sa.store(smem, tid);
  sb.store(smem + kTileBytes, tid);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * kBufBytes;
    const bool more = kt + 1 < nk;
    if (more) {
      sa.load(A, g.lda, m0, (kt + 1) * BK, tid);
      sb.load(B, g.ldb, n0, (kt + 1) * BK, tid);
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

  // ---- epilogue ----
  const int quad = lane >> 4, col_in = lane & 15;
  const float pscale = g.p > 0.f ? 1.f / (1.f - g.p) : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row0 = m0 + wm * 64 + 16 * i + 4 * quad;  // rows row0 .. row0+3
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + wn * 64 + 16 * j + col_in;
      f32x4 v = acc[i][j];
      if (EPI == kEpiAccumF32) {
        float* C = reinterpret_cast<float*>(g.C);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* p = C + (int64_t)(row0 + r) * g.ldc + col;
          *p += v[r];
        }
      } else if (EPI == kEpiStoreF32) {
        float* C = reinterpret_cast<float*>(g.C);
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(int64_t)(row0 + r) * g.ldc + col] = v[r];
      } else {
        bf16_t* C = reinterpret_cast<bf16_t*>(g.C);
        const float b = g.bias != nullptr ? bf2f(reinterpret_cast<const bf16_t*>(g.bias)[col]) : 0.f;
        float pre[4], out[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pre[r] = v[r] + b;
          out[r] = ACT == kActRelu ? fmaxf(pre[r], 0.f) : (ACT == kActGelu ? gelu_f(pre[r]) : pre[r]);
        }
        if (g.p > 0.f) {
          // the dropout layout (common.h drop_sub): word row & 3, half col & 1
          const uint4 w = Philox(g.seed, drop_sub(row0, col, g.N), g.offset).next4();
          const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) out[r] = drop_keep(ws[r], col & 1, g.threshold >> 16) ? out[r] * pscale : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (g.dact_in != nullptr && g.dact == kActReluBits)
            out[r] *= (reinterpret_cast<const uint8_t*>(g.dact_in)[(int64_t)(row0 + r) * g.ldd + (col >> 3)] >> (col & 7)) & 1
                          ? g.dact_scale : 0.f;
          else if (g.dact_in != nullptr)
            out[r] *= g.dact_scale *
                      dact_f(g.dact, bf2f(reinterpret_cast<const bf16_t*>(g.dact_in)[(int64_t)(row0 + r) * g.ldd + col]));
          if (g.res != nullptr) out[r] += bf2f(reinterpret_cast<const bf16_t*>(g.res)[(int64_t)(row0 + r) * g.ldr + col]);
          C[(int64_t)(row0 + r) * g.ldc + col] = f2bf(out[r]);
          if (g.aux != nullptr)
            reinterpret_cast<bf16_t*>(g.aux)[(int64_t)(row0 + r) * g.ldc + col] =
                f2bf(g.aux_grad ? gelu_grad_f(pre[r]) : pre[r]);
        }
      }
    }
  }
}

// ============================================================================
// Large-tile variant: 256x256x64, 8 waves (2 M x 4 N, 128x64 per wave as 8x4
// MFMA tiles), operand tiles staged by LDS-DMA (global_load_lds_dwordx4: no
// VGPR round trip, no ds_write), two 64 KiB LDS buffers, one barrier per K-tile.
// LDS images are lane-linear per wave-instruction (1 KiB), so the bank swizzle
// is applied to the per-lane *source* address and undone on the read (rule 21).
namespace big {

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int kThreads = 512;
constexpr int kTileBytes = BM * BK * 2;      // 32 KiB per operand tile
constexpr int kSmemBytes = 128 * 260 * 4;    // 130 KiB: 2 x 64 KiB operand buffers, reused by the epilogue

// The main loop keeps an I-contiguous B operand in THREE buffers (A in two;
// see the loop): 2 (A + B) + B = 160 KiB at W = 256, all of the CU's LDS.
template <bool B_KC, int W>
constexpr int smem_bytes() {
  constexpr int b3 = 2 * (kTileBytes + W * BK * 2) + W * BK * 2;
  return !B_KC && b3 > kSmemBytes ? b3 : kSmemBytes;
}

// I-contiguous image with 2W-byte rows (W = 256 or 128 i values; the B tile of
// the 256x128 variant is 128 wide).
template <int W>
__device__ __forceinline__ int ic_off_w(int r, int c8) { return r * (2 * W) + ((c8 ^ (ic_rk(r) << 2)) << 3); }

// LDS-DMA staging (global_load_lds_dwordx4: 16 bytes per lane, lane-linear
// 1 KiB per wave-instruction; the bank swizzle is applied to the per-lane
// SOURCE address).
//
// Loop-invariant per-lane byte offsets of the W/64 pieces a wave stages per
// W-wide operand tile; the K position lives in the scalar base, so each LDS-DMA is
// issued in SADDR form (SGPR base + 32-bit VGPR offset) with no per-tile
// address arithmetic.  gemm_supported() keeps rows * ld * 2 bytes < 4 GiB.
// Edge tiles: i indices past `lim` (M for A, N for B) are clamped onto the last
// valid row / 8-column chunk, so every DMA reads mapped memory; the garbage
// they produce lands only in accumulator rows/columns the epilogue masks off.
template <bool KC, int W>
__device__ __forceinline__ void stage_offsets(int64_t ld, int i0, int lim, int wave, int lane, uint32_t (&off)[W / 64]) {
  constexpr int NU = W / 64, LPR = W / 8;  // DMAs per wave; 16-byte chunks per I-contiguous row
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int inst = wave * NU + u;
    if (KC) {
      const int row = 8 * inst + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      const int gi = min(i0 + row, lim - 1);
      off[u] = (uint32_t)(((int64_t)gi * ld + 8 * c) * 2);
    } else {
      const int row = (64 / LPR) * inst + lane / LPR;
      const int c16 = (lane % LPR) ^ (ic_rk(row) << 1);
      const int gi = min(i0 + 8 * c16, lim - 8);
      off[u] = (uint32_t)(((int64_t)row * ld + gi) * 2);
    }
  }
}

// The I-contiguous A tile of the main loop is kept as two 128-wide halves
// (i 0-127, then 128-255; 16 KiB each, the W = 128 image), so each half is read
// by one wave group only.  Share s (0-7) stages rows 16 (s & 3) .. +16 of half
// s >> 2 -- the same LDS pieces stage_fast gives share s (4 KiB at 4 s KiB).
__device__ __forceinline__ void stage_offsets_halves(int64_t ld, int i0, int lim, int share, int lane,
                                                     uint32_t (&off)[4]) {
  const int half = share >> 2;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 4 * (4 * (share & 3) + u) + (lane >> 4);
    const int c16 = (lane & 15) ^ (ic_rk(row) << 1);
    const int gi = min(i0 + 128 * half + 8 * c16, lim - 8);
    off[u] = (uint32_t)(((int64_t)row * ld + gi) * 2);
  }
}

// Issued from inline asm on purpose: the compiler cannot prove that a DMA into
// one LDS buffer does not alias the ds_reads of the other, and after a
// __builtin_amdgcn_global_load_lds it inserts s_waitcnt vmcnt(0) before EVERY
// following ds_read -- each phase would wait for the next tile's DMA to land.
// Hidden from the waitcnt pass, the DMA is ordered only by the kernel's own
// counted waits (vmcnt before the barrier that precedes the read).
__device__ __forceinline__ void glds16_saddr(const char* base, uint32_t off, const char* lds_dst) {
  const uint32_t m0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)lds_dst);
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2"
      :
      : "s"(m0), "v"(off), "s"(base)
      : "memory", "m0");
}

// s_waitcnt vmcnt(N): all but the N most recently issued vector-memory ops done.
template <int N>
__device__ __forceinline__ void vmcnt_keep() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_waitcnt lgkmcnt(0) as the builtin's immediate (gfx9 encoding: vmcnt 63 in
// bits 15:14 and 3:0, expcnt 7 in 6:4 = no wait; lgkmcnt in 11:8 = 0).
constexpr int kWaitLgkm0 = 0xC07F;

// `base`: the operand's byte address at the tile's first K-row / K-column (a
// scalar the caller keeps and advances; no per-tile multiply here).
template <int W>
__device__ __forceinline__ void stage_fast(const char* base, const uint32_t (&off)[W / 64], char* tile, int wave) {
  constexpr int NU = W / 64;
#pragma unroll
  for (int u = 0; u < NU; ++u) glds16_saddr(base, off[u], tile + (wave * NU + u) * 1024);
}

// K position of the tile a wave group stages next, as running scalars: the
// A / B byte addresses of the tile (`a`, `b`), and for K-segmented operands
// (GemmArgs::seg_k) the segment, the local k in it and the NEXT segment's
// pointers.  init() is the only place that divides (a split-K block may start
// mid-segment); next() adds the loop-invariant byte steps and, where the local
// k reaches seg_k, switches to the pointers loaded when the segment before
// was entered -- so the straight path of the K loop has no scalar load and
// no wait for one, and the loop reads nothing else from the kernel arguments
// (the crossing block itself, taken once per seg_k / BK tiles, still waits
// for the two loads it issues: the compiler loads into spare registers).
// (seg_base(), which this replaces, re-read GemmArgs::A / a_seg[s] after every
// LDS-DMA -- the DMA asm clobbers memory -- and its s_waitcnt lgkmcnt(0)
// drained the fragment reads twice per K-tile, with a division each.)
struct KCursor {
  const char *a, *b;    // tile bases
  const char *na, *nb;  // segment seg + 1 (clamped to the array)
  int64_t step_a, step_b;
  int seg_k, kl, seg;

  __device__ __forceinline__ void load_next(const GemmArgs& g) {
    const int nx = min(seg + 1, GemmArgs::kMaxSegs - 1);
    na = reinterpret_cast<const char*>(g.a_seg[nx]);
    nb = reinterpret_cast<const char*>(g.b_seg[nx]);
  }
  template <bool A_KC, bool B_KC>
  __device__ __forceinline__ void init(const GemmArgs& g, int kt) {
    const int64_t lda = g.lda, ldb = g.ldb;
    step_a = A_KC ? BK * 2 : BK * lda * 2;
    step_b = B_KC ? BK * 2 : BK * ldb * 2;
    seg_k = g.seg_k;
    kl = kt * BK;
    seg = 0;
    a = na = reinterpret_cast<const char*>(g.A);
    b = nb = reinterpret_cast<const char*>(g.B);
    if (seg_k > 0) {
      seg = kl / seg_k;
      kl -= seg * seg_k;
      a = reinterpret_cast<const char*>(g.a_seg[seg]);
      b = reinterpret_cast<const char*>(g.b_seg[seg]);
      load_next(g);
    }
    a += A_KC ? (int64_t)kl * 2 : (int64_t)kl * lda * 2;
    b += B_KC ? (int64_t)kl * 2 : (int64_t)kl * ldb * 2;
  }
  __device__ __forceinline__ void next(const GemmArgs& g) {
    a += step_a;
    b += step_b;
    kl += BK;
    if (__builtin_expect(kl == seg_k, 0)) {  // never with seg_k == 0
      kl = 0;
      ++seg;
      a = na;
      b = nb;
      load_next(g);
    }
  }
};

template <bool KC, int W>
__device__ __forceinline__ bf16x8 frag(const char* tile, int ib, int s, int lane) {
  if (KC) {
    const int r = ib + (lane & 15);
    const int c = 4 * s + (lane >> 4);
    return *reinterpret_cast<const bf16x8*>(tile + kc_off(r, c));
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const int r0 = 32 * s + 8 * g + q;
    const int c8 = (ib >> 2) + p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + ic_off_w<W>(r0, c8)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + ic_off_w<W>(r0 + 4, c8)));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  }
}

// frag<false, W> with the address split into what a lane keeps in a register
// and what goes into the reads' immediate offset: ic_frag_off is the byte
// offset of the s = 0 `lo` read in the tile; k-step s lies 32 rows and the `hi`
// read 4 rows further down, and neither changes ic_rk (bits 0, 1 and 3 of the
// row), so both are constants for every lane.  ic_frag_at reads the fragment
// at LDS byte address `addr` (tile base + ic_frag_off) + `imm`.
template <int W>
__device__ __forceinline__ uint32_t ic_frag_off(int ib, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  return (uint32_t)ic_off_w<W>(8 * g + q, (ib >> 2) + p);
}

template <int W>
__device__ __forceinline__ bf16x8 ic_frag_at(uint32_t addr, int imm, int s) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(addr + (uint32_t)(imm + s * 32 * 2 * W)));
  const s16x4 hi =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(addr + (uint32_t)(imm + s * 32 * 2 * W + 4 * 2 * W)));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// Epilogue parameters as plain values, read from the kernel arguments once
// (through a GemmArgs reference the fields were re-loaded -- an s_load plus
// its wait -- after every store that might alias them).
struct EpiParams {
  uint64_t seed, offset;
  int N;
  float p, pscale;
  uint32_t threshold;
  int mask_row0, mask_col0, mask_ld;  // launch chunk -> full-matrix mask coordinates
};

// Register-phase bf16 epilogue of accumulator row block i (16 rows x 16 NJ
// cols of the wave's tile): bias, activation, dropout, in place.  One instantiation per i: as a loop, the Philox-heavy body is not
// unrolled and a runtime i demotes the whole accumulator array to scratch.
// Predicated throughout (no continue/break, for the same reason).
// EXTRA = false: bias + activation only (no dropout) -- straight-line code;
// with the dropout and aux-store branches merely present, the compiler's
// per-element control flow cost ~5 us per 256x256 tile round (K = 64 sweep).
template <int I, int ACT, int NJ, bool EXTRA>
__device__ __forceinline__ void epi_rows(const EpiParams ep, f32x4 (&acc)[8][NJ], int nrow, int ncol,
                                         const float (&bias)[NJ]) {
  if constexpr (!EXTRA) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pre = acc[I][j][r] + bias[j];
        acc[I][j][r] = ACT == kActRelu ? fmaxf(pre, 0.f) : (ACT == kActGelu ? gelu_f(pre) : pre);
      }
    return;
  }
  const int row0 = nrow + 16 * I;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = ncol + 16 * j;
    const float b = bias[j];
    uint32_t ws[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (ep.p > 0.f) {
      const uint4 w = Philox(ep.seed, drop_sub(row0 + ep.mask_row0, col + ep.mask_col0, ep.mask_ld), ep.offset).next4();
      ws[0] = w.x; ws[1] = w.y; ws[2] = w.z; ws[3] = w.w;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pre = acc[I][j][r] + b;
      float out = ACT == kActRelu ? fmaxf(pre, 0.f) : (ACT == kActGelu ? gelu_f(pre) : pre);
      if (ep.p > 0.f) out = drop_keep(ws[r], (col + ep.mask_col0) & 1, ep.threshold >> 16) ? out * ep.pscale : 0.f;
      acc[I][j][r] = out;
    }
  }
}

// Side operand of the bf16 store pass, a compile-time mode of the kernel (the
// launcher picks it from the GemmArgs fields), so a kernel carries the code of
// its own mode only:
//   kSideNone  -- nothing is read;
//   kSideRes   -- + res (the bf16 addend);
//   kSideBits  -- x the ReLU (+ dropout) bit mask (dact_in, kActReluBits), + res if given;
//   kSideSaved -- x dact_scale act'(saved) (dact_in as bf16), + res if given.
constexpr int kSideNone = 0, kSideRes = 1, kSideBits = 2, kSideSaved = 3;

// The side operands as plain values (see EpiParams).
struct SideArgs {
  const bf16_t* res;
  int64_t ldr;
  const bf16_t* dact_in;
  int64_t ldd;
  int dact;
  float dact_scale;
};

// An absent addend as registers: x + (-0) == x for every x, signed zeros
// included, so the arithmetic below needs no branch on `res`.
__device__ __forceinline__ bf16x8 neg_zero8() {
  return __builtin_bit_cast(bf16x8, s16x8{(short)0x8000, (short)0x8000, (short)0x8000, (short)0x8000,
                                          (short)0x8000, (short)0x8000, (short)0x8000, (short)0x8000});
}

// One 8-column chunk of the bf16 store pass: v x mask-or-act', then + res, then
// one bf16 rounding.  The interior and the edge path both call this.
template <int SIDE, bool RES>
__device__ __forceinline__ bf16x8 side_apply(const f32x4 lo, const f32x4 hi, uint32_t mb, const bf16x8 sv,
                                             const bf16x8 rv, int dact, float dact_scale) {
  float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  if (SIDE == kSideBits) {  // the ReLU (+ dropout) mask as bits: one byte
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= (mb >> e) & 1 ? dact_scale : 0.f;
  }
  if (SIDE == kSideSaved) {  // activation backward: x act'(saved); one uniform branch per chunk, not per element
    if (dact == kActSavedGrad) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= dact_scale * dact_f(kActSavedGrad, (float)sv[e]);
    } else if (dact == kActRelu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= dact_scale * dact_f(kActRelu, (float)sv[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= dact_scale * dact_f(kActGelu, (float)sv[e]);
    }
  }
  if (RES) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += (float)rv[e];
  }
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
  return o;
}

// The accumulators of wave group `pass` into the [128][W+4] fp32 LDS image
// (the 4-float row pad keeps the scattered 4-byte writes conflict-free).
template <int W>
__device__ __forceinline__ void spill_half(float* stg, const f32x4 (&acc)[8][W / 64], int pass, int wm, int wn,
                                           int lane) {
  constexpr int NJ = W / 64, WN = 16 * NJ, kStride = W + 4;  // NJ: 16-wide accumulator tiles per wave
  const int quad = lane >> 4, col_in = lane & 15;
  if (wm == pass) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          stg[(16 * i + 4 * quad + r) * kStride + wn * WN + 16 * j + col_in] = acc[i][j][r];
  }
}

// staged_store's bf16 pass with a side operand, for a tile that lies wholly
// inside M x N: straight-line code.  All side-operand loads of a pass are
// issued before the accumulator spill and its barrier, which hide them; one
// wait; then the LDS reads and the arithmetic of every chunk, and the pass's
// stores back to back.  (A branch and a load per chunk made the compiler wait
// vmcnt(0) per chunk, which on gfx9 also drains the chunk before's store: 16
// serialised memory round trips per tile.)  Kept apart from the edge path: in
// one control-flow graph with it, the wait counts of either leak into the other.
template <int W, int SIDE, bool RES>
__device__ __forceinline__ void staged_store_interior(char* smem, const f32x4 (&acc)[8][W / 64], int wm, int wn,
                                                      int lane, int tid, int m0, int n0, int64_t ldc, bf16_t* C,
                                                      const SideArgs sd) {
  constexpr int kStride = W + 4, CPR = W / 8, NU = 128 * CPR / kThreads, RS = kThreads / CPR;  // RS: rows per step u
  float* stg = reinterpret_cast<float*>(smem);
  const int crow = tid / CPR, c8 = tid % CPR;
  const int col = n0 + 8 * c8;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t row = m0 + pass * 128 + crow;  // chunk u: row + u RS
    bf16x8 rv[NU], sv[NU];
    uint32_t mb[NU];
    if (RES) {
      const bf16_t* p = sd.res + row * sd.ldr + col;
#pragma unroll
      for (int u = 0; u < NU; ++u) rv[u] = *reinterpret_cast<const bf16x8*>(p + u * RS * sd.ldr);
    }
    if (SIDE == kSideBits) {
      const uint8_t* p = reinterpret_cast<const uint8_t*>(sd.dact_in) + row * sd.ldd + (col >> 3);
#pragma unroll
      for (int u = 0; u < NU; ++u) mb[u] = p[u * RS * sd.ldd];
    }
    if (SIDE == kSideSaved) {
      const bf16_t* p = sd.dact_in + row * sd.ldd + col;
#pragma unroll
      for (int u = 0; u < NU; ++u) sv[u] = *reinterpret_cast<const bf16x8*>(p + u * RS * sd.ldd);
    }
    spill_half<W>(stg, acc, pass, wm, wn, lane);
    __syncthreads();
    bf16x8 o[NU];
    bf16_t* q = C + row * ldc + col;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const float* sp = stg + (crow + u * RS) * kStride + 8 * c8;
      o[u] = side_apply<SIDE, RES>(*reinterpret_cast<const f32x4*>(sp), *reinterpret_cast<const f32x4*>(sp + 4), mb[u],
                                   sv[u], rv[u], sd.dact, sd.dact_scale);
      if (SIDE == kSideSaved) {
        // act' one chunk at a time, each stored at once: interleaved over the pass's
        // chunks, or with the results held back, its temporaries spill.  (No wait
        // comes between the stores either way: every load was issued before them.)
        *reinterpret_cast<bf16x8*>(q + u * RS * ldc) = o[u];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (SIDE != kSideSaved) {
#pragma unroll
      for (int u = 0; u < NU; ++u) *reinterpret_cast<bf16x8*>(q + u * RS * ldc) = o[u];
    }
    __syncthreads();
  }
}

// Writes the block's result through LDS (two halves: waves wm = 0, then 1):
// each wave spills its 128 x W/4 accumulator tile into the fp32 image
// (spill_half), then all 512 threads stream whole rows out with 16-byte
// accesses -- 8 bf16 per store, fp32 read-modify-write (kEpiAccumF32) or fp32
// stores.  Starts with the LDS free, ends with a barrier.
// bf16 with a side operand (SIDE, and RES: with the addend): interior tiles go
// to staged_store_interior; edge tiles keep the per-chunk predicated loop
// here, so nothing is loaded or stored for a row >= M or a column >= N.
// Saved activation + addend stays on the predicated loop everywhere: the two
// operands of a pass do not fit the registers beside the accumulators.
template <int EPI, int W, int SIDE = kSideNone, bool RES = false>
__device__ __forceinline__ void staged_store(char* smem, const f32x4 (&acc)[8][W / 64], int wm, int wn, int lane,
                                             int tid, int m0, int n0, int M, int N, int64_t ldc, void* out,
                                             const SideArgs sd, bool trans = false) {
  constexpr int kStride = W + 4;
  float* stg = reinterpret_cast<float*>(smem);
  if constexpr (EPI == kEpiStoreBf16 && SIDE != kSideNone && !(SIDE == kSideSaved && RES)) {
    if (m0 + BM <= M && n0 + W <= N) {  // block-uniform
      staged_store_interior<W, SIDE, RES>(smem, acc, wm, wn, lane, tid, m0, n0, ldc, reinterpret_cast<bf16_t*>(out), sd);
      return;
    }
  }
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    spill_half<W>(stg, acc, pass, wm, wn, lane);
    __syncthreads();
    const int rbase = m0 + pass * 128;
    auto grow = [&](int R) { return rbase + R; };  // tile row of image row R
    if (EPI == kEpiStoreBf16) {
      bf16_t* C = reinterpret_cast<bf16_t*>(out);
      constexpr int CPR = W / 8;  // 128 rows x W/8 chunks of 8 columns
      constexpr int kEdgeUnroll = SIDE == kSideSaved ? 1 : 128 * CPR / kThreads;  // act' is long: its loop stays rolled
#pragma unroll kEdgeUnroll
      for (int u = 0; u < 128 * CPR / kThreads; ++u) {
        const int idx = tid + u * kThreads;
        const int row = idx / CPR, c8 = idx % CPR;
        const int col = n0 + 8 * c8;
        if (grow(row) >= M || col >= N) continue;
        const float* sp = stg + row * kStride + 8 * c8;
        uint32_t mb = 0;
        bf16x8 sv = {}, rv = {};
        if (SIDE == kSideBits) mb = reinterpret_cast<const uint8_t*>(sd.dact_in)[(int64_t)grow(row) * sd.ldd + (col >> 3)];
        if (SIDE == kSideSaved) sv = *reinterpret_cast<const bf16x8*>(sd.dact_in + (int64_t)grow(row) * sd.ldd + col);
        if (RES) rv = *reinterpret_cast<const bf16x8*>(sd.res + (int64_t)grow(row) * sd.ldr + col);
        *reinterpret_cast<bf16x8*>(C + (int64_t)grow(row) * ldc + col) =
            side_apply<SIDE, RES>(*reinterpret_cast<const f32x4*>(sp), *reinterpret_cast<const f32x4*>(sp + 4), mb, sv,
                                  rv, sd.dact, sd.dact_scale);
      }
    } else if (trans) {
      // C^T: element (row m, col n) to C[n * ldc + m].  Item (mq, n): rows
      // 4 mq .. 4 mq + 3 of column n, one 16-byte store; 8 consecutive items
      // are 8 row quads of one column (128 contiguous output bytes).
      float* C = reinterpret_cast<float*>(out);
#pragma unroll 4
      for (int u = 0; u < 32 * W / kThreads; ++u) {
        const int idx = tid + u * kThreads;
        const int mq = (idx & 7) + 8 * (idx / (8 * W)), n = (idx >> 3) % W;
        if (grow(4 * mq) >= M || n0 + n >= N) continue;
        const float* sp = stg + 4 * mq * kStride + n;
        const float4 v = make_float4(sp[0], sp[kStride], sp[2 * kStride], sp[3 * kStride]);
        float4* dst = reinterpret_cast<float4*>(C + (int64_t)(n0 + n) * ldc + grow(4 * mq));
        if (EPI == kEpiAccumF32) {
          const float4 o = *dst;
          *dst = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
        } else {
          *dst = v;
        }
      }
    } else {
      float* C = reinterpret_cast<float*>(out);
      constexpr int CPR4 = W / 4;  // 128 rows x W/4 chunks of 4 columns
#pragma unroll
      for (int u = 0; u < 128 * CPR4 / kThreads; ++u) {
        const int idx = tid + u * kThreads;
        const int row = idx / CPR4, c4 = idx % CPR4;
        if (grow(row) >= M || n0 + 4 * c4 >= N) continue;
        const float4 v = *reinterpret_cast<const float4*>(stg + row * kStride + 4 * c4);
        float4* dst = reinterpret_cast<float4*>(C + (int64_t)grow(row) * ldc + n0 + 4 * c4);
        if (EPI == kEpiAccumF32) {
          const float4 o = *dst;
          *dst = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
        } else {
          *dst = v;
        }
      }
    }
    __syncthreads();
  }
}

// The EXTRA epilogue (dropout and / or the aux output) in the STAGED layout:
// the pre-activation (acc + bias) goes through the LDS image once, and each
// thread then owns 4-row x 8-column blocks of it -- the 8 Philox calls of a
// block give exactly its 32 mask words (the (row / 4, col) layout of
// epi_rows and bias_act), and the block's rows leave as 16-byte stores of the
// output AND of the aux tensor (pre or GELU'(pre)).  In the register layout
// the aux tensor needed a staging pass of its own and the activation /
// dropout ran on the accumulator registers: GPT-2-XL's fc1 forward
// (18432 x 6400 x 1600, GELU, p 0.1, pre saved) cost 542 us against 358 plain
// (tools/epilogue_cost_probe.py).  Also the activation backward of a dgrad
// whose forward had dropout (dact_in with the mask regenerated).
// Everything the epilogue reads, as plain values (see EpiParams: read through a
// GemmArgs reference, the kernel arguments were re-loaded after every store).
struct ActParams {
  bf16_t* C;
  bf16_t* aux;
  const bf16_t* res;
  const bf16_t* dact_in;
  uint8_t* bits;
  int64_t ldc, ldr, ldd, ldbits, mask_ld;
  uint64_t seed, offset;
  int M, N, mask_row0, mask_col0, dact;
  float pscale, dact_scale;
  uint32_t thr16;
  bool drop, aux_grad;
};

// One 4-row x 8-column block of the EXTRA epilogue.  INTERIOR (the tile lies
// wholly inside M x N): straight-line; otherwise rows >= M are predicated off.
// The block's dact_in / res rows are loaded together, ahead of its first store.
template <int ACT, int W, bool INTERIOR, bool SIDE = true>
__device__ __forceinline__ void act_block(const ActParams& a, const float* stg, int rq, int c8, int row0, int col) {
  constexpr int kStride = W + 4;
  bf16x8 sv[4], rv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sv[r] = rv[r] = neg_zero8();
    if (SIDE && (INTERIOR || row0 + r < a.M)) {
      if (a.dact_in != nullptr) sv[r] = *reinterpret_cast<const bf16x8*>(a.dact_in + (int64_t)(row0 + r) * a.ldd + col);
      if (a.res != nullptr) rv[r] = *reinterpret_cast<const bf16x8*>(a.res + (int64_t)(row0 + r) * a.ldr + col);
    }
  }
  uint32_t wd[4][4];  // [column pair][row]: two 16-bit uniforms per word
  if (a.drop) {
    const uint64_t sub = drop_sub(row0 + a.mask_row0, col + a.mask_col0, a.mask_ld);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint4 w = Philox(a.seed, sub + e, a.offset).next4();
      wd[e][0] = w.x; wd[e][1] = w.y; wd[e][2] = w.z; wd[e][3] = w.w;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + r;
    if (!INTERIOR && row >= a.M) break;
    const float* sp = stg + (4 * rq + r) * kStride + 8 * c8;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(sp);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(sp + 4);
    const float pre[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    if (a.aux != nullptr) {
      bf16x8 x;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = (__bf16)(ACT == kActGelu && a.aux_grad ? gelu_grad_f(pre[e]) : pre[e]);
      *reinterpret_cast<bf16x8*>(a.aux + (int64_t)row * a.ldc + col) = x;
    }
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float o = ACT == kActRelu ? fmaxf(pre[e], 0.f) : (ACT == kActGelu ? gelu_f(pre[e]) : pre[e]);
      if (a.drop) o = drop_keep(wd[e >> 1][r], e & 1, a.thr16) ? o * a.pscale : 0.f;
      v[e] = o;
    }
    if (SIDE && a.dact_in != nullptr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= a.dact_scale * dact_f(a.dact, (float)sv[r][e]);
    }
    if (SIDE) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += (float)rv[r][e];  // -0 where there is no addend
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
    *reinterpret_cast<bf16x8*>(a.C + (int64_t)row * a.ldc + col) = o;
    if (a.bits != nullptr) {  // the output's nonzeros, for the consumer's dgrad (kActReluBits)
      uint32_t mb = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) mb |= (v[e] != 0.f ? 1u : 0u) << e;
      a.bits[(int64_t)row * a.ldbits + (col >> 3)] = (uint8_t)mb;
    }
  }
}

template <int ACT, int W>
__device__ __forceinline__ void staged_store_act(char* smem, const f32x4 (&acc)[8][W / 64], int wm, int wn,
                                                 int lane, int tid, int m0, int n0, const ActParams a) {
  constexpr int CB = W / 8;
  float* stg = reinterpret_cast<float*>(smem);
  const bool interior = m0 + BM <= a.M && n0 + W <= a.N;  // block-uniform
  const bool plain = a.dact_in == nullptr && a.res == nullptr;
  // (the pass loop and the block loops are left rolled: unrolled,
  // the Philox-heavy block body is compiled eight times over and the kernel
  // outgrows the instruction cache)
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    spill_half<W>(stg, acc, pass, wm, wn, lane);
    __syncthreads();
    const int rbase = m0 + pass * 128;
    if (interior && plain) {  // no side operand (the forward with dropout): nothing is loaded, stores only
#pragma unroll 1
      for (int u = 0; u < 32 * CB / kThreads; ++u) {
        const int idx = tid + u * kThreads;
        const int rq = idx / CB, c8 = idx % CB;  // consecutive lanes on consecutive 8-column chunks
        act_block<ACT, W, true, false>(a, stg, rq, c8, rbase + 4 * rq, n0 + 8 * c8);
      }
    } else if (interior) {
#pragma unroll 1
      for (int u = 0; u < 32 * CB / kThreads; ++u) {
        const int idx = tid + u * kThreads;
        const int rq = idx / CB, c8 = idx % CB;
        act_block<ACT, W, true>(a, stg, rq, c8, rbase + 4 * rq, n0 + 8 * c8);
      }
    } else {
#pragma unroll 1
      for (int u = 0; u < 32 * CB / kThreads; ++u) {
        const int idx = tid + u * kThreads;
        const int rq = idx / CB, c8 = idx % CB;
        const int col = n0 + 8 * c8, row0 = rbase + 4 * rq;
        if (col < a.N && row0 < a.M) act_block<ACT, W, false>(a, stg, rq, c8, row0, col);
      }
    }
    __syncthreads();
  }
}

// Main loop: whole-tile ping-pong.  The two wave groups (wm = 0: waves 0-3,
// wm = 1: waves 4-7; each SIMD hosts one wave of each) run one barrier
// interval apart, so in every interval one wave per SIMD issues the 64 MFMAs
// of its whole 128 x W/4 tile of a K-tile while its partner issues the LDS
// fragment reads (and the LDS-DMA staging) for its next one -- the LDS
// latency of one group hides behind the other's MFMAs instead of stalling
// both, and s_setprio keeps the MFMA wave ahead of the loading one.  One load
// and one MFMA interval per K-tile and wave (236-242 VGPRs, no scratch), two
// barriers per 1024 MFMA cycles.  The buffer hand-off, the staging shares that
// keep a DMA off bytes a sibling wave may still read, the three-buffer rotation
// of an I-contiguous B and the waits are described at the loop itself.
//
// Tried and lost, and no longer in this file: one barrier per K-tile with no
// ping-pong, ping-pong in four 16-MFMA phases per K-tile (with and without the
// B operand staged two K-tiles ahead) and in two 32-MFMA phases, a
// piece-staged variant, and a 4-wave kernel with a 128x128 tile per wave.  The
// whole-tile loop beat the best of the phased ones by 3-7 % (fewer, longer
// intervals pay the barriers less often: profiles/gemm_sched_ab.txt,
// profiles/gemm_schedules_ab.txt, and profiles/wgrad_flush_sched.txt for the
// weight-gradient layout); the 4-wave kernel measured 2-11 % slower at the
// power cap (profiles/gemm4w_r5.txt).

// W: block tile width along N -- 256, or 128 for grids where 256x256 tiles
// would leave CUs idle (256x128 block, 128x32 per wave).
// EXTRA: the bf16 epilogue also applies dropout and/or stores the
// pre-activation (otherwise it is branch-free bias + activation).
// X: main-loop extras, 0 none, kXEmit the A^T emission (GemmArgs::at), kXColsum
// the B-side bias fold (GemmArgs::colsum) -- separate instantiations, so the
// plain kernels keep their register allocation.
constexpr int kXEmit = 1, kXColsum = 2;

template <bool A_KC, bool B_KC, int EPI, int ACT, int W, bool EXTRA, int X = 0, int SIDE = kSideNone>
__global__ void __launch_bounds__(kThreads, 1) gemm256_kernel(GemmArgs g) {
  constexpr int NJ = W / 64;          // 16-wide MFMA column tiles per wave
  constexpr int WN = W / 4;           // wave tile width
  constexpr int kBuf = kTileBytes + W * BK * 2;  // A + B tile
  constexpr bool AH = !A_KC;          // A tile as two 128-wide halves (stage_offsets_halves)
  constexpr bool B3 = !B_KC;          // B tiles in three buffers (smem_bytes)
  constexpr bool II = AH && B3;       // both I-contiguous: own LDS map, K loop unrolled by two (below)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  int tm, tn;
  tile_coords((g.M + BM - 1) / BM, (g.N + W - 1) / W, tm, tn, g.group_m);
  tm = __builtin_amdgcn_readfirstlane(tm);  // block-uniform: scalar registers, not two VGPRs
  tn = __builtin_amdgcn_readfirstlane(tn);
  const int m0 = tm * BM, n0 = tn * W;
  f32x4 acc[8][NJ];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fused bias gradient (GemmArgs::rowsum): group-0 thread t sums the 4 rows
  // [16 tn + 4 (t & 3), +4) of K-row t >> 2 of every A tile (I-contiguous image)
  const bool rsum = g.rowsum != nullptr && tn < 16 && !A_KC;
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
  // The fold is split into its LDS read and its adds: the main loop issues
  // the read with the fragment reads and adds after the DMA issue, behind the
  // interval's own lgkmcnt(0) (adding right after the read put a second drain
  // of all the fragment reads in front of the DMA issue).
  auto rowsum_read = [&](const char* tile, s16x4& v) {
    if (rsum && wm == 0) {
      const int r = tid >> 2, c8 = 4 * tn + (tid & 3);
      v = *reinterpret_cast<const s16x4*>(
          AH ? tile + (tn >> 3) * (kTileBytes / 2) + ic_off_w<128>(r, c8 & 31) : tile + ic_off_w<256>(r, c8));
    }
  };
  auto rowsum_add = [&](const s16x4& v) {
    if (rsum && wm == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) rs[e] += __uint_as_float((uint32_t)(uint16_t)v[e] << 16);
    }
  };
  // fused bias gradient on the B side (GemmArgs::colsum): the tile column is cut
  // into slices of 16 cm columns spread over its tile rows -- block tm, wave
  // group wm sums slice tm + tiles_m wm; cm (1, 2, 4, 8) is the smallest that
  // lets the 2 tiles_m slices cover all W columns (gemm_colsum_ok).  Group-local
  // thread t sums the 4 columns [16 cm s + 4 q, +4), q = t mod 4 cm, of the
  // cm K-rows t / (4 cm) + j 64 / cm of every B tile it reads.  Four
  // accumulators per lane whatever cm is: more (two slices per lane) spilled
  // the main loop's DMA offsets.
  const int tiles_m = (g.M + BM - 1) / BM;
  const int cm_log = __builtin_amdgcn_readfirstlane(2 * tiles_m * 16 >= W ? 0 : 2 * tiles_m * 32 >= W ? 1
                                                    : 2 * tiles_m * 64 >= W ? 2 : 3);
  const int csl = tm + tiles_m * wm;  // this group's slice
  const bool csum = X == kXColsum && !B_KC && g.colsum != nullptr && csl < (W / 16 >> cm_log);
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  // Unlike the row fold this one is not split into read and adds: holding its
  // value across the DMA issue cost the X = kXColsum kernels 2-6 VGPRs more
  // than they had (254 -> 256, 168 -> 172).  The main loop runs the whole
  // step below the DMA issue instead -- the B tile read is not restaged before
  // the interval's barrier -- so its wait is the interval's own drain.
  auto colsum_step = [&](const char* btile) {
    if (csum) {
      const int t = tid & 255;
      const int q = t & ((4 << cm_log) - 1), r0 = t >> (2 + cm_log);
      for (int j = 0; j < (1 << cm_log); ++j) {
        const s16x4 v = *reinterpret_cast<const s16x4*>(
            btile + ic_off_w<W>(r0 + (j << (6 - cm_log)), (4 << cm_log) * csl + q));
#pragma unroll
        for (int e = 0; e < 4; ++e) cs[e] += __uint_as_float((uint32_t)(uint16_t)v[e] << 16);
      }
    }
  };
  // A^T emission is spread evenly: K-tile kt's 32 pieces (wave w, j = 0..3:
  // tile rows [8 (4 w + j), +8)) go to the tile-row's blocks in rotation --
  // piece (w, j) by block tn = (4 w + j + kt) mod tiles_n -- so a wave emits
  // at most one piece per K-tile (2 transposing reads, their wait, 1 store)
  // instead of one block stalling on all 32: few extra registers (the dropout
  // variant's main loop did not fit them otherwise) and no long stall.
  const int ntn = (g.N + W - 1) / W;
  const int ewb = __builtin_amdgcn_readfirstlane((4 * wave) % ntn);  // scalar: no VGPR held across the loop
  // A piece: two transposing reads issued BEFORE the fragment reads and one
  // store issued AFTER them, so its wait retires only the oldest reads and
  // hides behind the fragment loads (waiting right after the reads exposed
  // their latency in every load interval: +8-17 % on the forward GEMMs).
  auto emit_reads = [&](const char* atile, int j, s16x4& a, s16x4& b) {
    const int q = (lane & 15) >> 2, p = lane & 3, gq = lane >> 4;
    const int c16 = 2 * gq + (p >> 1);
    const int r = 8 * (4 * wave + j) + q;
    const int lo = r * 128 + ((c16 ^ ((r >> 1) & 7)) << 4) + 8 * (p & 1);
    const int hi = (r + 4) * 128 + ((c16 ^ (((r + 4) >> 1) & 7)) << 4) + 8 * (p & 1);
    a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(atile + lo));
    b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(atile + hi));
  };
  // (GemmArgs fields as locals: read through `g` inside the K loop they are
  // re-loaded after every LDS-DMA, see KCursor)
  bf16_t* const at_out = X == kXEmit ? reinterpret_cast<bf16_t*>(g.at) : nullptr;
  const int64_t ldat = X == kXEmit ? g.ldat : 0;
  const int M = g.M;
  auto emit_store = [&](int kt, int j, const s16x4& a, const s16x4& b) {
    const int rb = 4 * wave + j;
    bf16_t* at = at_out + (int64_t)(kt * BK + 16 * (lane >> 4) + (lane & 15)) * ldat + m0 + 8 * rb;
    if (m0 + 8 * rb < M) *reinterpret_cast<s16x8*>(at) = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  int kt0 = 0, nk = g.K / BK;
  if (g.k_splits > 1) {  // this block's share of the K-tiles
    const int total = nk;
    kt0 = (int)blockIdx.y * total / g.k_splits;
    nk = ((int)blockIdx.y + 1) * total / g.k_splits - kt0;
  }
  // Staging shares (see the loop): the waves of group 1 (which restage the
  // buffer their siblings are still reading) take bytes no sibling reads -- A rows 0-127 (group 0's half: share of "wave" w ^ 4; for
  // an I-contiguous A the tile is kept as two halves for this) and, for a
  // K-contiguous B, the first 32 of the 64 rows the wave itself reads (share
  // 2 wn; group 0 the other 32: 2 wn + 1).  An I-contiguous B (every wave
  // reads every k-row) rotates through three buffers instead and keeps the
  // per-wave k-row shares.
  const int shA = wave ^ 4;
  const int shB = B_KC ? 2 * wn + (wm == 0 ? 1 : 0) : wave;
  uint32_t offA[4], offB[NJ];
  if constexpr (AH) stage_offsets_halves(g.lda, m0, g.M, shA, lane, offA);
  else stage_offsets<A_KC, 256>(g.lda, m0, g.M, shA, lane, offA);
  stage_offsets<B_KC, W>(g.ldb, n0, g.N, shB, lane, offB);
  constexpr int NB = W / 64;  // B DMAs per wave per K-tile
  constexpr int NA = 4;       // A DMAs per wave per K-tile
  // `kc` runs ahead of the loop, always at the tile this wave group stages
  // next (tile u + 1 for group 0, u + 2 for group 1).
  // LDS map.  A of buffer i (tile parity) and B of slot s (B3: u mod 3, else
  // the parity): [A0 B0][A1 B1][B2], or, both operands I-contiguous (II),
  // [A0 A1][B0 B1 B2] -- the two A tiles inside one 64 KiB window, so that a
  // fragment address is ONE loop-invariant VGPR per 16-row block plus the
  // ds_read's 16-bit immediate, whichever tile is read (see the loop).
  auto abuf = [&](int i) { return II ? smem + i * kTileBytes : smem + i * kBuf; };
  auto bslot = [&](int s) {
    if (II) return smem + 2 * kTileBytes + s * (W * BK * 2);
    return s == 2 ? smem + 2 * kBuf : smem + s * kBuf + kTileBytes;
  };
  KCursor kc;
  kc.init<A_KC, B_KC>(g, kt0);
  stage_fast<256>(kc.a, offA, abuf(0), shA);
  stage_fast<W>(kc.b, offB, bslot(0), shB);
  kc.next(g);
  if (wm == 1 && nk > 1) {  // group 1 stages whole tiles one tile earlier (below)
    stage_fast<256>(kc.a, offA, abuf(1), shA);
    stage_fast<W>(kc.b, offB, bslot(1), shB);
    kc.next(g);
  }

  // Whole-tile ping-pong: one load and one MFMA interval per K-tile and wave
  // (64 MFMAs: the wave's whole 128x64 tile), barriers paid once per 1024
  // MFMA cycles.  Group 0 loads tile u in interval 2u, group 1 in 2u+1
  // (global count).  Tile u+1 goes into tile u-1's buffer, last read by
  // group 1 in 2u-1: group 1 stages its share right after those reads
  // (program order), group 0 in its load interval 2u.  Group 1's DMA into
  // tile u's buffer may land while a SIBLING wave still has reads of it
  // queued (no barrier separates the waves of a group; a sibling delayed by
  // its A^T emission piece was seen to read the next tile's rows once), so
  // group 1 restages only bytes none of its siblings reads: A rows 0-127
  // (shA above; an I-contiguous A is kept as two 128-row halves for that)
  // and, for a K-contiguous B, half of the i-rows the wave itself reads
  // (shB).  An I-contiguous B has no such share (every wave reads every
  // k-row of its columns), so its tiles rotate through three buffers: tile
  // u+2 goes into tile u-1's B buffer, whose last reads (group 1, interval
  // 2u-1) retired before the barrier ending that interval.  Tile u+1 must
  // have landed by the barrier ending 2u+1: group 0 drains after its MFMAs
  // (vmcnt(0)), group 1 in its load interval 2u+1 after staging tile u+2
  // (vmcnt(NA + NB)).
  // The load interval reads no kernel argument: the operand addresses of
  // the tile a group stages come from its KCursor `kc`, advanced once per
  // staged tile, and it has ONE LDS drain, the lgkmcnt(0) before its
  // barrier (static counts and timings: profiles/gemm_loop_scalar.txt).
  if (wm == 1 && nk > 1) vmcnt_keep<NA + NB>();
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();  // stagger group 1 by one interval
  bf16x8 af[8][2], bq[NJ][2];
  int ekt = kt0 % ntn;  // (kt0 + u) mod tiles_n (A^T emission rotation)
  int bs = 0;  // B3: slot of tile u (u mod 3; tiles kt0, kt0 + 1 were staged into slots 0, 1)
  // Both operands I-contiguous (II): the schedule, hand-offs, staging shares
  // and waits of the loop below (described there), unrolled by two so that
  // the tile's parity P is a constant.  The 8 + NJ column blocks of a fragment
  // each need an address VGPR of their own (the XOR swizzle differs per lane;
  // a K-contiguous operand gets by with two in all), and with the tile's buffer
  // a run-time value the load interval OPENED with 15 VALU adds (buffer base +
  // block address) before its first ds_read -- issued at priority 0 beside the
  // partner's MFMAs at priority 1, they made this layout's kernel 1.22x the
  // transposed one's cycles (profiles/wgrad_ii_loop.txt; now 1.12x, and level
  // with it per FLOP inside the training step).  Here the A buffer's offset in
  // its 64 KiB window (abuf) is part of each read's immediate, so the 8 A
  // addresses are computed once; the NJ B addresses take one add each for the
  // slot (three slots span 96 KiB, past the immediate), issued below the A
  // reads.  Which bytes a group restages, and when, is what it is below --
  // only where the buffers lie differs -- so the ownership argument given
  // there covers every wave pair here as it stands.
  if constexpr (II) {
    const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)smem);
    uint32_t aaddr[8], baddr[NJ];  // tile-relative fragment addresses of s = 0 (A: in this group's half)
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) aaddr[ii] = lds0 + wm * (kTileBytes / 2) + ic_frag_off<128>(16 * ii, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) baddr[j] = ic_frag_off<W>(wn * WN + 16 * j, lane);
    auto k_tile = [&](const int u, auto parity) {
      constexpr int P = decltype(parity)::value;
      char* cur = abuf(P);
      char* nxt = abuf(P ^ 1);
      char* bcur = bslot(bs);
#pragma unroll
      for (int ii = 0; ii < 8; ++ii)
#pragma unroll
        for (int s = 0; s < 2; ++s) af[ii][s] = ic_frag_at<128>(aaddr[ii], P * kTileBytes, s);
      const uint32_t bcur0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)bcur);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const uint32_t ba = bcur0 + baddr[j];
#pragma unroll
        for (int s = 0; s < 2; ++s) bq[j][s] = ic_frag_at<W>(ba, 0, s);
      }
      s16x4 rv;
      rowsum_read(cur, rv);
      const int ahead = wm == 0 ? 1 : 2;  // the tile this group stages now
      if (u + ahead < nk) {
        stage_fast<256>(kc.a, offA, wm == 0 ? nxt : cur, shA);
        int bn = bs + ahead;
        if (bn >= 3) bn -= 3;
        stage_fast<W>(kc.b, offB, bslot(bn), shB);
        kc.next(g);
      }
      bs = bs == 2 ? 0 : bs + 1;
      if (wm == 1) {
        if (u + 2 < nk) vmcnt_keep<NA + NB>();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_waitcnt(kWaitLgkm0);  // every read retired before the barrier (see below)
      rowsum_add(rv);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ii = 0; ii < 8; ++ii)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ii][s], bq[j][s], acc[ii][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      if (wm == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    };
    for (int u = 0; u < nk; u += 2) {
      k_tile(u, std::integral_constant<int, 0>{});
      if (u + 1 < nk) k_tile(u + 1, std::integral_constant<int, 1>{});
    }
  }
  for (int u = 0; !II && u < nk; ++u) {  // every other layout (II ran its K-tiles above)
    char* cur = smem + (u & 1) * kBuf;
    char* nxt = smem + ((u + 1) & 1) * kBuf;
    char* bcur = B3 ? bslot(bs) : cur + kTileBytes;
    // emission first: its reads precede this wave's DMA that may restage
    // `cur`, and its stores (waiting for those reads) precede the fragment
    // reads, so its 16 data registers are dead before the fragments load
    // this wave's A^T piece of K-tile kt0 + u, if any: j with (4 wave + j + kt) mod tiles_n == tn
    // (grids under 4 tile columns give a wave several pieces of a K-tile:
    // those are read and stored one after the other, here)
    int ej = -1;
    if (X == kXEmit && A_KC) {
      int e = ewb + ekt;
      while (e >= ntn) e -= ntn;
      ej = tn - e;  // first piece index (the wrap: tn + ntn - e)
      if (ej < 0) ej += ntn;
      if (ntn < 4) {
        for (int j = ej; j < 4; j += ntn) {
          s16x4 a, b;
          emit_reads(cur, j, a, b);
          emit_store(kt0 + u, j, a, b);
        }
        ej = -1;
      } else if (ej > 3) {
        ej = -1;
      }
    }
    s16x4 ea, eb;
    if (X == kXEmit && A_KC && ej >= 0) emit_reads(cur, ej, ea, eb);
#pragma unroll
    for (int ii = 0; ii < 8; ++ii)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        af[ii][s] = AH ? frag<false, 128>(cur + wm * (kTileBytes / 2), 16 * ii, s, lane)
                       : frag<A_KC, 256>(cur, wm * 128 + 16 * ii, s, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s) bq[j][s] = frag<B_KC, W>(bcur, wn * WN + 16 * j, s, lane);
    // row fold: read here, added below the DMA issue (the column fold runs there whole)
    s16x4 rv;
    rowsum_read(cur, rv);
    if (X == kXEmit && A_KC && ej >= 0) emit_store(kt0 + u, ej, ea, eb);
    ekt = ekt + 1 == ntn ? 0 : ekt + 1;
    // The DMA issue needs nothing but scalars already in registers (kc: no
    // kernel-argument load, no division, no wait), so it goes out while the
    // fragment reads above are still in flight.
    const int ahead = wm == 0 ? 1 : 2;  // the tile this group stages now
    if (u + ahead < nk) {
      char* dst = wm == 0 ? nxt : cur;
      stage_fast<256>(kc.a, offA, dst, shA);
      int bn = bs + ahead;
      if (bn >= 3) bn -= 3;
      stage_fast<W>(kc.b, offB, B3 ? bslot(bn) : dst + kTileBytes, shB);
      kc.next(g);  // a segment crossing loads the pointers of the segment after: retired by the wait below
    }
    bs = bs == 2 ? 0 : bs + 1;
    colsum_step(bcur);
    if (wm == 1) {
      if (u + 2 < nk) vmcnt_keep<NA + NB>();
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // Retire this interval's LDS reads BEFORE the barrier: right after it the
    // other group restages the buffer just read (group 0 DMAs tile u+1 over
    // tile u-1, group 1 tile u+2 over tile u), and a read still queued in
    // the LDS when that DMA lands returns the new tile -- an intermittent
    // wrong accumulator (tools/gemm_round_screen.py caught it: ~1 launch in
    // 3 of one shape).  Guide rule: restage one phase after a read only when
    // an lgkmcnt before the reading phase's barrier retired it.
    // The wait is the builtin, not asm, so that the compiler's own counting
    // sees it: the fold adds below and the MFMAs after the barrier then need
    // no further lgkmcnt wait, and this is the interval's only one.
    __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
    rowsum_add(rv);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int ii = 0; ii < 8; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ii][s], bq[j][s], acc[ii][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    if (wm == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();  // equalise the barrier count

  if (rsum) {  // K-rows -> one sum per row: lanes (xor over the K-row bits), then the 4 group-0 waves through LDS
    __syncthreads();  // every wave is done reading the operand buffers
    float* red = reinterpret_cast<float*>(smem);
    if (wm == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int o = 4; o < 64; o <<= 1) rs[e] += __shfl_xor(rs[e], o, 64);
      if (lane < 4)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave * 16 + 4 * lane + e] = rs[e];
    }
    __syncthreads();
    if (tid < 16) {
      const float v = red[tid] + red[16 + tid] + red[32 + tid] + red[48 + tid];
      const int row = m0 + 16 * tn + tid;
      if (row < g.M) g.rowsum[row] += v;
    }
  }
  if (X == kXColsum && g.colsum != nullptr) {  // the same reduction for the B-side column sums, per group
    __syncthreads();
    const int sw = 16 << cm_log;  // slice width
    float* red = reinterpret_cast<float*>(smem) + 64;  // [8 waves][sw columns]
#pragma unroll
    for (int e = 0; e < 4; ++e)
      for (int o = 4 << cm_log; o < 64; o <<= 1) cs[e] += __shfl_xor(cs[e], o, 64);
    if (lane < (4 << cm_log))
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wave * sw + 4 * lane + e] = cs[e];
    __syncthreads();
    if (tid < 2 * sw) {
      const int gq = tid >> (4 + cm_log), c = tid & (sw - 1);
      const int sl = tm + tiles_m * gq;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) v += red[(4 * gq + w) * sw + c];
      const int col = n0 + sw * sl + c;
      if (sl < (W / 16 >> cm_log) && col < g.N) {
        if (g.k_splits > 1) g.colsum[(int64_t)blockIdx.y * g.N + col] = v;  // split-K: a partial per split
        else g.colsum[col] += v;
      }
    }
  }
  // ---- epilogue ----
  // 1) element-wise epilogue in registers (accumulator layout): bias,
  //    activation, dropout (the mask is tied to this layout); with an aux
  //    output, the pre-activation (acc + bias) is first written out through
  //    the same staged path;
  // 2) staged_store: LDS-staged 16-byte row stores (+ residual addend), fp32
  //    read-modify-write for an accumulated weight gradient, fp32 stores for
  //    the first write of a step or a split-K partial.
  //    (The earlier direct 2-byte bf16 stores cost ~5 us per 256x256 tile at
  //    K = 64 more than this path: tools/gemm_k_sweep.py.)
  const int quad = lane >> 4, col_in = lane & 15;
  // The lane's NJ bias columns: one uniform branch, the loads issued together
  // ahead of the barrier (which hides them) and waited for once.  Columns
  // past N read the last valid entry: their results are never stored.
  uint32_t braw[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) braw[j] = 0;
  if (EPI == kEpiStoreBf16 && g.bias != nullptr) {
    const bf16_t* bp = reinterpret_cast<const bf16_t*>(g.bias);
    const int ncol = n0 + wn * WN + col_in, last = g.N - 1;
#pragma unroll
    for (int j = 0; j < NJ; ++j) braw[j] = bp[min(ncol + 16 * j, last)];
  }
  __syncthreads();  // every wave is done reading the operand buffers
  float bias[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    // pins the first use below the barrier (the conversion is otherwise hoisted
    // into the branch above, and its wait with it)
    if (EPI == kEpiStoreBf16) asm volatile("" : "+v"(braw[j]));
    bias[j] = __uint_as_float(braw[j] << 16);
  }
  if constexpr (EPI == kEpiStoreBf16 && EXTRA) {  // dropout and / or aux: the staged-layout epilogue does it all
    if (g.bias != nullptr) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i][j] += bias[j];
    }
    const bool drop = g.p > 0.f;
    const ActParams ap{reinterpret_cast<bf16_t*>(g.C), reinterpret_cast<bf16_t*>(g.aux),
                       reinterpret_cast<const bf16_t*>(g.res), reinterpret_cast<const bf16_t*>(g.dact_in),
                       reinterpret_cast<uint8_t*>(g.bits), g.ldc, g.ldr > 0 ? g.ldr : g.ldc, g.ldd, g.ldbits,
                       g.mask_ld > 0 ? g.mask_ld : g.N, g.seed, g.offset, g.M, g.N, g.mask_row0, g.mask_col0, g.dact,
                       drop ? 1.f / (1.f - g.p) : 1.f, g.dact_scale, g.threshold >> 16, drop, g.aux_grad};
    staged_store_act<ACT, W>(smem, acc, wm, wn, lane, tid, m0, n0, ap);
    return;
  } else {
    if (EPI == kEpiStoreBf16 && (ACT != kActNone || g.bias != nullptr)) {
      const int ncol = n0 + wn * WN + col_in, nrow = m0 + wm * 128 + 4 * quad;
      const float pscale = g.p > 0.f ? 1.f / (1.f - g.p) : 1.f;
      const EpiParams ep{g.seed, g.offset, g.N, g.p, pscale, g.threshold, g.mask_row0, g.mask_col0,
                         g.mask_ld > 0 ? g.mask_ld : g.N};
      epi_rows<0, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
      epi_rows<1, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
      epi_rows<2, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
      epi_rows<3, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
      epi_rows<4, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
      epi_rows<5, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
      epi_rows<6, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
      epi_rows<7, ACT, NJ, EXTRA>(ep, acc, nrow, ncol, bias);
    }
    void* out = EPI == kEpiStoreBf16 ? g.C
                                     : reinterpret_cast<void*>(reinterpret_cast<float*>(g.C) +
                                                               (int64_t)blockIdx.y * g.M * g.ldc);  // split-K partial y
    const SideArgs sd{reinterpret_cast<const bf16_t*>(g.res), g.ldr, reinterpret_cast<const bf16_t*>(g.dact_in), g.ldd,
                      g.dact, g.dact_scale};
    if (SIDE >= kSideBits && sd.res != nullptr)  // the activation backward's optional addend
      staged_store<EPI, W, SIDE, SIDE >= kSideBits>(smem, acc, wm, wn, lane, tid, m0, n0, g.M, g.N, g.ldc, out, sd);
    else
      staged_store<EPI, W, SIDE, SIDE == kSideRes>(smem, acc, wm, wn, lane, tid, m0, n0, g.M, g.N, g.ldc, out, sd,
                                                   EPI != kEpiStoreBf16 && g.trans_c && g.k_splits <= 1);
  }
}

}  // namespace big

int big_tiles(const GemmArgs& g, int w) { return ((g.M + big::BM - 1) / big::BM) * ((g.N + w - 1) / w); }

// ------------------------------------------------------------ the launch plan
// How a GemmArgs is launched is decided once, by gemm_plan() below, in this order; every later rule reads the earlier
// decisions, none is re-derived anywhere else.  The three knobs select between live paths (tests, A/B tools); nothing
// here reads the environment.
//
// 1. big: the 256-row kernel handles every shape (edge tiles masked); the 128x128 one only exact multiples of 128,
//    where it is kept for grids too small to fill the 256 CUs with 256x256 tiles (< 128 of them).  Segmented K, the
//    A^T emission, a transposed output and the two bias-gradient folds exist on the 256-row kernel only.  Chunks of a
//    per-round launch stay on it too: the last chunk of e.g. GPT-2-XL's fc1 forward (18432 x 6400, 7 rounds + 2 tile
//    rows) ran on the 128x128 kernel at ~250 TF/s.
// 2. k_splits, the factor the caller may ask for -- split-K for grids that leave CUs idle while K is long: the T =
//    2048 LM-head dgrad (2048 x 4096 x 28928 = 128 256x256 tiles), GPT-2-XL's weight gradients (1600 x 1600 = 49
//    tiles, 6400 x 1600 = 175, K = 4 x 8192).  s blocks per tile, each a contiguous share of the K-tiles, write fp32
//    partials; one reduction adds them (+ the residual / into main_grad).  s minimises rounds(tiles * s) / s of the
//    tile time (a round = 256 blocks, one per CU; a 256x256 tile at ~4.5 TFLOP/s per CU) plus the partials' HBM
//    traffic, (2 s + 1) * 4 * M * N bytes at ~4 TB/s.  Plain bf16 output (no bias / activation / dropout / aux: those
//    stay in the GEMM epilogue) or an fp32 weight gradient, on the 256-row kernel, K >= 8192, at least 16 K-tiles per
//    split.  Knob splitk: 0 off, 1 this rule, n >= 2 forces n (still capped by the K-tiles).  The caller allocates ws
//    (and colsum_ws) and sets g.k_splits; everything below is decided for the g.k_splits it is given.
// 3. width of the 256-row kernel: the knob's 128 / 256, else g.width's, else 256 under split-K, else 128 when the
//    grid of 256x256 tiles quantises badly onto the 256 CUs -- rounds of 256 tiles, a round of 256x128 tiles costing
//    ~0.73 of a 256x256 round (measured, 2048 x 12288 x 4096).  E.g. T = 2048: 2048 x 4096 is 128 256x256 tiles,
//    half the chip idle, or 256 256x128 tiles (1.2x faster, profiles/gemm_vs_hipblaslt.txt).
// 4. the kernel variant.  extra: dropout and / or the pre-activation output, the staged-layout epilogue of the bf16
//    store pass.  side, for the bf16 store pass without extra: the addend (res) for forward GEMMs (y = res + act(x
//    W^T + b), both operands K-contiguous) and dgrads, the two activation-backward modes (dact_in: the ReLU bit mask,
//    or a saved tensor) for dgrads (A K-contiguous, B not; no bias, no activation of their own, no A^T).  Any other
//    side operand has no kernel: kernel = false, and gemm_bf16 throws.  x: the A^T emission of a forward GEMM --
//    compiled into every forward variant but the GELU one with extra, which would spill its main loop's registers
//    (scratch reloads inside the K loop; gemm_emit_ok) -- or the column-sum fold of the transposed weight gradient.
//    (The compared-and-lost main loops and the 4-wave kernel are gone: see above gemm256_kernel.)
// 5. per-round launches: grids of several rounds whose last round is at most half full are launched one round of
//    tiles at a time: the LM head (4096 x 28928 x 4096, 1808 tiles = 7 rounds + 16 tiles) 812 -> 786 us, 2048 x 12288
//    x 4096 (384 tiles) 176 -> 167 us (hipBLASLt's time).  Whole rounds (4096 x 12288: 768 tiles, 292 vs 296 us) and
//    a last round over half full (2048 x 28928: 904 tiles, 407 vs 415 us) stay one launch
//    (tools/gemm_rounds_probe.py, warm clocks, arms alternated).  Only unsplit 256-wide grids; the grid is cut along
//    its longer tile dimension into at most 16 chunks of floor(256 / other) tiles, and never across a fold: the row
//    slices of rowsum need every tile column of a tile row, the column slices of colsum every tile row of a tile
//    column.  Short main loops (K < 4096: GPT-2-XL's K = 1600 GEMMs) go as ONE launch: a CU that finishes its tile
//    starts the next round's while the others store, so the fixed per-tile prologue / epilogue overlaps across rounds
//    (GPT-2-XL PP=1 64.7-64.8k -> 66.2-66.3k tok/s on one box; enc12, all K = 4096: unchanged).  Knob rounds: 0 one
//    launch, 1 this rule, 2 per round at any K.
// 6. what the caller may ask for.  rowsum_ok: the wgrad layout (A read as [K, M]), fp32 output, no split-K, and >= 16
//    tile columns (one 16-row slice per block of a tile row).  colsum_ok: A K-contiguous and B not, fp32 output, and
//    2 slices of <= 128 columns per block covering the width as launched, i.e. at the split factor of rule 2
//    (split-K: per-split partials, reduced after).  bits_ok: the extra epilogue with ReLU and dropout on the 256-row
//    kernel, unsplit, whole bytes of columns.
struct GemmKnobs {
  int width = 0;   // gemm_set_width: 0 rule 3, or 128 / 256
  int rounds = 1;  // gemm_set_rounds: 0 one launch, 1 rule 5, 2 per round at any K
  int splitk = 1;  // gemm_set_splitk: 0 off, 1 rule 2, n >= 2 forced n ways
};
GemmKnobs g_knobs;

bool plan_big(const GemmArgs& g) {
  return g.round_chunk || g.seg_k > 0 || g.at != nullptr || g.trans_c || g.colsum != nullptr || g.rowsum != nullptr ||
         g.M % BM != 0 || g.N % BN != 0 || big_tiles(g, 256) >= 128;
}

int plan_splits(const GemmArgs& g, bool big) {
  if (g_knobs.splitk == 0) return 1;
  const bool plain_bf16 = g.epi == kEpiStoreBf16 && g.act == kActNone && g.bias == nullptr && g.p <= 0.f &&
                          g.aux == nullptr && g.dact_in == nullptr;
  const bool f32_out = g.epi == kEpiAccumF32 || g.epi == kEpiStoreF32;
  if (!(plain_bf16 || f32_out) || !big || g.K < 8192) return 1;
  const int tiles = big_tiles(g, 256);
  const int kt = g.K / BK;
  if (g_knobs.splitk >= 2) return std::max(1, std::min(g_knobs.splitk, kt / 16));
  const double t_tile = 2.0 * 256 * 256 * (double)g.K / 4.5e12;
  const double mn = (double)g.M * g.N;
  int best = 1;
  double best_t = (double)((tiles + 255) / 256) * t_tile;
  for (int sp = 2; sp <= 8 && kt / sp >= 16; ++sp) {
    const double t = (double)((tiles * sp + 255) / 256) * t_tile / sp + (2.0 * sp + 1.0) * 4.0 * mn / 4.0e12;
    if (t < 0.97 * best_t) {
      best = sp;
      best_t = t;
    }
  }
  return best;
}

int plan_width(const GemmArgs& g, int splits) {
  if (g_knobs.width == 128 || g_knobs.width == 256) return g_knobs.width;
  if (g.width == 128 || g.width == 256) return g.width;
  if (splits > 1) return 256;
  const int r256 = (big_tiles(g, 256) + 255) / 256, r128 = (big_tiles(g, 128) + 255) / 256;
  return 0.75 * r128 < 1.0 * r256 ? 128 : 256;
}

// Run-time values as template arguments: f gets them as std::integral_constant tags.
template <typename F>
void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// The first of V, Vs... equal to v; the last one also stands for every other value.
template <int V, int... Vs, typename F>
void with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V>{});
  else if (v == V) f(std::integral_constant<int, V>{});
  else with_int<Vs...>(v, std::forward<F>(f));
}

// The variants of gemm256_kernel that are compiled (rule 4): the launcher instantiates these and no others.
template <bool A_KC, bool B_KC, int EPI, int ACT, bool EXTRA, int X, int SIDE>
constexpr bool has_kernel() {
  constexpr bool bf16 = EPI == kEpiStoreBf16;
  if (EXTRA && !bf16) return false;
  if (SIDE != big::kSideNone) {
    if (!bf16 || EXTRA) return false;
    if (A_KC && B_KC) return SIDE == big::kSideRes && X != big::kXColsum;
    return A_KC && !B_KC && ACT == kActNone && X == 0;
  }
  if (X == big::kXEmit) return A_KC && B_KC && bf16 && !(ACT == kActGelu && EXTRA);
  if (X == big::kXColsum) return A_KC && !B_KC && !bf16;
  return true;
}

template <bool A_KC, bool B_KC, int EPI, int ACT, int W, bool EXTRA, int X = 0, int SIDE = big::kSideNone>
void launch_big(const GemmArgs& g, hipStream_t s) {
  constexpr int smem = big::smem_bytes<B_KC, W>();
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&big::gemm256_kernel<A_KC, B_KC, EPI, ACT, W, EXTRA, X, SIDE>),
        hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  hipLaunchKernelGGL((big::gemm256_kernel<A_KC, B_KC, EPI, ACT, W, EXTRA, X, SIDE>), dim3(big_tiles(g, W), g.k_splits),
                     dim3(big::kThreads), smem, s, g);
}

// One launch of g, or of one of its per-round chunks, as the plan says.
template <bool A_KC, bool B_KC, int EPI, int ACT>
void launch_one(const GemmPlan& p, const GemmArgs& g, hipStream_t s) {
  if (!p.big) {
    const int blocks = (g.M / BM) * (g.N / BN);
    hipLaunchKernelGGL((gemm_kernel<A_KC, B_KC, EPI, ACT>), dim3(blocks), dim3(kThreads), kSmemBytes, s, g);
    return;
  }
  const auto no_kernel = [] {
    throw std::runtime_error("gemm_bf16: no kernel with this side operand (res / dact_in) for this operand layout");
  };
  if (!p.kernel) no_kernel();
  // of the chunks of a grid cut along N only the first emits A^T (every chunk holds the whole A)
  const int x = p.x == big::kXEmit && g.at == nullptr ? 0 : p.x;
  with_flag(p.extra, [&](auto extra) {
    with_int<big::kXEmit, big::kXColsum, 0>(x, [&](auto xm) {
      with_int<big::kSideRes, big::kSideBits, big::kSideSaved, big::kSideNone>(p.side, [&](auto side) {
        with_int<128, 256>(p.width, [&](auto w) {
          constexpr bool EXTRA = decltype(extra)::value;
          constexpr int X = decltype(xm)::value, SIDE = decltype(side)::value, W = decltype(w)::value;
          if constexpr (has_kernel<A_KC, B_KC, EPI, ACT, EXTRA, X, SIDE>()) launch_big<A_KC, B_KC, EPI, ACT, W, EXTRA, X, SIDE>(g, s);
          else no_kernel();
        });
      });
    });
  });
}

// C[M, N] (bf16, row stride ldc) = sum of the k_splits fp32 partials [s][M][N]
// (+ res): 8 columns per thread, 16-byte loads and stores.
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ ws, int splits, int M, int N,
                                                            int64_t ldc, const bf16_t* __restrict__ res, int64_t ldr,
                                                            bf16_t* __restrict__ C) {
  const int64_t chunks = (int64_t)M * (N / 8);
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= chunks) return;
  const int row = (int)(c / (N / 8)), col = (int)(c % (N / 8)) * 8;
  const int64_t at = (int64_t)row * N + col;
  f32x4 lo = *reinterpret_cast<const f32x4*>(ws + at);
  f32x4 hi = *reinterpret_cast<const f32x4*>(ws + at + 4);
  for (int s = 1; s < splits; ++s) {
    lo += *reinterpret_cast<const f32x4*>(ws + (int64_t)s * M * N + at);
    hi += *reinterpret_cast<const f32x4*>(ws + (int64_t)s * M * N + at + 4);
  }
  float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  const int64_t out = (int64_t)row * ldc + col;
  if (res != nullptr) {
    const bf16x8 r = *reinterpret_cast<const bf16x8*>(res + (int64_t)row * ldr + col);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += (float)r[e];
  }
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
  *reinterpret_cast<bf16x8*>(C + out) = o;
}

// C[M, N] (fp32, row stride ldc) (+)= sum of the k_splits fp32 partials: the
// split-K reduction of a weight gradient (accumulate: into main_grad).
// trans: C[n * ldc + m] (+)= the partials' (m, n) -- a thread reduces rows
// 4 m' .. 4 m' + 3 of one column n (consecutive threads: consecutive n, so the
// partials are read in coalesced rows) and writes them as one 16-byte chunk.
__global__ void __launch_bounds__(256) splitk_reduce_f32_kernel(const float* __restrict__ ws, int splits, int M, int N,
                                                                int64_t ldc, bool accumulate, bool trans,
                                                                float* __restrict__ C) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (trans) {
    if (c >= (int64_t)(M / 4) * N) return;
    const int m = (int)(c / N) * 4, n = (int)(c % N);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; ++s) {
      const float* p = ws + (int64_t)s * M * N + (int64_t)m * N + n;
      v += f32x4{p[0], p[N], p[2 * (int64_t)N], p[3 * (int64_t)N]};
    }
    f32x4* dst = reinterpret_cast<f32x4*>(C + (int64_t)n * ldc + m);
    if (accumulate) v += *dst;
    *dst = v;
    return;
  }
  const int64_t chunks = (int64_t)M * (N / 4);
  if (c >= chunks) return;
  const int row = (int)(c / (N / 4)), col = (int)(c % (N / 4)) * 4;
  const int64_t at = (int64_t)row * N + col;
  f32x4 v = *reinterpret_cast<const f32x4*>(ws + at);
  for (int s = 1; s < splits; ++s) v += *reinterpret_cast<const f32x4*>(ws + (int64_t)s * M * N + at);
  f32x4* dst = reinterpret_cast<f32x4*>(C + (int64_t)row * ldc + col);
  if (accumulate) v += *dst;
  *dst = v;
}

// colsum[n] += the k_splits per-split column sums ws[s][n] (fixed order: deterministic).
__global__ void __launch_bounds__(256) colsum_splits_kernel(const float* __restrict__ ws, int splits, int N,
                                                            float* __restrict__ colsum) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float v = 0.f;
  for (int s = 0; s < splits; ++s) v += ws[(int64_t)s * N + n];
  colsum[n] += v;
}

const char* byte_off(const void* p, int64_t bytes) {
  return p == nullptr ? nullptr : reinterpret_cast<const char*>(p) + bytes;
}

// One chunk of a per-round launch of g (rule 5): p.per tiles of the cut dimension, every operand and output moved to
// the chunk's corner of the full matrices.
GemmArgs round_chunk(const GemmArgs& g, const GemmPlan& p, int chunk) {
  const int t0 = chunk * p.per;
  const int cbytes = g.epi == kEpiStoreBf16 ? 2 : 4;
  GemmArgs c = g;
  c.round_chunk = true;
  c.width = 256;  // the full grid's width: the rowsum fold's slices assume its tile-column count
  const int lo = t0 * 256, hi = std::min((t0 + p.per) * 256, p.along_n ? g.N : g.M);
  c.mask_ld = g.mask_ld > 0 ? g.mask_ld : g.N;
  if (p.along_n) {
    c.N = hi - lo;
    c.mask_col0 = g.mask_col0 + lo;
    const int64_t boff = (g.b_kc ? (int64_t)lo * g.ldb : (int64_t)lo) * 2;
    c.B = byte_off(g.B, boff);
    for (int i = 0; i < GemmArgs::kMaxSegs; ++i) c.b_seg[i] = byte_off(g.b_seg[i], boff);
    c.C = const_cast<char*>(byte_off(g.C, (g.trans_c ? (int64_t)lo * g.ldc : (int64_t)lo) * cbytes));
    if (g.colsum != nullptr) c.colsum = g.colsum + lo;
    if (t0 > 0) c.at = nullptr;  // every chunk holds the whole A: the first one emits A^T
    c.bias = byte_off(g.bias, (int64_t)lo * 2);
    c.aux = const_cast<char*>(byte_off(g.aux, (int64_t)lo * 2));
    c.res = byte_off(g.res, (int64_t)lo * 2);
    c.dact_in = byte_off(g.dact_in, g.dact == kActReluBits ? (int64_t)lo / 8 : (int64_t)lo * 2);
    c.bits = const_cast<char*>(byte_off(g.bits, (int64_t)lo / 8));
  } else {
    c.M = hi - lo;
    c.mask_row0 = g.mask_row0 + lo;
    if (g.rowsum != nullptr) c.rowsum = g.rowsum + lo;
    const int64_t aoff = (g.a_kc ? (int64_t)lo * g.lda : (int64_t)lo) * 2;
    c.A = byte_off(g.A, aoff);
    for (int i = 0; i < GemmArgs::kMaxSegs; ++i) c.a_seg[i] = byte_off(g.a_seg[i], aoff);
    c.C = const_cast<char*>(byte_off(g.C, (g.trans_c ? (int64_t)lo : (int64_t)lo * g.ldc) * cbytes));
    c.at = const_cast<char*>(byte_off(g.at, (int64_t)lo * 2));  // A^T columns of this chunk's rows
    c.aux = const_cast<char*>(byte_off(g.aux, (int64_t)lo * g.ldc * 2));
    c.res = byte_off(g.res, (int64_t)lo * g.ldr * 2);
    c.dact_in = byte_off(g.dact_in, (int64_t)lo * g.ldd * (g.dact == kActReluBits ? 1 : 2));
    c.bits = const_cast<char*>(byte_off(g.bits, (int64_t)lo * g.ldbits));
  }
  return c;
}

// Every launch of g the plan asks for: one, or one per chunk.  Only the bf16 store pass has an activation.
void launch_planned(const GemmArgs& g, hipStream_t s) {
  const GemmPlan p = gemm_plan(g);
  with_layout(g.a_kc, g.b_kc, [&](auto a_kc, auto b_kc) {
    with_int<kEpiStoreBf16, kEpiAccumF32, kEpiStoreF32>(g.epi, [&](auto epi) {
      constexpr int EPI = decltype(epi)::value;
      with_int<kActRelu, kActGelu, kActNone>(EPI == kEpiStoreBf16 ? g.act : kActNone, [&](auto act) {
        constexpr int ACT = decltype(act)::value;
        if constexpr (EPI == kEpiStoreBf16 || ACT == kActNone) {
          constexpr bool A_KC = decltype(a_kc)::value, B_KC = decltype(b_kc)::value;
          if (!p.by_rounds) launch_one<A_KC, B_KC, EPI, ACT>(p, g, s);
          for (int i = 0; p.by_rounds && i < p.chunks; ++i) launch_one<A_KC, B_KC, EPI, ACT>(p, round_chunk(g, p, i), s);
        }
      });
    });
  });
}

}  // namespace

void gemm_set_width(int w) { g_knobs.width = w; }
void gemm_set_rounds(int on) { g_knobs.rounds = on; }
void gemm_set_splitk(int n) { g_knobs.splitk = n; }

bool gemm_emit_ok(int act, float p, bool aux) { return !(act == kActGelu && (p > 0.f || aux)); }

bool gemm_supported(int64_t M, int64_t N, int64_t K) {
  // 16-byte operand chunks along M/N (I-contiguous layouts) and whole 64-deep K tiles.
  // ... and 32-bit per-lane staging offsets: a K-contiguous operand spans < 4 GiB.
  return M >= 8 && N >= 8 && K > 0 && M % 8 == 0 && N % 8 == 0 && K % BK == 0 && M < (1LL << 30) &&
         N < (1LL << 30) && M * K < (1LL << 31) && N * K < (1LL << 31);
}

// The rules, and the measurements behind them, are in the table above GemmKnobs.
GemmPlan gemm_plan(const GemmArgs& g) {
  const bool bf16 = g.epi == kEpiStoreBf16, f32_out = g.epi == kEpiAccumF32 || g.epi == kEpiStoreF32;
  const int tm = (g.M + 255) / 256, tn = (g.N + 255) / 256;
  GemmPlan p;
  p.big = plan_big(g);                  // 1
  p.k_splits = plan_splits(g, p.big);   // 2
  p.width = plan_width(g, g.k_splits);  // 3
  if (p.big) {                          // 4
    p.extra = bf16 && (g.p > 0.f || g.aux != nullptr);
    if (bf16 && !p.extra)
      p.side = g.dact_in != nullptr ? (g.dact == kActReluBits ? big::kSideBits : big::kSideSaved)
                                    : (g.res != nullptr ? big::kSideRes : big::kSideNone);
    if (p.side != big::kSideNone) {
      const bool fwd = g.a_kc && g.b_kc && p.side == big::kSideRes;
      const bool dgrad = g.a_kc && !g.b_kc && g.act == kActNone && g.at == nullptr && g.bias == nullptr;
      p.kernel = fwd || dgrad;
      if (fwd && g.at != nullptr) p.x = big::kXEmit;
    } else if (g.at != nullptr && g.a_kc && g.b_kc && bf16 && gemm_emit_ok(g.act, g.p, g.aux != nullptr)) {
      p.x = big::kXEmit;
    } else if (g.colsum != nullptr && g.a_kc && !g.b_kc && !bf16) {
      p.x = big::kXColsum;
    }
  }
  const int last = (tm * tn) % 256;     // 5
  if (g_knobs.rounds != 0 && g.k_splits <= 1 && p.big && p.width == 256 && !(g_knobs.rounds == 1 && g.K < 4096) &&
      tm * tn > 256 && last != 0 && last <= 128) {
    const bool along_n = tn >= tm;
    const int per = 256 / (along_n ? tm : tn), chunks = per < 1 ? 0 : ((along_n ? tn : tm) + per - 1) / per;
    if ((along_n ? g.rowsum : g.colsum) == nullptr && per >= 1 && chunks <= 16) {
      p.by_rounds = true;
      p.along_n = along_n;
      p.per = per;
      p.chunks = chunks;
    }
  }
  p.rowsum_ok = !g.a_kc && f32_out && p.big && p.k_splits <= 1 && (g.N + p.width - 1) / p.width >= 16;  // 6
  p.colsum_ok = g.a_kc && !g.b_kc && f32_out && 2 * tm * 128 >= plan_width(g, p.k_splits);
  p.bits_ok = bf16 && g.act == kActRelu && g.p > 0.f && g.k_splits <= 1 && g.N % 8 == 0 && p.big;
  return p;
}

void gemm_bf16(const GemmArgs& gi, hipStream_t s) {
  GemmArgs g = gi;
  g.threshold = dropout_threshold(g.p);
  if (g.ldr == 0) g.ldr = g.ldc;
  if (g.ldd == 0) g.ldd = g.ldc;
  if (g.k_splits <= 1) {
    launch_planned(g, s);
    return;
  }
  // fp32 partials into the caller's workspace, then one reduction (+ res)
  GemmArgs p = g;
  p.epi = kEpiStoreF32;
  p.C = g.ws;
  p.ldc = g.N;
  p.res = nullptr;
  p.trans_c = false;  // partials row-major; the reduction transposes
  p.rowsum = nullptr;
  p.colsum = g.colsum != nullptr ? g.colsum_ws : nullptr;  // per-split column sums [k_splits][N]
  launch_planned(p, s);
  if (g.epi == kEpiStoreBf16) {
    const int64_t chunks = (int64_t)g.M * (g.N / 8);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, g.ws,
                       g.k_splits, g.M, g.N, g.ldc, reinterpret_cast<const bf16_t*>(g.res), g.ldr,
                       reinterpret_cast<bf16_t*>(g.C));
  } else {
    const int64_t chunks = (int64_t)g.M * (g.N / 4);  // = (M / 4) * N items when transposed
    hipLaunchKernelGGL(splitk_reduce_f32_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, g.ws,
                       g.k_splits, g.M, g.N, g.ldc, g.epi == kEpiAccumF32, g.trans_c, reinterpret_cast<float*>(g.C));
    if (g.colsum != nullptr)
      hipLaunchKernelGGL(colsum_splits_kernel, dim3((unsigned)((g.N + 255) / 256)), dim3(256), 0, s, g.colsum_ws,
                         g.k_splits, g.N, g.colsum);
  }
}

}  // namespace mipipe
