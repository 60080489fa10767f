// Flash attention for gfx950: forward, and backward as two kernels (dK/dV and
// dQ) plus a delta pre-pass.
//
// Layout: Q, K, V are read in place from the packed QKV projection output
// [B, S, 3, H, D] (token stride 3*H*D) and O / dO are [B, S, H, D]; the
// backward writes dQ, dK, dV straight into the packed dQKV buffer, so no
// transpose or concatenation ever touches HBM.
//
// Tiling: a workgroup = 4 waves = 64 query rows (forward, dQ) or 64 keys
// (dK/dV), 16 rows per wave on v_mfma_f32_16x16x32_bf16.  The streamed
// operand tiles (64 x D) are staged into LDS row-major with an XOR chunk
// swizzle that serves both the 16-byte row reads (ds_read_b128, B operand of
// Q.K^T / dO.V^T) and the transposing reads (ds_read_b64_tr_b16, B operand of
// P.V / dS.K / P^T.dO / dS^T.Q) from ONE image (T10 'one image for row reads
// and transposed reads').  Softmax probabilities take one LDS round trip per
// tile to move from the accumulator layout to the A-operand layout.
//
// Online softmax in fp32 with exp2; causal tiles above the diagonal are
// skipped entirely; attention dropout uses Philox keyed by (batch*head,
// query/4, key) -- word (query & 3) -- so forward, dQ and dK/dV regenerate the
// same mask without storing it.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace mipipe {

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int kRows = 64;      // rows per workgroup tile and per streamed tile
constexpr int kThreads = 256;  // 4 waves
constexpr float kLog2e = 1.4426950408889634f;

template <int D>
struct Img {
  static constexpr int kRowBytes = 2 * D;
  static constexpr int kChunks = D / 8;          // 16-byte chunks per row
  static constexpr int kBytes = kRows * kRowBytes;
  // 16-byte chunk c of row r sits at chunk c ^ f(r).  f is chosen (exhaustive
  // search over the linear maps of r mod 16, tools/lds_swizzle_check.py) so that
  // the three access patterns of these images are bank-conflict free on CDNA4:
  //   * row-fragment ds_read_b128 (rows rb + 0..15, chunks 4 s + 0..3): the 16-lane
  //     groups {0-3,12-15,20-27} etc. read rows {0-3,12-15} at chunk c and rows
  //     4-11 at c ^ 1 -- 16 distinct 16-byte slots of the 256-byte bank row;
  //   * column-fragment ds_read_b64_tr_b16 (rows 8 g + q (+4), 32-byte column
  //     strips): 32-lane halves cover 16 distinct slots;
  //   * the scattered bf16 writes of the S = 128 kernels (P~ / dS, and the
  //     backward's outputs staged through the chunk images).
  // The previous map ((r & 3) << 2 | (r >> 2) & 3, masked) cost 4 extra cycles
  // per ds_read_b128 on 256- and 512-byte rows and 12 (+ 2 per transposing read)
  // on the 128-byte rows of D = 64 / the S = 128 kernels' chunk images.
  __device__ static __forceinline__ int f(int r) {
    if constexpr (kChunks >= 16) return (((r ^ (r >> 2)) & 1) << 1) | ((r & 2) << 1) | (r & 8);
    else if constexpr (kChunks == 8) return ((((r >> 1) ^ (r >> 2)) & 1) << 1) | ((r >> 1) & 4);
    else return (((r & 3) << 2) | ((r >> 2) & 3)) & (kChunks - 1);
  }
  __device__ static __forceinline__ int off(int r, int c16) { return r * kRowBytes + ((c16 ^ f(r)) << 4); }
};

// Stage a 64 x D tile (rows t0.., row stride `ld` elements) into LDS.
template <int D>
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ base, int64_t ld, char* img, int tid) {
  constexpr int kPer = kRows * Img<D>::kChunks / kThreads;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int id = tid + u * kThreads;
    const int r = id / Img<D>::kChunks, c = id % Img<D>::kChunks;
    const uint4 v = *reinterpret_cast<const uint4*>(base + (int64_t)r * ld + c * 8);
    *reinterpret_cast<uint4*>(img + Img<D>::off(r, c)) = v;
  }
}

// Register prefetch of a 64 x D tile (T14): the next tile's global loads are
// issued right after the barrier that publishes the current one, so they are
// in flight during the current tile's MFMAs; the LDS write follows the next
// barrier.  Used for D <= 128 (D = 256 has no registers to spare).
// (named registers, not an array: a loop-carried uint4[] was kept in scratch)
struct TileRegs {
  uint4 r0, r1, r2, r3;
};
template <int D>
__device__ __forceinline__ uint4 load_piece(const bf16_t* __restrict__ base, int64_t ld, int tid, int u) {
  const int id = tid + u * kThreads;
  const int r = id / Img<D>::kChunks, c = id % Img<D>::kChunks;
  return *reinterpret_cast<const uint4*>(base + (int64_t)r * ld + c * 8);
}
template <int D>
__device__ __forceinline__ void store_piece(char* img, int tid, int u, const uint4& v) {
  const int id = tid + u * kThreads;
  *reinterpret_cast<uint4*>(img + Img<D>::off(id / Img<D>::kChunks, id % Img<D>::kChunks)) = v;
}
template <int D>
__device__ __forceinline__ void load_tile(const bf16_t* __restrict__ base, int64_t ld, int tid, TileRegs& t) {
  constexpr int P = kRows * Img<D>::kChunks / kThreads;
  static_assert(P <= 4, "register prefetch holds at most 4 pieces per thread");
  t.r0 = load_piece<D>(base, ld, tid, 0);
  if constexpr (P > 1) t.r1 = load_piece<D>(base, ld, tid, 1);
  if constexpr (P > 2) t.r2 = load_piece<D>(base, ld, tid, 2);
  if constexpr (P > 3) t.r3 = load_piece<D>(base, ld, tid, 3);
}
template <int D>
__device__ __forceinline__ void store_tile(char* img, int tid, const TileRegs& t) {
  constexpr int P = kRows * Img<D>::kChunks / kThreads;
  store_piece<D>(img, tid, 0, t.r0);
  if constexpr (P > 1) store_piece<D>(img, tid, 1, t.r1);
  if constexpr (P > 2) store_piece<D>(img, tid, 2, t.r2);
  if constexpr (P > 3) store_piece<D>(img, tid, 3, t.r3);
}

// B-operand fragment where B[k = d][n = row]: the n index is the image row
// (16 rows from rb), k = 32 s + 8 (lane >> 4) + j is the column  -> row read.
template <int D>
__device__ __forceinline__ bf16x8 frag_rows(const char* img, int rb, int s, int lane) {
  const int r = rb + (lane & 15);
  const int c = 4 * s + (lane >> 4);
  return *reinterpret_cast<const bf16x8*>(img + Img<D>::off(r, c));
}

// B-operand fragment where B[k = row][n = d]: k = 32 s + 8 g + j over image
// rows, n = db + (lane & 15) over columns -> two transposing reads.
template <int D>
__device__ __forceinline__ bf16x8 frag_cols(const char* img, int db, int s, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * s + 8 * g + q;
  const int c8 = (db >> 2) + p;
  const int o0 = Img<D>::off(r0, c8 >> 1) + 8 * (c8 & 1);
  const int o1 = Img<D>::off(r0 + 4, c8 >> 1) + 8 * (c8 & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o1));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// A-operand fragment straight from global memory: row (lane & 15) of a
// 16-row slab, k = 32 s + 8 (lane >> 4) + j.
__device__ __forceinline__ bf16x8 frag_global(const bf16_t* __restrict__ rowp, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(rowp + 32 * s + 8 * (lane >> 4));
}

// Per-wave scratch for the accumulator -> A-operand relayout of a 16 x 64
// tile M (lane (g = lane >> 4, c = lane & 15) holds M[4g + r][16j + c]).
// M is stored TRANSPOSED, T[col][row] (64 rows of 16 bf16 = 32 bytes), so a
// lane's 4 values M[4g .. 4g+3][col] are one contiguous 8-byte ds_write_b64
// (4 per tile instead of 16 ds_write_b16), and the A fragment (row c, k =
// 32 s + 8 g + 0..7) is a column of T: two ds_read_b64_tr_b16.
//   * rows are placed at phi(col) (bits 2 and 3 swapped), so the 8 rows a
//     32-lane group of a transposing read touches ({0-3, 8-11} + 16 t and
//     {4-7, 12-15} + 16 t) fill 256 contiguous bytes: all 64 banks once;
//   * the 8-byte chunk g of row col sits at chunk g ^ ((col >> 2) & 3), so
//     the 16 lanes of a ds_write_b64 group (cols 16 j + 0..15) hit 16
//     distinct 8-byte bank pairs of a 128-byte window.
// 2 KiB per tile (the 16 x 68 regions the kernels allocate hold it).
constexpr int kScrStride = 68;  // elements (region size unit: 16 * kScrStride per tile)
__device__ __forceinline__ int scr_row(int col) { return (col & ~12) | ((col & 4) << 1) | ((col & 8) >> 1); }
__device__ __forceinline__ int scr_off(int col, int chunk) { return scr_row(col) * 32 + ((chunk ^ ((col >> 2) & 3)) << 3); }
__device__ __forceinline__ void scratch_write(bf16_t* scr, const float (&v)[4][4], int lane) {
  const int g = lane >> 4, c = lane & 15;
  char* base = reinterpret_cast<char*>(scr);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t lo = (uint32_t)f2bf(v[j][0]) | ((uint32_t)f2bf(v[j][1]) << 16);
    const uint32_t hi = (uint32_t)f2bf(v[j][2]) | ((uint32_t)f2bf(v[j][3]) << 16);
    *reinterpret_cast<uint2*>(base + scr_off(16 * j + c, g)) = make_uint2(lo, hi);
  }
}
__device__ __forceinline__ bf16x8 scratch_frag(const bf16_t* scr, int s, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * s + 8 * g + q;
  const char* base = reinterpret_cast<const char*>(scr);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + scr_off(r0, p)));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + scr_off(r0 + 4, p)));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

__device__ __forceinline__ uint4 attn_mask_words(const AttnArgs& a, int bh, int q4, int key) {
  const uint64_t sub = ((uint64_t)bh * (uint64_t)(a.S >> 2) + (uint64_t)q4) * (uint64_t)a.S + (uint64_t)key;
  return Philox(a.seed, sub, a.offset).next4();
}

__device__ __forceinline__ float row_reduce_max16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float row_reduce_sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------ logit soft-capping
// SOFTCAP: the score s = scale * (q . k) becomes c * tanh(s / c) (c = a.softcap > 0) before the masks and the
// softmax.  With e = exp2(raw * cap_in), cap_in = 2 * scale * log2e / c, tanh(s / c) = 1 - 2 / (1 + e): one
// exp2 and one rcp, no division.  e = inf gives r = 0 and t = 1, e = 0 gives r = 1 and t = -1: no NaN at either
// end.  The absolute fp32 error of t is about 2e-7 (the cancellation in 1 - 2r near s = 0 is against 1, not
// against t), so the capped score is off by about c * 2e-7: negligible against bf16 P for c up to a few hundred,
// and growing with c.  Returns r; t = 1 - 2r, and the derivative 1 - t^2 = 4 r (1 - r).
__device__ __forceinline__ float softcap_r(float raw, float cap_in) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(raw * cap_in));
}

// ------------------------------------------------------------------ document masks
// DOCS (only with CAUSAL): packed sequences.  Query i sees the keys [lo(i), i], lo(i) = max(i - a.window + 1,
// doc_start[i]); key j is seen by the queries [j, hi(j)), hi(j) = min(j + a.window, doc_end[j]).  The window is
// merged at run time (the host passes a.window = S when there is none), so DOCS does not multiply with WINDOW.
// doc_start and doc_end are non-decreasing along a row, so a tile's first query row has the tile's smallest
// lower edge and a tile's last key the largest upper edge: the tile-loop bounds are one uniform load per block.
// They come from a tensor, so both are clamped to the range the causal loop visits -- a malformed tensor gives
// wrong numbers, never an access outside q, k, v, lse or delta.
__device__ __forceinline__ int doc_tbeg(const AttnArgs& a, int b, int q0, int qt) {
  const int lo = max(q0 - a.window + 1, a.doc_start[(int64_t)b * 2 * a.S + q0]);
  return min(max(lo, 0) / kRows, qt);  // first key tile row q0 sees, in [0, qt]
}
__device__ __forceinline__ int doc_nq(const AttnArgs& a, int b, int k0, int kt) {
  const int hi = min(k0 + kRows - 1 + a.window, a.doc_end[(int64_t)b * 2 * a.S + k0 + kRows - 1]);
  // one past the last query tile, in [kt + 1, S / 64]
  return min(max((max(hi, 1) - 1) / kRows + 1, kt + 1), a.S / kRows);
}
// The bounds of a lane's four rows row0 .. row0 + 3 (row0 % 4 == 0) in one 16-byte load.
__device__ __forceinline__ int4 doc_rows4(const int32_t* bounds, const AttnArgs& a, int b, int row0) {
  return *reinterpret_cast<const int4*>(bounds + (int64_t)b * 2 * a.S + row0);
}

// ------------------------------------------------------------------ forward
// SOFTCAP: the capped score (softcap_r) replaces the scaled one; lse is the log-sum-exp of the capped scores.
// WINDOW (only with CAUSAL): sliding-window attention, query i sees the a.window keys (i - a.window, i].  The
// key-tile loop then starts at the first tile that holds a visible key of the tile's first query row instead of
// at 0; the tiles wholly below the band are never loaded.  A later row of the query tile can find the first
// visited tile wholly masked: its running max stays -inf there and the m == -inf guards below give alpha = 0 and
// p = 0, as they do for a fresh row, so exp2 never sees (-inf) - (-inf).
// DOCS (only with CAUSAL, see above): the loop starts at the tile of lo(q0); the mask is key < lo(row).  The same
// guards cover a later row whose document starts after the first visited tile.
// SINK: a.sinks[h] joins the normalisation once, after the key-tile loop (see the epilogue); the loop is the
// sinkless one, and so are the dropout mask and the backward kernels, which read the lse stored here.
template <int D, bool CAUSAL, bool WINDOW = false, bool SOFTCAP = false, bool DOCS = false, bool SINK = false>
__global__ void __launch_bounds__(kThreads, D == 256 ? 1 : 2) attn_fwd_kernel(AttnArgs a) {
  static_assert(!WINDOW || CAUSAL, "the sliding window is a band of the causal mask");
  static_assert(!DOCS || (CAUSAL && !WINDOW), "documents mask the causal triangle and merge the window at run time");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kimg = smem;
  char* vimg = smem + Img<D>::kBytes;
  bf16_t* scr_all = reinterpret_cast<bf16_t*>(smem + 2 * Img<D>::kBytes);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = blockIdx.x;          // query tile
  const int bh = blockIdx.y;          // batch * head
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = qt * kRows;
  bf16_t* scr = scr_all + wave * 16 * kScrStride;

  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + (int64_t)b * a.sb_qkv + (int64_t)h * a.sh_qkv;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;
  const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;

  // Q fragments of this wave's 16 rows (A operand), kept in registers.
  constexpr int NS = D / 32;
  bf16x8 qf[NS];
  const bf16_t* qrow = Q + (int64_t)(q0 + wave * 16 + (lane & 15)) * a.ld_qkv;
#pragma unroll
  for (int s = 0; s < NS; ++s) qf[s] = frag_global(qrow, s, lane);

  constexpr int ND = D / 16;
  f32x4 o[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
  const float sl2 = a.scale * kLog2e;
  const float pscale = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const int qrow0 = q0 + wave * 16 + 4 * (lane >> 4);  // this lane's rows qrow0 .. +3
  const int ntiles = CAUSAL ? qt + 1 : a.S / kRows;
  const int tbeg = DOCS ? doc_tbeg(a, b, q0, qt)
                        : (WINDOW ? max(0, q0 - a.window + 1) / kRows : 0);  // first tile with a key row q0 sees
  const int wrow0 = WINDOW ? qrow0 - a.window : 0;                  // row qrow0 + r sees keys > wrow0 + r
  int dlo[4] = {0, 0, 0, 0};                                        // DOCS: row qrow0 + r sees keys >= dlo[r]
  if constexpr (DOCS) {
    const int4 st = doc_rows4(a.doc_start, a, b, qrow0);
    dlo[0] = max(qrow0 - a.window + 1, st.x);
    dlo[1] = max(qrow0 - a.window + 2, st.y);
    dlo[2] = max(qrow0 - a.window + 3, st.z);
    dlo[3] = max(qrow0 - a.window + 4, st.w);
  }
  const float cap_in = SOFTCAP ? 2.f * sl2 / a.softcap : 0.f;       // raw score -> exponent of e (softcap_r)
  const float cap_l2 = SOFTCAP ? a.softcap * kLog2e : 0.f;          // t -> capped score, log2 domain

  constexpr bool PF = D <= 128;
  TileRegs kr, vr;
  if constexpr (PF) {
    load_tile<D>(K + (int64_t)tbeg * kRows * a.ld_qkv, a.ld_qkv, tid, kr);
    load_tile<D>(V + (int64_t)tbeg * kRows * a.ld_qkv, a.ld_qkv, tid, vr);
  }
  for (int t = tbeg; t < ntiles; ++t) {
    const int k0 = t * kRows;
    __syncthreads();
    if constexpr (PF) {
      store_tile<D>(kimg, tid, kr);
      store_tile<D>(vimg, tid, vr);
    } else {
      stage_tile<D>(K + (int64_t)k0 * a.ld_qkv, a.ld_qkv, kimg, tid);
      stage_tile<D>(V + (int64_t)k0 * a.ld_qkv, a.ld_qkv, vimg, tid);
    }
    __syncthreads();
    if constexpr (PF) if (t + 1 < ntiles) {
      load_tile<D>(K + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, kr);
      load_tile<D>(V + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, vr);
    }

    f32x4 sacc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], frag_rows<D>(kimg, 16 * j, s, lane), sacc[j], 0, 0, 0);

    // online softmax (log2 domain)
    float sv[4][4];
    float tmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = k0 + 16 * j + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x;
        if constexpr (SOFTCAP) x = (1.f - 2.f * softcap_r(sacc[j][r], cap_in)) * cap_l2;
        else x = sacc[j][r] * sl2;
        if (CAUSAL && key > qrow0 + r) x = -INFINITY;
        if (WINDOW && key <= wrow0 + r) x = -INFINITY;
        if (DOCS && key < dlo[r]) x = -INFINITY;
        sv[j][r] = x;
        tmax[r] = fmaxf(tmax[r], x);
      }
    }
    float alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mx = row_reduce_max16(tmax[r]);
      const float mn = fmaxf(m[r], mx);
      alpha[r] = m[r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[r] - mn);
      m[r] = mn;
    }
    float psum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
      if (a.p > 0.f) {
        const uint4 mw = attn_mask_words(a, bh, qrow0 >> 2, k0 + 16 * j + (lane & 15));
        w[0] = mw.x; w[1] = mw.y; w[2] = mw.z; w[3] = mw.w;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = m[r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sv[j][r] - m[r]);
        psum[r] += pr;
        sv[j][r] = (a.p > 0.f) ? (w[r] >= a.threshold ? pr * pscale : 0.f) : pr;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) l[r] = l[r] * alpha[r] + row_reduce_sum16(psum[r]);
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[t2][r] *= alpha[r];

    scratch_write(scr, sv, lane);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's scratch writes done
    const bf16x8 p0 = scratch_frag(scr, 0, lane);
    const bf16x8 p1 = scratch_frag(scr, 1, lane);
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2) {
      o[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p0, frag_cols<D>(vimg, 16 * t2, 0, lane), o[t2], 0, 0, 0);
      o[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p1, frag_cols<D>(vimg, 16 * t2, 1, lane), o[t2], 0, 0, 0);
    }
  }

  // epilogue: O / l (bf16) and lse (natural log) per row
  bf16_t* O = reinterpret_cast<bf16_t*>(a.o) + (int64_t)b * a.sb_o + (int64_t)h * a.sh_o;
  // SINK: one more term of the online softmax, with no value vector: m' = max(m, sink), l' = l * c + exp2(sink -
  // m'), c = exp2(m - m'), and o scaled by c / l'.  A sink of -inf gives m' = m, c = 1 and l' = l + 0, so every
  // stored bit is the sinkless kernel's; a sink far above m gives c -> 0 and l' = 1, so o -> 0 and lse = sink,
  // all finite; a row that saw no key (m = -inf) has c = 0 by the guard, l' = 1, o = 0 and lse = sink.
  float rescale[4] = {1.f, 1.f, 1.f, 1.f};
  if constexpr (SINK) {
    const float s2 = a.sinks[h] * kLog2e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m[r], s2);
      rescale[r] = m[r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[r] - mn);
      const float es = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(s2 - mn);
      l[r] = l[r] * rescale[r] + es;
      m[r] = mn;
    }
  }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    inv[r] = l[r] > 0.f ? 1.f / l[r] : 0.f;
    if constexpr (SINK) inv[r] *= rescale[r];
  }
#pragma unroll
  for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      O[(int64_t)(qrow0 + r) * a.ld_o + 16 * t2 + (lane & 15)] = f2bf(o[t2][r] * inv[r]);
  if ((lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      a.lse[(int64_t)bh * a.S + qrow0 + r] = (m[r] + log2f(l[r] > 0.f ? l[r] : 1.f)) / kLog2e;
  }
}

// ------------------------------------------------------------------ forward, D = 64, 32 rows per wave
// At D = 64 the 16-row kernel above is LDS-bound: per 64-key tile a wave
// reads 16 KiB of K/V fragments for only 16 MFMAs (128 LDS clocks against 64
// MFMA clocks per CU).  Here each wave owns TWO 16-row blocks (a workgroup =
// 128 query rows) and every K/V fragment read from LDS feeds both, halving
// LDS traffic per MFMA.  The softmax is trimmed to what the tile needs:
//   * row max over the 16 lanes of a row by 4 DPP steps (quad_perm xor 1,
//     xor 2, row_half_mirror, row_mirror) instead of ds_bpermute shuffles;
//   * the row sum l stays a per-lane partial (alpha is uniform along a row)
//     and is reduced once after the last tile;
//   * causal masking is applied only to tiles that cross this wave's
//     diagonal, and tiles wholly above it are skipped (barriers kept);
//   * causal query tiles are issued longest-first, so the short ones fill the
//     tail of the grid.
// The dropout mask, lse and O are bit-compatible with attn_fwd_kernel (same
// Philox keying), so the backward kernels are unchanged.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_max16_dpp(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_mov<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_mov<0x141>(v));  // row_half_mirror
  v = fmaxf(v, dpp_mov<0x140>(v));  // row_mirror
  return v;
}

constexpr int kWideRows = 128;  // query rows per workgroup of the wide kernel

template <bool CAUSAL>
__global__ void __launch_bounds__(kThreads, 2) attn_fwd_wide_kernel(AttnArgs a) {
  constexpr int D = 64, NS = 2, ND = 4, RB = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kimg = smem;
  char* vimg = smem + Img<D>::kBytes;
  bf16_t* scr_all = reinterpret_cast<bf16_t*>(smem + 2 * Img<D>::kBytes);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = CAUSAL ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = qt * kWideRows;
  const int wrow0 = q0 + wave * 32;  // this wave's rows wrow0 .. wrow0 + 31

  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + (int64_t)b * a.sb_qkv + (int64_t)h * a.sh_qkv;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;
  const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;

  bf16x8 qf[RB][NS];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const bf16_t* qrow = Q + (int64_t)(wrow0 + 16 * rb + (lane & 15)) * a.ld_qkv;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[rb][s] = frag_global(qrow, s, lane);
  }
  f32x4 o[RB][ND];
  float m[RB][4], l[RB][4];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
    for (int t = 0; t < ND; ++t) o[rb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[rb][r] = -INFINITY;
      l[rb][r] = 0.f;
    }
  }
  const float sl2 = a.scale * kLog2e;
  const float pscale = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const int ntiles = CAUSAL ? (q0 + kWideRows) / kRows : a.S / kRows;

  TileRegs kr, vr;
  load_tile<D>(K, a.ld_qkv, tid, kr);
  load_tile<D>(V, a.ld_qkv, tid, vr);
  for (int t = 0; t < ntiles; ++t) {
    const int k0 = t * kRows;
    __syncthreads();
    store_tile<D>(kimg, tid, kr);
    store_tile<D>(vimg, tid, vr);
    __syncthreads();
    if (t + 1 < ntiles) {
      load_tile<D>(K + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, kr);
      load_tile<D>(V + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, vr);
    }
    if (CAUSAL && k0 > wrow0 + 31) continue;  // wholly above this wave's diagonal
    const bool diag = CAUSAL && k0 + kRows - 1 > wrow0;

    f32x4 sacc[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int j = 0; j < 4; ++j) sacc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 kf = frag_rows<D>(kimg, 16 * j, s, lane);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          sacc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[rb][s], kf, sacc[rb][j], 0, 0, 0);
      }

    bf16x8 pf[RB][2];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int qrow0 = wrow0 + 16 * rb + 4 * (lane >> 4);
      float sv[4][4];
      float tmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = k0 + 16 * j + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = sacc[rb][j][r] * sl2;
          if (diag && key > qrow0 + r) x = -INFINITY;
          sv[j][r] = x;
          tmax[r] = fmaxf(tmax[r], x);
        }
      }
      float alpha[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mn = fmaxf(m[rb][r], row_max16_dpp(tmax[r]));
        alpha[r] = m[rb][r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[rb][r] - mn);
        m[rb][r] = mn;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (a.p > 0.f) {
          const uint4 mw = attn_mask_words(a, bh, qrow0 >> 2, k0 + 16 * j + (lane & 15));
          w[0] = mw.x; w[1] = mw.y; w[2] = mw.z; w[3] = mw.w;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = m[rb][r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sv[j][r] - m[rb][r]);
          l[rb][r] = (j == 0 ? l[rb][r] * alpha[r] : l[rb][r]) + pr;
          sv[j][r] = (a.p > 0.f) ? (w[r] >= a.threshold ? pr * pscale : 0.f) : pr;
        }
      }
#pragma unroll
      for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[rb][t2][r] *= alpha[r];
      bf16_t* scr = scr_all + (wave * RB + rb) * 16 * kScrStride;
      scratch_write(scr, sv, lane);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's scratch writes done
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const bf16_t* scr = scr_all + (wave * RB + rb) * 16 * kScrStride;
      pf[rb][0] = scratch_frag(scr, 0, lane);
      pf[rb][1] = scratch_frag(scr, 1, lane);
    }
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 vf = frag_cols<D>(vimg, 16 * t2, s, lane);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          o[rb][t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[rb][s], vf, o[rb][t2], 0, 0, 0);
      }
  }

  bf16_t* O = reinterpret_cast<bf16_t*>(a.o) + (int64_t)b * a.sb_o + (int64_t)h * a.sh_o;
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int qrow0 = wrow0 + 16 * rb + 4 * (lane >> 4);
    float inv[4], lt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lt[r] = row_reduce_sum16(l[rb][r]);
      inv[r] = lt[r] > 0.f ? 1.f / lt[r] : 0.f;
    }
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        O[(int64_t)(qrow0 + r) * a.ld_o + 16 * t2 + (lane & 15)] = f2bf(o[rb][t2][r] * inv[r]);
    if ((lane & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        a.lse[(int64_t)bh * a.S + qrow0 + r] = (m[rb][r] + log2f(lt[r] > 0.f ? lt[r] : 1.f)) / kLog2e;
    }
  }
}
size_t wide_fwd_smem() { return 2 * Img<64>::kBytes + 4 * 2 * 16 * kScrStride * 2; }

// ------------------------------------------------------------------ delta = rowsum(dO * O)
__global__ void __launch_bounds__(256) attn_delta_kernel(AttnArgs a, int D) {
  // one wave per (b, s, h) row
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t total = (int64_t)a.B * a.S * a.H;
  if (row >= total) return;
  const int h = (int)(row % a.H);
  const int64_t bs = row / a.H;  // b * S + s
  const int64_t ob = (bs / a.S) * a.sb_o + (bs % a.S) * a.ld_o + (int64_t)h * a.sh_o;
  const bf16_t* o = reinterpret_cast<const bf16_t*>(a.o) + ob;
  const bf16_t* d = reinterpret_cast<const bf16_t*>(a.dout) + ob;
  float acc = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const u16x4 ov = *reinterpret_cast<const u16x4*>(o + c);
    const u16x4 dv = *reinterpret_cast<const u16x4*>(d + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc += bf2f(ov[i]) * bf2f(dv[i]);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const int b = (int)(bs / a.S), s = (int)(bs % a.S);
    a.delta[((int64_t)b * a.H + h) * a.S + s] = acc;
  }
}

// ------------------------------------------------------------------ delta on the MFMA (the windowed backward)
// delta_i = dO_i . O_i as the diagonal of a 16 x 16 MFMA tile of dO rows against O rows: the same instruction,
// operand layout and k order that give dP_ij = dO_i . V_j in the dQ and dK/dV kernels.  Where a query attends a
// single key (the first row of every sequence; every row at window = 1) O_i is V_j bit for bit, so delta_i equals
// dP_ij bit for bit and dS = P (dP - delta) is exactly 0, as in exact arithmetic -- attn_delta_kernel adds the
// same products in another order and leaves an ulp of |dO . V| there.  15 of the 16 columns of each tile are not
// used; the kernel stays bound by its reads of O and dO.  One wave per 16 rows, a workgroup per 64.
template <int D>
__global__ void __launch_bounds__(kThreads) attn_delta_mfma_kernel(AttnArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bh = blockIdx.y;
  const int b = bh / a.H, h = bh % a.H;
  const int row0 = blockIdx.x * kRows + wave * 16;
  const int64_t base = (int64_t)b * a.sb_o + (int64_t)h * a.sh_o + (int64_t)(row0 + (lane & 15)) * a.ld_o;
  const bf16_t* o = reinterpret_cast<const bf16_t*>(a.o) + base;
  const bf16_t* d = reinterpret_cast<const bf16_t*>(a.dout) + base;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < D / 32; ++s)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_global(d, s, lane), frag_global(o, s, lane), acc, 0, 0, 0);
  // lane (g = lane >> 4, c = lane & 15) holds M[4g + r][c]: the diagonal element of column c sits in the lanes
  // with c >> 2 == g, at r = c & 3
  const int g = lane >> 4, c = lane & 15, r = c & 3;
  if ((c >> 2) == g) {
    const float v = r == 0 ? acc[0] : (r == 1 ? acc[1] : (r == 2 ? acc[2] : acc[3]));
    a.delta[(int64_t)bh * a.S + row0 + c] = v;
  }
}

// ------------------------------------------------------------------ dsink
// The sink's probability of row (b, h, i) is exp(sink_h - lse) and it has no value vector (dP = 0), so dS = P (dP
// - delta) gives dsink_h = -sum_{b,i} exp(sink_h - lse[b,h,i]) * delta[b,h,i].  One block per head: each thread
// adds its rows in index order, then a wave butterfly and the four wave sums in order -- no atomics, so the same
// bits on every run.  S % 4 == 0 (16-byte loads inside one row); a sink of -inf adds exp2(-inf) = 0 every time.
__global__ void __launch_bounds__(kThreads) attn_dsink_kernel(const float* __restrict__ lse,
                                                             const float* __restrict__ delta,
                                                             const float* __restrict__ sinks,
                                                             float* __restrict__ dsinks, int B, int H, int S,
                                                             int accumulate) {
  __shared__ float part[kThreads / 64];
  const int h = blockIdx.x, tid = threadIdx.x;
  const float sk = sinks[h];
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const int64_t row = ((int64_t)b * H + h) * S;
    for (int i = tid * 4; i < S; i += kThreads * 4) {
      const float4 lv = *reinterpret_cast<const float4*>(lse + row + i);
      const float4 dv = *reinterpret_cast<const float4*>(delta + row + i);
      acc += __builtin_amdgcn_exp2f((sk - lv.x) * kLog2e) * dv.x;
      acc += __builtin_amdgcn_exp2f((sk - lv.y) * kLog2e) * dv.y;
      acc += __builtin_amdgcn_exp2f((sk - lv.z) * kLog2e) * dv.z;
      acc += __builtin_amdgcn_exp2f((sk - lv.w) * kLog2e) * dv.w;
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const float v = -(((part[0] + part[1]) + part[2]) + part[3]);
    dsinks[h] = accumulate ? dsinks[h] + v : v;
  }
}

// ------------------------------------------------------------------ dQ
// WINDOW, DOCS: the forward's key-tile range and band / document mask (see attn_fwd_kernel).
template <int D, bool CAUSAL, bool WINDOW = false, bool SOFTCAP = false, bool DOCS = false>
__global__ void __launch_bounds__(kThreads, D == 256 ? 1 : 2) attn_dq_kernel(AttnArgs a) {
  static_assert(!WINDOW || CAUSAL, "the sliding window is a band of the causal mask");
  static_assert(!DOCS || (CAUSAL && !WINDOW), "documents mask the causal triangle and merge the window at run time");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kimg = smem;
  char* vimg = smem + Img<D>::kBytes;
  bf16_t* scr_all = reinterpret_cast<bf16_t*>(smem + 2 * Img<D>::kBytes);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = blockIdx.x, bh = blockIdx.y;
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = qt * kRows;
  bf16_t* scr = scr_all + wave * 16 * kScrStride;
  const int64_t boff = (int64_t)b * a.sb_qkv + (int64_t)h * a.sh_qkv;
  const int64_t koff = (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;  // K / V: the group's head
  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + boff;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + koff;
  const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + koff;
  const bf16_t* dO = reinterpret_cast<const bf16_t*>(a.dout) + (int64_t)b * a.sb_o + (int64_t)h * a.sh_o;

  constexpr int NS = D / 32, ND = D / 16;
  bf16x8 qf[NS], df[NS];
  const int myrow = q0 + wave * 16 + (lane & 15);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    qf[s] = frag_global(Q + (int64_t)myrow * a.ld_qkv, s, lane);
    df[s] = frag_global(dO + (int64_t)myrow * a.ld_o, s, lane);
  }
  const int qrow0 = q0 + wave * 16 + 4 * (lane >> 4);
  float lse2[4], dl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lse2[r] = a.lse[(int64_t)bh * a.S + qrow0 + r] * kLog2e;
    dl[r] = a.delta[(int64_t)bh * a.S + qrow0 + r];
  }
  f32x4 dq[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = a.scale * kLog2e;
  const float pscale = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const int ntiles = CAUSAL ? qt + 1 : a.S / kRows;
  const int tbeg = DOCS ? doc_tbeg(a, b, q0, qt)
                        : (WINDOW ? max(0, q0 - a.window + 1) / kRows : 0);  // first tile with a key row q0 sees
  const int wrow0 = WINDOW ? qrow0 - a.window : 0;                  // row qrow0 + r sees keys > wrow0 + r
  int dlo[4] = {0, 0, 0, 0};                                        // DOCS: row qrow0 + r sees keys >= dlo[r]
  if constexpr (DOCS) {
    const int4 st = doc_rows4(a.doc_start, a, b, qrow0);
    dlo[0] = max(qrow0 - a.window + 1, st.x);
    dlo[1] = max(qrow0 - a.window + 2, st.y);
    dlo[2] = max(qrow0 - a.window + 3, st.z);
    dlo[3] = max(qrow0 - a.window + 4, st.w);
  }
  const float cap_in = SOFTCAP ? 2.f * sl2 / a.softcap : 0.f;       // as in attn_fwd_kernel
  const float cap_l2 = SOFTCAP ? a.softcap * kLog2e : 0.f;

  constexpr bool PF = D <= 128;
  TileRegs kr, vr;
  if constexpr (PF) {
    load_tile<D>(K + (int64_t)tbeg * kRows * a.ld_qkv, a.ld_qkv, tid, kr);
    load_tile<D>(V + (int64_t)tbeg * kRows * a.ld_qkv, a.ld_qkv, tid, vr);
  }
  for (int t = tbeg; t < ntiles; ++t) {
    const int k0 = t * kRows;
    __syncthreads();
    if constexpr (PF) {
      store_tile<D>(kimg, tid, kr);
      store_tile<D>(vimg, tid, vr);
    } else {
      stage_tile<D>(K + (int64_t)k0 * a.ld_qkv, a.ld_qkv, kimg, tid);
      stage_tile<D>(V + (int64_t)k0 * a.ld_qkv, a.ld_qkv, vimg, tid);
    }
    __syncthreads();
    if constexpr (PF) if (t + 1 < ntiles) {
      load_tile<D>(K + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, kr);
      load_tile<D>(V + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, vr);
    }
    f32x4 sacc[4], pacc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sacc[j] = pacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], frag_rows<D>(kimg, 16 * j, s, lane), sacc[j], 0, 0, 0);
        pacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[s], frag_rows<D>(vimg, 16 * j, s, lane), pacc[j], 0, 0, 0);
      }
    float ds[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = k0 + 16 * j + (lane & 15);
      uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
      if (a.p > 0.f) {
        const uint4 mw = attn_mask_words(a, bh, qrow0 >> 2, key);
        w[0] = mw.x; w[1] = mw.y; w[2] = mw.z; w[3] = mw.w;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pr, dcap = 1.f;  // dcap: d(capped score) / d(score) = 1 - t^2
        if constexpr (SOFTCAP) {
          const float rc = softcap_r(sacc[j][r], cap_in);
          pr = __builtin_amdgcn_exp2f((1.f - 2.f * rc) * cap_l2 - lse2[r]);
          dcap = 4.f * rc * (1.f - rc);
        } else {
          pr = __builtin_amdgcn_exp2f(sacc[j][r] * sl2 - lse2[r]);
        }
        if (CAUSAL && key > qrow0 + r) pr = 0.f;
        if (WINDOW && key <= wrow0 + r) pr = 0.f;
        if (DOCS && key < dlo[r]) pr = 0.f;
        float dp = pacc[j][r];
        if (a.p > 0.f) dp = w[r] >= a.threshold ? dp * pscale : 0.f;
        ds[j][r] = pr * (dp - dl[r]);
        if constexpr (SOFTCAP) ds[j][r] *= dcap;
      }
    }
    scratch_write(scr, ds, lane);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    const bf16x8 s0 = scratch_frag(scr, 0, lane);
    const bf16x8 s1 = scratch_frag(scr, 1, lane);
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2) {
      dq[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s0, frag_cols<D>(kimg, 16 * t2, 0, lane), dq[t2], 0, 0, 0);
      dq[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s1, frag_cols<D>(kimg, 16 * t2, 1, lane), dq[t2], 0, 0, 0);
    }
  }
  bf16_t* dQ = reinterpret_cast<bf16_t*>(a.dq) + boff;
#pragma unroll
  for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dQ[(int64_t)(qrow0 + r) * a.ld_qkv + 16 * t2 + (lane & 15)] = f2bf(dq[t2][r] * a.scale);
}

// ------------------------------------------------------------------ dQ, D = 64, 32 rows per wave
// Same restructuring as attn_fwd_wide_kernel: each K/V fragment read from LDS
// feeds the MFMAs of both 16-row blocks of the wave; tiles above the wave's
// diagonal are skipped and only diagonal tiles are masked.
template <bool CAUSAL>
__global__ void __launch_bounds__(kThreads, 2) attn_dq_wide_kernel(AttnArgs a) {
  constexpr int D = 64, NS = 2, ND = 4, RB = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kimg = smem;
  char* vimg = smem + Img<D>::kBytes;
  bf16_t* scr_all = reinterpret_cast<bf16_t*>(smem + 2 * Img<D>::kBytes);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = CAUSAL ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = qt * kWideRows;
  const int wrow0 = q0 + wave * 32;
  const int64_t boff = (int64_t)b * a.sb_qkv + (int64_t)h * a.sh_qkv;
  const int64_t koff = (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;  // K / V: the group's head
  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + boff;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + koff;
  const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + koff;
  const bf16_t* dO = reinterpret_cast<const bf16_t*>(a.dout) + (int64_t)b * a.sb_o + (int64_t)h * a.sh_o;

  bf16x8 qf[RB][NS], df[RB][NS];
  float lse2[RB][4], dl[RB][4];
  f32x4 dq[RB][ND];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int myrow = wrow0 + 16 * rb + (lane & 15);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      qf[rb][s] = frag_global(Q + (int64_t)myrow * a.ld_qkv, s, lane);
      df[rb][s] = frag_global(dO + (int64_t)myrow * a.ld_o, s, lane);
    }
    const int qrow0 = wrow0 + 16 * rb + 4 * (lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lse2[rb][r] = a.lse[(int64_t)bh * a.S + qrow0 + r] * kLog2e;
      dl[rb][r] = a.delta[(int64_t)bh * a.S + qrow0 + r];
    }
#pragma unroll
    for (int t = 0; t < ND; ++t) dq[rb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sl2 = a.scale * kLog2e;
  const float pscale = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const int ntiles = CAUSAL ? (q0 + kWideRows) / kRows : a.S / kRows;

  TileRegs kr, vr;
  load_tile<D>(K, a.ld_qkv, tid, kr);
  load_tile<D>(V, a.ld_qkv, tid, vr);
  for (int t = 0; t < ntiles; ++t) {
    const int k0 = t * kRows;
    __syncthreads();
    store_tile<D>(kimg, tid, kr);
    store_tile<D>(vimg, tid, vr);
    __syncthreads();
    if (t + 1 < ntiles) {
      load_tile<D>(K + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, kr);
      load_tile<D>(V + (int64_t)(k0 + kRows) * a.ld_qkv, a.ld_qkv, tid, vr);
    }
    if (CAUSAL && k0 > wrow0 + 31) continue;
    const bool diag = CAUSAL && k0 + kRows - 1 > wrow0;

    f32x4 sacc[RB][4], pacc[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int j = 0; j < 4; ++j) sacc[rb][j] = pacc[rb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 kfr = frag_rows<D>(kimg, 16 * j, s, lane);
        const bf16x8 vfr = frag_rows<D>(vimg, 16 * j, s, lane);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          sacc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[rb][s], kfr, sacc[rb][j], 0, 0, 0);
          pacc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[rb][s], vfr, pacc[rb][j], 0, 0, 0);
        }
      }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int qrow0 = wrow0 + 16 * rb + 4 * (lane >> 4);
      float ds[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = k0 + 16 * j + (lane & 15);
        uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (a.p > 0.f) {
          const uint4 mw = attn_mask_words(a, bh, qrow0 >> 2, key);
          w[0] = mw.x; w[1] = mw.y; w[2] = mw.z; w[3] = mw.w;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float pr = __builtin_amdgcn_exp2f(sacc[rb][j][r] * sl2 - lse2[rb][r]);
          if (diag && key > qrow0 + r) pr = 0.f;
          float dp = pacc[rb][j][r];
          if (a.p > 0.f) dp = w[r] >= a.threshold ? dp * pscale : 0.f;
          ds[j][r] = pr * (dp - dl[rb][r]);
        }
      }
      scratch_write(scr_all + (wave * RB + rb) * 16 * kScrStride, ds, lane);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    bf16x8 sf[RB][2];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const bf16_t* scr = scr_all + (wave * RB + rb) * 16 * kScrStride;
      sf[rb][0] = scratch_frag(scr, 0, lane);
      sf[rb][1] = scratch_frag(scr, 1, lane);
    }
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 kc = frag_cols<D>(kimg, 16 * t2, s, lane);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          dq[rb][t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sf[rb][s], kc, dq[rb][t2], 0, 0, 0);
      }
  }
  bf16_t* dQ = reinterpret_cast<bf16_t*>(a.dq) + boff;
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int qrow0 = wrow0 + 16 * rb + 4 * (lane >> 4);
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        dQ[(int64_t)(qrow0 + r) * a.ld_qkv + 16 * t2 + (lane & 15)] = f2bf(dq[rb][t2][r] * a.scale);
  }
}

// ------------------------------------------------------------------ dK, dV
// WINDOW (only with CAUSAL): key j is seen by the queries [j, j + a.window), so the query-tile loop ends at the
// tile of query k0 + 63 + a.window - 1 instead of at the sequence's last one.
// DOCS (only with CAUSAL): key j is seen by the queries [j, hi(j)); the loop ends at the tile of hi(k0 + 63) - 1
// and the mask is q >= hi(key).
template <int D, bool CAUSAL, bool WINDOW = false, bool SOFTCAP = false, bool DOCS = false>
__global__ void __launch_bounds__(kThreads, D >= 128 ? 1 : 2) attn_dkdv_kernel(AttnArgs a) {
  static_assert(!WINDOW || CAUSAL, "the sliding window is a band of the causal mask");
  static_assert(!DOCS || (CAUSAL && !WINDOW), "documents mask the causal triangle and merge the window at run time");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qimg = smem;
  char* dimg = smem + Img<D>::kBytes;
  bf16_t* scr_all = reinterpret_cast<bf16_t*>(smem + 2 * Img<D>::kBytes);
  float* stats = reinterpret_cast<float*>(smem + 2 * Img<D>::kBytes + 4 * 16 * kScrStride * 2);  // lse2[64], delta[64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kt = blockIdx.x, bh = blockIdx.y;
  const int b = bh / a.H, h = bh % a.H;
  const int k0 = kt * kRows;
  bf16_t* scr = scr_all + wave * 16 * kScrStride;
  const int64_t boff = (int64_t)b * a.sb_qkv + (int64_t)h * a.sh_qkv;
  const int64_t koff = (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;  // K / V: the group's head
  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + boff;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + koff;
  const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + koff;
  const bf16_t* dO = reinterpret_cast<const bf16_t*>(a.dout) + (int64_t)b * a.sb_o + (int64_t)h * a.sh_o;

  constexpr int NS = D / 32, ND = D / 16;
  bf16x8 kf[NS], vf[NS];
  const int mykey = k0 + wave * 16 + (lane & 15);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    kf[s] = frag_global(K + (int64_t)mykey * a.ld_qkv, s, lane);
    vf[s] = frag_global(V + (int64_t)mykey * a.ld_qkv, s, lane);
  }
  const int key0 = k0 + wave * 16 + 4 * (lane >> 4);  // this lane's keys key0 .. +3 (rows of S^T)
  f32x4 dk[ND], dv[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = a.scale * kLog2e;
  const float pscale = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const int first = CAUSAL ? kt : 0;
  // one past the last query tile: the loop end, computed once (the window is not read again)
  const int nq = DOCS ? doc_nq(a, b, k0, kt)
                      : (WINDOW ? min(a.S / kRows, (k0 + kRows - 1 + a.window - 1) / kRows + 1) : a.S / kRows);
  const int wkey0 = WINDOW ? key0 + a.window : 0;  // key key0 + r is seen by the queries < wkey0 + r
  int dhi[4] = {0, 0, 0, 0};                       // DOCS: key key0 + r is seen by the queries < dhi[r]
  if constexpr (DOCS) {
    const int4 en = doc_rows4(a.doc_end, a, b, key0);
    dhi[0] = min(key0 + a.window, en.x);
    dhi[1] = min(key0 + 1 + a.window, en.y);
    dhi[2] = min(key0 + 2 + a.window, en.z);
    dhi[3] = min(key0 + 3 + a.window, en.w);
  }
  const float cap_in = SOFTCAP ? 2.f * sl2 / a.softcap : 0.f;  // as in attn_fwd_kernel
  const float cap_l2 = SOFTCAP ? a.softcap * kLog2e : 0.f;

  constexpr bool PF = D <= 128;
  TileRegs qr, dr;
  if constexpr (PF) {
    load_tile<D>(Q + (int64_t)first * kRows * a.ld_qkv, a.ld_qkv, tid, qr);
    load_tile<D>(dO + (int64_t)first * kRows * a.ld_o, a.ld_o, tid, dr);
  }
  for (int t = first; t < nq; ++t) {
    const int q0 = t * kRows;
    __syncthreads();
    if constexpr (PF) {
      store_tile<D>(qimg, tid, qr);
      store_tile<D>(dimg, tid, dr);
    } else {
      stage_tile<D>(Q + (int64_t)q0 * a.ld_qkv, a.ld_qkv, qimg, tid);
      stage_tile<D>(dO + (int64_t)q0 * a.ld_o, a.ld_o, dimg, tid);
    }
    if (tid < 64) {
      stats[tid] = a.lse[(int64_t)bh * a.S + q0 + tid] * kLog2e;
      stats[64 + tid] = a.delta[(int64_t)bh * a.S + q0 + tid];
    }
    __syncthreads();
    if constexpr (PF) if (t + 1 < nq) {
      load_tile<D>(Q + (int64_t)(q0 + kRows) * a.ld_qkv, a.ld_qkv, tid, qr);
      load_tile<D>(dO + (int64_t)(q0 + kRows) * a.ld_o, a.ld_o, tid, dr);
    }
    f32x4 sacc[4], pacc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sacc[j] = pacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[s], frag_rows<D>(qimg, 16 * j, s, lane), sacc[j], 0, 0, 0);
        pacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[s], frag_rows<D>(dimg, 16 * j, s, lane), pacc[j], 0, 0, 0);
      }
    // S^T[key][q]: lane holds keys key0 + r, query q = q0 + 16 j + (lane & 15)
    float pd[4][4], ds[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ql = 16 * j + (lane & 15);
      const int q = q0 + ql;
      const float l2 = stats[ql], dl = stats[64 + ql];
      // Dropout words: element (q, key0 + r) uses word (q & 3) of
      // Philox(q >> 2, key0 + r).  The 4 lanes of a quad share q >> 2 and
      // key0 and each needs one word of each of the 4 Philox blocks, so each
      // lane generates ONE block (key0 + (lane & 3)) and the quad transposes
      // the 4 x 4 words with 4 lane shuffles (instead of 4 Philox calls each).
      uint32_t kw0 = 0xFFFFFFFFu, kw1 = 0xFFFFFFFFu, kw2 = 0xFFFFFFFFu, kw3 = 0xFFFFFFFFu;
      if (a.p > 0.f) {
        const int t = lane & 3;
        const uint4 mine = attn_mask_words(a, bh, q >> 2, key0 + t);
        auto word = [&](int i) { return i == 0 ? mine.x : (i == 1 ? mine.y : (i == 2 ? mine.z : mine.w)); };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int src = (lane & ~3) | ((t + k) & 3);
          const uint32_t got = (uint32_t)__shfl((int)word((t - k) & 3), src, 64);  // word t of key0 + ((t+k)&3)
          const int r = (t + k) & 3;
          kw0 = r == 0 ? got : kw0;
          kw1 = r == 1 ? got : kw1;
          kw2 = r == 2 ? got : kw2;
          kw3 = r == 3 ? got : kw3;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + r;
        float pr, dcap = 1.f;  // dcap: d(capped score) / d(score) = 1 - t^2
        if constexpr (SOFTCAP) {
          const float rc = softcap_r(sacc[j][r], cap_in);
          pr = __builtin_amdgcn_exp2f((1.f - 2.f * rc) * cap_l2 - l2);
          dcap = 4.f * rc * (1.f - rc);
        } else {
          pr = __builtin_amdgcn_exp2f(sacc[j][r] * sl2 - l2);
        }
        if (CAUSAL && key > q) pr = 0.f;
        if (WINDOW && q >= wkey0 + r) pr = 0.f;
        if (DOCS && q >= dhi[r]) pr = 0.f;
        float dp = pacc[j][r];
        float pdrop = pr;
        if (a.p > 0.f) {
          const uint32_t w = r == 0 ? kw0 : (r == 1 ? kw1 : (r == 2 ? kw2 : kw3));
          const bool keep = w >= a.threshold;
          pdrop = keep ? pr * pscale : 0.f;
          dp = keep ? dp * pscale : 0.f;
        }
        pd[j][r] = pdrop;
        ds[j][r] = pr * (dp - dl);
        if constexpr (SOFTCAP) ds[j][r] *= dcap;
      }
    }
    scratch_write(scr, pd, lane);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    bf16x8 f0 = scratch_frag(scr, 0, lane);
    bf16x8 f1 = scratch_frag(scr, 1, lane);
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2) {
      dv[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0, frag_cols<D>(dimg, 16 * t2, 0, lane), dv[t2], 0, 0, 0);
      dv[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, frag_cols<D>(dimg, 16 * t2, 1, lane), dv[t2], 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    scratch_write(scr, ds, lane);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    f0 = scratch_frag(scr, 0, lane);
    f1 = scratch_frag(scr, 1, lane);
#pragma unroll
    for (int t2 = 0; t2 < ND; ++t2) {
      dk[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0, frag_cols<D>(qimg, 16 * t2, 0, lane), dk[t2], 0, 0, 0);
      dk[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, frag_cols<D>(qimg, 16 * t2, 1, lane), dk[t2], 0, 0, 0);
    }
  }
  const DkvDst dst = dkv_dst<0>(blockIdx.y);  // 0: AttnArgs is this kernel's first (only) parameter
  bf16_t* dK = dst.dk;
  bf16_t* dV = dst.dv;
#pragma unroll
  for (int t2 = 0; t2 < ND; ++t2)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t o = (int64_t)(key0 + r) * dst.ld + 16 * t2 + (lane & 15);
      dK[o] = f2bf(dk[t2][r] * a.scale);
      dV[o] = f2bf(dv[t2][r]);
    }
}

// ------------------------------------------------------------------ fused backward, S = 128
// One 512-thread workgroup per (batch, head) computes dQ, dK and dV of the
// whole 128-token sequence in one pass (the reference's bptt = 128 case):
//   phase 1  S = Q K^T and dP = dO V^T for all 128 x 128 pairs, streamed over
//            D in 64-wide chunks (K, V chunks double-buffered in LDS; Q, dO
//            A-fragments straight from HBM); wave w owns query rows 16w..16w+15.
//            P = exp(S - lse), dropout replayed from Philox, and
//            delta_i = sum_j P~_ij dP_ij straight from registers (= rowsum(dO.O),
//            so no O read and no delta pre-pass);
//   phase 2  P~ and dS = P (dP~ - delta) go to two 128 x 128 bf16 LDS images;
//            per 64-wide D chunk K, Q and dO chunks are staged and
//            dQ = dS K, dK = dS^T Q, dV = P~^T dO come out of 48 MFMAs per wave
//            (transposed operands via ds_read_b64_tr_b16).
// vs. the general path (delta + dK/dV + dQ kernels) it reads Q, K, V, dO once
// and recomputes S / dP once instead of twice.
namespace shortseq {

constexpr int S = 128;
constexpr int kThreads = 512;      // 8 waves x 16 query rows
constexpr int kChunk = 64;         // D chunk
constexpr int kChunkImg = S * kChunk * 2;   // [128][64] bf16 = 16 KiB
constexpr int kSqImg = S * S * 2;           // [128][128] bf16 = 32 KiB
constexpr int kStageBytes = 3 * kChunkImg;  // phase 2: K, Q, dO chunks (48 KiB); phase 1 uses 4 chunk images
constexpr int kPOff = 4 * kChunkImg;        // 64 KiB
constexpr int kDsOff = kPOff + kSqImg;      // 96 KiB
constexpr int kSmem = kDsOff + kSqImg;      // 128 KiB
constexpr int kFwdPOff = 2 * kChunkImg;     // forward: 2 chunk buffers + P~ image = 64 KiB (2 workgroups / CU)
constexpr int kFwdSmem = kFwdPOff + kSqImg;

// [128][64] chunk image: Img<64> addressing (128-byte rows).
__device__ __forceinline__ int coff(int r, int c16) { return Img<64>::off(r, c16); }
// [128][128] image: Img<128> addressing (256-byte rows).
__device__ __forceinline__ int soff(int r, int c16) { return Img<128>::off(r, c16); }

// rows 0..127, columns [d0, d0 + 64) of a row-major matrix -> chunk image.
// (two named registers, not an array: a loop-carried uint4[2] was kept in scratch)
__device__ __forceinline__ void load_chunk(const bf16_t* __restrict__ base, int64_t ld, int d0, int tid, uint4& v0,
                                           uint4& v1) {
  const int r = tid >> 3, c = tid & 7;  // pieces tid and tid + 512 of 1024: rows r and r + 64
  v0 = *reinterpret_cast<const uint4*>(base + (int64_t)r * ld + d0 + 8 * c);
  v1 = *reinterpret_cast<const uint4*>(base + (int64_t)(r + 64) * ld + d0 + 8 * c);
}
__device__ __forceinline__ void store_chunk(char* img, int tid, const uint4& v0, const uint4& v1) {
  const int r = tid >> 3, c = tid & 7;
  *reinterpret_cast<uint4*>(img + coff(r, c)) = v0;
  *reinterpret_cast<uint4*>(img + coff(r + 64, c)) = v1;
}

// B[k = d][n = row] from a chunk image (16 rows from rb, k-step s of 32).
__device__ __forceinline__ bf16x8 crow(const char* img, int rb, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + coff(rb + (lane & 15), 4 * s + (lane >> 4)));
}
// B[k = row][n = d] from a chunk image (rows 32 s.., columns db..db+15).
__device__ __forceinline__ bf16x8 ccol(const char* img, int db, int s, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * s + 8 * g + q;
  const int c8 = (db >> 2) + p;
  const int o0 = coff(r0, c8 >> 1) + 8 * (c8 & 1);
  const int o1 = coff(r0 + 4, c8 >> 1) + 8 * (c8 & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o1));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// A[i = row][k = col] from a [128][128] image (rows rb.., k-step s of 32).
__device__ __forceinline__ bf16x8 srow(const char* img, int rb, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + soff(rb + (lane & 15), 4 * s + (lane >> 4)));
}
// A[i = col][k = row] from a [128][128] image (columns ib.., k-step s of 32 over rows).
__device__ __forceinline__ bf16x8 scol(const char* img, int ib, int s, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * s + 8 * g + q;
  const int c8 = (ib >> 2) + p;
  const int o0 = soff(r0, c8 >> 1) + 8 * (c8 & 1);
  const int o1 = soff(r0 + 4, c8 >> 1) + 8 * (c8 & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o1));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int D, bool CAUSAL>
__global__ void __launch_bounds__(kThreads, 1) attn_bwd_s128_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.x;
  const int b = bh / a.H, h = bh % a.H;
  const int64_t boff = (int64_t)b * a.sb_qkv + (int64_t)h * a.sh_qkv;
  const int64_t koff = (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;  // K / V: the group's head
  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + boff;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + koff;
  const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + koff;
  const bf16_t* dO = reinterpret_cast<const bf16_t*>(a.dout) + (int64_t)b * a.sb_o + (int64_t)h * a.sh_o;
  constexpr int NC = D / kChunk;

  // ---- phase 1: S and dP over D chunks ----
  f32x4 sacc[8], pacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) sacc[j] = pacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int myrow = wave * 16 + (lane & 15);
  const bf16_t* qrow = Q + (int64_t)myrow * a.ld_qkv;
  const bf16_t* drow = dO + (int64_t)myrow * a.ld_o;

  uint4 k0, k1, v0, v1;
  load_chunk(K, a.ld_qkv, 0, tid, k0, k1);
  load_chunk(V, a.ld_qkv, 0, tid, v0, v1);
  store_chunk(smem, tid, k0, k1);
  store_chunk(smem + kChunkImg, tid, v0, v1);
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < NC; ++c) {
    const char* kimg = smem + (c & 1) * 2 * kChunkImg;
    const char* vimg = kimg + kChunkImg;
    if (c + 1 < NC) {  // prefetch the next chunk into registers (T14)
      load_chunk(K, a.ld_qkv, (c + 1) * kChunk, tid, k0, k1);
      load_chunk(V, a.ld_qkv, (c + 1) * kChunk, tid, v0, v1);
    }
    bf16x8 qf[2], df[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      qf[s2] = frag_global(qrow + c * kChunk, s2, lane);
      df[s2] = frag_global(drow + c * kChunk, s2, lane);
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s2], crow(kimg, 16 * j, s2, lane), sacc[j], 0, 0, 0);
        pacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[s2], crow(vimg, 16 * j, s2, lane), pacc[j], 0, 0, 0);
      }
    if (c + 1 < NC) {
      char* nimg = smem + ((c + 1) & 1) * 2 * kChunkImg;
      store_chunk(nimg, tid, k0, k1);
      store_chunk(nimg + kChunkImg, tid, v0, v1);
    }
    __syncthreads();
  }

  // ---- softmax, dropout replay, delta, dS ----
  const int qrow0 = wave * 16 + 4 * (lane >> 4);  // this lane's rows qrow0 .. +3
  const float sl2 = a.scale * kLog2e;
  const float pscale = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  float lse2[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) lse2[r] = a.lse[(int64_t)bh * S + qrow0 + r] * kLog2e;
  float dsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int key = 16 * j + (lane & 15);
    uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (a.p > 0.f) {
      const uint4 mw = attn_mask_words(a, bh, qrow0 >> 2, key);
      w[0] = mw.x; w[1] = mw.y; w[2] = mw.z; w[3] = mw.w;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pr = __builtin_amdgcn_exp2f(sacc[j][r] * sl2 - lse2[r]);
      if (CAUSAL && key > qrow0 + r) pr = 0.f;
      float dp = pacc[j][r];
      float pd = pr;
      if (a.p > 0.f) {
        const bool keep = w[r] >= a.threshold;
        dp = keep ? dp * pscale : 0.f;
        pd = keep ? pr * pscale : 0.f;
      }
      sacc[j][r] = pr;  // P (undropped)
      pacc[j][r] = dp;  // dP~
      dsum[r] += pr * dp;
      // P~ into its image now (sacc is overwritten by dS below)
      *reinterpret_cast<bf16_t*>(smem + kPOff + soff(qrow0 + r, key >> 3) + 2 * (key & 7)) = f2bf(pd);
    }
  }
  float delta[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) delta[r] = row_reduce_sum16(dsum[r]);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int key = 16 * j + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ds = sacc[j][r] * (pacc[j][r] - delta[r]);
      *reinterpret_cast<bf16_t*>(smem + kDsOff + soff(qrow0 + r, key >> 3) + 2 * (key & 7)) = f2bf(ds);
    }
  }

  // ---- phase 2: dQ = dS K, dK = dS^T Q, dV = P~^T dO per D chunk ----
  const char* pimg = smem + kPOff;
  const char* dsimg = smem + kDsOff;
  char* kimg = smem;
  char* qimg = smem + kChunkImg;
  char* dimg = smem + 2 * kChunkImg;
  const int r0 = wave * 16;  // output rows (queries for dQ, keys for dK / dV)
  // The next chunk's K / Q / dO are loaded into registers while this chunk's
  // MFMAs run; results leave through the (then free) chunk images as 16-byte
  // row stores instead of 2-byte scattered ones.
  uint4 a0, a1, b0, b1, e0, e1;
  load_chunk(K, a.ld_qkv, 0, tid, a0, a1);
  load_chunk(Q, a.ld_qkv, 0, tid, b0, b1);
  load_chunk(dO, a.ld_o, 0, tid, e0, e1);
#pragma unroll 1
  for (int c = 0; c < NC; ++c) {
    const int d0 = c * kChunk;
    __syncthreads();  // previous chunk's output readers are done (and phase-1 images for c == 0)
    store_chunk(kimg, tid, a0, a1);
    store_chunk(qimg, tid, b0, b1);
    store_chunk(dimg, tid, e0, e1);
    __syncthreads();
    if (c + 1 < NC) {
      load_chunk(K, a.ld_qkv, d0 + kChunk, tid, a0, a1);
      load_chunk(Q, a.ld_qkv, d0 + kChunk, tid, b0, b1);
      load_chunk(dO, a.ld_o, d0 + kChunk, tid, e0, e1);
    }
    f32x4 dq[4], dk[4], dv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dq[t] = dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 a_dq = srow(dsimg, r0, ks, lane);   // dS[q][key], k = key
      const bf16x8 a_dk = scol(dsimg, r0, ks, lane);   // dS^T[key][q], k = q
      const bf16x8 a_dv = scol(pimg, r0, ks, lane);    // P~^T[key][q], k = q
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        dq[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_dq, ccol(kimg, 16 * t, ks, lane), dq[t], 0, 0, 0);
        dk[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_dk, ccol(qimg, 16 * t, ks, lane), dk[t], 0, 0, 0);
        dv[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_dv, ccol(dimg, 16 * t, ks, lane), dv[t], 0, 0, 0);
      }
    }
    const int orow = r0 + 4 * (lane >> 4);
    __syncthreads();  // every wave is done reading the input images
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = 16 * t + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = coff(orow + r, col >> 3) + 2 * (col & 7);
        *reinterpret_cast<bf16_t*>(kimg + at) = f2bf(dq[t][r] * a.scale);
        *reinterpret_cast<bf16_t*>(qimg + at) = f2bf(dk[t][r] * a.scale);
        *reinterpret_cast<bf16_t*>(dimg + at) = f2bf(dv[t][r]);
      }
    }
    __syncthreads();
    {
      const int r = tid >> 3, cc = tid & 7;  // pieces tid and tid + 512: rows r and r + 64
      // <0>: AttnArgs is this kernel's first (only) parameter
      const DkvDst dst = dkv_dst<0>(blockIdx.x);
      bf16_t* dK = dst.dk;
      bf16_t* dV = dst.dv;
      bf16_t* dQ = dq_dst<0>(blockIdx.x);
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int row = r + 64 * h2;
        const int off = coff(row, cc);
        const int64_t g = (int64_t)row * a.ld_qkv + d0 + 8 * cc;
        const int64_t gk = (int64_t)row * dst.ld + d0 + 8 * cc;
        *reinterpret_cast<uint4*>(dQ + g) = *reinterpret_cast<const uint4*>(kimg + off);
        *reinterpret_cast<uint4*>(dK + gk) = *reinterpret_cast<const uint4*>(qimg + off);
        *reinterpret_cast<uint4*>(dV + gk) = *reinterpret_cast<const uint4*>(dimg + off);
      }
    }
  }
}

// Forward, S = 128: one workgroup per (batch, head); with the whole key range
// in registers the softmax is exact (no online rescaling): S = Q K^T over D
// chunks, P = softmax (dropout applied), P~ to a [128][128] LDS image, then
// O = P~ V per 64-wide D chunk of V.
template <int D, bool CAUSAL>
__global__ void __launch_bounds__(kThreads, 2) attn_fwd_s128_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.x;
  const int b = bh / a.H, h = bh % a.H;
  const int64_t boff = (int64_t)b * a.sb_qkv + (int64_t)h * a.sh_qkv;
  const int64_t koff = (int64_t)b * a.sb_qkv + (int64_t)kv_head(a, h) * a.sh_qkv;  // K / V: the group's head
  const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + boff;
  const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + koff;
  const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + koff;
  constexpr int NC = D / kChunk;

  f32x4 sacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) sacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* qrow = Q + (int64_t)(wave * 16 + (lane & 15)) * a.ld_qkv;

  uint4 k0, k1;
  load_chunk(K, a.ld_qkv, 0, tid, k0, k1);
  store_chunk(smem, tid, k0, k1);
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < NC; ++c) {
    const char* kimg = smem + (c & 1) * kChunkImg;
    if (c + 1 < NC) load_chunk(K, a.ld_qkv, (c + 1) * kChunk, tid, k0, k1);
    bf16x8 qf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) qf[s2] = frag_global(qrow + c * kChunk, s2, lane);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s2], crow(kimg, 16 * j, s2, lane), sacc[j], 0, 0, 0);
    if (c + 1 < NC) store_chunk(smem + ((c + 1) & 1) * kChunkImg, tid, k0, k1);
    __syncthreads();
  }

  // exact softmax over the 128 keys (log2 domain), dropout, P~ -> LDS image
  const int qrow0 = wave * 16 + 4 * (lane >> 4);
  const float sl2 = a.scale * kLog2e;
  const float pscale = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int key = 16 * j + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = sacc[j][r] * sl2;
      if (CAUSAL && key > qrow0 + r) x = -INFINITY;
      sacc[j][r] = x;
      mx[r] = fmaxf(mx[r], x);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) mx[r] = row_reduce_max16(mx[r]);
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __builtin_amdgcn_exp2f(sacc[j][r] - mx[r]);
      sacc[j][r] = e;
      sum[r] += e;
    }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sum[r] = row_reduce_sum16(sum[r]);
    inv[r] = 1.f / sum[r];
  }
  char* pimg = smem + kFwdPOff;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int key = 16 * j + (lane & 15);
    uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (a.p > 0.f) {
      const uint4 mw = attn_mask_words(a, bh, qrow0 >> 2, key);
      w[0] = mw.x; w[1] = mw.y; w[2] = mw.z; w[3] = mw.w;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pv = sacc[j][r] * inv[r];
      if (a.p > 0.f) pv = w[r] >= a.threshold ? pv * pscale : 0.f;
      *reinterpret_cast<bf16_t*>(pimg + soff(qrow0 + r, key >> 3) + 2 * (key & 7)) = f2bf(pv);
    }
  }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a.lse[(int64_t)bh * S + qrow0 + r] = (mx[r] + log2f(sum[r])) / kLog2e;
  }

  // O = P~ V per D chunk (V chunks double-buffered in the phase-1 buffers)
  bf16_t* O = reinterpret_cast<bf16_t*>(a.o) + (int64_t)b * a.sb_o + (int64_t)h * a.sh_o;
  uint4 v0, v1;
  load_chunk(V, a.ld_qkv, 0, tid, v0, v1);
  store_chunk(smem, tid, v0, v1);
  __syncthreads();  // P~ image and V chunk 0 visible
  const int r0 = wave * 16;
#pragma unroll 1
  for (int c = 0; c < NC; ++c) {
    const char* vimg = smem + (c & 1) * kChunkImg;
    if (c + 1 < NC) load_chunk(V, a.ld_qkv, (c + 1) * kChunk, tid, v0, v1);
    f32x4 o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 ap = srow(pimg, r0, ks, lane);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap, ccol(vimg, 16 * t, ks, lane), o[t], 0, 0, 0);
    }
    const int orow = r0 + 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        O[(int64_t)(orow + r) * a.ld_o + c * kChunk + 16 * t + (lane & 15)] = f2bf(o[t][r]);
    if (c + 1 < NC) store_chunk(smem + ((c + 1) & 1) * kChunkImg, tid, v0, v1);
    __syncthreads();
  }
}

}  // namespace shortseq

template <int D>
size_t fwd_smem() { return 2 * Img<D>::kBytes + 4 * 16 * kScrStride * 2; }
template <int D>
size_t dkdv_smem() { return fwd_smem<D>() + 128 * sizeof(float); }

int g_attn_fused_bwd = 1;
// D = 64: 32-rows-per-wave forward (1, default) or the 16-row kernel (0); MIPIPE_ATTN_WIDE=0 for A/B runs.
const int g_attn_wide = [] {
  const char* e = getenv("MIPIPE_ATTN_WIDE");
  return e == nullptr ? 1 : atoi(e);
}();  // S == 128: whole-sequence forward/backward kernels (1) or the general ones (0)

template <typename Kern>
void set_smem(Kern k, size_t bytes) {
  hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <int D, bool CAUSAL>
void run_fwd(const AttnArgs& a, hipStream_t s) {
  if (a.S == shortseq::S && g_attn_fused_bwd) {
    static bool once_s = false;
    if (!once_s) {
      set_smem(shortseq::attn_fwd_s128_kernel<D, CAUSAL>, shortseq::kFwdSmem);
      once_s = true;
    }
    hipLaunchKernelGGL((shortseq::attn_fwd_s128_kernel<D, CAUSAL>), dim3(a.B * a.H), dim3(shortseq::kThreads),
                       shortseq::kFwdSmem, s, a);
    return;
  }
  if (D == 64 && a.S % kWideRows == 0 && g_attn_wide) {
    static bool once_w = false;
    if (!once_w) { set_smem(attn_fwd_wide_kernel<CAUSAL>, wide_fwd_smem()); once_w = true; }
    hipLaunchKernelGGL((attn_fwd_wide_kernel<CAUSAL>), dim3(a.S / kWideRows, a.B * a.H), dim3(kThreads),
                       wide_fwd_smem(), s, a);
    return;
  }
  const size_t sm = fwd_smem<D>();
  static bool once = false;
  if (!once) { set_smem(attn_fwd_kernel<D, CAUSAL>, sm); once = true; }
  hipLaunchKernelGGL((attn_fwd_kernel<D, CAUSAL>), dim3(a.S / kRows, a.B * a.H), dim3(kThreads), sm, s, a);
}

template <int D, bool CAUSAL>
void run_bwd(const AttnArgs& a, hipStream_t s) {
  const size_t sm = fwd_smem<D>(), sm2 = dkdv_smem<D>();
  static bool once = false;
  if (!once) {
    set_smem(attn_dq_kernel<D, CAUSAL>, sm);
    set_smem(attn_dkdv_kernel<D, CAUSAL>, sm2);
    once = true;
  }
  if (a.S == shortseq::S && g_attn_fused_bwd) {
    static bool once_s = false;
    if (!once_s) {
      set_smem(shortseq::attn_bwd_s128_kernel<D, CAUSAL>, shortseq::kSmem);
      once_s = true;
    }
    hipLaunchKernelGGL((shortseq::attn_bwd_s128_kernel<D, CAUSAL>), dim3(a.B * a.H), dim3(shortseq::kThreads),
                       shortseq::kSmem, s, a);
    return;
  }
  const int64_t rows = (int64_t)a.B * a.S * a.H;
  hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a, D);
  hipLaunchKernelGGL((attn_dkdv_kernel<D, CAUSAL>), dim3(a.S / kRows, a.B * a.H), dim3(kThreads), sm2, s, a);
  if (D == 64 && a.S % kWideRows == 0 && g_attn_wide) {
    static bool once_w = false;
    if (!once_w) { set_smem(attn_dq_wide_kernel<CAUSAL>, wide_fwd_smem()); once_w = true; }
    hipLaunchKernelGGL((attn_dq_wide_kernel<CAUSAL>), dim3(a.S / kWideRows, a.B * a.H), dim3(kThreads),
                       wide_fwd_smem(), s, a);
    return;
  }
  hipLaunchKernelGGL((attn_dq_kernel<D, CAUSAL>), dim3(a.S / kRows, a.B * a.H), dim3(kThreads), sm, s, a);
}

// A sliding window (0 < a.window < a.S, causal), a soft cap (a.softcap > 0), document masks (a.doc_start set, causal)
// and sinks (a.sinks set) always run the generic 64-row kernels, whatever S and D and in any combination -- the
// S = 128, wide D = 64 and long-sequence kernels know none of them.  Under documents the window is merged at run
// time (a.window = S when there is none), so there is no WINDOW && DOCS instantiation.
template <int D, bool CAUSAL, bool WINDOW, bool SOFTCAP, bool DOCS, bool SINK>
void launch_fwd_generic(const AttnArgs& a, hipStream_t s) {
  const size_t sm = fwd_smem<D>();
  static bool once = false;
  if (!once) { set_smem(attn_fwd_kernel<D, CAUSAL, WINDOW, SOFTCAP, DOCS, SINK>, sm); once = true; }
  hipLaunchKernelGGL((attn_fwd_kernel<D, CAUSAL, WINDOW, SOFTCAP, DOCS, SINK>), dim3(a.S / kRows, a.B * a.H),
                     dim3(kThreads), sm, s, a);
}

// The generic backward: delta from attn_delta_mfma_kernel on every path (a one-token document gives dS = 0
// exactly), then dK/dV and dQ.  SINK multiplies the forward kernel only: the backward of a call with sinks runs
// the sinkless instantiations on the forward's lse -- with sinks alone, the plain <D, CAUSAL> kernels.
template <int D, bool CAUSAL, bool WINDOW, bool SOFTCAP, bool DOCS>
void launch_bwd_generic(const AttnArgs& a, hipStream_t s) {
  const size_t sm = fwd_smem<D>(), sm2 = dkdv_smem<D>();
  static bool once = false;
  if (!once) {
    set_smem(attn_dq_kernel<D, CAUSAL, WINDOW, SOFTCAP, DOCS>, sm);
    set_smem(attn_dkdv_kernel<D, CAUSAL, WINDOW, SOFTCAP, DOCS>, sm2);
    once = true;
  }
  const dim3 grid(a.S / kRows, a.B * a.H);
  hipLaunchKernelGGL((attn_delta_mfma_kernel<D>), grid, dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL((attn_dkdv_kernel<D, CAUSAL, WINDOW, SOFTCAP, DOCS>), grid, dim3(kThreads), sm2, s, a);
  hipLaunchKernelGGL((attn_dq_kernel<D, CAUSAL, WINDOW, SOFTCAP, DOCS>), grid, dim3(kThreads), sm, s, a);
}

// A window that covers the sequence (or a non-causal call, which has none) is no window.
void normalise_window(AttnArgs& a) {
  if (!a.causal || a.window < 0 || a.window >= a.S) a.window = 0;
}

// Documents need the causal mask and both bounds; the kernels take "no window" as a window of S.
bool normalise_docs(AttnArgs& a) {
  if (a.doc_start == nullptr || a.doc_end == nullptr || !a.causal) {
    a.doc_start = a.doc_end = nullptr;
    return false;
  }
  if (a.window <= 0) a.window = a.S;
  return true;
}

// The arguments as the launchers below read them: late fields resolved, window and documents normalised.
AttnArgs prepared(const AttnArgs& ai) {
  AttnArgs a = attn_resolved(ai);
  a.threshold = dropout_threshold(a.p);
  normalise_window(a);
  normalise_docs(a);
  return a;
}

bool is_generic(const AttnArgs& a) {
  return a.doc_start != nullptr || a.window > 0 || a.softcap > 0.f || a.sinks != nullptr;
}

// Run-time values as template arguments: f gets them as std::integral_constant tags.
template <typename F>
void with_d(int D, F&& f) {
  if (D == 64) f(std::integral_constant<int, 64>{});
  else if (D == 128) f(std::integral_constant<int, 128>{});
  else f(std::integral_constant<int, 256>{});
}

template <typename F>
void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

// The mask mode of prepared() arguments, for the forward and the backward alike: documents (which carry the
// window) over a window over the causal mask over none.  f(CAUSAL, WINDOW, DOCS).
template <typename F>
void with_mask(const AttnArgs& a, F&& f) {
  using Y = std::true_type;
  using N = std::false_type;
  if (a.doc_start != nullptr) f(Y{}, N{}, Y{});
  else if (a.window > 0) f(Y{}, Y{}, N{});
  else if (a.causal) f(Y{}, N{}, N{});
  else f(N{}, N{}, N{});
}

}  // namespace

void attention_set_fused_bwd(int on) { g_attn_fused_bwd = on; }

void attention_dsink(const float* lse, const float* delta, const float* sinks, float* dsinks, int B, int H, int S,
                     bool accumulate, hipStream_t s) {
  hipLaunchKernelGGL(attn_dsink_kernel, dim3(H), dim3(kThreads), 0, s, lse, delta, sinks, dsinks, B, H, S,
                     accumulate ? 1 : 0);
}

bool attention_supported(int S, int D) { return S > 0 && S % kRows == 0 && (D == 64 || D == 128 || D == 256); }

// run_fwd / run_bwd are the plain paths (S = 128, wide D = 64 and the generic fallback); every option takes the
// generic launchers.
void attention_fwd(const AttnArgs& ai, hipStream_t s) {
  const AttnArgs a = prepared(ai);
  with_d(a.D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    if (!is_generic(a)) {
      with_flag(a.causal, [&](auto causal) { run_fwd<D, decltype(causal)::value>(a, s); });
      return;
    }
    with_mask(a, [&](auto causal, auto window, auto docs) {
      with_flag(a.softcap > 0.f, [&](auto cap) {
        with_flag(a.sinks != nullptr, [&](auto sink) {
          launch_fwd_generic<D, decltype(causal)::value, decltype(window)::value, decltype(cap)::value,
                             decltype(docs)::value, decltype(sink)::value>(a, s);
        });
      });
    });
  });
}

void attention_bwd(const AttnArgs& ai, hipStream_t s) {
  const AttnArgs a = prepared(ai);
  with_d(a.D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    if (!is_generic(a)) {
      with_flag(a.causal, [&](auto causal) { run_bwd<D, decltype(causal)::value>(a, s); });
      return;
    }
    with_mask(a, [&](auto causal, auto window, auto docs) {
      with_flag(a.softcap > 0.f, [&](auto cap) {
        launch_bwd_generic<D, decltype(causal)::value, decltype(window)::value, decltype(cap)::value,
                           decltype(docs)::value>(a, s);
      });
    });
  });
}

}  // namespace mipipe
