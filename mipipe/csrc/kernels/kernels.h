// Host-side launch interface of the mipipe HIP kernels.
//
// Kernel translation units include only HIP headers (fast to build); the
// torch-facing bindings (../bindings.cpp) include this header and call the
// launchers with raw pointers and the current HIP stream.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mipipe {

typedef uint16_t bf16_t;

// ------------------------------------------------------------------ LayerNorm
template <typename T>
struct LnArgs {
  const T* x = nullptr;      // branch input (dropout applies here)
  const T* res = nullptr;    // residual input (optional)
  const T* gamma = nullptr;
  const T* beta = nullptr;
  T* y = nullptr;
  T* z = nullptr;            // optional: saved pre-norm sum for backward
  float* mean = nullptr;
  float* rstd = nullptr;
  int rows = 0, cols = 0;
  float eps = 1e-5f;
  float p = 0.f;
  uint64_t seed = 0, offset = 0;
};

template <typename T>
struct LnBwdArgs {
  const T* dy = nullptr;
  const T* z = nullptr;
  const float* mean = nullptr;
  const float* rstd = nullptr;
  const T* gamma = nullptr;
  T* dz = nullptr;           // grad of z (= grad of the residual input)
  const T* addend = nullptr; // optional extra gradient of z, added to dz (fan-out fusion)
  T* dx = nullptr;           // grad of the dropout branch (nullptr if p == 0)
  float* dgamma_part = nullptr;  // [nparts, cols] workspace
  float* dbeta_part = nullptr;
  void* dgamma = nullptr;        // T (store) or fp32 (main_grad, may accumulate)
  void* dbeta = nullptr;
  bool out_f32 = false;
  bool accumulate = false;
  int rows = 0, cols = 0, nparts = 0;
  float p = 0.f;
  uint64_t seed = 0, offset = 0;
};

// out[c] (=|+=) sum over nparts partial rows; out is fp32 (out_f32) or bf16.
void reduce_parts(const float* part_a, const float* part_b, int nparts, int cols, void* out_a, void* out_b,
                  bool out_f32, bool accumulate, hipStream_t s);

int ln_max_vec(int cols);
int ln_bwd_parts(int rows, int cols);
template <typename T> void layernorm_fwd(const LnArgs<T>& a, hipStream_t s);
template <typename T> void layernorm_bwd(const LnBwdArgs<T>& a, hipStream_t s);

// ------------------------------------------------------------------ RMSNorm
// y = z * rsqrt(mean(z^2) + eps) * gamma with z = res + dropout(x): LnArgs
// without mean and beta (rmsnorm.hip).
template <typename T>
struct RmsArgs {
  const T* x = nullptr;      // branch input (dropout applies here)
  const T* res = nullptr;    // residual input (optional)
  const T* gamma = nullptr;
  T* y = nullptr;
  T* z = nullptr;            // optional: saved pre-norm sum for backward
  float* rstd = nullptr;
  int rows = 0, cols = 0;
  float eps = 1e-5f;
  float p = 0.f;
  uint64_t seed = 0, offset = 0;
};

template <typename T>
struct RmsBwdArgs {
  const T* dy = nullptr;
  const T* z = nullptr;
  const float* rstd = nullptr;
  const T* gamma = nullptr;
  T* dz = nullptr;           // grad of z (= grad of the residual input)
  const T* addend = nullptr; // optional extra gradient of z, added to dz (fan-out fusion)
  T* dx = nullptr;           // grad of the dropout branch (nullptr if p == 0)
  float* dgamma_part = nullptr;  // [nparts, cols] workspace
  void* dgamma = nullptr;        // T (store) or fp32 (main_grad, may accumulate)
  bool out_f32 = false;
  bool accumulate = false;
  int rows = 0, cols = 0, nparts = 0;
  float p = 0.f;
  uint64_t seed = 0, offset = 0;
};

// Vectors per thread of the one-row-per-group kernels (2, 4, 8), -1: width not supported
// (cols % 8 != 0 or cols > 16384).
int rms_max_vec(int cols);
int rms_bwd_parts(int rows, int cols);
template <typename T> void rmsnorm_fwd(const RmsArgs<T>& a, hipStream_t s);
// The sandwich norm: y = res + x * rsqrt(mean(x^2) + eps) * gamma (statistics from x alone; a.res required,
// a.rstd may be null, a.p / a.z unused).  Its backward is rmsnorm_bwd on (dy, x, rstd) with p = 0.
template <typename T> void rmsnorm_residual_fwd(const RmsArgs<T>& a, hipStream_t s);
template <typename T> void rmsnorm_bwd(const RmsBwdArgs<T>& a, hipStream_t s);

// ------------------------------------------------------------------ SwiGLU / RoPE (llama.hip)
// gu [rows, 2F] = [gate | up] per row, F % 8 == 0: h [rows, F] = silu(gate) * up.
template <typename T>
void swiglu_fwd(const T* gu, T* h, int64_t rows, int F, hipStream_t s);
// dgu [rows, 2F] = [dgate | dup] from dh [rows, F] and the forward's gu.
template <typename T>
void swiglu_bwd(const T* dh, const T* gu, T* dgu, int64_t rows, int F, hipStream_t s);
// GeGLU, the same layout and contract: h = gelu_tanh(gate) * up (the tanh approximation of GELU).
template <typename T>
void geglu_fwd(const T* gu, T* h, int64_t rows, int F, hipStream_t s);
template <typename T>
void geglu_bwd(const T* dh, const T* gu, T* dgu, int64_t rows, int F, hipStream_t s);
// Rotates Q and K of qkv [B, S, 3, H, D] (contiguous, D % 16 == 0) at positions pos0 + s, pairs
// (i, i + D/2); cos / sin: fp32 [>= pos0 + S, D/2].  out == qkv rotates in place (V untouched),
// otherwise V is copied.  inverse negates sin (the backward, on dqkv).
template <typename T>
void rope_packed(const T* qkv, const float* cos_t, const float* sin_t, T* out, int64_t B, int S, int H, int D, int pos0,
                 bool inverse, hipStream_t s);
// The same on x [B, S, n_rot + n_copy, D]: the first n_rot heads of a token are rotated, the last n_copy
// pass through (copied, or untouched when out == x).  rope_packed is (2 H, H); a grouped-query projection
// [B, S, H + 2 Hkv, D] is (H + Hkv, Hkv).
template <typename T>
void rope_heads(const T* x, const float* cos_t, const float* sin_t, T* out, int64_t B, int S, int n_rot, int n_copy,
                int D, int pos0, bool inverse, hipStream_t s);
// Grouped-query attention backward: dkv [B, S, 2, H, D] (contiguous) holds one dK and one dV partial per
// QUERY head; each group of H / Hkv consecutive heads is summed in fp32, rounded once and stored into the
// K (heads [H, H + Hkv)) and V (heads [H + Hkv, H + 2 Hkv)) slots of dqkv [B, S, H + 2 Hkv, D]
// (contiguous); the Q slots are not touched.  D % 8 == 0 (fp32: % 4), 16-byte aligned pointers.
template <typename T>
void gqa_reduce_dkv(const T* dkv, T* dqkv, int64_t tokens, int H, int Hkv, int D, hipStream_t s);

// ------------------------------------------------------------------ QK-norm (qknorm.hip)
// Per-head RMSNorm of the Q and K heads of x [tokens, n_q + n_k + n_v, D] (contiguous, rope_heads' layout; the
// n_v V heads pass through) fused with the rotary rotation: y = rotate(x rsqrt(mean(x^2) + eps) w) with w = wq [D]
// for the first n_q heads and wk [D] for the next n_k, fp32 arithmetic, one rounding at the store.  cos_t == nullptr
// drops the rotation (the norm alone); otherwise cos / sin are fp32 [>= pos0 + S, D/2] and a token's position is
// pos0 + token % S.  out == x works in place (V untouched), otherwise V is copied.  rstd (optional): fp32
// [tokens, n_q + n_k], written for the backward.  D must satisfy qknorm_supported; 16-byte aligned pointers.
bool qknorm_supported(int D);
template <typename T>
void qknorm_rope_fwd(const T* x, const T* wq, const T* wk, const float* cos_t, const float* sin_t, T* out, float* rstd,
                     int64_t tokens, int S, int n_q, int n_k, int n_v, int D, int pos0, float eps, hipStream_t s);
// dx (a tensor of its own) from dout, the forward's x and rstd: g = inverse-rotate(dout), xhat = x rstd, gy = g w,
// dx = rstd (gy - xhat mean(gy xhat)); V rows: dx = dout.  Block b writes its fp32 sums over rows of g xhat into
// part_q[b] and part_k[b] ([nparts, D] each, nparts = qknorm_bwd_parts(...)): the caller sums them with reduce_parts.
int qknorm_bwd_parts(int64_t tokens, int n_q, int n_k, int n_v, int D);
template <typename T>
void qknorm_rope_bwd(const T* dout, const T* x, const float* rstd, const T* wq, const T* wk, const float* cos_t,
                     const float* sin_t, T* dx, float* part_q, float* part_k, int nparts, int64_t tokens, int S,
                     int n_q, int n_k, int n_v, int D, int pos0, hipStream_t s);

// ------------------------------------------------------------------ mixture of experts (moe.hip)
// T tokens, Ne experts, k experts per token, C slots per expert, a = t * k + j token t's j-th choice.  All index
// tensors are int32; every kernel range-checks the indices it reads.  No float atomics: the same bits every run.
bool moe_route_supported(int Ne, int k);  // 2 <= Ne <= 256, 1 <= k <= min(8, Ne)
// Partial rows of probs_sum that moe_route_fwd writes (its grid).
int moe_route_parts(int64_t tokens, int Ne);
// logits [T, Ne] (finite or -inf, one finite value per row at least): idx [T, k] the k largest of a row in descending
// order, the lower expert first among equal values; gate [T, k] the softmax over those k; part [nparts, Ne] per-block
// sums over tokens of the full-row softmax, for reduce_parts.
template <typename T>
void moe_route_fwd(const T* logits, int32_t* idx, float* gate, float* part, int nparts, int64_t tokens, int Ne, int k,
                   hipStream_t s);
// dlogits [T, Ne]: gate_j (dgate_j - sum_i gate_i dgate_i) at the selected experts plus, with dprobs [Ne] (optional),
// p (dprobs - <dprobs, p>) with p the row's full softmax.
template <typename T>
void moe_route_bwd(const T* logits, const int32_t* idx, const float* gate, const float* dgate, const float* dprobs,
                   T* dlogits, int64_t tokens, int Ne, int k, hipStream_t s);
// slot [T, k] = e * C + pos or -1 (pos >= C: dropped), src [Ne * C] = a or -1, counts [Ne] before the capacity; pos
// is the number of earlier entries of the same expert in choice-major order (j first, then t).  ws: int32
// [moe_assign_blocks(T, k), Ne].  Ne * C < 2^31 (the caller checks).
int moe_assign_blocks(int64_t tokens, int k);
void moe_assign(const int32_t* idx, int32_t* slot, int32_t* src, int32_t* counts, int32_t* ws, int64_t tokens, int k,
                int Ne, int C, hipStream_t s);
// The sorted (dropless) layout: expert e's rows are [offsets[e], offsets[e + 1]) with offsets[e + 1] = offsets[e] +
// ceil128(counts[e]); slot [T, k] = offsets[e] + pos (-1 only for an expert outside [0, Ne)), src [rows] = a or -1
// (padding), tile_expert [rows / 128] the expert of a 128-row tile or -1 past offsets[Ne].  rows is a multiple of
// 128 that bounds offsets[Ne] (the caller checks).  ws as for moe_assign.
void moe_assign_sorted(const int32_t* idx, int32_t* slot, int32_t* src, int32_t* counts, int32_t* offsets,
                       int32_t* tile_expert, int32_t* ws, int64_t tokens, int k, int Ne, int rows, hipStream_t s);
// xe [nslots, E]: xe[s] = x[src[s] / k], zeros where src[s] < 0.  E * sizeof(T) % 16 == 0, 16-byte aligned pointers.
template <typename T>
void moe_gather_slots(const T* x, const int32_t* src, T* xe, int64_t nslots, int64_t tokens, int k, int E,
                      hipStream_t s);
// y [T, E]: y[t] = res[t] + sum_j w[t, j] ye[slot[t, j]] over the slots >= 0, fp32 in j order, one rounding; w
// (fp32 [T, k]) and res are optional.
template <typename T>
void moe_gather_tokens(const T* ye, const int32_t* slot, const float* w, const T* res, T* y, int64_t tokens, int k,
                       int64_t nslots, int E, hipStream_t s);
// One pass over the slots: dye[s] = gate[a] dy[t] (zeros for an empty slot) and dgate[a] = <dy[t], ye[s]>; dgate of
// a dropped entry is not written (the caller zero-fills it).
template <typename T>
void moe_combine_bwd(const T* dy, const T* ye, const float* gate, const int32_t* src, T* dye, float* dgate,
                     int64_t nslots, int64_t tokens, int k, int E, hipStream_t s);

// ------------------------------------------------------------------ elementwise
enum Activation : int { kActNone = 0, kActRelu = 1, kActGelu = 2 };
// Backward-only activation code: the saved tensor IS act'(pre) (a GELU forward
// GEMM wrote it with GemmArgs::aux_grad), so the backward is one multiply.
constexpr int kActSavedGrad = 3;
// Backward-only: the saved tensor is a 1-bit mask of a ReLU (+ dropout) output's nonzeros, [M][ld bytes], bit
// (col & 7) of byte col / 8 -- written by the forward GEMM (GemmArgs::bits) so the consumer's dgrad epilogue
// reads 1/16 of the bytes the saved bf16 output costs.
constexpr int kActReluBits = 4;

template <typename T>
void bias_act_dropout_fwd(const T* x, const T* bias, T* y, int64_t rows, int cols, int act, float p, uint64_t seed,
                          uint64_t offset, hipStream_t s);
template <typename T>
void bias_act_dropout_bwd(const T* dy, const T* saved, const T* bias, T* dx, int64_t rows, int cols, int act, float p,
                          uint64_t seed, uint64_t offset, hipStream_t s);
// Logit soft-capping y = cap * tanh(x / cap) (cap > 0) over `rows` rows of `cols` values, row r at r * ld of each
// tensor; y may be x.  The backward reads the saved output: dx = dy * (1 - (y / cap)^2); dx may be dy.
template <typename T>
void softcap_fwd(const T* x, int64_t ld_x, T* y, int64_t ld_y, int64_t rows, int64_t cols, float cap, hipStream_t s);
template <typename T>
void softcap_bwd(const T* dy, int64_t ld_dy, const T* y, int64_t ld_y, T* dx, int64_t ld_dx, int64_t rows,
                 int64_t cols, float cap, hipStream_t s);
int colsum_parts(int64_t rows, int64_t cols);
// Up to kColsumSegs equally shaped inputs whose stage-1 column sums run as one launch.
constexpr int kColsumSegs = 16;
struct ColsumSegs {
  const void* p[kColsumSegs] = {};
};
template <typename T>
bool column_sum_partial_multi(const ColsumSegs& segs, int nseg, int64_t rows, int cols, float* part, int nparts,
                              hipStream_t s);
// Stage 1 only: per-part column sums of `rows` rows into part[nparts][cols]
// (several inputs can write disjoint part slices and share one reduce_parts).
template <typename T>
void column_sum_partial(const T* x, int64_t rows, int cols, float* part, int nparts, hipStream_t s);
template <typename T>
void column_sum(const T* x, int64_t rows, int cols, float* part, int nparts, void* out, bool out_f32, bool accumulate,
                hipStream_t s);

// ------------------------------------------------------------------ GEMM
// kEpiStoreBf16 / kEpiStoreAct: the activation epilogue (bias, act, dropout,
// residual, aux) stored in the operand dtype (bf16 for gemm_bf16, fp32 for gemm_f32).
enum GemmEpilogue : int { kEpiStoreBf16 = 0, kEpiAccumF32 = 1, kEpiStoreF32 = 2, kEpiStoreAct = 0 };

struct GemmArgs {
  const void* A = nullptr;  // bf16
  const void* B = nullptr;  // bf16
  void* C = nullptr;        // bf16 or fp32 (epilogue)
  const void* bias = nullptr;  // bf16 [N] (kEpiStoreBf16 only)
  void* aux = nullptr;         // bf16 pre-activation output (optional)
  bool aux_grad = false;       // aux holds GELU'(pre) instead of pre (bf16 GEMMs, ACT = GELU)
  const void* res = nullptr;   // bf16 [M, ldr] added to the bf16 output (optional, kEpiStoreBf16)
  int64_t lda = 0, ldb = 0, ldc = 0;
  int64_t ldr = 0;             // row stride of res (0: ldc)
  // Activation backward in the bf16 epilogue (a dgrad GEMM whose output is the
  // gradient of an activation's output): C = acc [x dropout mask (p, seed,
  // offset: the forward's)] x act'(dact_in) x dact_scale.  dact_in is the
  // forward's saved pre-activation (GELU) or output (ReLU: its sign carries the
  // dropout mask too, so p = 0 and dact_scale = 1 / (1 - p)); row stride ldd.
  const void* dact_in = nullptr;
  int dact = 0;
  float dact_scale = 1.f;
  int64_t ldd = 0;
  int M = 0, N = 0, K = 0;
  bool a_kc = true;   // A stored [M, K] (true) or [K, M] (false)
  bool b_kc = true;   // B stored [N, K] (true) or [K, N] (false)
  int epi = kEpiStoreBf16;
  int act = kActNone;
  float p = 0.f;
  uint32_t threshold = 0;
  uint64_t seed = 0, offset = 0;
  int group_m = 8;  // tile-rows per group of the block -> tile order (L2 reuse of B tiles)
  // Split-K (plain bf16 output of an under-filled grid with a long K): the
  // K-tiles are divided among k_splits blocks per output tile, each writing
  // an fp32 partial into ws [k_splits][M][N]; a reduction adds them (+ res).
  int k_splits = 1;
  float* ws = nullptr;
  // Launch chunks of a larger GEMM (one round of tiles each): the chunk's
  // position in the full output, so the dropout mask (Philox counter
  // (row >> 2) * mask_ld + col) is the full matrix's.  mask_ld = 0: N.
  int mask_row0 = 0, mask_col0 = 0, mask_ld = 0;
  bool round_chunk = false;  // a chunk of a per-round launch: stays on the 256-row kernel even when small
  int width = 0;             // 256-row kernel block width forced by the caller (0: gemm_plan's rule)
  // K-segmented operands (deferred weight gradients: one GEMM over the
  // micro-batches of a step without concatenating them).  seg_k > 0: K-rows
  // [s*seg_k, (s+1)*seg_k) of A / B live at a_seg[s] / b_seg[s] (leading
  // dimensions lda / ldb); seg_k must be a multiple of 64.
  static constexpr int kMaxSegs = 16;
  int seg_k = 0;
  // Fused bias gradient of a weight-gradient GEMM (A = dY read as [K=T, M]):
  // rowsum[m] += sum_k A[k][m], fp32.  The 256 rows of a tile row are split
  // into 16-row slices summed by the blocks tn = 0..15 of that tile row, each
  // over the whole K (one writer per row: deterministic).  Needs
  // ceil(N / block width) >= 16 and k_splits == 1 (GemmPlan::rowsum_ok).
  float* rowsum = nullptr;
  // The same fold on the B side for the transposed weight-gradient GEMM
  // (C^T = X^T . dY, B = dY read as [K=T, N]): colsum[n] += sum_k B[k][n];
  // the W/16 16-column slices of a tile column are spread over its tile
  // rows, 2 per block (GemmPlan::colsum_ok: >= W/32 tile rows); with split-K
  // each split writes colsum_ws and one reduction adds them.
  float* colsum = nullptr;
  float* colsum_ws = nullptr;  // split-K: [k_splits][N] per-split column sums (the caller's workspace)
  // Transposed fp32 output (kEpiAccumF32 / kEpiStoreF32): element (m, n) of
  // the product goes to C[n * ldc + m] -- the weight gradient dW = (X^T dY)^T
  // lands in main_grad's [N_out, K_in] layout.
  bool trans_c = false;
  // A^T emission (forward GEMMs, A K-contiguous): the blocks also write
  // their A tiles transposed, at[k][m] (bf16, row stride ldat, 16-byte
  // aligned, m < M), from the LDS images they compute from -- each K-tile's
  // 8-row pieces shared out in rotation over the blocks of the tile row: X^T
  // for the layer's weight-gradient GEMM without a transposition pass
  // (tools/wgrad_layout_probe.py).
  void* at = nullptr;
  int64_t ldat = 0;
  // Forward ReLU + dropout (the EXTRA epilogue): also write the output's nonzero mask as bits (kActReluBits),
  // [M][ldbits bytes]; GemmPlan::bits_ok says whether this launch can.
  void* bits = nullptr;
  int64_t ldbits = 0;
  const void* a_seg[kMaxSegs] = {};
  const void* b_seg[kMaxSegs] = {};
};
bool gemm_supported(int64_t M, int64_t N, int64_t K);
// True if the forward GEMM with this epilogue can write A^T (GemmArgs::at).
bool gemm_emit_ok(int act, float p, bool aux);
// How gemm_bf16 launches g, decided once and in one order (the rule table is in gemm.hip, above GemmKnobs).
struct GemmPlan {
  bool big = false;   // the 256-row kernel (else the 128x128 one)
  int k_splits = 1;   // the split-K factor the caller may ask for (1 = none): it then provides g.ws with
                      // k_splits * M * N floats (and colsum_ws) and sets g.k_splits
  // the launch of g as given, its k_splits included
  int width = 256;    // block width of the 256-row kernel: 128 or 256
  bool extra = false;  // the staged epilogue: dropout and / or the pre-activation output
  int x = 0;          // 0, 1: also writes A^T (GemmArgs::at), 2: folds GemmArgs::colsum
  int side = 0;       // side operand of the bf16 store pass: 0 none, 1 res, 2 ReLU bit mask, 3 saved tensor
  bool kernel = true;  // false: no kernel takes this side operand in this operand layout (gemm_bf16 throws)
  bool by_rounds = false;  // one launch per round of tiles: `chunks` launches of `per` tile columns (along_n) or rows
  bool along_n = false;
  int per = 0, chunks = 0;
  // what the caller may ask for
  bool rowsum_ok = false;  // GemmArgs::rowsum can be folded (the wgrad layout, no split-K, >= 16 tile columns)
  bool colsum_ok = false;  // GemmArgs::colsum can be folded (B I-contiguous, fp32 out, >= W/32 tile rows)
  bool bits_ok = false;    // GemmArgs::bits can be written (forward ReLU + dropout, the staged epilogue)
};
GemmPlan gemm_plan(const GemmArgs& g);
// The operand layout as template arguments: f(a_kc, b_kc) gets two std::bool_constant tags.
template <typename F>
void with_layout(bool a_kc, bool b_kc, F&& f) {
  if (a_kc && b_kc) f(std::true_type{}, std::true_type{});
  else if (a_kc) f(std::true_type{}, std::false_type{});
  else if (b_kc) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}
// The 256-row GEMM has one main loop, the whole-tile ping-pong (gemm.hip, above gemm256_kernel, also
// names what it was compared against); the switches below select between live paths (tests, A/B tools).
void gemm_set_width(int w);    // 256-row GEMM block width: 0 auto, 128, 256
void gemm_set_rounds(int on);  // 1: multi-round grids launched one round at a time (default), 0: one launch
void gemm_set_splitk(int n);  // split-K factor: 0 off, 1 auto (GemmPlan::k_splits), n >= 2 forced (A/B tools)
void gemm_bf16(const GemmArgs& g, hipStream_t s);
// Grouped GEMMs over expert-sorted rows (gemm_grouped.hip): R rows in 128-row tiles, tile_expert [R / 128] the
// expert of a tile (-1: the tile stores zeros), wptr [Ne] a device table of the experts' bf16 weight pointers.
// R % 128 == 0, Nout % 128 == 0, Kred % 64 == 0 (grouped_gemm_supported).
bool grouped_gemm_supported(int64_t R, int64_t Nout, int64_t Kred);
// C[R, Nout] = A[R, Kred] . op(W_e): w_kc, W_e is [Nout, Kred] (the forward); otherwise [Kred, Nout] (the dgrad).
void grouped_gemm_rows(const bf16_t* A, const int64_t* wptr, const int32_t* tile_expert, bf16_t* C, int64_t R,
                       int64_t Nout, int64_t Kred, int Ne, bool w_kc, hipStream_t s);
// dW_e[N, K] (fp32) = or += dY[rows_e, N]^T . X[rows_e, K] with rows_e = [offsets[e], offsets[e + 1]), whole 128-row
// tiles.  dW_e is optr[e] (a device table) or, with optr null, obase + e * N * K.  An expert without rows is
// zero-filled, or left alone when accumulating.  N % 128 == 0, K % 128 == 0.
void grouped_gemm_wgrad(const bf16_t* dY, const bf16_t* X, const int32_t* offsets, const int64_t* optr, float* obase,
                        int64_t R, int64_t N, int64_t K, int Ne, bool accumulate, hipStream_t s);
// Same interface with fp32 operands (and fp32 bias / res / aux / C): v_mfma_f32_32x32x2_f32.
bool gemm_f32_supported(int64_t M, int64_t N, int64_t K);
void gemm_f32(const GemmArgs& g, hipStream_t s);

// ------------------------------------------------------------------ attention
struct AttnArgs {
  const void* q = nullptr;  // bf16, element (b, s, h, d) at b*S*ld_qkv + s*ld_qkv + h*D + d
  const void* k = nullptr;
  const void* v = nullptr;
  void* o = nullptr;        // bf16 [B, S, H, D], token stride ld_o
  const void* dout = nullptr;
  void* dq = nullptr;       // same layout as q/k/v (packed dQKV)
  void* dk = nullptr;
  void* dv = nullptr;
  float* lse = nullptr;     // [B, H, S]
  float* delta = nullptr;   // [B, H, S]
  int64_t ld_qkv = 0, ld_o = 0;      // token strides (elements)
  int64_t sb_qkv = 0, sh_qkv = 0;    // batch / head strides of q, k, v (and dq, dk, dv)
  int64_t sb_o = 0, sh_o = 0;        // batch / head strides of o and dout
  int B = 0, H = 0, S = 0, D = 0;
  float scale = 1.f, p = 0.f;
  uint32_t threshold = 0;
  uint64_t seed = 0, offset = 0;
  bool causal = false;
  // valid keys (0 = all S): keys >= kv_len are masked out (a zero-padded
  // non-causal sequence; fp32 kernels)
  int kv_len = 0;
  // long-sequence kernels with dropout: keep bits, one uint32 per (b*h, 32-query
  // block, key) written by the forward and read by the backward
  uint32_t* dmask = nullptr;
  // Grouped-query attention: query head h reads K and V of head h / group (k and v hold H / group heads
  // with q's strides).  Everything on the query side -- q, o, dout, dq, lse, delta, the Philox counters,
  // dmask -- keeps query-head indexing.  The dK / dV kernels keep one block per QUERY head and store its
  // partial at dk / dv + b*sb_dkv + s*ld_dkv + h*sh_dkv; 0 (group == 1) means q's strides, so dk / dv are
  // then the gradients themselves.  With group > 1 the caller points dk / dv at a scratch of H heads and
  // sums each group afterwards (gqa_reduce_dkv).
  int group = 1;
  uint32_t group_rcp = 1u << 20;  // ceil(2^20 / group): set by attn_resolved (kv_head)
  int64_t ld_dkv = 0, sb_dkv = 0, sh_dkv = 0;
  // Sliding-window attention (bf16 attention.hip, causal only): query i sees the `window` keys (i - window, i];
  // 0 = no window.  Kept the LAST member: no other member's offset in the kernel-argument segment moves.
  int window = 0;
  // Logit soft-capping (bf16 attention.hip's generic kernels): the scaled score s becomes softcap * tanh(s /
  // softcap) before the masks and the softmax; 0 = no cap, else a finite float > 0.  Appended after `window` for
  // the same reason.
  float softcap = 0.f;
  // Document-masked attention (bf16 attention.hip's generic kernels, causal only): rows 0 and 1 of one int32
  // [B, 2, S] tensor, so batch b's S entries start at doc_start / doc_end + b * 2 * S.  Query i sees the keys
  // [doc_start[i], i] (and inside the window, if any); key j is seen by the queries [j, doc_end[j]).  Both are
  // non-decreasing along a row.  nullptr = no documents.  Appended after `softcap` for the same reason.
  const int32_t* doc_start = nullptr;
  const int32_t* doc_end = nullptr;
  // Attention sinks (bf16 attention.hip's generic kernels): fp32 [H], one learned logit per QUERY head that joins
  // the softmax normalisation (after the cap and the masks, neither scaled nor capped) and has no value vector;
  // lse is then the log-sum-exp over the scores and the sink.  nullptr = no sinks; -inf = no sink for that head.
  // Only the forward reads it (the backward's P = exp(s - lse) is already right).  Appended after `doc_end` for
  // the same reason.
  const float* sinks = nullptr;
};
// K / V head of query head h: h / group as a scalar multiply by ceil(2^20 / group) and a shift instead of a
// division.  Exact for every h when group == 1 (the 64-bit product is h * 2^20) and while h * group < 2^20
// otherwise, which attn_group_ok checks for the callers (H <= 1024 always passes).
inline bool attn_group_ok(int64_t H, int64_t group) {
  return group >= 1 && H % group == 0 && (group == 1 || H * group < (int64_t(1) << 20));
}
#if defined(__HIPCC__)
__device__ __forceinline__ int kv_head(const AttnArgs& a, int h) {
  return (int)(((uint64_t)(uint32_t)h * a.group_rcp) >> 20);
}
// Where the dK / dV epilogue of block (batch * H + head) = bh stores: the two head bases and the token
// stride.  The dK / dV kernels of attention.hip are at their scalar-register limit through the main loop
// (100-106 SGPRs, the S = 128 backward with spills), so the epilogue reads what only it needs (dk, dv, the
// store strides, H) from the kernel-argument segment when the loop is over instead of holding it from the
// start.  (attention_long.hip's dK / dV kernels use 48-58 SGPRs and read a.sb_dkv ... in the plain way.)
//
// kArgOffset is the byte offset of the kernel's by-value AttnArgs parameter in its kernel-argument segment
// and must be given at every call: 0 for a kernel whose FIRST parameter is the AttnArgs (explicit arguments
// start the segment, in declaration order).  A kernel with anything before its AttnArgs must pass that
// parameter's offset, or these helpers read another argument's bytes.
struct DkvDst {
  bf16_t* dk;
  bf16_t* dv;
  int64_t ld;
};
template <int kArgOffset>
__device__ __forceinline__ const __attribute__((address_space(4))) AttnArgs* attn_args_late() {
  static_assert(kArgOffset >= 0 && kArgOffset % alignof(AttnArgs) == 0, "offset of an AttnArgs kernel parameter");
  typedef const __attribute__((address_space(4))) char* BytePtr;
  typedef const __attribute__((address_space(4))) AttnArgs* ArgPtr;
  ArgPtr ap = (ArgPtr)((BytePtr)__builtin_amdgcn_kernarg_segment_ptr() + kArgOffset);
  asm volatile("" : "+s"(ap));  // opaque from here on: loads through ap cannot move above this point
  return ap;
}
template <int kArgOffset>
__device__ __forceinline__ DkvDst dkv_dst(int bh) {
  const auto* ap = attn_args_late<kArgOffset>();
  const int H = ap->H, b = bh / H, h = bh - b * H;
  const int64_t off = (int64_t)b * ap->sb_dkv + (int64_t)h * ap->sh_dkv;
  return DkvDst{reinterpret_cast<bf16_t*>(ap->dk) + off, reinterpret_cast<bf16_t*>(ap->dv) + off, ap->ld_dkv};
}
// The dQ base of block bh, read late in the same way.
template <int kArgOffset>
__device__ __forceinline__ bf16_t* dq_dst(int bh) {
  const auto* ap = attn_args_late<kArgOffset>();
  const int H = ap->H, b = bh / H, h = bh - b * H;
  return reinterpret_cast<bf16_t*>(ap->dq) + (int64_t)b * ap->sb_qkv + (int64_t)h * ap->sh_qkv;
}
#endif
// Resolves the dK / dV store strides' default (q's) and checks the group; every attention launcher calls it.
inline AttnArgs attn_resolved(const AttnArgs& ai) {
  AttnArgs a = ai;
  if (a.group < 1) a.group = 1;
  a.group_rcp = ((1u << 20) + (uint32_t)a.group - 1) / (uint32_t)a.group;
  if (a.ld_dkv == 0 && a.sb_dkv == 0 && a.sh_dkv == 0) {
    a.ld_dkv = a.ld_qkv; a.sb_dkv = a.sb_qkv; a.sh_dkv = a.sh_qkv;
  }
  return a;
}
bool attention_supported(int S, int D);
// S == 128 backward: fused one-pass kernel (1, default) or delta + dK/dV + dQ kernels (0).
void attention_set_fused_bwd(int on);
void attention_fwd(const AttnArgs& a, hipStream_t s);
void attention_bwd(const AttnArgs& a, hipStream_t s);
// The sinks' gradient, after attention_bwd (which leaves delta): dsinks[h] (+)= -sum_{b,i} exp(sinks[h] -
// lse[b,h,i]) * delta[b,h,i], fp32, one block per head adding in a fixed order (no atomics: the same bits on
// every run).  lse, delta: [B, H, S]; sinks, dsinks: [H].  accumulate: add to dsinks (an fp32 main_grad view).
void attention_dsink(const float* lse, const float* delta, const float* sinks, float* dsinks, int B, int H, int S,
                     bool accumulate, hipStream_t s);
// fp32 q/k/v/o (v_mfma_f32_32x32x2_f32): S % 32 == 0, D == 64; "key-quad" dropout layout.
bool attention_f32_supported(int S, int D);
// bf16, D == 64, S >= 256, S % 64 == 0 (attention_long.hip): 32x32x16 MFMA, stored dropout bits.
bool attention_long_supported(int S, int D);
// Keep words made inside the forward kernel (default) or by their own kernel first.
void attention_long_set_fused_rng(bool on);
void attention_long_fwd(const AttnArgs& a, hipStream_t s);
// The forward reading keep words already in a.dmask (made by an earlier forward of the same Philox draw:
// a checkpoint recompute) instead of making them.
void attention_long_fwd_words(const AttnArgs& a, hipStream_t s);
void attention_long_bwd(const AttnArgs& a, hipStream_t s);
void attention_f32_fwd(const AttnArgs& a, hipStream_t s);
void attention_f32_bwd(const AttnArgs& a, hipStream_t s);

// ------------------------------------------------------------------ loss
// t_offset: logits are vocabulary columns [t_offset, t_offset + V) (split decoder).
template <typename T>
void cross_entropy_fwd(const T* logits, const int64_t* target, int64_t rows, int64_t V, int64_t ld,
                       int64_t ignore_index, float* loss, float* lse, hipStream_t s, int64_t t_offset = 0);
// Mean CE in two launches (row losses, then a one-block masked mean): loss[0] =
// mean over valid targets; weight[r] = valid / count (the backward's row scale).
template <typename T>
void cross_entropy_mean_fwd(const T* logits, const int64_t* target, int64_t rows, int64_t V, int64_t ld,
                            int64_t ignore_index, float* loss_row, float* lse, float* weight, float* loss,
                            hipStream_t s);
// lse / row_scale read with strides ld_lse / ld_rs (floats); stat_out: (lse,
// scale) written to nslot fp32 words per row (split-decoder gradient slots).
template <typename T>
void cross_entropy_bwd(const T* logits, const int64_t* target, const float* lse, const float* scale,
                       const float* row_scale, int64_t rows, int64_t V, int64_t ld, int64_t ld_out,
                       int64_t ignore_index, T* dlogits, int64_t zero_to, hipStream_t s, int64_t t_offset = 0,
                       int64_t ld_lse = 1, int64_t ld_rs = 1, float* stat_out = nullptr, int64_t ld_stat = 0,
                       int nslot = 0);
// Split-decoder head forward: out[r] = [x[r] (E values) | lse, target logit, 0 ...]
// (nslot fp32 words); E * sizeof(T) % 16 == 0, 16-byte aligned rows.
template <typename T>
void vsplit_head_fwd(const T* logits, int64_t ld, int64_t rows, int64_t V, const int64_t* target, const T* x,
                     int64_t ldx, int64_t E, T* out, int64_t ldo, int nslot, hipStream_t s);
// Split-decoder tail forward: full lse per row from this slice and the head's
// slot statistics (stats: lse_a, t_a at stride ld_st floats), the mean loss
// into loss[0] and per-row weights valid / count.
template <typename T>
void vsplit_tail_fwd(const T* logits, int64_t ld, int64_t rows, int64_t V, const int64_t* target, int64_t t_offset,
                     int64_t ignore_index, const float* stats, int64_t ld_st, float* lse, float* loss_row,
                     float* weight_row, float* loss, hipStream_t s);

// ------------------------------------------------------------------ embedding
// pe (optional): position table [>= seq_len, E], fp32 (pe_f32) or T.
template <typename T>
void embedding_fwd(const int64_t* tokens, const T* weight, const void* pe, bool pe_f32, T* out, int64_t rows,
                   int seq_len, int E, int64_t V, float scale, float p, uint64_t seed, uint64_t offset, hipStream_t s);
// dpe (optional): fp32 [>= seq_len, E] learned-position gradient, += the masked rows by position.
template <typename T>
void embedding_bwd(const int64_t* tokens, const T* dout, float* dweight, int64_t rows, int E, int64_t V, float scale,
                   float p, uint64_t seed, uint64_t offset, hipStream_t s, float* dpe = nullptr, int seq_len = 0);

// ------------------------------------------------------------------ optimizer
struct AdamHyper {
  float lr = 1e-3f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f, weight_decay = 0.f;
  float bias_correction1 = 1.f, bias_correction2 = 1.f;
  float max_norm = 0.f;  // <= 0: no clipping
  int adamw = 0;
};
int sumsq_parts(int64_t n);
void sumsq(const float* g, int64_t n, float* partial, int nparts, float* out, hipStream_t s);
// 0: grid-stride kernel, 2 vectors of loads in flight per thread;
// 1: one-shot tiles of 4 vectors per thread (default, ~10 % faster).
void adam_set_variant(int v);
template <typename M>
void adam_step(float* master, M* model, const float* grad, float* m, float* v, int64_t n, const AdamHyper& h,
               const float* sumsq_ptr, hipStream_t s);

// ------------------------------------------------------------------ misc
void gpu_sleep(int64_t microseconds, hipStream_t s);
// out[c * ldo + r] = x[r * ldx + c], 2-byte elements; rows, cols, ldx, ldo
// multiples of 8 and both pointers 16-byte aligned (the caller checks).
void transpose_b16(const uint16_t* x, int64_t rows, int64_t cols, int64_t ldx, uint16_t* out, int64_t ldo,
                   hipStream_t s);

}  // namespace mipipe
