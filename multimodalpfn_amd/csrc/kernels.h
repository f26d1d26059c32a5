// Internal launch interface of the MMPFN HIP kernels (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "weight_pack.h"

namespace mmpfn {

// PREC_F32 (parity mode): every large contraction on bf16 MFMA with both operands split into
// bf16 hi + lo planes, x = hi + lo to 2^-17, and the three significant products hi.hi + hi.lo +
// lo.hi accumulated in fp32 (the dropped lo.lo term is 2^-16 relative) -- 3 bf16 MFMAs at 16x the
// fp32-input rate; PREC_F32_MFMA: the same forward on fp32-input MFMA (exact fp32 fma chains)
// PREC_F16: the reference's fp16 autocast -- the inter-kernel state X stored in fp16, every layer
// contraction on fp16 MFMA operands (the item attention's P.V on bf16: its P needs bf16's range), fp32
// accumulation, LayerNorm and softmax statistics (featrow / rowgemm / mlp_rows / attention_pipe F16 forms)
// PREC_*_F8 / PREC_*_F8E5: the 16-bit modes with the sample-axis attention's P.V on block-scaled fp8
// MFMA (V^T e4m3; P e4m3 / e5m2; attention_pipe.hip) -- config E's fp8 path, opt-in
enum Prec : int {
  PREC_F32 = 0,
  PREC_BF16 = 1,
  PREC_F32_MFMA = 2,
  PREC_BF16_F8 = 3,
  PREC_BF16_F8E5 = 4,
  PREC_F16 = 5,
  PREC_F16_F8 = 6,
  PREC_F16_F8E5 = 7
};
// the precision the layer kernels run in, and the fp8 P.V variant (0: none)
inline int base_prec(int p) {
  return p == PREC_BF16_F8 || p == PREC_BF16_F8E5 ? PREC_BF16 : p == PREC_F16_F8 || p == PREC_F16_F8E5 ? PREC_F16 : p;
}
inline int f8_of(int p) {
  return p == PREC_BF16_F8 || p == PREC_F16_F8 ? 1 : p == PREC_BF16_F8E5 || p == PREC_F16_F8E5 ? 2 : 0;
}
inline bool prec_ok(int p) { return p >= PREC_F32 && p <= PREC_F16_F8E5; }
inline bool prec16(int p) { return p == PREC_BF16 || p == PREC_F16; }  // a 16-bit performance mode (base)

// element type of a launcher's operand; a combination with no kernel returns hipErrorInvalidValue
enum class DType : int { F32, BF16, F16 };

enum Epi : int {
  EPI_STORE = 0,      // C[row] = act(acc + bias)
  EPI_ITEM_QKV = 1,   // scatter to attention Q / K / V^T layouts: row m -> (b = m / a_rdiv, pos = a_roff + m % a_rdiv)
                      //   Q [b][h][pos][32] (S rows), K [b][h][pos][32] (Npad rows), V^T [b][h][32][Npad]
  EPI_RES_LN = 3,     // X[row] = LayerNorm(X[row] + acc), N == 192 (no affine)
  EPI_GLU = 4,        // paired tiles: out = a * sigmoid(b) (weights row-interleaved)
  EPI_REMAP = 5,      // grouped: dest row = (m / rdiv2) * rmul2 + z * zmul + m % rdiv2
};

enum Act : int { ACT_NONE = 0, ACT_GELU = 1 };

struct GemmArgs {
  // A: logical row m -> memory row (m / a_rdiv) * a_rmul + (m % a_rdiv) * a_rmul2 + a_roff
  const void* A;
  int64_t lda;
  int64_t a_rdiv, a_rmul, a_rmul2, a_roff;
  int64_t a_zstride;  // elements between groups (blockIdx.z)
  const void* W;      // [N][K] compute dtype, row-major (PREC_F32: the bf16 hi plane)
  int64_t w_zstride;
  int64_t w_lo_off;   // PREC_F32: elements from W to its bf16 lo plane
  const float* bias;  // [N] or null
  int64_t b_zstride;
  int M, N, K;
  int act;
  // plain / remap / glu output
  void* C;
  int64_t ldc;
  int64_t c_zstride;
  int64_t rdiv2, rmul2, zmul;
  // attention scatter
  void* q;  // Q  [B][H][S][d]
  void* k;  // K  [B][H][Npad][d]
  void* v;  // V^T[B][H][d][Npad]
  int S, Npad, T, H;
  // LN epilogue
  float* X;  // residual in / normalised out, ld = 192
  float ln_eps;
};

// Launch C = A . W^T with the given epilogue.  `a_f32` says whether A is stored
// as fp32 (otherwise bf16); `out_f32` likewise for C / scatter targets.  Instantiated: PREC_F32_MFMA every
// epilogue; PREC_F32 STORE / GLU / REMAP (the mixers; the layers run rowgemm3.hip), both fp32 in and out; PREC_BF16
// STORE and GLU (bf16 in and out), REMAP (bf16 in, fp32 out), ITEM_QKV (fp32 in, bf16 out), RES_LN (bf16 in, fp32
// out).  Anything else: hipErrorInvalidValue.
hipError_t launch_gemm(const GemmArgs& a, int prec, int epi, bool a_f32, bool out_f32, int groups,
                       hipStream_t st);

// MGM head bank, bf16 or fp16 (t: A, W and C): C[M][N/2] = GLU(A[M][K] . W^T + bias) with W rows GLU-interleaved in 16-row
// blocks (capi.cpp); large-tile, XCD-ordered (gemm.hip gemm_glu_big_kernel); N % 256 == 0, K % 64 == 0
// MGM per-head down-projection (bf16, E = 192): C[(r / n_mod) * nheads n_mod + z n_mod + r % n_mod][E] =
// A[r][z K .. z K + K) (row stride lda) . W[z][E][K]^T + bias[z][E]; A and W in t (bf16 or fp16), C in c_t: fp32 or t
hipError_t launch_gemm_remap_big(const void* A, int64_t lda, const void* W, const float* bias, void* C, DType c_t,
                                 int M, int K, int nheads, int n_mod, int E, hipStream_t st, DType t = DType::BF16);
hipError_t launch_gemm_glu_big(const void* A, const void* W, const float* bias, void* C, int M, int N, int K,
                               hipStream_t st, DType t = DType::BF16);

// fused MLP sublayer of the fp32 modes: X <- LN(X + GELU(X W1^T) W2^T); PREC_F32_MFMA: W1 [Fh][E], W2 [E][Fh]
// fp32; PREC_F32: W1 natural and W2 in the pack_mlp2_perm order, each as bf16 hi | lo planes
hipError_t launch_mlp_fused(float* X, const void* W1, const void* W2, int64_t M, int E, int Fh, float eps, int prec,
                            hipStream_t st);

// row-resident MLP sublayer (the 16-bit modes, mlp_rows.hip): W1 [Fh][E] bf16, W2 [E][Fh] bf16 in the
// permuted hidden order of pack_mlp2_perm (capi.cpp); Fh % 32 == 0, E == 192
// W1perm: W1 with its K (feature) order permuted to the Y^T lane layout (capi.cpp pack_mlp1_perm);
// O / Wout non-null: X <- LN(X + O Wout^T) first (the item-attention out-projection, fused)
// x_t: the state's type, fp32 (bf16 operands) or fp16 (PREC_F16: X / O fp16, W1 natural, W2 (pack_mlp2_perm) and
// Wout with f16_row_perm-ordered rows)
hipError_t launch_mlp_rows(void* X, const void* W1perm, const void* W2perm, int64_t M, int E, int Fh, float eps,
                           hipStream_t st, const void* O = nullptr, const void* Wout = nullptr,
                           DType x_t = DType::F32);

// one set of rows through one q|k|v (N = 576) or q (N = 192) weight [N][192], for the row-resident projections:
// logical row m -> memory row (m / rdiv) * rmul + (m % rdiv) * rmul2 + roff of X; scattered to b = m / rdiv,
// pos = roff + m % rdiv of Q [b][h][pos][32], K [b][h][pos][32] (Npad rows) and V^T [b][h][32][Npad]
struct RowSet {
  int64_t rdiv, rmul, rmul2, roff;
  int M, N;
  const void* W = nullptr;  // the launcher's operand form (launch_proj3_qkv: the hi plane of split_bf16)
  int64_t w_lo = 0;         // launch_proj3_qkv: elements from W to its lo plane
};

// row-resident item-attention projections (bf16, K = 192, rowgemm.hip):
//   QKV: one or two row sets of X (train rows: q|k|v, test rows: q; W [N][192]) in ONE launch, the second set's blocks
//        last; one set launches that set's blocks alone
//   RES_LN: X <- LN(X + O . W^T), O [M][192] bf16, W [192][192] bf16
//   x_t: the state's type, fp32 (bf16 W) or fp16 (PREC_F16: X fp16, W fp16); Q / K and V^T are bf16 in both;
//   RES_LN: O bf16 / X fp32, or both fp16 with W rows in f16_row_perm order (weight_pack.h)
hipError_t launch_rowgemm_qkv(const void* X, const RowSet* sets, int nset, void* q, void* k, void* vt, int S, int Npad,
                              int H, hipStream_t st, DType x_t = DType::F32);
// C = (ln ? LayerNorm(A) : A) . W^T + bias: A fp32, bf16 or fp16 (a_t) [M][192], W [N][192] bf16, C bf16 [M][N], N % 64 == 0;
// with CT: outputs [vt_from, N) transposed per group of Mk rows into CT [M / Mk][N - vt_from][Mk] (Mk % 32 == 0),
// C then [M][vt_from]
hipError_t launch_rowgemm_ln_store(const void* A, DType a_t, const void* W, const float* bias, void* C, int64_t M,
                                   int N, float eps, bool ln, hipStream_t st, void* CT = nullptr, int vt_from = -1,
                                   int Mk = 0);
hipError_t launch_rowgemm_resln(const void* O, const void* W, int64_t M, void* X, float eps, hipStream_t st,
                                DType x_t = DType::F32);

// parity-mode (x3 split-bf16) row-resident projections of width 192 (rowgemm3.hip), fp32 in and out:
// W = the hi plane [N][192] of split_bf16 (weight_pack.h), its lo plane at W + w_lo elements.
//   QKV: up to two row sets of X in one launch (fp32 Q / K / V^T)
//   RES_LN: X <- LN(X + O . W^T), O fp32 [M][192]
hipError_t launch_proj3_qkv(const float* X, const RowSet* sets, int nset, void* q, void* k, void* vt, int S, int Npad,
                            int H, hipStream_t st);
hipError_t launch_proj3_resln(const float* O, const void* W, int64_t w_lo, int64_t M, float* X, float eps,
                              hipStream_t st);

// row-resident attention-between-features sublayer (the 16-bit modes, featrow.hip): one wave per
// table row, T <= 64 tokens; `pack` (capi.cpp pack_feat_rows) = LDS images with 416-B rows:
// per head [96][FEAT_IMG_STRIDE] (Wq rows permuted & scaled by log2(e)/sqrt(32) | Wk rows
// permuted | Wv), then the out-projection [192][FEAT_IMG_STRIDE] with permuted head columns
// (FEAT_IMG_STRIDE, FEAT_PACK_LAYER: weight_pack.h)
// X holds M members [M][T][S][E]; one launch covers the M*S rows
// x_t: the state's type, fp32 (bf16 images) or fp16 (PREC_F16: the fp16 images with the out-projection rows permuted,
// pack_feat_rows res_perm)
// last: only token T-1 of every row is computed and stored (the pruned last layer; bit for bit the full form's)
hipError_t launch_feat_rows(void* X, const void* pack, int S, int T, int M, int E, int H, float eps, hipStream_t st,
                            DType x_t = DType::F32, bool last = false);

// ---- attention -------------------------------------------------------------------
// generic MFMA attention over a batch (blockIdx.z) of independent sequences:
//   Q  [b][h][pos][32] (row = s0 + q), K [b][kvh][key][32], V^T [b][kvh][32][kpad],
//   O row = b * o_bstride + (s0 + q) * o_qstride, element row*(H*32) + h*32 + d.
struct AttnArgs {
  const void* q;
  const void* k;
  const void* vt;
  void* o;
  int64_t q_bstride, q_hstride, kv_bstride, kv_hstride;
  int kpad;
  int64_t o_bstride, o_qstride;
  int s0, nq, nk, kvh_fixed, H;
};
// one wave per block: PREC_BF16, PREC_F32 (split-bf16 products; the T <= 64 self-attention of the feature sublayer
// takes its one-wave-per-(row, head) kernel) and PREC_F32_MFMA; four waves: PREC_F32_MFMA only
hipError_t launch_attn(const AttnArgs& a, int batches, int prec, int waves_per_block, hipStream_t st);

// sample-axis (item) attention of one layer, the one entry to it (attention.hip):
//   own-head rows [a0, a0+na) of every head against that head's K/V, and rows [b0, b0+nb) of
//   every head against K/V head kvb (nb = 0: none); keys [0, nk), Npad % 64 == 0.
//   kv_bstride > 0: K / V^T hold head 0 only, column blocks kv_bstride elements apart (train-KV
//   cache; then na = 0 and kvb = 0)
// base_prec (PrecMode::base) picks the kernel and the element type of q, k, vt and out:
//   PREC_BF16, PREC_F16  the software-pipelined kernel in one launch (attention_pipe.hip, attn_pipe_kernel):
//     f8 != 0: P.V and the row sums on block-scaled fp8 MFMA with vt8 = V^T in e4m3 (launch_vt_fp8), P in
//     e4m3 (1) or e5m2 (2); vt (bf16) still serves the exact re-run path
//     qk_t: Q and K bf16, or fp16 (S on the f16 MFMA; then o_t is fp16 too: the fp16 tap); o_t: O bf16 or fp16
//     (PREC_F16's forward: bf16 Q / K, fp16 O); V^T stays bf16
//   PREC_F32             attn_item3_kernel on fp32 Q / K / V^T (split bf16 three-product MFMAs), fp32 O, one launch
//   PREC_F32_MFMA        attn_item_kernel<0, 4> on fp32 operands: the own-head rows in one launch, the shared-KV rows
//     in a second (a set of no rows: no launch)
//   the prescale, fp8 and element-type fields apply to the 16-bit modes only
struct AttnLayerArgs {
  const void* q;
  const void* k;
  const void* vt;
  void* out;
  int S, T, H, Npad, nk;
  int a0, na;                  // own-head query rows
  int b0, nb, kvb;             // shared-KV query rows against kv head kvb
  int64_t kv_bstride = 0;      // 0: no cache stride (K / V^T hold every head)
  bool q_prescaled = false;    // Q already scaled by log2(e)/sqrt(32)
  const void* vt8 = nullptr;
  int f8 = 0;
  DType qk_t = DType::BF16, o_t = DType::BF16;
};
constexpr int ATTN_ITEM_QPB = 256;  // queries per task of the 16-bit and PREC_F32 kernels' task maps
hipError_t launch_attn_layer(const AttnLayerArgs& a, int base_prec, hipStream_t st);
// bf16 -> e4m3 (saturating) of n elements (n % 8 == 0): the F8 attention's V^T operand
hipError_t launch_vt_fp8(const void* vt, void* vt8, int64_t n, hipStream_t st);

// ---- encoders / decoder ------------------------------------------------------------
struct SlotParams {  // per (group, slot): how to transform raw column -> model input
  int src;           // source column or -1 (zero fill)
  float fill;        // NaN/inf replacement (train nanmean)
  float lo, hi;      // soft outlier bounds (or -inf/+inf when disabled)
  float mean, sd;    // train z-score (sd already includes the +1e-20)
  float scale;       // 1 if the slot's column is used (non-constant after normalisation), else 0
};
// encoder statistics of one member: x-encoder slots [G * fpg] (train rows [0, N) of S) and the label mean
// ymean[0] over y[0, ny), one launch
hipError_t launch_encode_stats(const float* x /*[S][F]*/, int S, int F, int N, int G, int fpg, float sigma,
                               SlotParams* slots, const float* y, int ny, float* ymean, hipStream_t st);
// the member's input state X [T][S][E] (T = G + C + 1), fp32 or fp16 (x_t): x tokens from the slots, mixer
// tokens + positional rows, the label token (labels y[0, N); rows >= N are test rows); NaN -> flag bits 1 / 2
hipError_t launch_assemble(const float* x, int S, int F, int G, int fpg, int nf, const SlotParams* slots,
                           const float* w_enc /*[E][2nf]*/, const float* posemb /*[G+C][E]*/,
                           const float* tok /*[S][C][E]*/, int C, const float* y, int N, const float* uniq, int U,
                           const float* yw /*[E][2]*/, const float* yb, const float* ymean, void* X, DType x_t, int E,
                           int* flag, hipStream_t st, bool value_target = false);  // value_target: uniq / U unused
hipError_t launch_pos_emb(const float* rnd /*[n][E/4]*/, int n, const float* w /*[E][E/4]*/,
                          const float* b, float* out /*[n][E]*/, int E, hipStream_t st);
// M members' decoders: X + m*xm [Q][E] -> out + m*om [Q][n_out]; scratch >= M*(Fh/64)*Q*n_out floats
hipError_t launch_decoder(const float* X /*[Q][E]*/, int Q, const float* w1t /*[E][Fh]*/, const float* b1, int Fh,
                          const float* w2, const float* b2, int n_out, float* out, int E, hipStream_t st, int M,
                          int64_t xm, int64_t om, float* scratch);

// the 16-bit modes' decoder on MFMA: X (x_t) fp32 (bf16 operands) or fp16 (fp16 operands); W1 [Fh][E] and W2p
// [16][Fh] (pack_mlp2_perm order, rows >= n_out zero) in the operand type; Fh % 128 == 0, n_out <= 16
hipError_t launch_decoder_mfma(const void* X, DType x_t, int Q, const void* W1, const float* b1, int Fh, const void* W2p,
                               const float* b2, int n_out, float* out, int E, hipStream_t st, int M, int64_t xm,
                               int64_t om);
// the value-target decoder (decoder_wide.hip), any n_out: X + m*xm [Q][E] in x_t -> hidden [M*Q][Fh] in op_t (a
// workspace) -> out [M][Q][n_out] fp32; W1 [Fh][E] and W2 [n_out][Fh] natural, in op_t.  (x_t, op_t): (F32, F32) on
// fp32-input MFMA, (F32, BF16), (F16, F16); E % 32 == 0, Fh % 32 == 0
hipError_t launch_decoder_wide(const void* X, DType x_t, int Q, int64_t xm, int M, const void* W1, const float* b1,
                               int Fh, const void* W2, const float* b2, int n_out, DType op_t, void* hidden, float* out,
                               int E, hipStream_t st);
// PREC_F16 state conversions: nb blocks of per_block elements (per_block % 4 == 0) at the given block
// strides (elements); the state [T][S][E] fp16 -> the reference order [S][T][E] fp32
hipError_t launch_f32_to_f16(const float* in, int64_t in_bstride, void* out, int64_t out_bstride, int64_t per_block,
                             int nb, hipStream_t st);
hipError_t launch_f16_to_f32(const void* in, int64_t in_bstride, float* out, int64_t out_bstride, int64_t per_block,
                             int nb, hipStream_t st);
hipError_t launch_state_f16_to_f32(const void* X, float* out, int S, int T, int E, hipStream_t st);
// Row embeddings (embrows.hip): rows [r0, r0 + n) of the target token's column T-1 of M members' states
// X [M][T][S][E] (x_t: fp32 or fp16) -> out fp32 [M][n][E], 16 bytes of the state per thread; X and out 16-byte
// aligned, E % 8 == 0
hipError_t launch_target_rows(const void* X, DType x_t, int S, int T, int E, int M, int r0, int n, float* out,
                              hipStream_t st);

hipError_t launch_aggregate(const float* logits /*[M][Q][n_out]*/, int M, int Q, int n_out,
                            const int* perms /*[M][n_cls] or null*/, int n_cls, float temp, int avg_before,
                            const float* class_weights /*[n_cls] or null*/, float* probs, hipStream_t st);

// Bar-distribution head (barhead.hip): M members' logits [M][Q][B] -> the ensemble's final log-probabilities [Q][B]
// (null: not stored), mean / mode [Q] and quantiles [K][Q] under the renormalised criterion.  idx / share [M][ldt]
// (ldt >= B + 1) are the host's per-border tables (idx -1 / -2: the CDF forced to 0 / 1); cancel [M][ldc] bytes
// (ldc >= B) or null.  Rows padded to a multiple of 4 entries (and 16-byte bases) are read in 16- / 4-byte pieces.
constexpr int kBarHeadMaxBars = 8192, kBarHeadMaxMembers = 1024, kBarHeadMaxLevels = 64;
struct BarScoreArgs;  // below; non-null: the finished row's scores as well
hipError_t launch_bar_head(const float* logits, int M, int Q, int B, const unsigned char* cancel, int ldc,
                           const int* idx, const float* share, int ldt, float inv_temp, int avg_before, const float* borders,
                           const float* means, const float* mode_means, const float* widths, const float* levels,
                           int K, float* out_logits, float* mean, float* mode, float* quantiles, hipStream_t st,
                           const BarScoreArgs* score = nullptr);

// Scores of a finished row of bars (barhead.hip bar_score_row): what depends on the borders alone comes from the host
// (bar_distribution.FullSupportBarDistribution.score_tables): log_widths / mean_squares / ei_mids [B] and ends
// [kBarScoreEnds], indexed by the kEnd* below.  ys [Q][J] targets (J <= kBarScoreMaxTargets); nll / cdf / pi / ei
// [Q][J] and mean_of_square [Q], each may be null.  launch_bar_head takes borders / widths from its own arguments.
constexpr int kBarScoreMaxTargets = 64, kBarScoreEnds = 9;
enum BarScoreEnd {
  kEndS0 = 0,        // scale of the first bucket's half-normal (half its weight inside the bucket's width)
  kEndSL = 1,        // ... of the last bucket's
  kEndInvS0 = 2,     // 1 / scale
  kEndInvSL = 3,
  kEndInv2Var0 = 4,  // 1 / (2 scale^2)
  kEndInv2VarL = 5,
  kEndK0 = 6,        // the half-normal's log density at 0 plus the log of the bucket's width
  kEndKL = 7,
  kEndCentre = 8,    // the border ei_mids is centred on
};
struct BarScoreArgs {
  const float* borders;       // [B + 1]
  const float* widths;        // [B]
  const float* log_widths;    // [B]
  const float* mean_squares;  // [B]
  const float* ei_mids;       // [B] plain bucket means minus ends[kEndCentre]; 0 in the two end buckets
  const float* ends;          // [kBarScoreEnds]
  const float* ys;            // [Q][J] or null
  float* nll;
  float* cdf;
  float* pi;
  float* ei;
  float* mean_of_square;
  int J;
};
hipError_t launch_bar_score(const float* logits /*[Q][B]*/, int Q, int B, float inv_temp, const BarScoreArgs& score,
                            hipStream_t st);

// Draws from the rows' distributions (barsample.hip bar_sample_kernel): n draws per row of softmax(logits * inv_temp),
// blocks of kBarSampleChunk draws (grid Q x chunks).  Draw J = first_draw + j of row q reads the level uniforms[q][j],
// or without uniforms the Philox4x32-10 word of (seed, q, J); tails 1: the two end buckets follow their half-normals
// (ends [kBarScoreEnds], may be null with tails 0).  out [Q][n]; u_out [Q][n] the levels used, or null.
constexpr int kBarSampleChunk = 4096;
constexpr int64_t kBarSampleMaxDraws = (int64_t)65535 * kBarSampleChunk;
struct BarSampleArgs {
  const float* logits;    // [Q][B]
  const float* borders;   // [B + 1]
  const float* ends;      // [kBarScoreEnds] or null (tails 0)
  const float* uniforms;  // [Q][n] or null
  float* out;             // [Q][n]
  float* u_out;           // [Q][n] or null
  uint64_t seed, first_draw;
  int64_t n;
  int B, tails;
  float inv_temp;
};
hipError_t launch_bar_sample(const BarSampleArgs& a, int Q, hipStream_t st);

// Member preprocessing of the test rows (xform.hip xform_kernel): a compiled program (device_transform.py) over rows
// [0, Q) of x, all arithmetic in float64.  ops [n_ops][kXformOpInts] = (code, width in, width out, int offset, double
// offset, a, b, c); a kXformMap column is kXformMapInts ints (source, kind, double offset, n, aux).  width: the widest
// row of the program, at most kXformMaxWidth -- a block keeps xform_rows_per_block(width) rows twice in 64 KiB of LDS.
// An infinite input cell ORs kXformInfFlag into *flag (the lane's NaN flag word, read by mmpfn_status).
constexpr int kXformMaxWidth = 4096, kXformMaxRows = 8, kXformThreads = 256, kXformOpInts = 8, kXformMapInts = 5;
constexpr int kXformGather = 1, kXformMap = 2, kXformSvd = 3, kXformFingerprint = 4;
constexpr int kXformPass = 0, kXformLookup = 1, kXformQuantile = 2, kXformScale = 3;
constexpr int kXformInfFlag = 0x100;
struct XformArgs {
  const int32_t* ops;
  const int32_t* ints;
  const double* dbl;
  const void* x;  // [Q][ldx] float32, or float64 with x_f64
  float* out32;   // [Q][ld32]
  double* out64;  // [Q][ld64] the values before the final rounding, or null
  int* flag;
  int64_t ldx, ld32, ld64;
  int x_f64, Q, n_ops, n_in, n_out, width;
  int rows;  // set by launch_xform
};
int xform_rows_per_block(int width);
hipError_t launch_xform(const XformArgs& a, hipStream_t st);

// ---- mixer helpers -----------------------------------------------------------------
hipError_t launch_layernorm_rows(const float* in, int64_t rows, int dim, float eps, void* out, DType out_t,
                                 const float* gamma, const float* beta, hipStream_t st);
// whether the CAP attention has a kernel for head dim hd = E / cap_heads (mixer.hip CapDims, the one list)
bool cap_head_dim_supported(int hd);
// kv and out both fp32 (the fp32 modes) or both bf16; hipErrorInvalidValue unless cap_head_dim_supported(E / cap)
hipError_t launch_cap_attention(const float* qp /*[cap][E]*/, const void* kv /*[S][M][2E]*/, DType kv_t,
                                void* out /*[S][cap][E]*/, DType out_t, int S, int M, int cap, int E, hipStream_t st);
// CAP core on MFMA (bf16; head dim 8, 24 heads = cap queries, M % 32 == 0, M <= 128): K [S*M][E], V^T [S][E][M]
// bf16 (launch_rowgemm_ln_store's transposed form), O bf16 [S][cap][E]; hipErrorNotSupported for other shapes
hipError_t launch_cap_attention_mfma(const float* qp, const void* K, const void* VT, void* out, int S, int M, int cap,
                                     int E, hipStream_t st);
// CAP tail (mlp_rows.hip, E = 192): out = LN(o2) g + b + FFN(o2), o2 = O Wout^T + bo, over M pooled tokens; O bf16,
// Wout [E][E] bf16, W1perm / W2perm the FFN in mlp_rows order (pack_mlp1_perm / pack_mlp2_perm), vecs = [bo | b0 | g |
// b + b3] fp32 (5E floats)
hipError_t launch_cap_tail(const void* O, const void* Wout, const void* W1perm, const void* W2perm, const float* vecs,
                           float* out, int64_t M, int E, float eps, hipStream_t st);
hipError_t launch_ln_add(const float* o, const float* f, const float* g, const float* b, float* out,
                         int64_t rows, int E, float eps, hipStream_t st);
hipError_t launch_gate_softmax(const float* x /*[S][D]*/, int64_t ldx, int S, int D, const float* w /*[n][D]*/,
                               const float* b, int n, float* probs, hipStream_t st);
hipError_t launch_scale_tokens(float* tok /*[S][n][E]*/, const float* probs /*[S][n]*/, int S, int n, int E,
                               hipStream_t st);

}  // namespace mmpfn
