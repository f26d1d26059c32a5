/*
 * mmpfn_hip.h -- C ABI of the MI355X (gfx950) MMPFN in-context inference engine.
 *
 * Plain pointers and sizes only (no torch types).  All data pointers are DEVICE
 * pointers unless a parameter says "host".  The caller owns input/output buffers;
 * the context owns packed weights and workspace.  Calls on one context are
 * serialised on its stream and are asynchronous unless documented otherwise.
 *
 * Reference interfaces replaced (paths under too-z/MultiModalPFN/mmpfn/models/mmpfn/):
 *   mmpfn_create / mmpfn_set_model / mmpfn_load_weight / mmpfn_finalize_weights
 *       <- model/loading.py:401-542  load_model(): PerFeatureTransformer(...) +
 *          model.load_state_dict(state_dict, strict=False)
 *   mmpfn_mixer_forward
 *       <- model/transformer.py:755-761  self.mgm / self.cap / self.moe applied to image
 *          (MultiheadGatedMLP :33-57, CrossAttentionPooler :60-88, MoE :91-128)
 *   mmpfn_forward
 *       <- model/transformer.py:462-545,555-867  PerFeatureTransformer.forward(
 *          None, X_full[S,1,F], image_full, y_train[N], single_eval_pos=N,
 *          only_return_standard_out=True) as called at inference.py:343-348
 *   mmpfn_embed / mmpfn_run_layers / mmpfn_decode / mmpfn_copy_state
 *       <- the same forward split at its seams (embedded_input :788,
 *          transformer_encoder :799-808, decoder :850-853) for parity taps
 *   mmpfn_item_attention
 *       <- model/layer.py:341-379 attn_between_items (one token column batch)
 *   mmpfn_item_attention_layer
 *       <- model/layer.py:341-379 attn_between_items of one layer: train rows
 *          (:362-372) and test rows against head 0's K/V (:344-358) together
 *   mmpfn_item_attention_cached
 *       <- model/layer.py:344-358 with multi_head_attention.py:461-472: test rows of
 *          every head against the cached head-0 K/V of the train rows (fit_with_cache)
 *   mmpfn_bar_head
 *       <- regressor.py:652-706 (temperature, cancel mask, translate_probs_across_borders, ensemble mean) and
 *          :732-765 _logits_to_output on the renormalised FullSupportBarDistribution
 *   mmpfn_bar_score / mmpfn_bar_head_score
 *       <- model/bar_distribution.py:487-571 forward (the negative log density), :59-97 cdf, :629-675 pi,
 *          :677-758 ei, :600-626 mean_of_square of FullSupportBarDistribution; alone, or fused into mmpfn_bar_head
 *   mmpfn_bar_sample
 *       <- model/bar_distribution.py:577-585 sample (one uniform level per draw, then :256-283 icdf), many draws
 *          per row; the levels from Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel Random Numbers: As Easy
 *          as 1, 2, 3", SC'11) where the reference calls torch.rand
 *   mmpfn_xform_create / mmpfn_xform_free / mmpfn_member_transform
 *       <- model/preprocessing.py:443-1200 (the members' fitted steps, test form) as preprocessing.py:416-473 chains
 *          them, called per member at inference.py:294-349
 *   mmpfn_status
 *       <- model/transformer.py:727-731,790-796 NaN checks (ValueError)
 *   mmpfn_feature_attention / mmpfn_item_attention_block / mmpfn_mlp_ln
 *       <- model/layer.py:332-339 / :341-379 / :410-424 with the post-norms :437-455
 *          (one PerFeatureEncoderLayer sublayer each)
 *   mmpfn_outproj_mlp_ln
 *       <- model/layer.py:341-379's out-projection with its post-norm, then :410-424 with its own (:437-455):
 *          what follows the item attention's softmax(QK^T)V in one PerFeatureEncoderLayer
 *   mmpfn_item_qkv
 *       <- model/layer.py:341-372's q / k / v projections, train rows (:362-372) and test rows (:344-358):
 *          what precedes the item attention's softmax(QK^T)V
 *   mmpfn_item_attention_forward
 *       <- model/layer.py:341-379's softmax(QK^T)V itself, in the three forms the forwards launch it in
 *   mmpfn_mgm / mmpfn_cap
 *       <- model/transformer.py:33-57 MultiheadGatedMLP / :60-88 CrossAttentionPooler
 */
#ifndef MMPFN_HIP_H_
#define MMPFN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMPFN_OK 0
#define MMPFN_ERR_INVALID (-1)   /* bad argument / shape */
#define MMPFN_ERR_HIP (-2)       /* HIP runtime error (see mmpfn_last_error) */
#define MMPFN_ERR_NAN (-3)       /* NaN in the embedded input (reference raises ValueError) */
#define MMPFN_ERR_STATE (-4)     /* call order (weights not finalised, ...) */
#define MMPFN_ERR_WEIGHT (-5)    /* missing / mis-shaped weight */

#define MMPFN_PREC_F32 0      /* parity mode: fp32 tensors; contractions on bf16 MFMA with every operand split into
                                  bf16 hi + lo planes (hi.hi + hi.lo + lo.hi, fp32 accumulate: ~2^-16 relative) */
#define MMPFN_PREC_BF16 1     /* performance mode: bf16 MFMA operands, fp32 accumulate / residual / LN */
#define MMPFN_PREC_F32_MFMA 2 /* parity mode on fp32-input MFMA (exact fp32 fma chains, 1/16 of the bf16 rate) */
#define MMPFN_PREC_BF16_F8 3  /* MMPFN_PREC_BF16 with the sample-axis attention's P.V and row sums on block-scaled fp8
                                  MFMA (V^T e4m3, P e4m3 under a per-query power-of-two scale): config E's fp8 path
                                  (multi_head_attention.py:693-729 in fp8); the train-KV cache keeps bf16 */
#define MMPFN_PREC_BF16_F8E5 4 /* as MMPFN_PREC_BF16_F8 with P in e5m2 (wider range, 2 mantissa bits) */
#define MMPFN_PREC_F16 5      /* the reference's fp16 autocast (utils.py:150-190, layer.py:60-62): the state X kept in
                                  fp16 between kernels, every layer contraction on fp16 MFMA operands (the item
                                  attention's Q / K and P.V on bf16), fp32 accumulation / LayerNorm / softmax
                                  statistics; tables of more than 64 tokens per row run MMPFN_PREC_BF16 */
#define MMPFN_PREC_F16_F8 6   /* MMPFN_PREC_F16 with the fp8 P.V of MMPFN_PREC_BF16_F8 */
#define MMPFN_PREC_F16_F8E5 7 /* MMPFN_PREC_F16 with the fp8 P.V of MMPFN_PREC_BF16_F8E5 */

#define MMPFN_MIXER_NONE 0
#define MMPFN_MIXER_MGM 1
#define MMPFN_MIXER_MGM_CAP 2
#define MMPFN_MIXER_MOE 3

#define MMPFN_TARGET_CLASS 0 /* class codes sum(y > uniq) (MulticlassClassificationTargetEncoder, encoders.py:949-974) */
#define MMPFN_TARGET_VALUE 1 /* the target itself, as the caller standardised it (a regression model: no class-code
                                step; uniq / U of the forward entry points are ignored and may be NULL / 0; the
                                y encoder's Linear is y_encoder.1.layer.*, the decoder n_out = the criterion's bars wide) */

typedef struct mmpfn_ctx mmpfn_ctx;

typedef struct mmpfn_model_desc {
  int emsize;             /* E = 192 */
  int nhead;              /* 6 (head dim must be 32) */
  int nlayers;            /* 12 */
  int nhid;               /* 768 (MLP hidden, decoder hidden, modality width); with a mixer a multiple of 384 */
  int features_per_group; /* model grouping (yaml) */
  int encoder_features;   /* encoder width nf (checkpoint config.features_per_group) */
  int n_out;              /* decoder outputs (10) */
  int mixer_type;         /* MMPFN_MIXER_* */
  int mgm_heads;          /* MGM heads, or MoE experts */
  int cap_heads;          /* CAP queries/heads: a divisor of 192 other than 1 */
  int two_sets_of_queries;
  int remove_duplicate_features; /* encoder Linear step index 6 instead of 5 */
  float ln_eps;           /* 1e-5 */
  float outlier_sigma;    /* 12 for classification; <= 0 disables soft clipping */
  int target_kind;        /* MMPFN_TARGET_*: what the label token embeds (the y encoder of loading.py:374-398) */
} mmpfn_model_desc;

/* ---- lifecycle ------------------------------------------------------------------ */
mmpfn_ctx* mmpfn_create(int device, void* hip_stream);
void mmpfn_destroy(mmpfn_ctx* ctx);
const char* mmpfn_last_error(const mmpfn_ctx* ctx);
int mmpfn_set_stream(mmpfn_ctx* ctx, void* hip_stream);
const char* mmpfn_version(void);

/* ---- weights (checkpoint ABI: reference state_dict names, fp32 host data) --------
 * mmpfn_set_model is the one place that checks the model: a geometry that some kernel behind it cannot run is
 * refused here with MMPFN_ERR_INVALID (mmpfn_last_error names the field), never by a launch in a forward:
 *   emsize 192 in 6 heads of 32; nhid a multiple of 192, and with a mixer a multiple of 384 (nhid / 2, the
 *   modality heads' down-projection depth, must be a multiple of 64: nhid 192 and 576 are refused);
 *   nlayers, n_out >= 1; target_kind one of MMPFN_TARGET_*; 1 <= features_per_group <= encoder_features <= 8;
 *   MGM+CAP: cap_heads a divisor of 192 other than 1 (head dims 96 .. 1 have a CAP attention kernel, head dim 192
 *   has none: cap_heads 1 is refused). */
int mmpfn_set_model(mmpfn_ctx* ctx, const mmpfn_model_desc* desc);
int mmpfn_load_weight(mmpfn_ctx* ctx, const char* name, const float* host_data, int64_t numel);
int mmpfn_finalize_weights(mmpfn_ctx* ctx); /* pack / fold / convert / upload; synchronous */

/* ---- modality projection heads --------------------------------------------------
 * image [S][n_mod][nhid] -> tokens [S][C][E]; C = mmpfn_mixer_tokens(ctx, n_mod). */
int mmpfn_mixer_tokens(const mmpfn_ctx* ctx, int n_mod);
int mmpfn_mixer_forward(mmpfn_ctx* ctx, const float* image, int S, int n_mod, float* tokens, int precision);

/* ---- one ensemble member's forward ------------------------------------------------
 * x        [S][F] fp32 (NULL when tabular input is absent)
 * tokens   [S][C][E] mixer tokens (NULL / C = 0 when there is no image)
 * y_train  [N] fp32 class codes; uniq [U] sorted unique train codes (after NaN fill) -- MMPFN_TARGET_VALUE: the
 *          standardised targets, uniq / U unused
 * pos_rand [G + C][E/4]: torch.randn from the model's CPU generator
 *          (transformer.py:421-424,925-931), G = ceil(F / features_per_group)
 * logits   [S - N][n_out] fp32 output                                               */
int mmpfn_forward(mmpfn_ctx* ctx, const float* x, int S, int F, const float* tokens, int C, const float* y_train,
                  int N, const float* uniq, int U, const float* pos_rand, float* logits, int precision);

/* The last layer of the forward entry points (mmpfn_forward, mmpfn_forward_batch, mmpfn_cache_build,
 * mmpfn_cache_predict) computes only what the decoder reads: the feature attention of every row at its target token,
 * then the item attention, out-projection and MLP of the target token's column alone, for its test rows (a cache build: that
 * column's K / V^T and nothing after).  Every kernel computes a state row from that row's own inputs, so the logits
 * are bit for bit those of a full last layer.  After such a forward the last layer's state is defined only at the
 * target token's test rows -- mmpfn_copy_state then returns the rest as earlier sublayers left it.
 * mmpfn_run_layers always runs full layers, so mmpfn_copy_state after it is the whole state as before; so do the
 * per-sublayer taps.
 * mmpfn_set_full_last_layer(ctx, 1) makes the forward entry points of this context run the last layer in full
 * too (the pruned form's reference and A/B handle); 0, the default, prunes. */
int mmpfn_set_full_last_layer(mmpfn_ctx* ctx, int on);

/* ---- row embeddings -----------------------------------------------------------------
 * The reference's forward with only_return_standard_out=False returns, beside the logits, the target token's final
 * state of every row (transformer.py:850-864): train_embeddings [N][1][E] and test_embeddings [S - N][1][E].
 * mmpfn_forward_embed is mmpfn_forward with these two as outputs: train_emb [N][E] and test_emb [S - N][E], fp32
 * on the device, 16-byte aligned (the fp16 state of MMPFN_PREC_F16* widened exactly).  Each of logits, train_emb and
 * test_emb may be NULL (a NULL logits skips the decoder); all three NULL: MMPFN_ERR_INVALID.  N == S gives a
 * test_emb of zero rows.
 *   test_emb alone   the decoder's input rows: what mmpfn_forward launches, plus one gather kernel.
 *   train_emb        the last layer runs in a third, column form -- the target token's column of all S rows: the
 *                    feature attention as the pruned form runs it, then the item attention (the full layer's task
 *                    map on that one column per member), out-projection and MLP of that column alone.  Bit for bit
 *                    the column a full last layer leaves; with mmpfn_set_full_last_layer(ctx, 1) the last layer
 *                    runs in full here too.
 * mmpfn_forward_batch_embed: the same over mmpfn_forward_batch; outputs [M][N][E] and [M][S - N][E].
 * mmpfn_cache_predict_embed: mmpfn_cache_predict plus test_emb [Q][E], the decoder's input rows of that predict
 *   (logits or test_emb may be NULL, not both).  The train rows' embeddings of a cache build are not served. */
int mmpfn_forward_embed(mmpfn_ctx* ctx, const float* x, int S, int F, const float* tokens, int C, const float* y_train,
                        int N, const float* uniq, int U, const float* pos_rand, float* logits, float* train_emb,
                        float* test_emb, int precision);
int mmpfn_forward_batch_embed(mmpfn_ctx* ctx, int M, const float* const* x, int S, int F, const float* tokens, int C,
                              const float* const* y, int N, const float* const* uniq, const int* U,
                              const float* pos_rand, float* logits, float* train_emb, float* test_emb, int precision);

/* forward split at its seams (parity taps) */
int mmpfn_embed(mmpfn_ctx* ctx, const float* x, int S, int F, const float* tokens, int C, const float* y_train, int N,
                const float* uniq, int U, const float* pos_rand, int precision);
int mmpfn_run_layers(mmpfn_ctx* ctx, int layer_begin, int layer_end);
int mmpfn_decode(mmpfn_ctx* ctx, float* logits);
/* copies the current state in reference order [S][T][E] (fp32) */
int mmpfn_copy_state(mmpfn_ctx* ctx, float* out, int64_t capacity_elems);
int mmpfn_state_tokens(const mmpfn_ctx* ctx); /* T of the current state */

/* Ensemble aggregation (classifier.py:541-566, replaces the torch post-processing):
 * logits [M][Q][n_out]; perms [M][n_cls] int32 (NULL: no class permutation);
 * temperature != 1 slices to n_cls and divides; average_before_softmax 0/1;
 * class_weights [n_cls] (balance_probabilities) or NULL; probs [Q][C] with
 * C = n_cls when sliced or permuted, else n_out. */
int mmpfn_aggregate(mmpfn_ctx* ctx, const float* logits, int M, int Q, int n_out, const int* perms, int n_cls,
                    float temperature, int average_before_softmax, const float* class_weights, float* probs);

/* Bar-distribution head of the regression ensemble (regressor.py:691-706, utils.py:659-700; then the renormalised
 * criterion's mean / mode / icdf, bar_distribution.py:239-332,588-597), always fp32, one pass over the logits:
 * logits [M][Q][B]; cancel [M][ldc] bytes (ldc >= B), non-zero = the bar's logit is -inf for that member (NULL: no
 *   member cancels);
 * idx / share [M][ldt] (ldt >= B + 1): per member and target border j, the member's bucket that holds the border and the
 *   border's share of it as utils.py:662-670 computes them (in float32, on the host: they depend on the borders
 *   only); idx -1 / -2: the member's CDF at that border is 0 / 1 whatever the row (utils.py:675-676,697-698).
 *   Dense rows (ldt = B + 1, ldc = B) are fine; rows padded to a multiple of 4 entries on 16-byte-aligned bases are
 *   read in 16-byte (tables) and 4-byte (mask) pieces, which is what HipEngine.bar_head uploads;
 * inv_temperature = 1 / softmax_temperature; average_before_softmax 0/1 (regressor.py:700-703);
 * of the renormalised criterion (regressor.py:516-518): borders [B + 1], bucket_means [B] with the two half-normal
 *   end means (bar_distribution.py:588-597), mode_means [B] the plain ones and widths [B] (:328-332);
 * levels [K] quantile levels (the median is the level 0.5).
 * Outputs: out_logits [Q][B] the ensemble's log-probabilities (NULL: not stored); mean [Q], mode [Q],
 * quantiles [K][Q] of softmax(out_logits), as the reference's criterion applies it again.
 * B <= MMPFN_BAR_MAX_BARS, M <= MMPFN_BAR_MAX_MEMBERS, K <= MMPFN_BAR_MAX_LEVELS, else MMPFN_ERR_INVALID. */
#define MMPFN_BAR_MAX_BARS 8192
#define MMPFN_BAR_MAX_MEMBERS 1024
#define MMPFN_BAR_MAX_LEVELS 64
int mmpfn_bar_head(mmpfn_ctx* ctx, const float* logits, int M, int Q, int B, const unsigned char* cancel, int ldc,
                   const int* idx, const float* share, int ldt, float inv_temperature, int average_before_softmax,
                   const float* borders, const float* bucket_means, const float* mode_means, const float* widths,
                   const float* levels, int K, float* out_logits, float* mean, float* mode, float* quantiles);

/* Scores of a bar distribution at given targets (the rest of FullSupportBarDistribution, bar_distribution.py:59-97,
 * 487-571, 600-675, 706-758), always fp32, one block per row:
 * logits [Q][B] (any: the head's out_logits or one member's; -inf is a bar of weight zero), softmax(logits *
 *   inv_temperature) as the head's last stage computes it;
 * borders [B + 1], widths [B] and the score tables, all from FullSupportBarDistribution.score_tables() (what depends
 *   on the borders alone, float32): log_widths [B]; mean_squares [B] (the per-bucket means of squares, :606-624);
 *   ei_mids [B] (the interior buckets' plain means minus the border ends[8]; 0 in the two end buckets);
 *   ends [MMPFN_BAR_SCORE_ENDS]: per end bucket (first, last) the half-normal's scale [0..1], 1 / scale [2..3],
 *   1 / (2 scale^2) [4..5], its log density at 0 plus the log of the bucket's width [6..7]; [8] the centre of ei_mids;
 * ys [Q][J] targets on the borders' scale, 0 <= J <= MMPFN_BAR_MAX_TARGETS.
 * Outputs, each may be NULL: nll [Q][J] the negative log density (forward, :487-571; 0 at a NaN target), cdf (:59-97),
 * pi (:629-675) and ei (:706-758) with the target as best_f, [Q][J], NaN at a NaN target; mean_of_square [Q]
 * (:600-626).  The bucket of a target is searchsorted(borders, y) - 1 (left side), clamped.
 * MMPFN_ERR_INVALID: J or B (2 .. MMPFN_BAR_MAX_BARS) out of range, a per-target output without ys.  Q = 0 is fine. */
#define MMPFN_BAR_MAX_TARGETS 64
#define MMPFN_BAR_SCORE_ENDS 9
int mmpfn_bar_score(mmpfn_ctx* ctx, const float* logits, int Q, int B, float inv_temperature, const float* borders,
                    const float* widths, const float* log_widths, const float* mean_squares, const float* ei_mids,
                    const float* ends, const float* ys, int J, float* nll, float* cdf, float* pi, float* ei,
                    float* mean_of_square);

/* mmpfn_bar_head with the scores of every finished row from the same kernel: mmpfn_bar_head's arguments, then
 * mmpfn_bar_score's tables (borders and widths are the head's own), targets and outputs.  Every output of
 * mmpfn_bar_head is bit for bit what that call gives, and the scores are those of mmpfn_bar_score on its out_logits at
 * inv_temperature 1; out_logits may be NULL, so the [Q][B] log-probabilities need not reach memory. */
int mmpfn_bar_head_score(mmpfn_ctx* ctx, const float* logits, int M, int Q, int B, const unsigned char* cancel, int ldc,
                         const int* idx, const float* share, int ldt, float inv_temperature, int average_before_softmax,
                         const float* borders, const float* bucket_means, const float* mode_means, const float* widths,
                         const float* levels, int K, float* out_logits, float* mean, float* mode, float* quantiles,
                         const float* log_widths, const float* mean_squares, const float* ei_mids, const float* ends,
                         const float* ys, int J, float* nll, float* cdf, float* pi, float* ei, float* mean_of_square);

/* Draws from bar distributions (FullSupportBarDistribution.sample, bar_distribution.py:577-585, with many levels per
 * row), always fp32, blocks of MMPFN_BAR_SAMPLE_CHUNK draws of one row:
 * logits [Q][B], softmax(logits * inv_temperature) as mmpfn_bar_score computes it (inv_temperature = 1 / t of the
 *   reference's sample(logits, t)); borders [B + 1]; ends [MMPFN_BAR_SCORE_ENDS] as mmpfn_bar_score's (NULL is fine
 *   with tails 0);
 * n draws per row, 0 <= n <= MMPFN_BAR_MAX_DRAWS, out [Q][n]; draw j of the call is draw J = first_draw + j of the row.
 * Its level u: uniforms[q][j] clamped into [2^-24, 1 - 2^-24] (a NaN level gives a NaN draw), or with uniforms NULL
 *   word J & 3 (Random123's output order) of Philox4x32-10 at counter (lo32(J >> 2), hi32(J >> 2), q, 0) and key
 *   (lo32(seed), hi32(seed)), mapped to u = (2 (x >> 9) + 1) 2^-24: a draw depends on (seed, q, J) alone, not on n or
 *   on how a row's draws are split over calls.  u_out [Q][n] (NULL: not stored) receives the levels used.
 * The draw, tails 0: lv = min(u, the row's rounded total); j the first bar whose inclusive cumulative sum reaches lv
 *   (:256-283); share = clamp((lv - sum before j) / p_j, 0, 1); y = borders[j] + (borders[j + 1] - borders[j]) share.
 *   The min and the clamp are this engine's own: every draw is finite and inside [borders[0], borders[B]].
 * tails 1: the two end buckets follow the half-normals that forward / pi / ei give them (:487-571), the draws the
 *   density mmpfn_bar_score's nll scores: in the last bucket y = borders[B - 1] + ends[1] sqrt(2) erfinv(min(share,
 *   1 - 2^-24)), in the first y = borders[1] - ends[0] sqrt(2) erfinv(min(1 - share, 1 - 2^-24)).
 * A row whose total is 0 or NaN (no finite largest logit) gives NaN draws and nothing else.
 * MMPFN_ERR_INVALID: B (2 .. MMPFN_BAR_MAX_BARS) or n out of range, inv_temperature <= 0, tails not 0 / 1 (or 1 with
 * ends NULL), out NULL with n > 0.  Q = 0 or n = 0 launch nothing. */
#define MMPFN_BAR_SAMPLE_CHUNK 4096
#define MMPFN_BAR_MAX_DRAWS (65535LL * MMPFN_BAR_SAMPLE_CHUNK)
int mmpfn_bar_sample(mmpfn_ctx* ctx, const float* logits, int Q, int B, float inv_temperature, const float* borders,
                     const float* ends, int tails, const float* uniforms, uint64_t seed, uint64_t first_draw, int64_t n,
                     float* out, float* u_out);

/* Member preprocessing of the test rows on the device.  Replaces, per member and predict, the host's
 * preprocessor.transform(X).X of inference.py:294-349: the fitted steps of model/preprocessing.py (constant removal
 * :443-473, the distribution reshape with its ColumnTransformer, uniform QuantileTransformer, guarded scalers and
 * TruncatedSVD :579-995, the ordinal re-encoding :998-1200, the fingerprint :476-523, the column shuffle :526-571) as
 * preprocessing.py:416-473 chains them, with the estimator's ordinal front encoder (classifier.py:529-532) in front.
 * A program is what multimodalpfn_amd/device_transform.py compiles from the fitted state and documents:
 *   ops [n_ops][8] int32 (code, width in, width out, int offset, double offset, a, b, c), codes 1 gather, 2 map
 *   (five ints per column: source, kind 0 pass / 1 lookup / 2 uniform quantile / 3 guarded scale, double offset, n,
 *   aux), 3 svd, 4 fingerprint; ints and doubles are the parameter blobs the offsets point into.
 * The create call copies the three arrays (HOST pointers) to the device after checking every width, offset and index
 * in them: MMPFN_ERR_INVALID (mmpfn_last_error says why) for an op or map kind out of range, widths that do not chain,
 * a row wider than MMPFN_XFORM_MAX_WIDTH doubles (two working rows of that width are the 64 KiB of LDS a block
 * holds), or anything that points outside a blob or a row.  The program belongs to the context; free it with
 * the free call below (which waits for the context's streams).
 * The transform call runs a program over rows [0, Q) of x (device, row-major [Q][ldx], float32 or float64 by
 * x_is_f64) on the bound stream, one launch, all arithmetic in float64, and writes out32 [Q][ld32] (float32, round
 * to nearest even) and, if not NULL, out64 [Q][ld64] (the float64 values before that rounding).  F_in must be the
 * program's input width, ldx >= F_in, ld32 / ld64 >= the program's output width, else MMPFN_ERR_INVALID.  NaN cells
 * are data (as on the host); a +-inf cell sets a flag that mmpfn_status reports as MMPFN_ERR_NAN with the host
 * path's message ("Input X contains infinity ...").  Q = 0 launches nothing. */
#define MMPFN_XFORM_MAX_WIDTH 4096
typedef struct mmpfn_xform mmpfn_xform;
int mmpfn_xform_create(mmpfn_ctx* ctx, const int32_t* ops, int n_ops, const int32_t* ints, int64_t n_ints,
                       const double* doubles, int64_t n_doubles, int n_in, mmpfn_xform** out);
void mmpfn_xform_free(mmpfn_ctx* ctx, mmpfn_xform* prog);
int mmpfn_member_transform(mmpfn_ctx* ctx, const mmpfn_xform* prog, const void* x, int x_is_f64, int Q, int F_in,
                           int64_t ldx, float* out32, int64_t ld32, double* out64, int64_t ld64);

/* Synchronises the context stream and reports deferred device-side errors
 * (MMPFN_ERR_NAN when the embedded input held NaNs, or a device X held an infinity). */
int mmpfn_status(mmpfn_ctx* ctx);

/* ---- raw kernels (benchmarks / unit parity) ------------------------------------
 * Sample-axis attention for one layout batch:
 *   q  [T][H][S][32], k [T][H][Npad][32], vt [T][H][32][Npad], out [T][S][H*32]
 *   queries s in [s0, s0+nq) attend keys [0, nk); kv_head_fixed >= 0 forces a KV head.
 *   softmax(q k^T / sqrt(32)): q as projected (the engine's own bf16 forward passes q pre-multiplied
 *   by log2(e)/sqrt(32) internally; these taps do not).
 * Element type: fp32 (MMPFN_PREC_F32) or bf16 (MMPFN_PREC_BF16). */
int mmpfn_item_attention(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S, int T,
                         int H, int Npad, int s0, int nq, int nk, int kv_head_fixed, int precision);

/* M ensemble members of one geometry (same S, N, F, C) in one batched forward: the
 * state of all members is stacked [M][T][S][E] so every layer kernel runs once over the
 * batch (M*S rows, M*T attention columns).  x, y, uniq: HOST arrays of M device pointers
 * (as mmpfn_forward's arguments of each member); U: host array of M unique-label counts;
 * logits: device [M][S-N][n_out].  Replaces the per-member model call of the ensemble loop
 * (inference.py:294-349 -> transformer.py:462-545) for members that share a geometry. */
int mmpfn_forward_batch(mmpfn_ctx* ctx, int M, const float* const* x, int S, int F, const float* tokens, int C,
                        const float* const* y, int N, const float* const* uniq, const int* U,
                        const float* pos_rand, float* logits, int precision);

/* Forward lanes: independent per-member workspaces sharing the context's weights.
 * Selects the lane used by the following embed / run_layers / decode / forward /
 * copy_state calls (lane 0 at creation).  Members run concurrently when the caller binds a
 * different stream (mmpfn_set_stream) to each lane; mmpfn_status checks every lane.
 * Replaces nothing in the reference: its ensemble loop runs members one after another
 * (inference.py:294-349); lanes let independent members overlap on one GPU. */
#define MMPFN_MAX_LANES 8
int mmpfn_select_lane(mmpfn_ctx* ctx, int lane);

/* The whole sample-axis attention of one layer in one launch (bf16 only): train queries
 * s in [0, N) of head h against K/V head h, test queries s in [N, S) of every head against
 * K/V head 0; keys [0, N).  Layouts as mmpfn_item_attention. */
int mmpfn_item_attention_layer(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S,
                               int T, int H, int Npad, int N);

/* mmpfn_item_attention_layer in a 16-bit precision code: MMPFN_PREC_BF16 (as mmpfn_item_attention_layer),
 * MMPFN_PREC_F16 (q, k and out in fp16, vt bf16), or either with the fp8 P.V (MMPFN_PREC_*_F8: P e4m3,
 * *_F8E5: P e5m2; vt is the bf16 V^T, converted to e4m3 inside).  A code 5-7 OR MMPFN_ATTN_QK_BF16 runs the
 * fp16 mode's forward form: q and k in bf16 (as the engine writes them), out fp16. */
#define MMPFN_ATTN_QK_BF16 0x100
int mmpfn_item_attention_layer_ex(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S,
                                  int T, int H, int Npad, int N, int precision);

/* The train-KV cache's attention (bf16 only): queries s in [0, S) of every head against a
 * head-0-only K [T][Npad][32] / V^T [T][32][Npad] (the layout mmpfn_cache_build keeps per
 * layer); keys [0, N).  Q / out as mmpfn_item_attention. */
int mmpfn_item_attention_cached(mmpfn_ctx* ctx, const void* q, const void* k0, const void* vt0, void* out, int S,
                                int T, int H, int Npad, int N);

/* Train-KV cache (fit_mode="fit_with_cache"), one per ensemble member.
 * mmpfn_cache_build: forward of the N train rows only (x [N][F], tokens [N][C][E], y_train [N]);
 *   keeps, per layer, head 0's K and V^T of the train rows -- the only K/V the test rows read
 *   (multiquery item attention, layer.py:341-358; only_cache_first_head_kv, :362-372) -- and the
 *   train statistics of the x / y encoders and the positional embeddings.  Replaces
 *   InferenceEngineCacheKV.prepare's ens_model.forward(..., single_eval_pos=len(X))
 *   (inference.py:425-436; cache_kv=True, multi_head_attention.py:461-472).  Of the last layer only the target
 *   token's column is kept (the pruned last layer above): its other columns' blocks keep their place in the
 *   layout and in mmpfn_cache_bytes, and are never written or read.
 * mmpfn_cache_predict: Q test rows (x [Q][F], tokens [Q][C][E]) through the layers against the
 *   cache (use_cached_kv, layer.py:344-358), logits [Q][n_out] in the cache's precision.  Replaces
 *   iter_outputs' model(None, X_test, None, single_eval_pos=None) (inference.py:499-507).
 * Equal to the test rows of a full forward over train + test rows, except that the x encoder's
 * constant-column and used-feature tests see the train rows only (as the reference's cache).
 * The cache belongs to the context that built it; free it with mmpfn_cache_free. */
typedef struct mmpfn_cache mmpfn_cache;
int mmpfn_cache_build(mmpfn_ctx* ctx, const float* x, int N, int F, const float* tokens, int C, const float* y_train,
                      const float* uniq, int U, const float* pos_rand, int precision, mmpfn_cache** out);
int mmpfn_cache_predict(mmpfn_ctx* ctx, const mmpfn_cache* cache, const float* x, int Q, int F, const float* tokens,
                        int C, float* logits);
/* (row embeddings above) */
int mmpfn_cache_predict_embed(mmpfn_ctx* ctx, const mmpfn_cache* cache, const float* x, int Q, int F,
                              const float* tokens, int C, float* logits, float* test_emb);
int64_t mmpfn_cache_bytes(const mmpfn_cache* cache);
void mmpfn_cache_free(mmpfn_ctx* ctx, mmpfn_cache* cache);

/* Measurement hook (no reference counterpart): while enabled, every sample-axis attention
 * launch of the bf16 forward is bracketed by HIP events on its own stream.  enable=1 clears
 * and starts a window, enable=0 stops it; _read synchronises and returns the summed launch
 * durations, the launch count and their algorithmic flops (4*T*(N+Q)*N*E each).  Only the full-shape
 * launches count: a pruned last layer's one-column launch is neither bracketed nor added. */
int mmpfn_kernel_timing(mmpfn_ctx* ctx, int enable);
int mmpfn_kernel_timing_read(mmpfn_ctx* ctx, double* total_ms, int64_t* launches, double* flops);

/* Per-sublayer taps: one sublayer of layer `layer` on a caller-provided state, in place, on the
 * context stream (the forward itself fuses across these seams: the 16-bit modes' item-attention
 * out-projection runs inside the MLP kernel there -- mmpfn_outproj_mlp_ln below is the tap on that).  X: device [T][S][E] fp32, the engine's
 * token-major state of ONE member (reference order [S][T][E] transposed).  `rows` = S * T. */
int mmpfn_feature_attention(mmpfn_ctx* ctx, int layer, float* X, int S, int T, int precision);
/* The same sublayer, X <- LN(X + FeatAttn_layer(X)), in every form the forwards run it: X is device [M][T][S][E] fp32,
 * the states of M members one behind the other (a batched forward's state), through the host function the forwards'
 * layers call.  mmpfn_feature_attention is the M = 1, last = 0 call of this one.
 * Which kernel runs, by (precision, T):
 *   MMPFN_PREC_BF16*, T <= 64   feat_rows_kernel on the fp32 state: one wave per table row, all M * S rows in one
 *                               launch (a 4-row block may hold rows of two members); 1 .. 4 token tiles of 16 by T
 *                               (T <= 16, 32, 48, 64), the three-tile full form with its last tile's attention output
 *                               parked in LDS.
 *   MMPFN_PREC_F16*,  T <= 64   the same kernel's fp16 form on an fp16 copy of the state (out-projection rows
 *                               permuted, the residual taken from the row's own fragments).
 *   MMPFN_PREC_F16*,  T > 64    run as MMPFN_PREC_BF16: bit for bit that mode's result.
 *   MMPFN_PREC_BF16*, T > 64,   the general path, member by member: the q|k|v projection GEMM, the key-tiled attention
 *   MMPFN_PREC_F32_MFMA         kernel (64-key tiles, fixed-reference softmax), the out-projection + LayerNorm GEMM.
 *   MMPFN_PREC_F32              the general path on split-bf16 products; T <= 64 on the one-wave-per-(row, head)
 *                               parity attention kernel, T > 64 on the key-tiled one.
 * last != 0: the form of a forward's pruned last layer, which reads this sublayer's output at the target token T - 1
 * only.  feat_rows_kernel then computes and stores token T - 1 of every row alone -- bit for bit what last = 0 stores
 * there -- and leaves every other token of X as it was (MMPFN_PREC_F16*: as the fp16 copy holds it).  The general path
 * ignores `last` and runs in full.
 * MMPFN_ERR_INVALID (mmpfn_last_error says which) for S <= 0, T <= 0, M <= 0, a layer outside [0, nlayers) or an
 * unknown precision; a null ctx or X returns it without a message; nothing is launched then. */
int mmpfn_feature_attention_ex(mmpfn_ctx* ctx, int layer, float* X, int S, int T, int M, int last, int precision);
/* train rows [0, N) attend their own heads, rows [N, S) head 0's K/V (MQA) */
int mmpfn_item_attention_block(mmpfn_ctx* ctx, int layer, float* X, int S, int T, int N, int precision);
int mmpfn_mlp_ln(mmpfn_ctx* ctx, int layer, float* X, int64_t rows, int precision);
/* The step behind the item attention as the forwards run it, attention output -> state:
 *   X <- LN(X' + MLP_layer(X')),  X' = LN(X + O . Wout_layer^T)
 * X [rows][E] fp32, in place (MMPFN_PREC_F16: through an fp16 copy, as the other taps).  O [rows][E] is the item
 * attention's output, O[row][32 h + d] of head h, in the mode's attention-output element type, taken as it is (the
 * convention of mmpfn_item_attention_layer_ex): fp32 for MMPFN_PREC_F32 / _F32_MFMA, bf16 for MMPFN_PREC_BF16*, fp16
 * for MMPFN_PREC_F16*.  Row-wise: any row count >= 1, no token limit.
 * Which kernels the three row-wise taps run, by mode:
 *   mmpfn_outproj_mlp_ln        16-bit: mlp_rows_kernel with the out-projection prologue (RES), one launch -- the
 *                               kernel of every 16-bit forward; fp32: the out-projection + LN kernel, then the MLP
 *                               kernel -- the forwards' two launches.  The forwards and this tap share one host function.
 *   mmpfn_item_attention_block  16-bit: its out-projection runs the stand-alone rowgemm kernel (launch_rowgemm_resln),
 *                               which no 16-bit forward launches; fp32: the forwards' kernels.
 *   mmpfn_mlp_ln                16-bit: mlp_rows_kernel without the prologue (RES = false), which no 16-bit forward
 *                               launches; fp32: the forwards' kernel.
 *   mmpfn_item_qkv (below)      every mode: the forwards' projection kernel(s), through the host function the forwards
 *                               share with it -- 16-bit rowgemm_qkv2_kernel, MMPFN_PREC_F32 proj3_kernel,
 *                               MMPFN_PREC_F32_MFMA gemm_kernel with the EPI_ITEM_QKV epilogue.
 * MMPFN_ERR_INVALID (mmpfn_last_error says which) for rows <= 0, a null O, a layer outside [0, nlayers) or an
 * unknown precision; nothing is launched then. */
int mmpfn_outproj_mlp_ln(mmpfn_ctx* ctx, int layer, float* X, const void* O, int64_t rows, int precision);
/* The item attention's projection alone, through the host function the forwards' layers call.
 * X: device [M][T][S][E] fp32, not modified.  N > 0: rows [0, N) through q|k|v, rows [N, S) through the test rows' q
 * (N == S: no test rows, a cache build's form).  N == 0: the train-KV cache's predict form, all S rows through the test
 * rows' q; k / vt unused and may be null.  last != 0: the pruned last layer's form, column T-1 of every member only.
 * q [TM][H][S][32], k [TM][H][Npad][32], vt [TM][H][32][Npad], TM = last ? M : M * T, Npad = ceil(N / 64) * 64, in
 * the mode's operand type (fp32: MMPFN_PREC_F32 / _F32_MFMA; bf16: every 16-bit code), written in place into the
 * caller's buffers: what the kernels do not store stays as the caller left it -- K rows and V^T columns [N, Npad), and
 * all of k / vt when N == 0.  The 16-bit modes' q comes out times log2(e) / sqrt(32), as their attention kernel takes it
 * (q_prescaled); the fp32 modes' q is the plain projection.  The precision is decoded as mmpfn_item_attention_block
 * decodes it: MMPFN_PREC_F16* at T > 64 runs as MMPFN_PREC_BF16*, and the fp8 codes run their base mode's projection.
 * MMPFN_PREC_F16* projects an fp16 copy of X held by the context.
 * Which kernel runs, by mode:
 *   MMPFN_PREC_BF16*, _F16*   rowgemm_qkv2_kernel: both row sets in one launch, 128-row blocks per column, the test
 *                             rows' q-only blocks last.
 *   MMPFN_PREC_F32            proj3_kernel (split-bf16 products): both sets in one launch, 32-row tiles over all rows.
 *   MMPFN_PREC_F32_MFMA       gemm_kernel with the EPI_ITEM_QKV epilogue, one launch per non-empty row set.
 * MMPFN_ERR_INVALID (mmpfn_last_error says which) for S <= 0, T <= 0, M <= 0, N < 0, N > S, a null q, a null k or vt
 * with N > 0, a layer outside [0, nlayers) or an unknown precision; a null ctx or X returns it without a message;
 * nothing is launched then. */
int mmpfn_item_qkv(mmpfn_ctx* ctx, int layer, const float* X, int S, int T, int N, int M, int last, int precision,
                   void* q, void* k, void* vt);
/* The item attention's softmax(Q K^T) V alone, launched with the arguments the forwards launch it with (one host
 * function builds them for the layers and for this tap): what sits between mmpfn_item_qkv and mmpfn_outproj_mlp_ln.
 *   form 0  a full layer: train rows [0, N) of head h against K / V head h, test rows [N, S) of every head against
 *           K / V head 0; every row of out is written.  N == S (no test rows) is a cache build's form.
 *   form 1  the pruned last layer: the test rows, and of the train rows only [N - N % 256, N), which share the test
 *           rows' first 256-query task; rows [0, N - N % 256) of out are not written.  Needs N < S.
 *   form 2  a train-KV cache's predict: all S rows are test rows, against a head-0-only k [T][Npad][32] and
 *           vt [T][32][Npad] of N keys (mmpfn_cache_build's layout); an fp8 code runs the bf16 P.V, as the cache does.
 * q [T][H][S][32], k [T][H][Npad][32], vt [T][H][32][Npad], out [T][S][H*32], T token columns, keys [0, N), Npad a
 * multiple of 64 and >= N, H <= 8.  The operands are taken as the forward of the mode takes them: the 16-bit codes read
 * bf16 q (already times log2(e) / sqrt(32), as mmpfn_item_qkv writes it), bf16 k and vt, and write out in bf16
 * (MMPFN_PREC_BF16*) or fp16 (MMPFN_PREC_F16*); the fp8 codes convert vt to e4m3 inside; MMPFN_PREC_F32 / _F32_MFMA
 * read the plain fp32 projection and write fp32.  The precision is decoded as mmpfn_item_attention_block decodes it
 * (MMPFN_PREC_F16* at T > 64 runs as MMPFN_PREC_BF16*).  q, k and vt are not modified; K rows and V^T columns
 * [N, Npad) may hold anything.
 * MMPFN_ERR_INVALID (mmpfn_last_error says which) for a form outside 0..2, an unknown precision, T <= 0, S <= 0,
 * N <= 0, N > S in forms 0 and 1, N == S in form 1, N > Npad, Npad % 64 != 0, H outside [1, 8]; a null pointer returns
 * it without a message; nothing is launched then. */
int mmpfn_item_attention_forward(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S,
                                 int T, int H, int Npad, int N, int form, int precision);
/* modality heads: image [S][n_mod][nhid] -> MGM tokens [S][mgm*n_mod][E] (head-major, as the
 * reference concatenates them); MGM tokens [S][M][E] -> CAP tokens [S][cap][E] */
int mmpfn_mgm(mmpfn_ctx* ctx, const float* image, int S, int n_mod, float* tokens, int precision);
int mmpfn_cap(mmpfn_ctx* ctx, const float* mgm_tokens, int S, int M, float* tokens, int precision);

/* Host helper of the predict path (no GPU, no context): the fingerprint feature's row hash
 * (model/preprocessing.py:476-479, Python hash(row.tobytes()) under PYTHONHASHSEED=0 = SipHash-2-4 with the
 * all-zero key, -1 mapped to -2).  rows: host, n_rows x row_bytes contiguous; out: host int64[n_rows]. */
int mmpfn_siphash24_rows(const void* rows, int64_t n_rows, int64_t row_bytes, int64_t* out);

#ifdef __cplusplus
}
#endif

#endif /* MMPFN_HIP_H_ */
