// C ABI of the MMPFN engine: context, weight packing (checkpoint ABI) and the
// native orchestration of one ensemble member's PerFeatureTransformer forward.
//
// Forward (transformer.py:555-867) per member, all on the context stream:
//   pos-emb  -> x encoder (+pos-emb) -> mixer tokens (+pos-emb) -> y token
//   -> nlayers x [feature attn | item attn | MLP] (layer.py:272-457)
//   -> decoder on the test rows of the target token.
// State layout in HBM: X[T][S][E] fp32 (token-major), so every token column of the
// sample-axis attention is a contiguous [S][E] slab; fp16 under PREC_F16 (the encoders and the
// decoder run in fp32 and convert at the seams).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mmpfn_hip.h"
#include "devbuf.h"
#include "kernels.h"
#include "weight_pack.h"

using namespace mmpfn;

namespace {

// The weights of one finalised model, every one [N][K] row-major in each form its kernels read (Weight); the orders
// of the forms are stated where they are filled (the finalize_* functions).  Built afresh by every finalize, so
// nothing of an earlier model survives one.
struct LayerW {
  Weight feat_qkv, feat_out, item_qkv, item_qtest, item_out, mlp1, mlp2;
  Weight feat_pack;  // 16-bit LDS images of the feature-attention weights (featrow.hip)
};

struct HeadBank {  // the MGM heads or the MoE experts, stacked
  Weight w1, w2;
  DevBuf b1, b2;
};
struct ModelWeights {
  std::vector<LayerW> layers;
  DevBuf enc_w, y_w, y_b, pe_w, pe_b, dec_b1, dec_b2;
  // class targets: fp32 forms, and 16-bit forms (the MFMA decoder) only where n_out <= 16 && nhid % 128 == 0; a value
  // target: natural [Fh][E] / [n_out][Fh] in fp32, bf16 and fp16 (launch_decoder_wide), nothing else
  Weight dec_w1, dec_w2;
  HeadBank mgm, moe;      // fp16 forms (PREC_F16's MGM head bank) only in mgm_f16_shape
  DevBuf moe_gw, moe_gb;
  Weight cap_kv, cap_o, cap_f0, cap_f3;
  DevBuf cap_qp, cap_kv_b, cap_o_b, cap_f0_b, cap_f3_b, cap_ng, cap_nb, cap_vecs;  // vecs: [bo | b0 | g | b + b3]
};

// per-member forward state of one lane: independent forward workspaces sharing the weights, so members can run
// concurrently on different streams
struct Lane {
  DevBuf ws_X, ws_O, ws_big, ws_pe, ws_slots, ws_scr, ws_flag;
  // current forward geometry (M members of equal geometry stacked as [M][T][S][E]); prec: the base mode the layer
  // kernels run, f8: the fp8 P.V variant of the item attention (PrecMode below)
  int S = 0, T = 0, N = 0, G = 0, C = 0, Npad = 0, prec = 0, M = 1, f8 = 0;
  bool embedded = false;
};

}  // namespace

// train-KV cache of one ensemble member (fit_mode="fit_with_cache"): per layer the head-0 K and
// V^T of the train rows (all test rows read, layer.py:344-358), plus the train statistics of the
// input encoders and the positional embeddings, so a predict runs only the test rows
struct mmpfn_cache {
  int N = 0, F = 0, G = 0, C = 0, T = 0, Npad = 0, prec = 0, U = 0;
  DevBuf kv;     // [L][K: T x Npad x 32 | V^T: T x 32 x Npad], element size of prec; a pruned last layer writes
                 // and reads column T-1 of layer L-1 only (its other columns: never written, never read)
  DevBuf slots;  // x-encoder SlotParams [G * fpg]
  DevBuf ymean;  // y-encoder train nanmean
  DevBuf uniq;   // sorted unique train labels [U]
  DevBuf pe;     // positional embeddings [G + C][E]
};

// a member's compiled preprocessing program (device_transform.py) on the device, checked when it was made
struct mmpfn_xform {
  DevBuf ops, ints, dbl;
  int n_ops = 0, n_in = 0, n_out = 0, width = 0;
};

struct mmpfn_ctx : Lane {  // the Lane base is the selected lane
  int device = 0;
  hipStream_t stream = nullptr;
  // every stream bound since the last mmpfn_status: lanes run on their own streams and the NaN
  // flags they set must be read behind all of them
  std::vector<hipStream_t> seen_streams;
  std::string err;
  bool have_model = false, finalized = false;
  mmpfn_model_desc d{};
  std::map<std::string, std::vector<float>> host;

  ModelWeights w;

  DevBuf mx[8];
  DevBuf tap_v8;   // e4m3 V^T of the fp8 attention tap
  DevBuf tap_x16;  // PREC_F16 taps: the caller's fp32 state as fp16
  // the lanes that are not selected are parked here (mmpfn_select_lane swaps whole Lane objects)
  std::vector<Lane> lanes;  // lanes[cur] is stale while cur is selected
  int cur = 0;
  // live timing of the sample-axis attention launches (mmpfn_kernel_timing): HIP events
  // recorded on the launching stream around every item-attention launch while enabled
  mmpfn_cache* cache_out = nullptr;       // being built by the current forward (train rows only)
  const mmpfn_cache* cache_in = nullptr;  // used by the current forward (test rows only)
  bool full_last = false;  // mmpfn_set_full_last_layer: the forwards run their last layer in full
  bool kt_on = false;
  std::vector<hipEvent_t> kt_pool;  // event pairs, reused across windows
  size_t kt_used = 0;
  double kt_flops = 0.0;
};

namespace {

#define HIPCHK(expr) HIPCHK_ON(ctx, expr)
#define GETW(var, name, n) GETW_ON(ctx, var, name, n)

// the shape the fp16 MGM head bank's big-tile GLU kernel takes (uploaded by finalize, used by mixer_mgm)
bool mgm_f16_shape(const mmpfn_model_desc& d) { return (d.mgm_heads * d.nhid) % 256 == 0; }

// the lane's NaN flag: zeroed once when allocated, then only ORed into by the encoder kernels and
// cleared by mmpfn_status after it has been read, so a NaN in ANY forward queued on the lane since
// the last status check is reported (not only the last forward's)
int ensure_flag(mmpfn_ctx* ctx, DevBuf& b, hipStream_t st) {
  if (b.p) return MMPFN_OK;
  RC(ensure(ctx, b, 256));
  HIPCHK(hipMemsetAsync(b.p, 0, 256, st));
  return MMPFN_OK;
}

// ---- finalize: the host weights of ctx->d packed into a fresh ModelWeights, part by part.  Every fill names the forms
//      it uploads; their matrix order is the packing function in its argument (none: natural [N][K]).
int finalize_layers(mmpfn_ctx* ctx, ModelWeights& w) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, HD = E, Fh = d.nhid;
  w.layers.resize(d.nlayers);
  for (int l = 0; l < d.nlayers; ++l) {
    const std::string p = "transformer_encoder.layers." + std::to_string(l) + ".";
    LayerW& L = w.layers[l];
    GETW(fq, p + "self_attn_between_features._w_qkv", (size_t)3 * HD * E);
    GETW(fo, p + "self_attn_between_features._w_out", (size_t)HD * E);
    GETW(io, p + "self_attn_between_items._w_out", (size_t)HD * E);
    GETW(m1, p + "mlp.linear1.weight", (size_t)Fh * E);
    GETW(m2, p + "mlp.linear2.weight", (size_t)E * Fh);
    const std::vector<float> fo_t = transpose_out(*fo, HD, E), io_t = transpose_out(*io, HD, E);
    const std::vector<float> m2p = pack_mlp2_perm(*m2, E, Fh);
    RC(fill(ctx, L.feat_qkv, *fq, Weight::GEMM));
    RC(fill(ctx, L.feat_out, fo_t, Weight::GEMM));
    RC(fill(ctx, L.feat_pack, pack_feat_rows(*fq, fo_t, d.nhead, E), Weight::BF16));
    RC(fill(ctx, L.feat_pack, pack_feat_rows(*fq, fo_t, d.nhead, E, true), Weight::F16));
    RC(fill(ctx, L.item_out, io_t, Weight::GEMM));
    RC(fill(ctx, L.item_out, permute_rows_f16(io_t, E, HD), Weight::F16));
    RC(fill(ctx, L.mlp1, *m1, Weight::F32 | Weight::F16 | Weight::SPLIT));
    RC(fill(ctx, L.mlp1, pack_mlp1_perm(*m1, E, Fh), Weight::BF16));
    RC(fill(ctx, L.mlp2, *m2, Weight::F32));
    RC(fill(ctx, L.mlp2, m2p, Weight::BF16 | Weight::SPLIT));  // (SPLIT: mlp_x3_kernel)
    RC(fill(ctx, L.mlp2, permute_rows_f16(m2p, E, Fh), Weight::F16));
    // item attention: q|k|v of the train rows, q of the test rows
    std::vector<float> wtrain((size_t)3 * HD * E), wtest((size_t)HD * E);
    if (d.two_sets_of_queries) {
      GETW(wq, p + "self_attn_between_items._w_q", (size_t)2 * HD * E);
      GETW(wkv, p + "self_attn_between_items._w_kv", (size_t)2 * HD * E);
      std::copy(wq->begin(), wq->begin() + (size_t)HD * E, wtrain.begin());
      std::copy(wkv->begin(), wkv->end(), wtrain.begin() + (size_t)HD * E);
      std::copy(wq->begin() + (size_t)HD * E, wq->end(), wtest.begin());
    } else {
      GETW(wqkv, p + "self_attn_between_items._w_qkv", (size_t)3 * HD * E);
      wtrain = *wqkv;
      std::copy(wqkv->begin(), wqkv->begin() + (size_t)HD * E, wtest.begin());
    }
    RC(fill(ctx, L.item_qkv, wtrain, Weight::F32 | Weight::SPLIT));
    RC(fill(ctx, L.item_qtest, wtest, Weight::F32 | Weight::SPLIT));
    prescale_item_q(wtrain, (size_t)HD * E, E / d.nhead);  // the 16-bit forms: prescaled Q rows
    prescale_item_q(wtest, wtest.size(), E / d.nhead);
    RC(fill(ctx, L.item_qkv, wtrain, Weight::BF16 | Weight::F16));
    RC(fill(ctx, L.item_qtest, wtest, Weight::BF16 | Weight::F16));
  }
  return MMPFN_OK;
}

int finalize_encoders_decoder(mmpfn_ctx* ctx, ModelWeights& w) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, Fh = d.nhid, nf = d.encoder_features;
  GETW(ew, d.remove_duplicate_features ? "encoder.6.layer.weight" : "encoder.5.layer.weight", (size_t)E * 2 * nf);
  // the Linear step follows the class-code step, which a value target's y encoder does not have (loading.py:374-398)
  const std::string yl = d.target_kind == MMPFN_TARGET_VALUE ? "y_encoder.1.layer." : "y_encoder.2.layer.";
  GETW(yw, yl + "weight", (size_t)E * 2);
  GETW(yb, yl + "bias", (size_t)E);
  GETW(pw, "feature_positional_embedding_embeddings.weight", (size_t)E * (E / 4));
  GETW(pb, "feature_positional_embedding_embeddings.bias", (size_t)E);
  GETW(dw1, "decoder_dict.standard.0.weight", (size_t)Fh * E);
  GETW(db1, "decoder_dict.standard.0.bias", (size_t)Fh);
  GETW(dw2, "decoder_dict.standard.2.weight", (size_t)d.n_out * Fh);
  GETW(db2, "decoder_dict.standard.2.bias", (size_t)d.n_out);
  for (auto [buf, v] : {std::pair{&w.enc_w, ew}, {&w.y_w, yw}, {&w.y_b, yb}, {&w.pe_w, pw}, {&w.pe_b, pb},
                        {&w.dec_b1, db1}, {&w.dec_b2, db2}})
    RC(upload(ctx, *buf, *v));
  if (d.target_kind == MMPFN_TARGET_VALUE) {  // launch_decoder_wide: both natural, one form per operand type
    RC(fill(ctx, w.dec_w1, *dw1, Weight::F32 | Weight::BF16 | Weight::F16));
    RC(fill(ctx, w.dec_w2, *dw2, Weight::F32 | Weight::BF16 | Weight::F16));
    return MMPFN_OK;
  }
  RC(fill(ctx, w.dec_w1, transpose_out(*dw1, Fh, E), Weight::F32));  // launch_decoder: W1 [E][Fh], W2 natural
  RC(fill(ctx, w.dec_w2, *dw2, Weight::F32));
  if (d.n_out <= 16 && Fh % 128 == 0) {  // launch_decoder_mfma: W1 natural, W2 zero-padded to [16][Fh] and permuted
    std::vector<float> w2p((size_t)16 * Fh, 0.f);
    std::copy(dw2->begin(), dw2->end(), w2p.begin());
    RC(fill(ctx, w.dec_w1, *dw1, Weight::BF16 | Weight::F16));
    RC(fill(ctx, w.dec_w2, pack_mlp2_perm(w2p, 16, Fh), Weight::BF16 | Weight::F16));
  }
  return MMPFN_OK;
}

// the MGM head bank (glu) or the MoE experts, heads stacked, every form in the one order: W1 [n][N1][D] with the
// LayerNorm folded in -- MGM: N1 = D, the GLU halves interleaved (glu_interleave); MoE: N1 = D/2 -- and W2 [n][E][D/2]
int finalize_heads(mmpfn_ctx* ctx, HeadBank& hb, const std::string& prefix, bool glu) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, D = d.nhid, n = d.mgm_heads, N1 = glu ? D : D / 2;
  std::vector<float> W1((size_t)n * N1 * D), B1((size_t)n * N1), W2((size_t)n * E * (D / 2)), B2((size_t)n * E);
  for (int h = 0; h < n; ++h) {
    const std::string p = prefix + std::to_string(h) + ".";
    GETW(g, p + "0.weight", (size_t)D);
    GETW(b, p + "0.bias", (size_t)D);
    GETW(w1, p + "1.weight", (size_t)N1 * D);
    GETW(b1, p + "1.bias", (size_t)N1);
    GETW(w2, p + "4.weight", (size_t)E * (D / 2));
    GETW(b2, p + "4.bias", (size_t)E);
    std::vector<float> wf = *w1, c = *b1;
    fold_ln(wf, c, g->data(), b->data(), N1, D);
    if (glu) glu_interleave(wf, c, D);
    std::copy(wf.begin(), wf.end(), W1.begin() + (size_t)h * N1 * D);
    std::copy(c.begin(), c.end(), B1.begin() + (size_t)h * N1);
    std::copy(w2->begin(), w2->end(), W2.begin() + (size_t)h * E * (D / 2));
    std::copy(b2->begin(), b2->end(), B2.begin() + (size_t)h * E);
  }
  // (fp16: PREC_F16's MGM head bank, the big-tile kernels only)
  const unsigned forms = glu && mgm_f16_shape(d) ? Weight::GEMM | Weight::F16 : Weight::GEMM;
  RC(fill(ctx, hb.w1, W1, forms));
  RC(fill(ctx, hb.w2, W2, forms));
  RC(upload(ctx, hb.b1, B1));
  return upload(ctx, hb.b2, B2);
}

int finalize_cap(mmpfn_ctx* ctx, ModelWeights& w) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, cap = d.cap_heads;
  GETW(qs, "cap.queries", (size_t)cap * E);
  GETW(qpw, "cap.q_proj.weight", (size_t)E * E);
  GETW(inw, "cap.mha.in_proj_weight", (size_t)3 * E * E);
  GETW(inb, "cap.mha.in_proj_bias", (size_t)3 * E);
  GETW(ow, "cap.mha.out_proj.weight", (size_t)E * E);
  GETW(ob, "cap.mha.out_proj.bias", (size_t)E);
  GETW(kg, "cap.k_norm.weight", (size_t)E);
  GETW(kb, "cap.k_norm.bias", (size_t)E);
  GETW(qg, "cap.q_norm.weight", (size_t)E);
  GETW(qb, "cap.q_norm.bias", (size_t)E);
  GETW(ng, "cap.out_norm.weight", (size_t)E);
  GETW(nb, "cap.out_norm.bias", (size_t)E);
  GETW(f0w, "cap.ffn.0.weight", (size_t)2 * E * E);
  GETW(f0b, "cap.ffn.0.bias", (size_t)2 * E);
  GETW(f3w, "cap.ffn.3.weight", (size_t)2 * E * E);
  GETW(f3b, "cap.ffn.3.bias", (size_t)E);
  RC(upload(ctx, w.cap_qp, cap_query_path(qs->data(), qg->data(), qb->data(), qpw->data(), inw->data(), inb->data(),
                                          cap, E, d.ln_eps)));
  // K/V in-projection with k_norm's affine folded in (k = v = k_norm(src))
  std::vector<float> wkv(inw->begin() + (size_t)E * E, inw->end());
  std::vector<float> bkv(inb->begin() + E, inb->end());
  fold_ln(wkv, bkv, kg->data(), kb->data(), 2 * E, E);
  RC(fill(ctx, w.cap_kv, wkv, Weight::GEMM));
  RC(fill(ctx, w.cap_o, *ow, Weight::GEMM));
  // the FFN's bf16 forms are read by the 16-bit modes' tail alone (launch_cap_tail: mlp_rows_kernel's CAP form)
  RC(fill(ctx, w.cap_f0, *f0w, Weight::F32 | Weight::SPLIT));
  RC(fill(ctx, w.cap_f0, pack_mlp1_perm(*f0w, E, 2 * E), Weight::BF16));
  RC(fill(ctx, w.cap_f3, *f3w, Weight::F32 | Weight::SPLIT));
  RC(fill(ctx, w.cap_f3, pack_mlp2_perm(*f3w, E, 2 * E), Weight::BF16));
  std::vector<float> v;  // [bo | b0 | g | b + b3]
  for (const std::vector<float>* part : {ob, f0b, ng}) v.insert(v.end(), part->begin(), part->end());
  for (int e = 0; e < E; ++e) v.push_back((*nb)[e] + (*f3b)[e]);
  RC(upload(ctx, w.cap_vecs, v));
  RC(upload(ctx, w.cap_kv_b, bkv));
  for (auto [buf, b] : {std::pair{&w.cap_o_b, ob}, {&w.cap_f0_b, f0b}, {&w.cap_f3_b, f3b}, {&w.cap_ng, ng},
                        {&w.cap_nb, nb}})
    RC(upload(ctx, *buf, *b));
  return MMPFN_OK;
}

int finalize(mmpfn_ctx* ctx) {
  const mmpfn_model_desc& d = ctx->d;
  ctx->w = ModelWeights();  // the previous model's set goes first: a re-finalise never holds two sets on the device
  ModelWeights w;
  RC(finalize_layers(ctx, w));
  RC(finalize_encoders_decoder(ctx, w));
  if (d.mixer_type == MMPFN_MIXER_MGM || d.mixer_type == MMPFN_MIXER_MGM_CAP)
    RC(finalize_heads(ctx, w.mgm, "mgm.projs.", true));
  if (d.mixer_type == MMPFN_MIXER_MGM_CAP) RC(finalize_cap(ctx, w));
  if (d.mixer_type == MMPFN_MIXER_MOE) {
    RC(finalize_heads(ctx, w.moe, "moe.experts.", false));
    GETW(gw, "moe.gate.weight", (size_t)d.mgm_heads * d.nhid);
    GETW(gb, "moe.gate.bias", (size_t)d.mgm_heads);
    RC(upload(ctx, w.moe_gw, *gw));
    RC(upload(ctx, w.moe_gb, *gb));
  }
  HIPCHK(hipDeviceSynchronize());
  ctx->w = std::move(w);
  return MMPFN_OK;
}

GemmArgs gargs() {
  GemmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.a_rdiv = a.rdiv2 = 1ll << 62, a.a_rmul2 = 1, a.ln_eps = 1e-5f;
  return a;
}

// a public precision code, decoded once (decode_prec) for the forward or the tap that it selects
struct PrecMode {
  int base = PREC_F32;  // the mode the layer kernels run: PREC_F32, PREC_F32_MFMA, PREC_BF16 or PREC_F16
  int f8 = 0;           // the fp8 P.V variant of the item attention (0: none)
  bool is16() const { return prec16(base); }
  bool f16() const { return base == PREC_F16; }
  // PREC_F16 runs the bf16 mode's kernels in their F16 forms: launch_gemm, launch_attn and Weight::gemm_operand see
  // PREC_BF16
  int gemm() const { return is16() ? PREC_BF16 : base; }
  DType w16() const { return f16() ? DType::F16 : DType::BF16; }  // the 16-bit modes' weight form (Weight::op16)
  // the inter-kernel state X: fp32, or fp16 under PREC_F16 (then the attention output O too)
  DType state() const { return f16() ? DType::F16 : DType::F32; }
  int state_bytes() const { return f16() ? 2 : 4; }
  int op_bytes() const { return is16() ? 2 : 4; }  // Q / K / V^T and the 16-bit modes' GEMM operands
  // the 16-bit modes' item attention: bf16 Q, K and V^T (every MFMA a bf16 one); O in the state's 16-bit type
  DType attn_out() const { return f16() ? DType::F16 : DType::BF16; }
};
// T: tokens per table row (T < 0: a row-wise sublayer, no token limit).  PREC_F16's layer kernels hold a row's tokens
// as up to four 16-token tiles; wider tables run PREC_BF16 -- the forward and the per-sublayer taps alike
PrecMode decode_prec(int code, int T) {
  PrecMode m{base_prec(code), f8_of(code)};
  if (m.base == PREC_F16 && T > 64) m.base = PREC_BF16;
  return m;
}
PrecMode lane_prec(const Lane& l) { return PrecMode{l.prec, l.f8}; }

// ---- The steps of a layer that every mode runs on a kernel family of its own: the q|k|v projection and the
//      out-projection + residual + LayerNorm here, the item attention behind launch_attn_layer(a, pm.base), the MLP in
//      mlp_sublayer.  Precision meets kernel family in these and nowhere else in the layer path.
//      rows16: the 16-bit modes run their row-resident kernels (rowgemm.hip); false (the feature attention of tables
//      wider than featrow.hip's 64 tokens): the generic bf16 GEMM on the fp32 state.
struct QkvRows {  // r's rows of X through w; project_qkv fills r.W / r.w_lo in the mode's form
  const Weight& w;
  RowSet r;
};
// X's row sets (one or two) -> Q [b][H][pos][32], K [b][H][pos][32] (Npad rows), V^T [b][H][32][Npad]; S: rows of Q
int project_qkv(mmpfn_ctx* ctx, PrecMode pm, bool rows16, const void* X, const QkvRows* sets, int nset, void* Q,
                void* K, void* Vt, int S, int Npad, int H) {
  hipStream_t st = ctx->stream;
  RowSet rs[2];
  if (nset < 1 || nset > 2) return fail(ctx, MMPFN_ERR_INVALID, "project_qkv: one or two row sets");
  for (int i = 0; i < nset; ++i) rs[i] = sets[i].r;
  if (pm.is16() && rows16) {
    for (int i = 0; i < nset; ++i) rs[i].W = sets[i].w.op16(pm.w16());
    HIPCHK(launch_rowgemm_qkv(X, rs, nset, Q, K, Vt, S, Npad, H, st, pm.state()));
  } else if (pm.base == PREC_F32) {  // parity mode: split-bf16 products, every set in one launch (rowgemm3.hip)
    for (int i = 0; i < nset; ++i) rs[i].W = sets[i].w.split.p, rs[i].w_lo = sets[i].w.numel;
    HIPCHK(launch_proj3_qkv((const float*)X, rs, nset, Q, K, Vt, S, Npad, H, st));
  } else {
    for (int i = 0; i < nset; ++i) {
      const RowSet& r = rs[i];
      if (r.M <= 0) continue;
      GemmArgs a = gargs();
      a.A = X, a.lda = ctx->d.emsize, a.a_rdiv = r.rdiv, a.a_rmul = r.rmul, a.a_rmul2 = r.rmul2, a.a_roff = r.roff;
      sets[i].w.gemm_operand(a, pm.gemm());
      a.M = r.M, a.N = r.N, a.K = ctx->d.emsize;
      a.q = Q, a.k = K, a.v = Vt, a.S = S, a.Npad = Npad, a.T = (int)(r.M / r.rdiv), a.H = H;
      HIPCHK(launch_gemm(a, pm.gemm(), EPI_ITEM_QKV, true, !pm.is16(), 1, st));
    }
  }
  return MMPFN_OK;
}

// X <- LN(X + O W^T) over `rows` tokens (O: an attention output, W: its out-projection)
int out_proj_ln(mmpfn_ctx* ctx, PrecMode pm, bool rows16, const Weight& W, const void* O, void* X, int64_t rows) {
  const mmpfn_model_desc& d = ctx->d;
  hipStream_t st = ctx->stream;
  if (pm.is16() && rows16) {
    HIPCHK(launch_rowgemm_resln(O, W.op16(pm.w16()), rows, X, d.ln_eps, st, pm.state()));
  } else if (pm.base == PREC_F32) {
    HIPCHK(launch_proj3_resln((const float*)O, W.split.p, W.numel, rows, (float*)X, d.ln_eps, st));
  } else {  // (bf16: O bf16, X fp32)
    GemmArgs b = gargs();
    b.A = O, b.lda = d.emsize, W.gemm_operand(b, pm.gemm());
    b.M = (int)rows, b.N = d.emsize, b.K = d.emsize, b.X = (float*)X, b.ln_eps = d.ln_eps;
    HIPCHK(launch_gemm(b, pm.gemm(), EPI_RES_LN, !pm.is16(), true, 1, st));
  }
  return MMPFN_OK;
}

// the selected lane's workspaces for M members of S x T tokens with Npad padded train rows: ws_X (own_state; a tap
// runs on the caller's) and ws_O hold the state and the attention output, ws_big the Q / K / V^T of the feature
// attention (member by member) or of the item attention (all members at once)
int lane_workspace(mmpfn_ctx* ctx, int S, int T, int Npad, int M, bool own_state) {
  const size_t E = ctx->d.emsize, R = (size_t)S * T, Tpad = (T + 63) / 64 * 64;
  const size_t feat = R * E + (size_t)2 * S * Tpad * E, item = (size_t)M * (R * E + (size_t)2 * T * Npad * E);
  if (own_state) RC(ensure(ctx, ctx->ws_X, (size_t)M * R * E * 4));
  RC(ensure(ctx, ctx->ws_O, (size_t)M * R * E * 4));
  return ensure(ctx, ctx->ws_big, std::max(feat, item) * 4);
}

// member m (of M, all of the geometry set by member 0) -> X[m] = embedded input [T][S][E]
int embed(mmpfn_ctx* ctx, const float* x, int S, int F, const float* tokens, int C, const float* y, int N,
          const float* uniq, int U, const float* pos_rand, int precision, int m = 0, int M = 1) {
  const mmpfn_model_desc& d = ctx->d;
  if (!ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "weights not finalised");
  const bool value_target = d.target_kind == MMPFN_TARGET_VALUE;  // no class codes: uniq / U unused
  if (S <= 0 || N <= 0 || N > S || (x && F <= 0) || C < 0 || (!value_target && U <= 0))
    return fail(ctx, MMPFN_ERR_INVALID, "bad forward geometry");
  if (!x && C == 0) return fail(ctx, MMPFN_ERR_INVALID, "no input tokens");
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  const int E = d.emsize, fpg = d.features_per_group;
  const int G = x ? (F + fpg - 1) / fpg : 0;
  const int T = G + C + 1;
  const PrecMode pm = decode_prec(precision, T);
  const int Npad = (N + 63) / 64 * 64;
  const size_t R = (size_t)S * T;
  hipStream_t st = ctx->stream;
  int* flag;
  if (m == 0) {
    ctx->S = S, ctx->T = T, ctx->N = N, ctx->G = G, ctx->C = C, ctx->Npad = Npad, ctx->prec = pm.base, ctx->M = M;
    ctx->f8 = pm.f8;
    RC(lane_workspace(ctx, S, T, Npad, M, true));
    RC(ensure(ctx, ctx->ws_pe, (size_t)(G + C + 1) * E * 4));
    RC(ensure(ctx, ctx->ws_slots, (size_t)(G + 1) * fpg * sizeof(SlotParams)));
    RC(ensure(ctx, ctx->ws_scr, 256));
    RC(ensure_flag(ctx, ctx->ws_flag, st));
    flag = (int*)ctx->ws_flag.p;
    HIPCHK(launch_pos_emb(pos_rand, G + C, (const float*)ctx->w.pe_w.p, (const float*)ctx->w.pe_b.p,
                          (float*)ctx->ws_pe.p, E, st));
  } else {
    if (S != ctx->S || T != ctx->T || N != ctx->N || G != ctx->G || C != ctx->C || pm.base != ctx->prec ||
        pm.f8 != ctx->f8 || m >= ctx->M)
      return fail(ctx, MMPFN_ERR_INVALID, "batched members must share S, N, F, C and precision");
    flag = (int*)ctx->ws_flag.p;
  }
  // the encoders write the state dtype directly (fp16 in PREC_F16)
  void* X = (char*)ctx->ws_X.p + (size_t)m * R * E * pm.state_bytes();
  HIPCHK(launch_encode_stats(x, S, F, N, G, fpg, d.outlier_sigma, (SlotParams*)ctx->ws_slots.p, y, N,
                             (float*)ctx->ws_scr.p, st));
  HIPCHK(launch_assemble(x, S, F, G, fpg, d.encoder_features, (const SlotParams*)ctx->ws_slots.p,
                         (const float*)ctx->w.enc_w.p, (const float*)ctx->ws_pe.p, tokens, C, y, N, uniq, U,
                         (const float*)ctx->w.y_w.p, (const float*)ctx->w.y_b.p, (const float*)ctx->ws_scr.p, X,
                         pm.state(), E, flag, st, value_target));
  ctx->embedded = true;
  return MMPFN_OK;
}

// test rows against a train-KV cache, in the cache's precision: every row of the state is a test row (N = 0), the
// encoders apply the cached train statistics (transformer.py:779-784 use_cached_embeddings; encoders.py
// steps with cache_trainset_representation)
int embed_cached(mmpfn_ctx* ctx, const mmpfn_cache* cc, const float* x, int S, int F, const float* tokens, int C) {
  const mmpfn_model_desc& d = ctx->d;
  if (!ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "weights not finalised");
  if (S <= 0 || F != cc->F || C != cc->C || (F > 0 && !x) || (C > 0 && !tokens))
    return fail(ctx, MMPFN_ERR_INVALID, "test rows must match the cache's features, tokens and precision");
  const int E = d.emsize, fpg = d.features_per_group, G = cc->G, T = cc->T;
  hipStream_t st = ctx->stream;
  ctx->S = S, ctx->T = T, ctx->N = 0, ctx->G = G, ctx->C = C, ctx->Npad = 0, ctx->prec = cc->prec, ctx->M = 1;
  ctx->f8 = 0;  // the cache keeps bf16 V^T: its test rows run the bf16 P.V
  RC(lane_workspace(ctx, S, T, 0, 1, true));
  RC(ensure_flag(ctx, ctx->ws_flag, st));
  int* flag = (int*)ctx->ws_flag.p;
  HIPCHK(launch_assemble(x, S, F, G, fpg, d.encoder_features, (const SlotParams*)cc->slots.p,
                         (const float*)ctx->w.enc_w.p, (const float*)cc->pe.p, tokens, C, nullptr, 0,
                         (const float*)cc->uniq.p, cc->U, (const float*)ctx->w.y_w.p, (const float*)ctx->w.y_b.p,
                         (const float*)cc->ymean.p, ctx->ws_X.p, lane_prec(*ctx).state(), E, flag, st,
                         d.target_kind == MMPFN_TARGET_VALUE));
  ctx->embedded = true;
  return MMPFN_OK;
}

// ---- attention between features (layer.py:332-339): X [M][T][S][E] <- LN(X + FeatAttn(X)), batch = row s
//      last: only the target token T-1 of every row is needed (a pruned last layer); the row-resident kernel then
//      computes and stores that token alone, the other paths run in full
int feat_sublayer(mmpfn_ctx* ctx, const LayerW& L, void* Xv, int S, int T, int M, PrecMode pm, bool last = false) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, H = d.nhead;
  const int64_t R = (int64_t)S * T;
  const int eb = pm.op_bytes();
  hipStream_t st = ctx->stream;
  void* O = ctx->ws_O.p;
  unsigned char* big = (unsigned char*)ctx->ws_big.p;
  if (pm.is16() && T <= 64) {
    // one wave per row (all M members' rows in one launch), the whole sublayer in registers (featrow.hip); an
    // fp16 state always comes here (decode_prec keeps PREC_F16 to T <= 64)
    HIPCHK(launch_feat_rows(Xv, L.feat_pack.op16(pm.w16()), S, T, M, E, H, d.ln_eps, st, pm.state(),
                            last));
    return MMPFN_OK;
  }
  const int Tpad = (T + 63) / 64 * 64;
  void* Qf = big;
  void* Kf = big + (size_t)R * E * eb;
  void* Vf = (unsigned char*)Kf + (size_t)S * H * Tpad * 32 * eb;
  for (int m = 0; m < M; ++m) {  // member by member (the scratch holds one member)
    float* X = (float*)Xv + (size_t)m * R * E;
    // logical rows m = s*T + t: A row t*S + s; scatter batch b = s, position t
    const QkvRows rows{L.feat_qkv, {T, 1, S, 0, (int)R, 3 * E}};
    RC(project_qkv(ctx, pm, false, X, &rows, 1, Qf, Kf, Vf, T, Tpad, H));
    AttnArgs f;
    f.q = Qf, f.k = Kf, f.vt = Vf, f.o = O;
    f.q_bstride = (int64_t)H * T * 32, f.q_hstride = (int64_t)T * 32;
    f.kv_bstride = (int64_t)H * Tpad * 32, f.kv_hstride = (int64_t)Tpad * 32, f.kpad = Tpad;
    f.o_bstride = 1, f.o_qstride = S;  // O[t][s]
    f.s0 = 0, f.nq = T, f.nk = T, f.kvh_fixed = -1, f.H = H;
    HIPCHK(launch_attn(f, S, pm.gemm(), 1, st));
    RC(out_proj_ln(ctx, pm, false, L.feat_out, O, X, R));
  }
  return MMPFN_OK;
}

// ---- the item attention's q|k|v projection of layer l: the one place that builds its row sets.  Rows of all members:
//      logical row (member*T + t)*N + n -> memory row (member*T + t)*S + n, attention batch member*T + t.
//      Not cached: the train rows [0, N) through q|k|v and the test rows [N, S) through the test rows' q, in one launch
//      where the mode has one (test-row blocks last; an empty test set launches no block: its M is 0 whatever its
//      divisor).  cached (a predict against a train-KV cache): every one of the S rows through the test rows' q; K / Vt
//      are not written.  last: the pruned last layer's form, the target-token column T-1 of every member only -- M
//      columns, T*S state rows apart, into compact Q [M][H][S][32], K [M][H][Npad][32], V^T [M][H][32][Npad].
//      item_sublayer and the mmpfn_item_qkv tap both come here: what the tap runs is what the forwards run.
int item_project(mmpfn_ctx* ctx, int l, const void* Xv, int S, int T, int N, int Npad, int M, PrecMode pm, bool last,
                 bool cached, void* Q, void* K, void* Vt) {
  const LayerW& L = ctx->w.layers[l];
  const int E = ctx->d.emsize, H = ctx->d.nhead;
  const int TM = last ? M : T * M;               // token columns of the batch (attention batches)
  const int64_t cs = last ? (int64_t)T * S : S;  // state rows between consecutive columns
  if (last) Xv = (const char*)Xv + (size_t)(T - 1) * S * E * pm.state_bytes();
  if (cached) {
    const QkvRows rows{L.item_qtest, {S, cs, 1, 0, TM * S, E}};
    return project_qkv(ctx, pm, true, Xv, &rows, 1, Q, K, Vt, S, Npad, H);
  }
  const int nq = S - N;
  const QkvRows rows[2] = {{L.item_qkv, {N, cs, 1, 0, TM * N, 3 * E}},
                           {L.item_qtest, {nq > 0 ? nq : 1, cs, 1, N, TM * nq, E}}};
  return project_qkv(ctx, pm, true, Xv, rows, 2, Q, K, Vt, S, Npad, H);
}

// ---- the item attention's launch arguments as the forwards build them, in one place: the task map (own-head rows,
//      shared-KV rows, the cache stride) and the operand form of the mode.  TM token columns of S rows, N train rows
//      (keys), K / V^T rows padded to Npad; the caller adds the operands' addresses (and the fp8 V^T).
//      full:   train rows [0, N) against their own heads, test rows [N, S) of every head against head 0's K / V (MQA).
//      last:   the pruned last layer: of the train rows only those that share the test rows' first 256-query task.
//      cached: every row is a test row, against a head-0-only K / V^T (column blocks Npad * 32 elements apart).
//      item_sublayer and the mmpfn_item_attention_forward tap both come here: what the tap launches is what the
//      forwards launch.
enum ItemAttnForm { ITEM_ATTN_FULL = 0, ITEM_ATTN_LAST = 1, ITEM_ATTN_CACHED = 2 };
AttnLayerArgs item_attn_args(ItemAttnForm form, int S, int N, int TM, int H, int Npad, PrecMode pm) {
  AttnLayerArgs a{nullptr, nullptr, nullptr, nullptr, S, TM, H, Npad, N};
  if (form == ITEM_ATTN_CACHED) {
    a.a0 = 0, a.na = 0, a.b0 = 0, a.nb = S, a.kvb = 0;  // every row against head 0 of the cache
    a.kv_bstride = (int64_t)Npad * 32;
  } else {
    // train rows (own heads) and test rows (head-0 K/V, MQA)
    a.a0 = 0, a.na = N, a.b0 = N, a.nb = S - N, a.kvb = 0;
    if (form == ITEM_ATTN_LAST) a.na = N % ATTN_ITEM_QPB, a.a0 = N - a.na;
  }
  a.q_prescaled = pm.is16(), a.o_t = pm.attn_out();  // (qk_t: bf16 in every forward)
  return a;
}

// ---- attention between items (layer.py:341-379) of layer l over the rows of all members (item_project has the row
//      map).
//      fuse_out: the out-projection + residual + LN is left to the caller's layer_tail (the attention output
//      stays in ws_O; the 16-bit modes run it as the MLP kernel's prologue); otherwise -- the
//      mmpfn_item_attention_block tap -- X <- LN(X + O Wout^T) here.
//      last: the pruned form of a forward's last layer (last_layer_tail): the target-token column T-1 of every
//      member only -- M columns, T*S rows apart, into compact Q / K / V^T scratch and a compact O [M][S][E] -- and
//      of its queries only the test rows; the out-projection is left to the caller.  The test rows keep the places
//      they have in the full launch's 256-query tasks (the train rows that share their first task ride along), so
//      every block that holds one sees the same queries and takes the same wave-wide re-run decisions as there.
//      last && all_rows: the column form (last_layer_column): the same one column per member, every query of it --
//      the full task map on M columns, so column T-1's queries sit in the 256-query tasks they have in the full layer.
int item_sublayer(mmpfn_ctx* ctx, int l, void* Xv, int S, int T, int N, int Npad, int M, PrecMode pm, bool fuse_out,
                  bool last = false, bool all_rows = false) {
  const mmpfn_model_desc& d = ctx->d;
  const LayerW& L = ctx->w.layers[l];
  const int E = d.emsize, H = d.nhead, Q = S - N;
  const int TM = last ? M : T * M;     // token columns of the batch (attention batches)
  const int64_t RM = (int64_t)S * TM;  // tokens of the batch
  const int c0 = last ? T - 1 : 0, nc = last ? 1 : T;  // the columns of one member, as the cache numbers them
  const int eb = pm.op_bytes();
  hipStream_t st = ctx->stream;
  void* O = ctx->ws_O.p;
  unsigned char* big = (unsigned char*)ctx->ws_big.p;
  void* Qi = big;
  void* Ki = big + (size_t)RM * E * eb;
  void* Vi = (unsigned char*)Ki + (size_t)TM * H * Npad * 32 * eb;
  RC(item_project(ctx, l, Xv, S, T, N, Npad, M, pm, last, ctx->cache_in != nullptr, Qi, Ki, Vi));
  if (ctx->cache_in) {  // every row is a test row: Q only, against the cached train K/V of head 0
    const mmpfn_cache* cc = ctx->cache_in;
    const size_t kvl = (size_t)T * cc->Npad * 32 * eb;
    const size_t ccol = (size_t)c0 * cc->Npad * 32 * eb;  // the first column's K (V^T) block inside the layer's
    const unsigned char* Kc = (const unsigned char*)cc->kv.p + (size_t)l * 2 * kvl + ccol;
    AttnLayerArgs a = item_attn_args(ITEM_ATTN_CACHED, S, cc->N, TM, H, cc->Npad, pm);
    a.q = Qi, a.k = Kc, a.vt = Kc + kvl, a.out = O;
    HIPCHK(launch_attn_layer(a, pm.base, st));
  } else {
    if (ctx->cache_out) {  // keep head 0's K / V^T of every column (the test rows' KV, layer.py:344-358)
      mmpfn_cache* cc = ctx->cache_out;
      const size_t blk = (size_t)Npad * 32 * eb, kvl = (size_t)T * blk;
      unsigned char* Kc = (unsigned char*)cc->kv.p + (size_t)l * 2 * kvl + c0 * blk;
      HIPCHK(hipMemcpy2DAsync(Kc, blk, Ki, (size_t)H * blk, blk, nc, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpy2DAsync(Kc + kvl, blk, Vi, (size_t)H * blk, blk, nc, hipMemcpyDeviceToDevice, st));
    }
    if (last && !all_rows && Q == 0) return MMPFN_OK;  // (a cache build: nothing reads the last layer's train-row outputs)
    AttnLayerArgs a = item_attn_args(last && !all_rows ? ITEM_ATTN_LAST : ITEM_ATTN_FULL, S, N, TM, H, Npad, pm);
    a.q = Qi, a.k = Ki, a.vt = Vi, a.out = O;
    hipEvent_t* ev = nullptr;
    if (pm.is16()) {  // the live timing and the fp8 P.V exist for the pipelined kernel only
      if (ctx->kt_on && !last) {  // (the roofline's launches all have the full layer's shape)
        if (ctx->kt_used + 2 > ctx->kt_pool.size()) {
          for (int i = 0; i < 64; ++i) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            ctx->kt_pool.push_back(e);
          }
        }
        ev = &ctx->kt_pool[ctx->kt_used];
        ctx->kt_used += 2;
        ctx->kt_flops += 4.0 * TM * (double)(N + Q) * N * E;
      }
      if (pm.f8) {  // e4m3 V^T after the bf16 one (ws_big holds twice the bf16 Q / K / V^T bytes)
        void* V8 = (unsigned char*)Vi + (size_t)TM * H * Npad * 32 * eb;
        HIPCHK(launch_vt_fp8(Vi, V8, (int64_t)TM * H * Npad * 32, st));
        a.vt8 = V8, a.f8 = pm.f8;
      }
    }
    if (ev) HIPCHK(hipEventRecord(ev[0], st));
    HIPCHK(launch_attn_layer(a, pm.base, st));
    if (ev) HIPCHK(hipEventRecord(ev[1], st));
  }
  if (fuse_out || last) return MMPFN_OK;
  return out_proj_ln(ctx, pm, true, L.item_out, O, Xv, RM);
}

// ---- MLP (mlp.py:93-104) + residual + LN over RM tokens; O non-null (the 16-bit modes): the item attention's
//      out-projection + residual + LN first, as the kernel's prologue
int mlp_sublayer(mmpfn_ctx* ctx, const LayerW& L, void* Xv, int64_t RM, PrecMode pm, const void* O) {
  const mmpfn_model_desc& d = ctx->d;
  float* Xall = (float*)Xv;
  if (pm.is16()) {
    const DType t = pm.w16();
    HIPCHK(launch_mlp_rows(Xv, L.mlp1.op16(t), L.mlp2.op16(t), RM, d.emsize, d.nhid, d.ln_eps, ctx->stream, O,
                           O ? L.item_out.op16(t) : nullptr, pm.state()));
  } else if (pm.base == PREC_F32) {  // parity mode: mlp_x3_kernel on split-bf16 products (W1 / W2 hi | lo planes)
    HIPCHK(launch_mlp_fused(Xall, L.mlp1.split.p, L.mlp2.split.p, RM, d.emsize, d.nhid, d.ln_eps, PREC_F32,
                            ctx->stream));
  } else {
    HIPCHK(launch_mlp_fused(Xall, L.mlp1.f32.p, L.mlp2.f32.p, RM, d.emsize, d.nhid, d.ln_eps, PREC_F32_MFMA,
                            ctx->stream));
  }
  return MMPFN_OK;
}

// ---- attention output -> state, the step behind the item attention: X <- LN(X' + MLP(X')), X' = LN(X + O Wout^T)
//      over `rows` tokens.  O: the item attention's output in the mode's type (PrecMode::attn_out; fp32 in the fp32
//      modes).  The 16-bit modes run it as one kernel (the out-projection is the MLP kernel's prologue), the fp32 modes
//      as two.  run_layer, last_layer_tail and the mmpfn_outproj_mlp_ln tap all come here: what the tap runs is what
//      the forwards run.
int layer_tail(mmpfn_ctx* ctx, const LayerW& L, void* X, const void* O, int64_t rows, PrecMode pm) {
  if (pm.is16()) return mlp_sublayer(ctx, L, X, rows, pm, O);
  RC(out_proj_ln(ctx, pm, true, L.item_out, O, X, rows));
  return mlp_sublayer(ctx, L, X, rows, pm, nullptr);
}

int run_layer(mmpfn_ctx* ctx, int l) {
  const LayerW& L = ctx->w.layers[l];
  const int S = ctx->S, T = ctx->T, N = ctx->N, Npad = ctx->Npad, M = ctx->M;
  const PrecMode pm = lane_prec(*ctx);
  void* Xall = ctx->ws_X.p;
  RC(feat_sublayer(ctx, L, Xall, S, T, M, pm));
  RC(item_sublayer(ctx, l, Xall, S, T, N, Npad, M, pm, true));  // the attention output stays in ws_O
  return layer_tail(ctx, L, Xall, ctx->ws_O.p, (int64_t)S * T * M, pm);
}

// The last layer has three forms: run_layer (in full: the taps, and the forwards under mmpfn_set_full_last_layer),
// last_layer_tail (what the decoder reads: every forward by default) and last_layer_column (what the train rows'
// embeddings need besides: mmpfn_forward_embed with train_emb, and nothing else).
//
// The last layer of a forward, pruned to what the decoder reads: the test rows [N, S) of the target token (column
// T-1) of every member.  Exact, since every kernel computes a state row from that row's own inputs:
//   feature attention   every row (a test row's target token attends over the row's tokens; a train row's is the
//                       K / V of column T-1), its output at token T-1 (the row-resident kernel's LAST form computes
//                       only that one; the T > 64 and fp32 paths run in full);
//   item attention      column T-1 only: K / V^T of its train rows, Q of its test rows (item_sublayer, last);
//   out-projection, MLP the Q test rows of that column, member by member.
// Afterwards the state holds this layer's output at those rows only; every other row is left as this layer's
// feature attention or the layer before wrote it.
int last_layer_tail(mmpfn_ctx* ctx, int l) {
  const LayerW& L = ctx->w.layers[l];
  const int S = ctx->S, T = ctx->T, N = ctx->N, Npad = ctx->Npad, M = ctx->M, E = ctx->d.emsize;
  const PrecMode pm = lane_prec(*ctx);
  RC(feat_sublayer(ctx, L, ctx->ws_X.p, S, T, M, pm, true));
  RC(item_sublayer(ctx, l, ctx->ws_X.p, S, T, N, Npad, M, pm, true, true));
  const int64_t Q = S - N;
  if (Q == 0) return MMPFN_OK;
  const size_t ob = pm.op_bytes();  // the attention output's element: 16-bit in the 16-bit modes
  for (int m = 0; m < M; ++m) {
    void* X = (char*)ctx->ws_X.p + (((size_t)m * T + T - 1) * S + N) * E * pm.state_bytes();
    const void* O = (const char*)ctx->ws_O.p + ((size_t)m * S + N) * E * ob;  // compact: one column per member
    RC(layer_tail(ctx, L, X, O, Q, pm));
  }
  return MMPFN_OK;
}

// The last layer of a forward that returns the train rows' embeddings (mmpfn_forward_embed with train_emb): the
// column form, the target-token column T-1 of every member, all S rows.  last_layer_tail with the train rows kept:
//   feature attention   as there (token T-1 of every row);
//   item attention      column T-1 only, Q of all its rows, the full layer's task map on M columns (item_sublayer,
//                       last and all_rows) -- the launch of a full layer that had no other column;
//   out-projection, MLP the S rows of that column, member by member, O compact [M][S][E].
// Exact for the same reason, so column T-1 afterwards holds what run_layer leaves there bit for bit; the other
// columns are left as last_layer_tail leaves them.
int last_layer_column(mmpfn_ctx* ctx, int l) {
  const LayerW& L = ctx->w.layers[l];
  const int S = ctx->S, T = ctx->T, N = ctx->N, Npad = ctx->Npad, M = ctx->M, E = ctx->d.emsize;
  const PrecMode pm = lane_prec(*ctx);
  RC(feat_sublayer(ctx, L, ctx->ws_X.p, S, T, M, pm, true));
  RC(item_sublayer(ctx, l, ctx->ws_X.p, S, T, N, Npad, M, pm, true, true, true));
  const size_t ob = pm.op_bytes();
  for (int m = 0; m < M; ++m) {
    void* X = (char*)ctx->ws_X.p + ((size_t)m * T + T - 1) * S * E * pm.state_bytes();
    const void* O = (const char*)ctx->ws_O.p + (size_t)m * S * E * ob;
    RC(layer_tail(ctx, L, X, O, S, pm));
  }
  return MMPFN_OK;
}

// every layer of a forward entry point: the last one pruned -- to the test rows of the target token, or with
// `column` (a forward that returns the train rows' embeddings) to all of its rows -- unless
// mmpfn_set_full_last_layer asked for it in full
int run_forward_layers(mmpfn_ctx* ctx, bool column = false) {
  const int nl = ctx->d.nlayers;
  for (int l = 0; l < nl; ++l) {
    if (l < nl - 1 || ctx->full_last) RC(run_layer(ctx, l));
    else RC(column ? last_layer_column(ctx, l) : last_layer_tail(ctx, l));
  }
  return MMPFN_OK;
}

// decoder over the test rows of M batched members (logits [M][Q][n_out]); the tile partials go
// through the attention-output workspace, free once the last layer has run
int decode(mmpfn_ctx* ctx, float* logits, int M = 1) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, S = ctx->S, T = ctx->T, N = ctx->N, Q = S - N;
  const PrecMode pm = lane_prec(*ctx);
  const size_t off = ((size_t)(T - 1) * S + N) * E;
  const float* Xl = (const float*)ctx->ws_X.p + off;
  int64_t xm = (int64_t)S * T * E;
  const ModelWeights& w = ctx->w;
  if (d.target_kind == MMPFN_TARGET_VALUE) {  // n_out bars: two GEMMs in the mode's operand type, hidden through ws_O
    const DType op = pm.is16() ? pm.w16() : DType::F32;
    RC(ensure(ctx, ctx->ws_O, (size_t)M * Q * d.nhid * pm.op_bytes()));
    const void* X = (const char*)ctx->ws_X.p + off * pm.state_bytes();
    HIPCHK(launch_decoder_wide(X, pm.state(), Q, xm, M, pm.is16() ? w.dec_w1.op16(op) : w.dec_w1.f32.p,
                               (const float*)w.dec_b1.p, d.nhid, pm.is16() ? w.dec_w2.op16(op) : w.dec_w2.f32.p,
                               (const float*)w.dec_b2.p, d.n_out, op, ctx->ws_O.p, logits, E, ctx->stream));
    return MMPFN_OK;
  }
  if (pm.is16() && w.dec_w1.bf16.p) {  // the state as it is (fp32 / fp16) into 16-bit MFMA operands
    const void* X = (const char*)ctx->ws_X.p + off * pm.state_bytes();
    HIPCHK(launch_decoder_mfma(X, pm.state(), Q, w.dec_w1.op16(pm.w16()), (const float*)w.dec_b1.p, d.nhid,
                               w.dec_w2.op16(pm.w16()), (const float*)w.dec_b2.p, d.n_out, logits, E, ctx->stream, M,
                               xm, (int64_t)Q * d.n_out));
    return MMPFN_OK;
  }
  if (pm.f16()) {  // the target token's test rows of every member to fp32 (the big workspace is free)
    RC(ensure(ctx, ctx->ws_big, (size_t)M * Q * E * 4));
    HIPCHK(launch_f16_to_f32((const uint16_t*)ctx->ws_X.p + off, xm, (float*)ctx->ws_big.p, (int64_t)Q * E,
                             (int64_t)Q * E, M, ctx->stream));
    Xl = (const float*)ctx->ws_big.p, xm = (int64_t)Q * E;
  }
  RC(ensure(ctx, ctx->ws_O, (size_t)M * (d.nhid / 32 + 1) * Q * d.n_out * sizeof(float)));
  HIPCHK(launch_decoder(Xl, Q, (const float*)w.dec_w1.f32.p, (const float*)w.dec_b1.p, d.nhid,
                        (const float*)w.dec_w2.f32.p, (const float*)w.dec_b2.p, d.n_out, logits, E, ctx->stream, M,
                        xm, (int64_t)Q * d.n_out, (float*)ctx->ws_O.p));
  return MMPFN_OK;
}

// rows [r0, r0 + n) of the target token's final state of the lane's M members -> out fp32 [M][n][E]: the train rows'
// embeddings (r0 = 0, n = N) or the test rows' (r0 = N, n = S - N), transformer.py:850-864
int target_rows(mmpfn_ctx* ctx, int r0, int n, float* out) {
  HIPCHK(launch_target_rows(ctx->ws_X.p, lane_prec(*ctx).state(), ctx->S, ctx->T, ctx->d.emsize, ctx->M, r0, n, out,
                            ctx->stream));
  return MMPFN_OK;
}

// what the embedding entry points refuse before anything is launched
int check_outputs(mmpfn_ctx* ctx, const char* who, const float* logits, const float* train_emb, const float* test_emb) {
  if (!logits && !train_emb && !test_emb) return fail(ctx, MMPFN_ERR_INVALID, std::string(who) + ": no output asked for");
  if (((uintptr_t)train_emb | (uintptr_t)test_emb) % 16 != 0)
    return fail(ctx, MMPFN_ERR_INVALID, std::string(who) + ": the embedding outputs must be 16-byte aligned");
  return MMPFN_OK;
}

// the layers, the embeddings and the decoder of a forward whose members are embedded (mmpfn_forward_embed and its
// batch and cache forms); null outputs are skipped, train_emb alone selects the column form of the last layer
int forward_outputs(mmpfn_ctx* ctx, float* logits, float* train_emb, float* test_emb, int M) {
  RC(run_forward_layers(ctx, train_emb != nullptr));
  // (before the decoder: one of its forms converts the fp16 test rows through the big workspace, none writes the state)
  if (train_emb) RC(target_rows(ctx, 0, ctx->N, train_emb));
  if (test_emb) RC(target_rows(ctx, ctx->N, ctx->S - ctx->N, test_emb));
  return logits ? decode(ctx, logits, M) : MMPFN_OK;
}

// MGM head bank (transformer.py:33-57): image [S][n_mod][D] -> tokens [S][mgm*n_mod][E] (head-major)
// tok_t: the tokens' type -- fp32, or the head bank's 16-bit operand type (the MGM+CAP chain's intermediate).
// PREC_F16 runs the head bank on fp16 operands (LN output, GLU hidden, weights) where finalize uploaded the fp16
// bank (mgm_f16_shape), else in the bf16 mode: fp16's 3 extra mantissa bits cut the mixer's share of the logits
// error ~7x, and the reference's own fp16 autocast runs these linears in fp16.
DType mgm_operands(const mmpfn_ctx* ctx, PrecMode pm) {
  return !pm.is16() ? DType::F32 : pm.f16() && ctx->w.mgm.w1.f16.p ? DType::F16 : DType::BF16;
}

int mixer_mgm(mmpfn_ctx* ctx, const float* image, int S, int n_mod, void* mtok, PrecMode pm,
              DType tok_t = DType::F32) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, D = d.nhid;
  const DType t = mgm_operands(ctx, pm);
  const HeadBank& w = ctx->w.mgm;
  const bool b16 = pm.is16();
  const int eb = pm.op_bytes();
  hipStream_t st = ctx->stream;
  const int64_t rows = (int64_t)S * n_mod;
  const int mg = d.mgm_heads, M = mg * n_mod;
  RC(ensure(ctx, ctx->mx[0], (size_t)rows * D * eb));             // normalised image
  RC(ensure(ctx, ctx->mx[1], (size_t)rows * mg * (D / 2) * eb));  // GLU output
  HIPCHK(launch_layernorm_rows(image, rows, D, 1e-5f, ctx->mx[0].p, t, nullptr, nullptr, st));
  if (b16 && (mg * D) % 256 == 0) {
    HIPCHK(launch_gemm_glu_big(ctx->mx[0].p, w.w1.op16(t), (const float*)w.b1.p,
                               ctx->mx[1].p, (int)rows, mg * D, D, st, t));
  } else {
    GemmArgs a = gargs();
    a.A = ctx->mx[0].p, a.lda = D, w.w1.gemm_operand(a, pm.gemm());
    a.bias = (const float*)w.b1.p;
    a.M = (int)rows, a.N = mg * D, a.K = D, a.C = ctx->mx[1].p, a.ldc = (int64_t)mg * (D / 2);
    HIPCHK(launch_gemm(a, pm.gemm(), EPI_GLU, !b16, !b16, 1, st));
  }
  if (b16) {  // the big-tile down-projection (16-bit tokens possible)
    HIPCHK(launch_gemm_remap_big(ctx->mx[1].p, (int64_t)mg * (D / 2), w.w2.op16(t),
                                 (const float*)w.b2.p, mtok, tok_t, (int)rows, D / 2, mg, n_mod, E, st, t));
    return MMPFN_OK;
  }
  GemmArgs b = gargs();
  b.A = ctx->mx[1].p, b.lda = (int64_t)mg * (D / 2), b.a_zstride = D / 2;
  w.w2.gemm_operand(b, pm.base), b.w_zstride = (int64_t)E * (D / 2);
  b.bias = (const float*)w.b2.p, b.b_zstride = E;
  b.M = (int)rows, b.N = E, b.K = D / 2;
  b.C = mtok, b.ldc = E, b.rdiv2 = n_mod, b.rmul2 = M, b.zmul = n_mod;
  HIPCHK(launch_gemm(b, pm.base, EPI_REMAP, true, true, mg, st));
  return MMPFN_OK;
}

// CrossAttentionPooler (transformer.py:60-88): MGM tokens [S][M][E] (in_t: fp32, or mixer_mgm's 16-bit form) ->
// tokens [S][cap][E]; PREC_F16 runs the pooler in the bf16 mode from the row pass on (its K|V, attention and tail
// stay bf16)
int mixer_cap(mmpfn_ctx* ctx, const void* mtok, int S, int M, float* tokens, PrecMode pm, DType in_t = DType::F32) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize;
  const int eb = pm.op_bytes();
  hipStream_t st = ctx->stream;
  const int cap = d.cap_heads;
  const ModelWeights& w = ctx->w;
  const int64_t srows = (int64_t)S * M;
  RC(ensure(ctx, ctx->mx[3], (size_t)srows * E * eb));        // k_norm(src) (affine folded)
  RC(ensure(ctx, ctx->mx[4], (size_t)srows * 2 * E * eb));    // K|V
  RC(ensure(ctx, ctx->mx[5], (size_t)S * cap * E * 4));       // attention out (heads concat)
  RC(ensure(ctx, ctx->mx[6], (size_t)S * cap * E * 4));       // out_proj
  RC(ensure(ctx, ctx->mx[7], (size_t)S * cap * 2 * E * 4));   // ffn hidden (+ ffn out after)
  const int64_t crow = (int64_t)S * cap;
  if (pm.is16()) {
    // 24 heads over M % 32 == 0 tokens: K [S*M][E] and V^T [S][E][M] for the MFMA attention
    const bool mf = cap == 24 && M % 32 == 0 && M <= 128;
    void* vt = (char*)ctx->mx[4].p + (size_t)srows * E * 2;
    // k_norm + K|V projection in one row pass (normalised rows stay in registers)
    HIPCHK(launch_rowgemm_ln_store(mtok, in_t, w.cap_kv.bf16.p, (const float*)w.cap_kv_b.p, ctx->mx[4].p, srows,
                                   2 * E, 1e-5f, true, st, mf ? vt : nullptr, E, M));
    // attention out in bf16, then the whole tail in one row-resident pass
    if (mf)
      HIPCHK(launch_cap_attention_mfma((const float*)w.cap_qp.p, ctx->mx[4].p, vt, ctx->mx[5].p, S, M, cap, E, st));
    else
      HIPCHK(launch_cap_attention((const float*)w.cap_qp.p, ctx->mx[4].p, DType::BF16, ctx->mx[5].p, DType::BF16, S,
                                  M, cap, E, st));
    HIPCHK(launch_cap_tail(ctx->mx[5].p, w.cap_o.bf16.p, w.cap_f0.bf16.p, w.cap_f3.bf16.p, (const float*)w.cap_vecs.p,
                           tokens, crow, E, 1e-5f, st));
    return MMPFN_OK;
  }
  // the fp32 modes: fp32 activations throughout
  const int prec = pm.base;
  HIPCHK(launch_layernorm_rows((const float*)mtok, srows, E, 1e-5f, ctx->mx[3].p, DType::F32, nullptr, nullptr, st));
  // C [rows][N] = act(A [rows][K] . W^T + bias)
  auto linear = [&](const DevBuf& A, const Weight& W, const DevBuf& bias, int64_t rows, int N, int K, int act,
                    const DevBuf& C) {
    GemmArgs g = gargs();
    g.A = A.p, g.lda = K, W.gemm_operand(g, prec), g.bias = (const float*)bias.p, g.act = act;
    g.M = (int)rows, g.N = N, g.K = K, g.C = C.p, g.ldc = N;
    return launch_gemm(g, prec, EPI_STORE, true, true, 1, st);
  };
  HIPCHK(linear(ctx->mx[3], w.cap_kv, w.cap_kv_b, srows, 2 * E, E, ACT_NONE, ctx->mx[4]));
  HIPCHK(launch_cap_attention((const float*)w.cap_qp.p, ctx->mx[4].p, DType::F32, ctx->mx[5].p, DType::F32, S, M, cap,
                              E, st));
  HIPCHK(linear(ctx->mx[5], w.cap_o, w.cap_o_b, crow, E, E, ACT_NONE, ctx->mx[6]));
  HIPCHK(linear(ctx->mx[6], w.cap_f0, w.cap_f0_b, crow, 2 * E, E, ACT_GELU, ctx->mx[7]));
  HIPCHK(linear(ctx->mx[7], w.cap_f3, w.cap_f3_b, crow, E, 2 * E, ACT_NONE, ctx->mx[5]));  // reuse mx5 for ffn out
  HIPCHK(launch_ln_add((const float*)ctx->mx[6].p, (const float*)ctx->mx[5].p, (const float*)w.cap_ng.p,
                       (const float*)w.cap_nb.p, tokens, crow, E, 1e-5f, st));
  return MMPFN_OK;
}

int mixer(mmpfn_ctx* ctx, const float* image, int S, int n_mod, float* tokens, PrecMode pm) {
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, D = d.nhid;
  if (d.mixer_type == MMPFN_MIXER_MGM) return mixer_mgm(ctx, image, S, n_mod, tokens, pm);
  if (d.mixer_type == MMPFN_MIXER_MGM_CAP) {
    const int M = d.mgm_heads * n_mod;
    RC(ensure(ctx, ctx->mx[2], (size_t)S * M * E * 4));
    const DType tok_t = mgm_operands(ctx, pm);  // 16-bit intermediate tokens in the 16-bit modes (half the HBM bytes)
    RC(mixer_mgm(ctx, image, S, n_mod, ctx->mx[2].p, pm, tok_t));
    return mixer_cap(ctx, ctx->mx[2].p, S, M, tokens, pm, tok_t);
  }
  // the MoE mixer: PREC_F16 runs the bf16 mode
  const bool b16 = pm.is16();
  const int eb = pm.op_bytes(), prec = pm.gemm();
  hipStream_t st = ctx->stream;
  if (d.mixer_type == MMPFN_MIXER_MOE) {
    const int ne = d.mgm_heads;
    const HeadBank& w = ctx->w.moe;
    RC(ensure(ctx, ctx->mx[0], (size_t)S * D * eb));
    RC(ensure(ctx, ctx->mx[1], (size_t)S * ne * (D / 2) * eb));
    RC(ensure(ctx, ctx->mx[2], (size_t)S * ne * 4));
    // modality 0 rows: image + s*n_mod*D  -> normalise with row stride n_mod*D
    // (ln kernel assumes contiguous rows; handle stride by normalising all rows when n_mod==1,
    //  else gather modality 0 first)
    const float* x0 = image;
    if (n_mod != 1) {
      RC(ensure(ctx, ctx->mx[3], (size_t)S * D * 4));
      HIPCHK(hipMemcpy2DAsync(ctx->mx[3].p, (size_t)D * 4, image, (size_t)n_mod * D * 4, (size_t)D * 4, S,
                              hipMemcpyDeviceToDevice, st));
      x0 = (const float*)ctx->mx[3].p;
    }
    HIPCHK(launch_layernorm_rows(x0, S, D, 1e-5f, ctx->mx[0].p, b16 ? DType::BF16 : DType::F32, nullptr, nullptr, st));
    GemmArgs a = gargs();
    a.A = ctx->mx[0].p, a.lda = D, w.w1.gemm_operand(a, prec), a.bias = (const float*)w.b1.p;
    a.act = ACT_GELU, a.M = S, a.N = ne * (D / 2), a.K = D, a.C = ctx->mx[1].p, a.ldc = (int64_t)ne * (D / 2);
    HIPCHK(launch_gemm(a, prec, EPI_STORE, !b16, !b16, 1, st));
    GemmArgs b = gargs();
    b.A = ctx->mx[1].p, b.lda = (int64_t)ne * (D / 2), b.a_zstride = D / 2;
    w.w2.gemm_operand(b, prec), b.w_zstride = (int64_t)E * (D / 2);
    b.bias = (const float*)w.b2.p, b.b_zstride = E;
    b.M = S, b.N = E, b.K = D / 2, b.C = tokens, b.ldc = E, b.rdiv2 = 1, b.rmul2 = ne, b.zmul = 1;
    HIPCHK(launch_gemm(b, prec, EPI_REMAP, !b16, true, ne, st));
    HIPCHK(launch_gate_softmax(x0, D, S, D, (const float*)ctx->w.moe_gw.p, (const float*)ctx->w.moe_gb.p, ne,
                               (float*)ctx->mx[2].p, st));
    HIPCHK(launch_scale_tokens(tokens, (const float*)ctx->mx[2].p, S, ne, E, st));
    return MMPFN_OK;
  }
  return fail(ctx, MMPFN_ERR_INVALID, "model has no mixer");
}

// a tap on the caller's fp32 state: PREC_F16 runs it on an fp16 copy and converts the result back
template <typename F>
int state_tap(mmpfn_ctx* ctx, float* X, int64_t n, PrecMode pm, F&& run) {
  if (!pm.f16()) return run((void*)X);
  RC(ensure(ctx, ctx->tap_x16, (size_t)n * 2));
  HIPCHK(launch_f32_to_f16(X, 0, ctx->tap_x16.p, 0, n, 1, ctx->stream));
  RC(run(ctx->tap_x16.p));
  HIPCHK(launch_f16_to_f32(ctx->tap_x16.p, 0, X, 0, n, 1, ctx->stream));
  return MMPFN_OK;
}
// the same for a tap that only reads the state: nothing is converted back, the caller's X is left alone
template <typename F>
int state_tap_ro(mmpfn_ctx* ctx, const float* X, int64_t n, PrecMode pm, F&& run) {
  if (!pm.f16()) return run((const void*)X);
  RC(ensure(ctx, ctx->tap_x16, (size_t)n * 2));
  HIPCHK(launch_f32_to_f16(X, 0, ctx->tap_x16.p, 0, n, 1, ctx->stream));
  return run((const void*)ctx->tap_x16.p);
}

}  // namespace

// ===================================================================== C ABI
extern "C" {

const char* mmpfn_version(void) { return "mmpfn-hip 0.1 (gfx950)"; }

mmpfn_ctx* mmpfn_create(int device, void* stream) {
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  mmpfn_ctx* c = new mmpfn_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  c->seen_streams.push_back(c->stream);
  return c;
}

void mmpfn_destroy(mmpfn_ctx* ctx) {
  if (!ctx) return;
  // teardown: errors here have no caller to report to
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipDeviceSynchronize();  // lanes may still be running on other streams
  for (hipEvent_t e : ctx->kt_pool) (void)hipEventDestroy(e);
  delete ctx;  // frees every device buffer the context, its layers and its lanes own
}

int mmpfn_select_lane(mmpfn_ctx* ctx, int lane) {
  if (!ctx || lane < 0 || lane >= MMPFN_MAX_LANES) return MMPFN_ERR_INVALID;
  if (lane == ctx->cur) return MMPFN_OK;
  if ((int)ctx->lanes.size() < MMPFN_MAX_LANES) ctx->lanes.resize(MMPFN_MAX_LANES);
  Lane& sel = *ctx;
  std::swap(sel, ctx->lanes[ctx->cur]);  // park the selected lane
  std::swap(sel, ctx->lanes[lane]);      // bring the requested one in
  ctx->cur = lane;
  return MMPFN_OK;
}

const char* mmpfn_last_error(const mmpfn_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int mmpfn_set_stream(mmpfn_ctx* ctx, void* stream) {
  if (!ctx) return MMPFN_ERR_INVALID;
  ctx->stream = (hipStream_t)stream;
  bool known = false;
  for (hipStream_t s : ctx->seen_streams) known |= s == ctx->stream;
  if (!known) ctx->seen_streams.push_back(ctx->stream);
  return MMPFN_OK;
}

// The engine's model contract, checked here and nowhere else: emsize E = 192 in six heads of 32, and an MLP / image
// width nhid that is a multiple of 192 -- with a mixer, of 384 (nhid / 2, the head banks' down-projection K, a
// multiple of 64) -- and for MGM+CAP a cap_heads whose head dim E / cap_heads the CAP attention is instantiated for
// (cap_head_dim_supported: every divisor of 192 but 1).  Everything behind a finalised model relies on it -- the
// row-resident kernels (featrow, rowgemm, rowgemm3, mlp_rows) and the MGM big-tile GEMMs always apply, and the dispatch below
// branches only on what still varies: the precision mode, T <= 64, mgm_heads * nhid % 256, the 16-bit decoder's
// n_out <= 16 && nhid % 128 == 0, and the CAP MFMA shape (24 heads, M % 32 == 0, M <= 128).
int mmpfn_set_model(mmpfn_ctx* ctx, const mmpfn_model_desc* desc) {
  if (!ctx || !desc) return MMPFN_ERR_INVALID;
  const mmpfn_model_desc& d = *desc;
  if (d.emsize != 192 || d.nhead * 32 != d.emsize)
    return fail(ctx, MMPFN_ERR_INVALID, "engine is specialised for emsize 192 with head dim 32");
  if (d.nhid % 192 != 0 || d.nlayers <= 0 || d.features_per_group <= 0 || d.features_per_group > 8 ||
      d.encoder_features < d.features_per_group || d.encoder_features > 8 || d.n_out <= 0)
    return fail(ctx, MMPFN_ERR_INVALID, "unsupported model geometry");
  if (d.target_kind != MMPFN_TARGET_CLASS && d.target_kind != MMPFN_TARGET_VALUE)
    return fail(ctx, MMPFN_ERR_INVALID, "target_kind " + std::to_string(d.target_kind) + ": not an MMPFN_TARGET_* code");
  // the head banks' down-projection contracts over K = nhid / 2, in 64-wide slices in the bf16 and split-bf16 GEMMs
  if (d.mixer_type != MMPFN_MIXER_NONE && (d.nhid / 2) % 64 != 0)
    return fail(ctx, MMPFN_ERR_INVALID,
                "nhid " + std::to_string(d.nhid) + ": a model with a mixer needs nhid / 2 to be a multiple of 64");
  if (d.mixer_type == MMPFN_MIXER_MGM_CAP && (d.cap_heads <= 0 || d.emsize % d.cap_heads != 0))
    return fail(ctx, MMPFN_ERR_INVALID, "cap_heads must divide emsize");
  if (d.mixer_type == MMPFN_MIXER_MGM_CAP && !cap_head_dim_supported(d.emsize / d.cap_heads))
    return fail(ctx, MMPFN_ERR_INVALID,
                "cap_heads " + std::to_string(d.cap_heads) + ": the CAP attention has no kernel for head dim " +
                    std::to_string(d.emsize / d.cap_heads));
  ctx->d = d;
  ctx->have_model = true;
  ctx->finalized = false;
  ctx->host.clear();
  return MMPFN_OK;
}

int mmpfn_load_weight(mmpfn_ctx* ctx, const char* name, const float* data, int64_t numel) {
  if (!ctx || !name || (!data && numel)) return MMPFN_ERR_INVALID;
  if (!ctx->have_model) return fail(ctx, MMPFN_ERR_STATE, "mmpfn_set_model first");
  ctx->host[name].assign(data, data + numel);
  ctx->finalized = false;
  return MMPFN_OK;
}

int mmpfn_finalize_weights(mmpfn_ctx* ctx) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (!ctx->have_model) return fail(ctx, MMPFN_ERR_STATE, "mmpfn_set_model first");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->finalized = false;  // finalize releases the previous weights before anything can fail
  int rc = finalize(ctx);
  if (rc == MMPFN_OK) {
    ctx->finalized = true;
    ctx->host.clear();
  }
  return rc;
}

int mmpfn_mixer_tokens(const mmpfn_ctx* ctx, int n_mod) {
  if (!ctx) return MMPFN_ERR_INVALID;
  switch (ctx->d.mixer_type) {
    case MMPFN_MIXER_MGM: return ctx->d.mgm_heads * n_mod;
    case MMPFN_MIXER_MGM_CAP: return ctx->d.cap_heads;
    case MMPFN_MIXER_MOE: return ctx->d.mgm_heads;
  }
  return 0;
}

int mmpfn_mixer_forward(mmpfn_ctx* ctx, const float* image, int S, int n_mod, float* tokens, int precision) {
  if (!ctx || !image || !tokens || S <= 0 || n_mod <= 0) return MMPFN_ERR_INVALID;
  if (!ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "weights not finalised");
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  HIPCHK(hipSetDevice(ctx->device));
  // (PREC_F16: the MGM head bank on fp16 operands, the pooler and MoE in the bf16 mode; the tokens enter the state
  // through the fp32 encoders)
  return mixer(ctx, image, S, n_mod, tokens, decode_prec(precision, -1));
}

int mmpfn_embed(mmpfn_ctx* ctx, const float* x, int S, int F, const float* tokens, int C, const float* y, int N,
                const float* uniq, int U, const float* pos_rand, int precision) {
  if (!ctx) return MMPFN_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  return embed(ctx, x, S, F, tokens, C, y, N, uniq, U, pos_rand, precision);
}

int mmpfn_run_layers(mmpfn_ctx* ctx, int l0, int l1) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (!ctx->embedded || !ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "mmpfn_embed first");
  if (l0 < 0 || l1 > ctx->d.nlayers || l0 > l1) return fail(ctx, MMPFN_ERR_INVALID, "bad layer range");
  HIPCHK(hipSetDevice(ctx->device));
  for (int l = l0; l < l1; ++l) RC(run_layer(ctx, l));
  return MMPFN_OK;
}

int mmpfn_decode(mmpfn_ctx* ctx, float* logits) {
  if (!ctx || !logits) return MMPFN_ERR_INVALID;
  if (!ctx->embedded || !ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "mmpfn_embed first");
  HIPCHK(hipSetDevice(ctx->device));
  return decode(ctx, logits);
}

int mmpfn_forward(mmpfn_ctx* ctx, const float* x, int S, int F, const float* tokens, int C, const float* y, int N,
                  const float* uniq, int U, const float* pos_rand, float* logits, int precision) {
  if (!ctx || !logits) return MMPFN_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  RC(embed(ctx, x, S, F, tokens, C, y, N, uniq, U, pos_rand, precision));
  RC(run_forward_layers(ctx));
  return decode(ctx, logits);
}

int mmpfn_forward_batch(mmpfn_ctx* ctx, int M, const float* const* x, int S, int F, const float* tokens, int C,
                        const float* const* y, int N, const float* const* uniq, const int* U, const float* pos_rand,
                        float* logits, int precision) {
  const bool codes = ctx && ctx->d.target_kind == MMPFN_TARGET_CLASS;  // a value target reads neither uniq nor U
  if (!ctx || !logits || M <= 0 || !y || (codes && (!uniq || !U))) return MMPFN_ERR_INVALID;
  if (F > 0 && !x) return MMPFN_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  for (int m = 0; m < M; ++m)
    RC(embed(ctx, F > 0 ? x[m] : nullptr, S, F, tokens, C, y[m], N, codes ? uniq[m] : nullptr, codes ? U[m] : 0, pos_rand,
             precision, m, M));
  RC(run_forward_layers(ctx));
  return decode(ctx, logits, M);
}

int mmpfn_forward_embed(mmpfn_ctx* ctx, const float* x, int S, int F, const float* tokens, int C, const float* y, int N,
                        const float* uniq, int U, const float* pos_rand, float* logits, float* train_emb,
                        float* test_emb, int precision) {
  if (!ctx) return MMPFN_ERR_INVALID;
  RC(check_outputs(ctx, "mmpfn_forward_embed", logits, train_emb, test_emb));
  HIPCHK(hipSetDevice(ctx->device));
  RC(embed(ctx, x, S, F, tokens, C, y, N, uniq, U, pos_rand, precision));
  return forward_outputs(ctx, logits, train_emb, test_emb, 1);
}

int mmpfn_forward_batch_embed(mmpfn_ctx* ctx, int M, const float* const* x, int S, int F, const float* tokens, int C,
                              const float* const* y, int N, const float* const* uniq, const int* U,
                              const float* pos_rand, float* logits, float* train_emb, float* test_emb, int precision) {
  const bool codes = ctx && ctx->d.target_kind == MMPFN_TARGET_CLASS;  // a value target reads neither uniq nor U
  if (!ctx || M <= 0 || !y || (codes && (!uniq || !U))) return MMPFN_ERR_INVALID;
  if (F > 0 && !x) return MMPFN_ERR_INVALID;
  RC(check_outputs(ctx, "mmpfn_forward_batch_embed", logits, train_emb, test_emb));
  HIPCHK(hipSetDevice(ctx->device));
  for (int m = 0; m < M; ++m)
    RC(embed(ctx, F > 0 ? x[m] : nullptr, S, F, tokens, C, y[m], N, codes ? uniq[m] : nullptr, codes ? U[m] : 0, pos_rand,
             precision, m, M));
  return forward_outputs(ctx, logits, train_emb, test_emb, M);
}

int mmpfn_state_tokens(const mmpfn_ctx* ctx) { return ctx ? ctx->T : 0; }

int mmpfn_copy_state(mmpfn_ctx* ctx, float* out, int64_t cap) {
  if (!ctx || !out) return MMPFN_ERR_INVALID;
  const int S = ctx->S, T = ctx->T, E = ctx->d.emsize;
  if (cap < (int64_t)S * T * E) return fail(ctx, MMPFN_ERR_INVALID, "state buffer too small");
  if (lane_prec(*ctx).f16()) {
    HIPCHK(launch_state_f16_to_f32(ctx->ws_X.p, out, S, T, E, ctx->stream));
    return MMPFN_OK;
  }
  // [T][S][E] -> [S][T][E]
  for (int t = 0; t < T; ++t)
    HIPCHK(hipMemcpy2DAsync(out + (size_t)t * E, (size_t)T * E * 4, (const float*)ctx->ws_X.p + (size_t)t * S * E,
                            (size_t)E * 4, (size_t)E * 4, S, hipMemcpyDeviceToDevice, ctx->stream));
  return MMPFN_OK;
}

int mmpfn_aggregate(mmpfn_ctx* ctx, const float* logits, int M, int Q, int n_out, const int* perms, int n_cls,
                    float temperature, int avg_before, const float* cw, float* probs) {
  if (!ctx || !logits || !probs || M <= 0 || Q < 0 || n_out <= 0 || n_cls <= 0 || n_cls > n_out)
    return MMPFN_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(launch_aggregate(logits, M, Q, n_out, perms, n_cls, temperature, avg_before, cw, probs, ctx->stream));
  return MMPFN_OK;
}

static_assert(MMPFN_BAR_MAX_BARS == kBarHeadMaxBars && MMPFN_BAR_MAX_MEMBERS == kBarHeadMaxMembers &&
                  MMPFN_BAR_MAX_LEVELS == kBarHeadMaxLevels,
              "the header's mmpfn_bar_head limits are the kernel's");

int mmpfn_bar_head(mmpfn_ctx* ctx, const float* logits, int M, int Q, int B, const unsigned char* cancel, int ldc,
                   const int* idx, const float* share, int ldt, float inv_temperature, int avg_before, const float* borders,
                   const float* bucket_means, const float* mode_means, const float* widths, const float* levels, int K,
                   float* out_logits, float* mean, float* mode, float* quantiles) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (!logits || !idx || !share || !borders || !bucket_means || !mode_means || !widths || !mean || !mode || Q < 0 ||
      K < 0 || (K > 0 && (!levels || !quantiles)) || !(inv_temperature > 0.f))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_head: null argument, negative size or temperature <= 0");
  if (ldt < B + 1 || (cancel && ldc < B))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_head: ldt < B + 1 or ldc < B");
  if (B < 1 || B > MMPFN_BAR_MAX_BARS || M < 1 || M > MMPFN_BAR_MAX_MEMBERS || K > MMPFN_BAR_MAX_LEVELS)
    return fail(ctx, MMPFN_ERR_INVALID,
                "mmpfn_bar_head: B, M or K beyond the kernel (B " + std::to_string(B) + ", M " + std::to_string(M) +
                    ", K " + std::to_string(K) + ")");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(launch_bar_head(logits, M, Q, B, cancel, ldc, idx, share, ldt, inv_temperature, avg_before, borders, bucket_means,
                         mode_means, widths, levels, K, out_logits, mean, mode, quantiles, ctx->stream));
  return MMPFN_OK;
}

static_assert(MMPFN_BAR_MAX_TARGETS == kBarScoreMaxTargets && MMPFN_BAR_SCORE_ENDS == kBarScoreEnds,
              "the header's scoring limits are the kernel's");

// what both scoring entry points refuse before a launch; null: fine
static const char* bar_score_refusal(int B, const float* log_widths, const float* mean_squares, const float* ei_mids,
                                     const float* ends, const float* ys, int J, const float* nll, const float* cdf,
                                     const float* pi, const float* ei) {
  if (!log_widths || !mean_squares || !ei_mids || !ends) return "null score table";
  if (B < 2 || B > MMPFN_BAR_MAX_BARS) return "B outside 2 .. MMPFN_BAR_MAX_BARS";
  if (J < 0 || J > MMPFN_BAR_MAX_TARGETS) return "J outside 0 .. MMPFN_BAR_MAX_TARGETS";
  if (!ys && (nll || cdf || pi || ei)) return "a per-target output without targets";
  return nullptr;
}

int mmpfn_bar_score(mmpfn_ctx* ctx, const float* logits, int Q, int B, float inv_temperature, const float* borders,
                    const float* widths, const float* log_widths, const float* mean_squares, const float* ei_mids,
                    const float* ends, const float* ys, int J, float* nll, float* cdf, float* pi, float* ei,
                    float* mean_of_square) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (!logits || !borders || !widths || Q < 0 || !(inv_temperature > 0.f))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_score: null argument, negative size or temperature <= 0");
  if (const char* why = bar_score_refusal(B, log_widths, mean_squares, ei_mids, ends, ys, J, nll, cdf, pi, ei))
    return fail(ctx, MMPFN_ERR_INVALID, std::string("mmpfn_bar_score: ") + why);
  HIPCHK(hipSetDevice(ctx->device));
  const BarScoreArgs s{borders, widths, log_widths, mean_squares, ei_mids, ends, ys, nll, cdf, pi, ei, mean_of_square, J};
  HIPCHK(launch_bar_score(logits, Q, B, inv_temperature, s, ctx->stream));
  return MMPFN_OK;
}

int mmpfn_bar_head_score(mmpfn_ctx* ctx, const float* logits, int M, int Q, int B, const unsigned char* cancel, int ldc,
                         const int* idx, const float* share, int ldt, float inv_temperature, int avg_before,
                         const float* borders, const float* bucket_means, const float* mode_means, const float* widths,
                         const float* levels, int K, float* out_logits, float* mean, float* mode, float* quantiles,
                         const float* log_widths, const float* mean_squares, const float* ei_mids, const float* ends,
                         const float* ys, int J, float* nll, float* cdf, float* pi, float* ei, float* mean_of_square) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (!logits || !idx || !share || !borders || !bucket_means || !mode_means || !widths || !mean || !mode || Q < 0 ||
      K < 0 || (K > 0 && (!levels || !quantiles)) || !(inv_temperature > 0.f))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_head_score: null argument, negative size or temperature <= 0");
  if (ldt < B + 1 || (cancel && ldc < B))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_head_score: ldt < B + 1 or ldc < B");
  if (M < 1 || M > MMPFN_BAR_MAX_MEMBERS || K > MMPFN_BAR_MAX_LEVELS)
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_head_score: M or K beyond the kernel (M " + std::to_string(M) +
                                            ", K " + std::to_string(K) + ")");
  if (const char* why = bar_score_refusal(B, log_widths, mean_squares, ei_mids, ends, ys, J, nll, cdf, pi, ei))
    return fail(ctx, MMPFN_ERR_INVALID, std::string("mmpfn_bar_head_score: ") + why);
  HIPCHK(hipSetDevice(ctx->device));
  const BarScoreArgs s{borders, widths, log_widths, mean_squares, ei_mids, ends, ys, nll, cdf, pi, ei, mean_of_square, J};
  HIPCHK(launch_bar_head(logits, M, Q, B, cancel, ldc, idx, share, ldt, inv_temperature, avg_before, borders, bucket_means,
                         mode_means, widths, levels, K, out_logits, mean, mode, quantiles, ctx->stream, &s));
  return MMPFN_OK;
}

static_assert(MMPFN_BAR_SAMPLE_CHUNK == kBarSampleChunk && MMPFN_BAR_MAX_DRAWS == kBarSampleMaxDraws,
              "the header's sampling limits are the kernel's");

int mmpfn_bar_sample(mmpfn_ctx* ctx, const float* logits, int Q, int B, float inv_temperature, const float* borders,
                     const float* ends, int tails, const float* uniforms, uint64_t seed, uint64_t first_draw, int64_t n,
                     float* out, float* u_out) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (!logits || !borders || Q < 0 || !(inv_temperature > 0.f))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_sample: null argument, negative size or temperature <= 0");
  if (B < 2 || B > MMPFN_BAR_MAX_BARS) return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_sample: B outside 2 .. MMPFN_BAR_MAX_BARS");
  if (n < 0 || n > MMPFN_BAR_MAX_DRAWS)
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_sample: n outside 0 .. MMPFN_BAR_MAX_DRAWS");
  if ((tails != 0 && tails != 1) || (tails == 1 && !ends))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_sample: tails outside 0 / 1, or half-normal tails without ends");
  if (n > 0 && !out) return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_bar_sample: draws without an output");
  if (Q == 0 || n == 0) return MMPFN_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const BarSampleArgs a{logits, borders, ends, uniforms, out, u_out, seed, first_draw, n, B, tails, inv_temperature};
  HIPCHK(launch_bar_sample(a, Q, ctx->stream));
  return MMPFN_OK;
}

// Why a program cannot be run (null: it can), and its output width and widest row.  Every index the kernel forms is
// checked here, against the host copies of the blobs, so the kernel itself never indexes past its buffers.
static const char* xform_refusal(const int32_t* ops, int n_ops, const int32_t* ints, int64_t n_ints, int64_t n_dbl,
                                 int n_in, int& n_out, int& widest) {
  if (n_ops < 0 || n_ints < 0 || n_dbl < 0 || (n_ops > 0 && !ops) || (n_ints > 0 && !ints)) return "null blob or negative size";
  if (n_in < 1 || n_in > kXformMaxWidth) return "input width outside 1 .. MMPFN_XFORM_MAX_WIDTH";
  int w = n_in;
  widest = n_in;
  for (int k = 0; k < n_ops; ++k) {
    const int32_t* op = ops + (int64_t)k * kXformOpInts;
    const int code = op[0], w_in = op[1], w_out = op[2];
    const int64_t ioff = op[3], doff = op[4];
    if (w_in != w) return "an op's input width is not its predecessor's output width";
    if (w_out < 1 || w_out > kXformMaxWidth) return "an op's output width outside 1 .. MMPFN_XFORM_MAX_WIDTH";
    if (ioff < 0 || ioff > n_ints || doff < 0 || doff > n_dbl) return "an op's blob offset out of range";
    if (code == kXformGather) {
      if (ioff + w_out > n_ints) return "gather indices past the int blob";
      for (int j = 0; j < w_out; ++j)
        if (ints[ioff + j] < 0 || ints[ioff + j] >= w_in) return "gather index outside the input row";
    } else if (code == kXformMap) {
      if (ioff + (int64_t)kXformMapInts * w_out > n_ints) return "map columns past the int blob";
      for (int j = 0; j < w_out; ++j) {
        const int32_t* c = ints + ioff + (int64_t)j * kXformMapInts;
        const int64_t off = c[2], n = c[3], aux = c[4];
        if (c[0] < 0 || c[0] >= w_in) return "map source outside the input row";
        if (c[1] == kXformPass) continue;
        if (off < 0 || n < 0) return "map parameters at a negative offset or count";
        if (c[1] == kXformLookup) {
          if (off + 2 + 2 * n > n_dbl) return "lookup table past the double blob";
        } else if (c[1] == kXformQuantile) {
          if (n < 1 || off + n > n_dbl || aux < 0 || aux + n > n_dbl) return "quantiles past the double blob";
        } else if (c[1] == kXformScale) {
          if (off + 4 > n_dbl) return "scaler parameters past the double blob";
        } else {
          return "map kind out of range";
        }
      }
    } else if (code == kXformSvd) {
      const int64_t a = op[5], b = op[6], c = op[7];
      if (a < 0 || b < 1 || c < 1 || a + b != w_in || a + c != w_out) return "svd widths do not fit the op";
      if (doff + b * c > n_dbl) return "svd components past the double blob";
    } else if (code == kXformFingerprint) {
      if (w_out != w_in + 1 || doff + 1 > n_dbl) return "fingerprint width or salt out of range";
    } else {
      return "op code out of range";
    }
    w = w_out;
    if (w > widest) widest = w;
  }
  n_out = w;
  return nullptr;
}

int mmpfn_xform_create(mmpfn_ctx* ctx, const int32_t* ops, int n_ops, const int32_t* ints, int64_t n_ints,
                       const double* doubles, int64_t n_doubles, int n_in, mmpfn_xform** out) {
  if (!ctx || !out) return MMPFN_ERR_INVALID;
  *out = nullptr;
  if (n_doubles > 0 && !doubles) return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_xform_create: null double blob");
  int n_out = 0, widest = 0;
  if (const char* why = xform_refusal(ops, n_ops, ints, n_ints, n_doubles, n_in, n_out, widest))
    return fail(ctx, MMPFN_ERR_INVALID, std::string("mmpfn_xform_create: ") + why);
  HIPCHK(hipSetDevice(ctx->device));
  mmpfn_xform* p = new mmpfn_xform;
  p->n_ops = n_ops, p->n_in = n_in, p->n_out = n_out, p->width = widest;
  const std::pair<DevBuf*, std::pair<const void*, size_t>> parts[] = {
      {&p->ops, {ops, (size_t)n_ops * kXformOpInts * 4}}, {&p->ints, {ints, (size_t)n_ints * 4}},
      {&p->dbl, {doubles, (size_t)n_doubles * 8}}};
  for (const auto& [buf, src] : parts) {
    int rc = ensure(ctx, *buf, src.second ? src.second : 8);  // an empty blob still gets an address
    if (rc == MMPFN_OK && src.second && hipMemcpy(buf->p, src.first, src.second, hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(ctx, MMPFN_ERR_HIP, "mmpfn_xform_create: upload failed");
    if (rc != MMPFN_OK) {
      delete p;
      return rc;
    }
  }
  *out = p;
  return MMPFN_OK;
}

void mmpfn_xform_free(mmpfn_ctx* ctx, mmpfn_xform* prog) {
  if (!prog) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    for (hipStream_t s : ctx->seen_streams) (void)hipStreamSynchronize(s);
  }
  delete prog;
}

int mmpfn_member_transform(mmpfn_ctx* ctx, const mmpfn_xform* prog, const void* x, int x_is_f64, int Q, int F_in,
                           int64_t ldx, float* out32, int64_t ld32, double* out64, int64_t ld64) {
  if (!ctx || !prog) return MMPFN_ERR_INVALID;
  if (Q < 0 || F_in != prog->n_in || ldx < F_in || ld32 < prog->n_out || (out64 && ld64 < prog->n_out))
    return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_member_transform: Q < 0, F_in is not the program's input width (" +
                                            std::to_string(prog->n_in) + "), or a leading dimension below its row");
  if (Q == 0) return MMPFN_OK;
  if (!x || !out32) return fail(ctx, MMPFN_ERR_INVALID, "mmpfn_member_transform: null x or out32");
  HIPCHK(hipSetDevice(ctx->device));
  RC(ensure_flag(ctx, ctx->ws_flag, ctx->stream));
  XformArgs a{};
  a.ops = (const int32_t*)prog->ops.p, a.ints = (const int32_t*)prog->ints.p, a.dbl = (const double*)prog->dbl.p;
  a.x = x, a.out32 = out32, a.out64 = out64, a.flag = (int*)ctx->ws_flag.p;
  a.ldx = ldx, a.ld32 = ld32, a.ld64 = ld64;
  a.x_f64 = x_is_f64 != 0, a.Q = Q, a.n_ops = prog->n_ops, a.n_in = prog->n_in, a.n_out = prog->n_out;
  a.width = prog->width;
  HIPCHK(launch_xform(a, ctx->stream));
  return MMPFN_OK;
}

static_assert(MMPFN_XFORM_MAX_WIDTH == kXformMaxWidth, "the header's row limit is the kernel's");

int mmpfn_status(mmpfn_ctx* ctx) {
  if (!ctx) return MMPFN_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  // wait for every stream a forward may have been queued on (lanes), not only the bound one
  for (hipStream_t s : ctx->seen_streams) HIPCHK(hipStreamSynchronize(s));
  ctx->seen_streams.assign(1, ctx->stream);
  std::vector<void*> flags{ctx->ws_flag.p};
  for (size_t i = 0; i < ctx->lanes.size(); ++i)
    if ((int)i != ctx->cur) flags.push_back(ctx->lanes[i].ws_flag.p);
  int bad = 0;
  for (void* fp : flags) {
    if (!fp) continue;
    int f = 0;
    HIPCHK(hipMemcpy(&f, fp, 4, hipMemcpyDeviceToHost));
    if (f) {
      bad |= f;
      HIPCHK(hipMemset(fp, 0, 4));  // reported once; the next forwards start clean
    }
  }
  if (bad & kXformInfFlag)  // mmpfn_member_transform met +-inf in a device X: validate_X_predict's error on the host path
    return fail(ctx, MMPFN_ERR_NAN, "Input X contains infinity or a value too large for dtype('float64').");
  if (bad) return fail(ctx, MMPFN_ERR_NAN, "There should be no NaNs in the encoded x and y (flag " + std::to_string(bad) + ")");
  return MMPFN_OK;
}

// The four item-attention taps' null and geometry check and their AttnLayerArgs: own-head rows [a0, a0 + na),
// shared-KV rows [b0, b0 + nb) against head kvb, keys [0, nk).  Hmax: the heads the entry point's kernels take.  Every
// entry point keeps its own precision rule.
static int attn_tap_args(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S, int T, int H,
                         int Hmax, int Npad, int nk, int a0, int na, int b0, int nb, int kvb, AttnLayerArgs& a) {
  if (!ctx || !q || !k || !vt || !out) return MMPFN_ERR_INVALID;
  if (a0 < 0 || na < 0 || a0 + na > S || b0 < 0 || nb < 0 || b0 + nb > S || nk <= 0 || nk > Npad || Npad % 64 ||
      H <= 0 || H > Hmax || T <= 0 || kvb >= H)
    return fail(ctx, MMPFN_ERR_INVALID, "bad attention geometry");
  HIPCHK(hipSetDevice(ctx->device));
  a = AttnLayerArgs{q, k, vt, out, S, T, H, Npad, nk};
  a.a0 = a0, a.na = na, a.b0 = b0, a.nb = nb, a.kvb = kvb;
  return MMPFN_OK;
}

int mmpfn_item_attention(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S, int T, int H,
                         int Npad, int s0, int nq, int nk, int kvh, int precision) {
  AttnLayerArgs a;
  // kvh < 0: the rows against their own heads; else every head against K/V head kvh
  if (kvh < 0) RC(attn_tap_args(ctx, q, k, vt, out, S, T, H, INT32_MAX, Npad, nk, s0, nq, 0, 0, -1, a));
  else RC(attn_tap_args(ctx, q, k, vt, out, S, T, H, INT32_MAX, Npad, nk, 0, 0, s0, nq, kvh, a));
  // this entry point runs the bf16 and the two fp32 element forms only; fp16 Q / K and the fp8 P.V variants go
  // through mmpfn_item_attention_layer_ex
  if (precision != PREC_F32 && precision != PREC_BF16 && precision != PREC_F32_MFMA)
    return fail(ctx, MMPFN_ERR_INVALID, "bad precision (PREC_F32, PREC_BF16 or PREC_F32_MFMA; 16-bit / fp8 Q.K forms: "
                                        "mmpfn_item_attention_layer_ex)");
  HIPCHK(launch_attn_layer(a, precision, ctx->stream));
  return MMPFN_OK;
}

int mmpfn_cache_build(mmpfn_ctx* ctx, const float* x, int N, int F, const float* tokens, int C, const float* y_train,
                      const float* uniq, int U, const float* pos_rand, int precision, mmpfn_cache** out) {
  if (!ctx || !out || !y_train || !pos_rand) return MMPFN_ERR_INVALID;
  if (ctx->d.target_kind == MMPFN_TARGET_VALUE) uniq = nullptr, U = 0;  // no class codes to keep
  else if (!uniq) return MMPFN_ERR_INVALID;
  *out = nullptr;
  HIPCHK(hipSetDevice(ctx->device));
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  // the cache keeps bf16 K / V^T: fp8 P.V codes build a bf16 cache
  RC(embed(ctx, x, N, F, tokens, C, y_train, N, uniq, U, pos_rand, base_prec(precision)));
  const mmpfn_model_desc& d = ctx->d;
  const int E = d.emsize, fpg = d.features_per_group, eb = lane_prec(*ctx).op_bytes();
  mmpfn_cache* cc = new mmpfn_cache;
  cc->N = N, cc->F = F, cc->G = ctx->G, cc->C = C, cc->T = ctx->T, cc->Npad = ctx->Npad, cc->prec = ctx->prec;
  cc->U = U;
  hipStream_t st = ctx->stream;
  auto build = [&]() -> int {
    RC(ensure(ctx, cc->kv, (size_t)d.nlayers * 2 * cc->T * cc->Npad * 32 * eb));
    RC(ensure(ctx, cc->slots, (size_t)(cc->G + 1) * fpg * sizeof(SlotParams)));
    RC(ensure(ctx, cc->ymean, 4));
    if (U) RC(ensure(ctx, cc->uniq, (size_t)U * 4));
    RC(ensure(ctx, cc->pe, (size_t)(cc->G + C + 1) * E * 4));
    if (cc->G)
      HIPCHK(hipMemcpyAsync(cc->slots.p, ctx->ws_slots.p, (size_t)cc->G * fpg * sizeof(SlotParams),
                            hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(cc->ymean.p, ctx->ws_scr.p, 4, hipMemcpyDeviceToDevice, st));
    if (U) HIPCHK(hipMemcpyAsync(cc->uniq.p, uniq, (size_t)U * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(cc->pe.p, ctx->ws_pe.p, (size_t)(cc->G + C) * E * 4, hipMemcpyDeviceToDevice, st));
    ctx->cache_out = cc;
    const int rc = run_forward_layers(ctx);
    ctx->cache_out = nullptr;
    return rc;
  };
  const int rc = build();
  if (rc) {
    (void)hipStreamSynchronize(st);
    delete cc;
    return rc;
  }
  *out = cc;
  return MMPFN_OK;
}

int mmpfn_cache_predict(mmpfn_ctx* ctx, const mmpfn_cache* cache, const float* x, int Q, int F, const float* tokens,
                        int C, float* logits) {
  if (!ctx || !cache || !logits) return MMPFN_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  RC(embed_cached(ctx, cache, x, Q, F, tokens, C));
  ctx->cache_in = cache;
  const int rc = run_forward_layers(ctx);
  ctx->cache_in = nullptr;
  if (rc) return rc;
  return decode(ctx, logits);
}

int mmpfn_cache_predict_embed(mmpfn_ctx* ctx, const mmpfn_cache* cache, const float* x, int Q, int F,
                              const float* tokens, int C, float* logits, float* test_emb) {
  if (!ctx || !cache) return MMPFN_ERR_INVALID;
  RC(check_outputs(ctx, "mmpfn_cache_predict_embed", logits, nullptr, test_emb));
  HIPCHK(hipSetDevice(ctx->device));
  RC(embed_cached(ctx, cache, x, Q, F, tokens, C));
  ctx->cache_in = cache;
  // every row of the state is a test row (N = 0): the pruned last layer as it is, then its rows
  const int rc = forward_outputs(ctx, logits, nullptr, test_emb, 1);
  ctx->cache_in = nullptr;
  return rc;
}

int64_t mmpfn_cache_bytes(const mmpfn_cache* cache) {
  if (!cache) return 0;
  return (int64_t)(cache->kv.bytes + cache->slots.bytes + cache->ymean.bytes + cache->uniq.bytes + cache->pe.bytes);
}

void mmpfn_cache_free(mmpfn_ctx* ctx, mmpfn_cache* cache) {
  if (!cache) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  delete cache;
}

int mmpfn_set_full_last_layer(mmpfn_ctx* ctx, int on) {
  if (!ctx) return MMPFN_ERR_INVALID;
  ctx->full_last = on != 0;
  return MMPFN_OK;
}

int mmpfn_kernel_timing(mmpfn_ctx* ctx, int enable) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (enable) ctx->kt_used = 0, ctx->kt_flops = 0.0;
  ctx->kt_on = enable != 0;
  return MMPFN_OK;
}

int mmpfn_kernel_timing_read(mmpfn_ctx* ctx, double* total_ms, int64_t* launches, double* flops) {
  if (!ctx || !total_ms || !launches || !flops) return MMPFN_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  double tot = 0.0;
  for (size_t i = 0; i + 1 < ctx->kt_used; i += 2) {
    HIPCHK(hipEventSynchronize(ctx->kt_pool[i + 1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->kt_pool[i], ctx->kt_pool[i + 1]));
    tot += ms;
  }
  *total_ms = tot, *launches = (int64_t)(ctx->kt_used / 2), *flops = ctx->kt_flops;
  return MMPFN_OK;
}

int mmpfn_item_attention_layer(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S, int T,
                               int H, int Npad, int N) {
  AttnLayerArgs a;
  RC(attn_tap_args(ctx, q, k, vt, out, S, T, H, 8, Npad, N, 0, N, N, S - N, 0, a));
  HIPCHK(launch_attn_layer(a, PREC_BF16, ctx->stream));
  return MMPFN_OK;
}

int mmpfn_item_attention_layer_ex(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S,
                                  int T, int H, int Npad, int N, int precision) {
  AttnLayerArgs a;
  RC(attn_tap_args(ctx, q, k, vt, out, S, T, H, 8, Npad, N, 0, N, N, S - N, 0, a));
  const bool qkb = (precision & MMPFN_ATTN_QK_BF16) != 0;  // the fp16 forward's form: bf16 q / k, fp16 out
  precision &= ~MMPFN_ATTN_QK_BF16;
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  const PrecMode pm = decode_prec(precision, -1);  // the caller's operand types, whatever the table's width
  if (!pm.is16() || (qkb && !pm.f16())) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  if (pm.f8) {
    const int64_t n = (int64_t)T * H * 32 * Npad;
    RC(ensure(ctx, ctx->tap_v8, (size_t)n));
    HIPCHK(launch_vt_fp8(vt, ctx->tap_v8.p, n, ctx->stream));
    a.vt8 = ctx->tap_v8.p, a.f8 = pm.f8;
  }
  a.qk_t = pm.f16() && !qkb ? DType::F16 : DType::BF16, a.o_t = pm.attn_out();
  HIPCHK(launch_attn_layer(a, pm.base, ctx->stream));
  return MMPFN_OK;
}

int mmpfn_item_attention_cached(mmpfn_ctx* ctx, const void* q, const void* k0, const void* vt0, void* out, int S,
                                int T, int H, int Npad, int N) {
  AttnLayerArgs a;
  // every row against head 0 of the cache layout
  RC(attn_tap_args(ctx, q, k0, vt0, out, S, T, H, 8, Npad, N, 0, 0, 0, S, 0, a));
  if (S <= 0) return fail(ctx, MMPFN_ERR_INVALID, "bad attention geometry");
  a.kv_bstride = (int64_t)Npad * 32;
  HIPCHK(launch_attn_layer(a, PREC_BF16, ctx->stream));
  return MMPFN_OK;
}

int mmpfn_item_attention_forward(mmpfn_ctx* ctx, const void* q, const void* k, const void* vt, void* out, int S,
                                 int T, int H, int Npad, int N, int form, int precision) {
  if (!ctx) return MMPFN_ERR_INVALID;
  if (form < ITEM_ATTN_FULL || form > ITEM_ATTN_CACHED) return fail(ctx, MMPFN_ERR_INVALID, "bad attention form");
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  PrecMode pm = decode_prec(precision, T);
  if (form == ITEM_ATTN_CACHED) pm.f8 = 0;  // the cache keeps bf16 V^T: its test rows run the bf16 P.V (embed_cached)
  const AttnLayerArgs f = item_attn_args((ItemAttnForm)form, S, N, T, H, Npad, pm);
  AttnLayerArgs a;
  // the taps' geometry rules on the forwards' row sets (T <= 0, N <= 0, N > S -- a negative test-row count --, N > Npad)
  RC(attn_tap_args(ctx, q, k, vt, out, S, T, H, 8, Npad, N, f.a0, f.na, f.b0, f.nb, f.kvb, a));
  if (form == ITEM_ATTN_LAST && N == S)  // (the forwards launch nothing then: a cache build reads no last-layer output)
    return fail(ctx, MMPFN_ERR_INVALID, "the last layer's form needs test rows");
  if (f.na + f.nb <= 0) return fail(ctx, MMPFN_ERR_INVALID, "bad attention geometry");  // (S <= 0 in the cached form)
  a.kv_bstride = f.kv_bstride, a.q_prescaled = f.q_prescaled, a.o_t = f.o_t;
  if (pm.is16() && pm.f8) {  // as item_sublayer: e4m3 V^T beside the bf16 one
    const int64_t n = (int64_t)T * H * 32 * Npad;
    RC(ensure(ctx, ctx->tap_v8, (size_t)n));
    HIPCHK(launch_vt_fp8(vt, ctx->tap_v8.p, n, ctx->stream));
    a.vt8 = ctx->tap_v8.p, a.f8 = pm.f8;
  }
  HIPCHK(launch_attn_layer(a, pm.base, ctx->stream));
  return MMPFN_OK;
}

// ---- per-sublayer taps ------------------------------------------------------------
static int tap_check(mmpfn_ctx* ctx, int layer, const void* X, int precision) {
  if (!ctx || !X) return MMPFN_ERR_INVALID;
  if (!ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "weights not finalised");
  if (layer < 0 || layer >= ctx->d.nlayers) return fail(ctx, MMPFN_ERR_INVALID, "bad layer index");
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  HIPCHK(hipSetDevice(ctx->device));
  return MMPFN_OK;
}

int mmpfn_feature_attention_ex(mmpfn_ctx* ctx, int layer, float* X, int S, int T, int M, int last, int precision) {
  RC(tap_check(ctx, layer, X, precision));
  if (S <= 0 || T <= 0) return fail(ctx, MMPFN_ERR_INVALID, "bad state geometry");
  if (M <= 0) return fail(ctx, MMPFN_ERR_INVALID, "bad member count");
  RC(lane_workspace(ctx, S, T, 64, M, false));  // (a tap runs on the caller's state)
  const PrecMode pm = decode_prec(precision, T);
  return state_tap(ctx, X, (int64_t)M * S * T * ctx->d.emsize, pm, [&](void* Xs) {
    return feat_sublayer(ctx, ctx->w.layers[layer], Xs, S, T, M, pm, last != 0);
  });
}

int mmpfn_feature_attention(mmpfn_ctx* ctx, int layer, float* X, int S, int T, int precision) {
  return mmpfn_feature_attention_ex(ctx, layer, X, S, T, 1, 0, precision);
}

int mmpfn_item_attention_block(mmpfn_ctx* ctx, int layer, float* X, int S, int T, int N, int precision) {
  RC(tap_check(ctx, layer, X, precision));
  if (S <= 0 || T <= 0 || N <= 0 || N > S) return fail(ctx, MMPFN_ERR_INVALID, "bad state geometry");
  const int Npad = (N + 63) / 64 * 64;
  RC(lane_workspace(ctx, S, T, Npad, 1, false));
  const PrecMode pm = decode_prec(precision, T);
  return state_tap(ctx, X, (int64_t)S * T * ctx->d.emsize, pm, [&](void* Xs) {
    return item_sublayer(ctx, layer, Xs, S, T, N, Npad, 1, pm, false);
  });
}

int mmpfn_item_qkv(mmpfn_ctx* ctx, int layer, const float* X, int S, int T, int N, int M, int last, int precision,
                   void* q, void* k, void* vt) {
  RC(tap_check(ctx, layer, X, precision));
  if (S <= 0 || T <= 0 || N < 0 || N > S) return fail(ctx, MMPFN_ERR_INVALID, "bad state geometry");
  if (M <= 0) return fail(ctx, MMPFN_ERR_INVALID, "bad member count");
  if (!q || (N > 0 && (!k || !vt))) return fail(ctx, MMPFN_ERR_INVALID, "null projection output");
  const int Npad = (N + 63) / 64 * 64;
  const PrecMode pm = decode_prec(precision, T);
  return state_tap_ro(ctx, X, (int64_t)M * S * T * ctx->d.emsize, pm, [&](const void* Xs) {
    return item_project(ctx, layer, Xs, S, T, N, Npad, M, pm, last != 0, N == 0, q, k, vt);
  });
}

int mmpfn_mlp_ln(mmpfn_ctx* ctx, int layer, float* X, int64_t rows, int precision) {
  RC(tap_check(ctx, layer, X, precision));
  if (rows <= 0) return fail(ctx, MMPFN_ERR_INVALID, "bad row count");
  const PrecMode pm = decode_prec(precision, -1);  // row-wise: no token limit
  return state_tap(ctx, X, rows * ctx->d.emsize, pm, [&](void* Xs) {
    return mlp_sublayer(ctx, ctx->w.layers[layer], Xs, rows, pm, nullptr);
  });
}

int mmpfn_outproj_mlp_ln(mmpfn_ctx* ctx, int layer, float* X, const void* O, int64_t rows, int precision) {
  RC(tap_check(ctx, layer, X, precision));
  if (rows <= 0) return fail(ctx, MMPFN_ERR_INVALID, "bad row count");
  if (!O) return fail(ctx, MMPFN_ERR_INVALID, "null attention output");
  const PrecMode pm = decode_prec(precision, -1);  // row-wise: no token limit
  return state_tap(ctx, X, rows * ctx->d.emsize, pm, [&](void* Xs) {
    return layer_tail(ctx, ctx->w.layers[layer], Xs, O, rows, pm);
  });
}

int mmpfn_mgm(mmpfn_ctx* ctx, const float* image, int S, int n_mod, float* tokens, int precision) {
  if (!ctx || !image || !tokens || S <= 0 || n_mod <= 0) return MMPFN_ERR_INVALID;
  if (!ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "weights not finalised");
  if (ctx->d.mixer_type != MMPFN_MIXER_MGM && ctx->d.mixer_type != MMPFN_MIXER_MGM_CAP)
    return fail(ctx, MMPFN_ERR_INVALID, "model has no MGM head bank");
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  HIPCHK(hipSetDevice(ctx->device));
  return mixer_mgm(ctx, image, S, n_mod, tokens, decode_prec(precision, -1));
}

int mmpfn_cap(mmpfn_ctx* ctx, const float* mgm_tokens, int S, int M, float* tokens, int precision) {
  if (!ctx || !mgm_tokens || !tokens || S <= 0 || M <= 0) return MMPFN_ERR_INVALID;
  if (!ctx->finalized) return fail(ctx, MMPFN_ERR_STATE, "weights not finalised");
  if (ctx->d.mixer_type != MMPFN_MIXER_MGM_CAP) return fail(ctx, MMPFN_ERR_INVALID, "model has no CAP");
  if (!prec_ok(precision)) return fail(ctx, MMPFN_ERR_INVALID, "bad precision");
  HIPCHK(hipSetDevice(ctx->device));
  return mixer_cap(ctx, mgm_tokens, S, M, tokens, decode_prec(precision, -1));
}

}  // extern "C"
