"""GPU: every per-sublayer C-ABI tap (include/mmpfn_hip.h) against the oracle's matching function.

Inputs are the oracle's own intermediate states of a golden case (so each tap is checked in
isolation), plus config-C-sized states for the kernels' production shapes.  Tolerances:
fp32 parity mode (prec 0: split-bf16 three-product MFMAs) <= 5e-5 relative to max(1, max|ref|) per
sublayer (the oracle runs fp64); fp32-input MFMA mode (prec 2) <= 2e-5; bf16 mode <= 2e-2 (bf16
operands, fp32 accumulation / LayerNorm); fp16 mode (prec 5: fp16 state and operands, the item
attention's P.V on bf16) <= 1e-2.

Which kernels a layer tap runs.  In the fp32 modes (0, 2) every tap runs the forwards' kernels.  In the 16-bit modes
(1, 5) the forwards fuse the item attention's out-projection + LayerNorm into the MLP kernel as its prologue
(``mlp_rows_kernel<2, RES = true>``), so of the three taps here
  ``mmpfn_feature_attention``     runs the forwards' ``feat_rows_kernel`` (T <= 64);
  ``mmpfn_item_attention_block``  runs the forwards' q|k|v projection and attention, but its out-projection on
                                  ``launch_rowgemm_resln``, which no 16-bit forward launches;
  ``mmpfn_mlp_ln``                runs ``mlp_rows_kernel<2, RES = false>``, which no 16-bit forward launches either.
The forwards' own kernel is behind a fourth tap, ``mmpfn_outproj_mlp_ln``, tested alone in
tests/test_layer_tail_gpu.py.
"""

import pytest
import torch

from helpers import load_case, oracle_spec, rel_err, torch_sd
from oracle.forward import embed_inputs, feat_sublayer, item_sublayer, mlp_sublayer, oracle_cap, oracle_mgm

pytestmark = pytest.mark.gpu

TOL = {0: 5e-5, 1: 2e-2, 2: 2e-5, 5: 1e-2}


def _engine(cfg, sd):
    from multimodalpfn_amd.model.transformer import PerFeatureTransformer

    model = PerFeatureTransformer(cfg)
    model.load_state_dict(torch_sd(sd))
    norm = next(e for e in model.encoder if "InputNormalizationEncoderStep" in str(e.__class__))
    norm.remove_outliers, norm.remove_outliers_sigma = True, cfg.remove_outliers_sigma or 12.0
    return model.to("cuda").engine()


def _golden_states(case):
    z, meta, cfg, sd = load_case(case)
    spec, w = oracle_spec(cfg), torch_sd(sd)
    x = torch.from_numpy(z["x"]) if "x" in z else None
    im = torch.from_numpy(z["image"]) if "image" in z else None
    y = torch.from_numpy(z["y_train"])
    X0 = embed_inputs(spec, w, x, im, y, dtype=torch.float64)
    return cfg, sd, spec, {k: v.double() for k, v in w.items()}, X0, len(y), im


@pytest.mark.parametrize("prec", [0, 1, 2, 5])
@pytest.mark.parametrize("case", ["mgmcap_edge", "pad_ufes_12l", "two_queries"])
def test_layer_sublayer_taps_match_oracle(case, prec):
    cfg, sd, spec, w, X0, N, _ = _golden_states(case)
    eng = _engine(cfg, sd)
    for l in {0, cfg.nlayers - 1}:
        Xf = feat_sublayer(spec, w, l, X0)
        got = eng.feature_attention(l, X0.float(), prec).cpu()
        print(f"{case} layer {l} prec {prec}: feature {rel_err(got.numpy(), Xf.numpy()):.2e}")
        assert rel_err(got.numpy(), Xf.numpy()) <= TOL[prec], ("feature", l)
        Xi = item_sublayer(spec, w, l, Xf, N)
        got = eng.item_attention_block(l, Xf.float(), N, prec).cpu()
        print(f"{case} layer {l} prec {prec}: item {rel_err(got.numpy(), Xi.numpy()):.2e}")
        assert rel_err(got.numpy(), Xi.numpy()) <= TOL[prec], ("item", l)
        Xm = mlp_sublayer(spec, w, l, Xi)
        got = eng.mlp_ln(l, Xi.float(), prec).cpu()
        print(f"{case} layer {l} prec {prec}: mlp {rel_err(got.numpy(), Xm.numpy()):.2e}")
        assert rel_err(got.numpy(), Xm.numpy()) <= TOL[prec], ("mlp", l)
        X0 = Xm


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("case", ["mgmcap_edge", "mgm_two_mod"])
def test_mixer_taps_match_oracle(case, prec):
    z, meta, cfg, sd = load_case(case)
    spec, w = oracle_spec(cfg), {k: v.double() for k, v in torch_sd(sd).items()}
    eng = _engine(cfg, sd)
    im = torch.from_numpy(z["image"])
    ref = oracle_mgm(spec, w, im.double())
    got = eng.mgm(im, prec).cpu()
    assert got.shape == ref.shape
    assert rel_err(got.numpy(), ref.numpy()) <= 10 * TOL[prec]
    if cfg.mixer_type == "MGM+CAP":
        ref_c = oracle_cap(spec, w, ref)
        got_c = eng.cap(ref.float(), prec).cpu()
        assert got_c.shape == ref_c.shape
        assert rel_err(got_c.numpy(), ref_c.numpy()) <= 10 * TOL[prec]


@pytest.mark.parametrize("prec", [0, 1, 2, 5])
def test_taps_at_config_c_shape(prec):
    """Production shape (S = 2298, N = 1838, T = 36) of each layer tap against the oracle evaluated
    in fp32 on the same GPU (random O(1) state, layer 0 weights of the config-C model)."""
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    torch.backends.cuda.matmul.allow_tf32 = False
    cfg = ModelConfig(nlayers=1, mgm_heads=8, cap_heads=4)
    sd = synth_state_dict(state_dict_spec(cfg), 2)
    eng = _engine(cfg, sd)
    spec, w = oracle_spec(cfg), {k: v.cuda() for k, v in torch_sd(sd).items()}
    g = torch.Generator(device="cpu").manual_seed(3)
    X = torch.randn(2298, 36, 192, generator=g).cuda()
    N = 1838
    with torch.inference_mode():
        for name, ref, got in [
            ("feature", feat_sublayer(spec, w, 0, X), eng.feature_attention(0, X, prec)),
            ("item", item_sublayer(spec, w, 0, X, N), eng.item_attention_block(0, X, N, prec)),
            ("mlp", mlp_sublayer(spec, w, 0, X), eng.mlp_ln(0, X, prec)),
        ]:
            err = rel_err(got.cpu().numpy(), ref.cpu().numpy())
            print(f"{name} prec {prec}: rel err {err:.2e}")
            assert err <= (TOL[prec] if prec in (1, 5) else 1e-4), (name, err)


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("n_mod,S", [(1, 301), (2, 97), (1, 1)])
def test_mixer_taps_at_config_c_shape(n_mod, S, prec):
    """MGM 64 + CAP 24 (the config C / D mixer: M = 64 / 128 MGM tokens per row) against the oracle in fp32 on
    the GPU.  In the bf16 mode this shape takes the MFMA CAP attention (K and V^T from the projection, one wave
    per row, S % 4 != 0 leaves a block's waves idle) and the row-resident CAP tail (mlp_rows CAP form)."""
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    torch.backends.cuda.matmul.allow_tf32 = False
    cfg = ModelConfig(nlayers=1, mgm_heads=64, cap_heads=24)
    sd = synth_state_dict(state_dict_spec(cfg), 4)
    eng = _engine(cfg, sd)
    spec, w = oracle_spec(cfg), {k: v.cuda() for k, v in torch_sd(sd).items()}
    g = torch.Generator(device="cpu").manual_seed(5 + n_mod)
    im = torch.randn(S, n_mod, 768, generator=g).cuda()
    with torch.inference_mode():
        ref = oracle_mgm(spec, w, im)
        got = eng.mgm(im, prec)
        err = rel_err(got.cpu().numpy(), ref.cpu().numpy())
        print(f"mgm n_mod {n_mod} prec {prec}: rel err {err:.2e}")
        assert err <= (TOL[prec] if prec == 1 else 1e-4), err
        ref_c = oracle_cap(spec, w, ref)
        got_c = eng.cap(ref, prec)
        assert got_c.shape == ref_c.shape and torch.isfinite(got_c).all()
        err = rel_err(got_c.cpu().numpy(), ref_c.cpu().numpy())
        print(f"cap n_mod {n_mod} prec {prec}: rel err {err:.2e}")
        assert err <= (TOL[prec] if prec == 1 else 1e-4), err


@pytest.mark.parametrize("prec", [1, 0, 5])
@pytest.mark.parametrize("S,T", [(1, 1), (5, 16), (130, 17), (7, 33), (66, 48), (3, 49), (129, 64), (9, 65)])
def test_taps_ragged_shapes(S, T, prec):
    """Shape edges of the layer kernels against the oracle (fp32 on the same GPU): token counts at and
    past each 16-token tile of the feature block (T = 1 .. 64; T = 65 takes the general feature kernel),
    row counts that leave a block's waves partly empty (S = 1, 3, 5, 7, 9, 66, 129, 130), one train row."""
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    torch.backends.cuda.matmul.allow_tf32 = False
    cfg = ModelConfig(nlayers=1, mgm_heads=8, cap_heads=4)
    sd = synth_state_dict(state_dict_spec(cfg), 3)
    eng = _engine(cfg, sd)
    spec, w = oracle_spec(cfg), {k: v.cuda() for k, v in torch_sd(sd).items()}
    g = torch.Generator(device="cpu").manual_seed(S * 131 + T)
    X = torch.randn(S, T, 192, generator=g).cuda()
    X0 = X.clone()
    N = max(1, (2 * S) // 3)
    with torch.inference_mode():
        for name, ref, got in [
            ("feature", feat_sublayer(spec, w, 0, X), eng.feature_attention(0, X, prec)),
            ("item", item_sublayer(spec, w, 0, X, N), eng.item_attention_block(0, X, N, prec)),
            ("mlp", mlp_sublayer(spec, w, 0, X), eng.mlp_ln(0, X, prec)),
        ]:
            assert got.shape == ref.shape, name
            assert torch.isfinite(got).all(), name
            err = rel_err(got.cpu().numpy(), ref.cpu().numpy())
            print(f"S={S} T={T} {name} prec {prec}: rel err {err:.2e}")
            assert err <= (TOL[prec] if prec in (1, 5) else 1e-4), (name, err)
    assert torch.equal(X, X0)  # the taps work on a copy (S = 1 or T = 1 once aliased the caller's state)
