"""GPU: the regression path below and above the bar head (``test_regression_head_gpu`` has the head alone).

1. the label token of a value target (``assemble_kernel`` with ``target_kind`` 1) against the restatement;
2. the wide decoder alone (``decoder_wide.hip``), from a read-back state, against its own arithmetic in fp64;
3. the model-level fixtures in the four base modes; cached predict and batched members against single forwards;
4. ``MMPFNRegressor`` end to end on the API fixtures.
"""

import math

import numpy as np
import pytest
import torch

import regression_oracle as ro
from helpers import oracle_spec, rel_err, report, torch_sd
from test_encoder_gpu import _gelu64
from test_regression_head import PROB_FLOOR
from test_regression_host import API_NAMES, MODEL_NAMES, api_case, model_case, write_ckpt

from multimodalpfn_amd import MMPFNRegressor
from multimodalpfn_amd.model.spec import ModelConfig

pytestmark = pytest.mark.gpu

EMBED_TOL = 1e-5  # test_encoder_gpu.EMBED_TOL
DEC32_TOL = 2e-5  # the project's fp32 decoder bound (test_encoder_gpu.DEC32_TOL)
GOLDEN_BAND = {0: 1e-4, 2: 1e-4, 1: 2e-2, 5: 1e-2}  # logits vs the reference, of max(1, max|ref|), per base mode
_ENGINES: dict = {}


def _engine(cfg, sd, key):
    from multimodalpfn_amd.engine import HipEngine

    if key not in _ENGINES:
        _ENGINES[key] = HipEngine(cfg, sd, torch.device("cuda"))
    return _ENGINES[key]


def _model_setup(name):
    case, z, cfg, sd, d = model_case(name)
    eng = _engine(cfg, sd, ("model", name))
    x = None if d["x"] is None else torch.from_numpy(d["x"]).cuda()
    img = None if d["image"] is None else torch.from_numpy(d["image"]).cuda()
    return case, z, cfg, sd, d, eng, x, img


# ------------------------------------------------------------------------------------------------ 1. label token


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_value_target_embedding_matches_restatement(name):
    """``embed_state`` of a value-target model against ``embed_inputs_value`` (the engine's own mixer tokens, so
    the encoders are what is compared): fp32 state rel_err <= 1e-5; fp16 state per element
    ``|got - ref| <= 2^-11 |ref| + 1e-5 max(1, max|ref|)``.  The label token is also the reference's recorded one."""
    case, z, cfg, sd, d, eng, x, img = _model_setup(name)
    with torch.inference_mode():
        tok = None if img is None else eng.mixer_tokens(img, 0)
        X0 = eng.embed_state(x, tok, d["y_train"], 0).cpu().numpy()
        X5 = eng.embed_state(x, tok, d["y_train"], 5).cpu().numpy()
        eng.status()
    ref = ro.embed_inputs_value(oracle_spec(cfg), torch_sd(sd), None if x is None else x.cpu(),
                                None if img is None else img.cpu(), torch.from_numpy(d["y_train"]),
                                mixer_tokens=None if tok is None else tok.cpu()).double().numpy()
    e0 = rel_err(X0, ref)
    d5 = np.abs(X5.astype(np.float64) - ref)
    lim5 = 2.0 ** -11 * np.abs(ref) + EMBED_TOL * max(1.0, np.abs(ref).max())
    ey = rel_err(X0[:, -1], z["y_token"])
    report(f"value-target embedding {name}: fp32 rel err {e0:.2e}, label token vs reference {ey:.2e}; fp16 worst "
           f"|d| / bound {float((d5 / lim5).max()):.3f}")
    assert X0.shape == ref.shape == X5.shape
    assert e0 <= EMBED_TOL and ey <= EMBED_TOL
    assert np.isfinite(X5).all() and (d5 <= lim5).all()
    # the label column differs between rows (a class-code embedding of these targets would not follow the values)
    assert len(np.unique(X0[:case["N"], -1, 0])) > case["N"] // 2


# ------------------------------------------------------------------------------------------------ 2. wide decoder

WIDE_Q = (1, 17, 33)
WIDE_OUT = (17, 100, 257, 5000)
WIDE_N, WIDE_WSEED = 24, 51
# worst rel_err of the 16-bit forms against their own arithmetic in fp64, over WIDE_Q x WIDE_OUT, measured on an
# MI355X; the bound is 4 x that, as for dec_mfma_kernel
WIDE16_MEASURED = {1: 3.365e-5, 5: 9.491e-5}


def _wide_ref(h, sd, op=None):
    """``GELU(h W1^T + b1) W2^T + b2`` in fp64; ``op``: the kernel's own arithmetic -- h, W1, W2 rounded to the
    operand type, exact sums, exact-erf GELU, the hidden activations rounded to the operand type."""
    q = (lambda t: t.to(op).double()) if op is not None else (lambda t: t.double())
    w = {k: torch.from_numpy(sd["decoder_dict.standard." + k]) for k in ("0.weight", "0.bias", "2.weight", "2.bias")}
    G = _gelu64(q(h) @ q(w["0.weight"]).T + w["0.bias"].double())
    if op is not None:
        G = G.float().to(op).double()
    return G @ q(w["2.weight"]).T + w["2.bias"].double()


def _wide_state(n_out, Q, prec):
    """A value-target model with ``n_out`` bars, a small table through its one layer, the decoder's input rows read
    back (in precision 5 exactly the fp16 state); nothing runs between the read-back and ``decode``."""
    from synth import synth_table

    cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2, max_num_classes=0, num_buckets=n_out,
                      remove_outliers_sigma=None)
    sd = ro.reg_state_dict(cfg, WIDE_WSEED)
    eng = _engine(cfg, sd, ("wide", n_out))
    S = WIDE_N + Q
    x = torch.from_numpy(synth_table(S, 3, 400 + Q)).cuda()
    y = np.random.default_rng(400 + Q).standard_normal(WIDE_N).astype(np.float32)
    eng.embed_state(x, None, y, prec)
    X = eng.run_layers(0, 1)
    eng.status()
    h = X[WIDE_N:, -1].cpu()
    assert h.shape == (Q, cfg.emsize) and torch.isfinite(h).all() and len(torch.unique(h, dim=0)) == Q
    return cfg, sd, eng, h


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("n_out", WIDE_OUT)
def test_wide_decoder_fp32_in_isolation(n_out, prec):
    """Both fp32 modes run the wide decoder on fp32-input MFMA: rel_err <= 2e-5 against fp64, Q around the 16- and
    32-row tiles, n_out below, across and far beyond the 64-column block tile."""
    worst = 0.0
    with torch.inference_mode():
        for Q in WIDE_Q:
            cfg, sd, eng, h = _wide_state(n_out, Q, prec)
            got = eng.decode(Q).cpu()
            ref = _wide_ref(h, sd)
            assert got.shape == (Q, n_out) == ref.shape and torch.isfinite(got).all()
            err = rel_err(got.numpy(), ref.numpy())
            worst = max(worst, err)
            assert err <= DEC32_TOL, (Q, err)
    report(f"wide decoder fp32 prec {prec} n_out {n_out}: worst rel err vs fp64 {worst:.2e}")


@pytest.mark.parametrize("prec", [1, 5])
@pytest.mark.parametrize("n_out", WIDE_OUT)
def test_wide_decoder_16bit_against_quantising_reference(n_out, prec):
    """The bf16 / fp16 forms against the same arithmetic in fp64 (``_wide_ref`` with ``op``).  What is left between
    the two is the fp32 accumulation of the MFMAs, the fp32 GELU and the hidden values whose rounding to the operand
    type the two sides decide differently.  Measured on an MI355X, the maximum of rel_err over Q per n_out = 17 /
    100 / 257 / 5000: bf16 3.37e-5 / 2.75e-5 / 2.75e-5 / 2.38e-5, fp16 6.23e-5 / 7.52e-5 / 9.49e-5 / 9.28e-5
    (``WIDE16_MEASURED`` holds the maximum per precision); the bound is 4 x that, 1.35e-4 (bf16) and 3.80e-4 (fp16)."""
    op = torch.bfloat16 if prec == 1 else torch.float16
    worst = 0.0
    with torch.inference_mode():
        for Q in WIDE_Q:
            cfg, sd, eng, h = _wide_state(n_out, Q, prec)
            if prec == 5:
                assert torch.equal(h, h.half().float())
            got = eng.decode(Q).cpu()
            ref = _wide_ref(h, sd, op)
            assert got.shape == (Q, n_out) == ref.shape and torch.isfinite(got).all()
            err = rel_err(got.numpy(), ref.numpy())
            print(f"wide decoder prec {prec} n_out {n_out} Q {Q}: rel err {err:.3e}")
            worst = max(worst, err)
    report(f"wide decoder 16-bit prec {prec} n_out {n_out}: worst rel err vs quantising fp64 {worst:.3e}")
    assert worst <= 4 * WIDE16_MEASURED[prec], (worst, WIDE16_MEASURED[prec])


# ------------------------------------------------------------------------------------------------ 3. model level


@pytest.mark.parametrize("prec", [0, 2, 1, 5])
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_logits_match_reference(name, prec):
    """The reference model's logits ``[Q, B]`` in every base mode, within the project's golden bands."""
    case, z, cfg, sd, d, eng, x, img = _model_setup(name)
    with torch.inference_mode():
        tok = None if img is None else eng.mixer_tokens(img, prec)
        out = eng.forward(x, tok, d["y_train"], prec).cpu().numpy()
    err = rel_err(out, z["logits"])
    report(f"regression model {name} prec {prec}: logits rel err {err:.2e} (band {GOLDEN_BAND[prec]:.0e})")
    assert out.shape == z["logits"].shape and np.isfinite(out).all()
    assert err <= GOLDEN_BAND[prec]


@pytest.mark.parametrize("prec", [0, 5])
def test_cached_predict_and_batched_members_equal_single_forwards(prec):
    """``n_out = 5000``: ``cache_build`` + ``cache_predict`` give the full forward's logits bitwise, and a two-member
    ``forward_many`` (batched, and over two lanes) gives each member's single forward bitwise."""
    case, z, cfg, sd, d, eng, x, img = _model_setup("reg_img_b5000")
    N = case["N"]
    y = d["y_train"]
    with torch.inference_mode():
        tok = eng.mixer_tokens(img, prec)
        full = eng.forward(x, tok, y, prec)
        cache = eng.cache_build(x[:N], tok[:N], y, prec)
        got = eng.cache_predict(cache, x[N:], tok[N:])
        eng.status()
        cache.free()
        items = [(x, tok, y), (torch.roll(x, 1, dims=1), tok, (-y).copy())]
        singles = [eng.forward(*it, prec) for it in items]
        batched = eng.forward_many(items, prec, lanes=1, batch=2)
        laned = eng.forward_many(items, prec, lanes=2, batch=1)
        eng.status()
    assert torch.isfinite(full).all() and full.shape == (case["S"] - N, 5000)
    assert torch.equal(got, full)
    assert torch.equal(singles[0], full) and not torch.equal(singles[1], full)
    for k in range(2):
        assert torch.equal(batched[k], singles[k]) and torch.equal(laned[k], singles[k]), k


# ------------------------------------------------------------------------------------------------ 4. end to end


def _fit(case, tmp_path, variant, **over):
    d = ro.api_case_data(case)
    path, _, _ = write_ckpt(case, tmp_path)
    kw = ro.api_regressor_kwargs(case, variant) | over
    reg = MMPFNRegressor(model_path=str(path), **kw)
    reg.fit(d["X_train"], None, d["y_train"])
    return reg, d


def _head64(z, logits, avg, levels):
    masks = [z[f"m{m}_cancel"] if z[f"m{m}_cancel"].any() else None for m in range(4)]
    return ro.head(logits, [z[f"m{m}_borders"].astype(np.float32) for m in range(4)], z["std_borders"], masks,
                   temperature=0.9, average_before_softmax=avg, crit_borders=z["crit_borders"], levels=levels,
                   dtype=torch.float64)


@pytest.mark.parametrize("name", API_NAMES)
def test_regressor_end_to_end_fp32(name, tmp_path):
    """``MMPFNRegressor`` in fp32 on the API fixtures.  Per-member logits within 1e-4 of the reference (of max(1,
    max|ref|)).  Final mean / median / quantiles against the float64 head of the reference members' logits, the mean
    as a fraction of the span of the criterion's inner borders, the quantiles in probability space: the logit
    band is propagated through that head -- each member's reference logits perturbed by +-1e-4 max(1, max|ref|)
    under random sign patterns, the largest change of each output taken -- and the bound is 2 x that change plus
    the head's own bound (``test_regression_head_gpu``: max(2 d_ref, 64 x 2^-24)).  ``full`` returns the reference's
    keys and shapes."""
    case, z = api_case(name)
    levels = ro.API_QUANTILES
    span = float(z["crit_borders"][-2] - z["crit_borders"][1])
    ref_logits = [torch.from_numpy(z[f"m{m}_logits"]) for m in range(4)]
    for variant in case["variants"]:
        tag, avg = variant["tag"], variant["average_before_softmax"]
        reg, d = _fit(case, tmp_path, variant)
        dev = reg.predict_device(d["X_test"], None, quantiles=levels + [0.5])
        got_members = dev["member_logits"].cpu()
        worst_lg = 0.0
        for m in range(4):
            e = rel_err(got_members[m].numpy(), ref_logits[m].numpy())
            worst_lg = max(worst_lg, e)
            assert e <= 1e-4, (m, e)
        full = reg.predict(d["X_test"], None, output_type="full", quantiles=levels)
        assert list(full) == ["criterion", "logits", "mean", "median", "mode", "quantiles"]
        Q, B = case["Q"], case["num_buckets"]
        assert tuple(full["logits"].shape) == (Q, B) == z[f"{tag}_logits"].shape and full["logits"].device.type == "cpu"
        assert full["criterion"] is reg.renormalized_criterion_
        assert full["mean"].shape == full["median"].shape == full["mode"].shape == (Q,)
        assert len(full["quantiles"]) == len(levels) and all(q.shape == (Q,) for q in full["quantiles"])
        # the band of the logits through the float64 head: mean as a fraction of the span, quantiles in probability
        # space under the float64 CDF of the reference logits' own final distribution (as the head's tests)
        lv_all = levels + [0.5]
        base = _head64(z, ref_logits, avg, lv_all)
        b64 = torch.from_numpy(z["crit_borders"]).double()
        lv = torch.tensor(lv_all, dtype=torch.float64)[:, None]

        def dist(mean, quantiles):
            return {"mean": float((mean.double() - base["mean"]).abs().max()) / span,
                    "quantiles": float((ro.final_cdf64(base["probs"], b64, quantiles) - lv).abs().max())}

        d_ref = dist(torch.from_numpy(z[f"{tag}_mean"]),
                     torch.from_numpy(np.concatenate([z[f"{tag}_quantiles"], z[f"{tag}_median"][None]])))
        g = torch.Generator().manual_seed(5)
        move = {"mean": 0.0, "quantiles": 0.0}
        for _ in range(4):
            pert = [lg + (torch.randint(0, 2, lg.shape, generator=g) * 2.0 - 1.0)
                    * 1e-4 * max(1.0, float(lg.abs().max())) for lg in ref_logits]
            p = _head64(z, pert, avg, lv_all)
            for k, v in dist(p["mean"], p["quantiles"]).items():
                move[k] = max(move[k], v)
        err = dist(torch.from_numpy(full["mean"]), torch.from_numpy(np.stack(full["quantiles"] + [full["median"]])))
        for k in move:
            bound = 2 * move[k] + max(2 * d_ref[k], PROB_FLOOR)
            report(f"regressor {name} {tag}: member logits rel err {worst_lg:.2e}; {k} error {err[k]:.3e}, bound "
                   f"{bound:.3e} (the logit band moves it {move[k]:.3e}, the reference's own fp32 error {d_ref[k]:.3e})")
            assert err[k] <= bound, (k, err[k], bound)
        # the single output types are the composite's entries
        assert np.array_equal(reg.predict(d["X_test"], None), full["mean"])
        assert np.array_equal(reg.predict(d["X_test"], None, output_type="median"), full["median"])
        assert np.array_equal(reg.predict(d["X_test"], None, output_type="mode"), full["mode"])
        qs = reg.predict(d["X_test"], None, output_type="quantiles", quantiles=levels)
        assert all(np.array_equal(a, b) for a, b in zip(qs, full["quantiles"]))
        main = reg.predict(d["X_test"], None, output_type="main", quantiles=levels)
        assert list(main) == ["mean", "median", "mode", "quantiles"] and np.array_equal(main["mean"], full["mean"])


def test_regressor_fit_modes(tmp_path):
    """``fit_with_cache`` gives the default fit mode's outputs bit for bit.  ``low_memory`` re-fits its members at
    every predict from a seed of its own (another draw of the member seeds, in the reference too): it runs, and
    twice the same."""
    case, z = api_case("b100")
    variant = case["variants"][0]
    outs = {}
    for mode in ("fit_preprocessors", "fit_with_cache", "low_memory"):
        reg, d = _fit(case, tmp_path, variant, fit_mode=mode)
        out = reg.predict(d["X_test"], None, output_type="full", quantiles=ro.API_QUANTILES)
        outs[mode] = [out["logits"].numpy(), out["mean"], out["median"], out["mode"], *out["quantiles"]]
        if mode == "low_memory":
            again = reg.predict(d["X_test"], None, output_type="mean")
            assert np.array_equal(again, out["mean"])
    for a, b in zip(outs["fit_with_cache"], outs["fit_preprocessors"]):
        assert np.array_equal(a, b)
    assert all(np.isfinite(a).all() for a in outs["low_memory"][1:])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_regressor_16bit_modes_report(dtype, tmp_path):
    """The 16-bit modes run end to end; their distance from the fp32 reference is reported, not bounded."""
    case, z = api_case("b100")
    reg, d = _fit(case, tmp_path, case["variants"][0], inference_precision=dtype)
    full = reg.predict(d["X_test"], None, output_type="main", quantiles=ro.API_QUANTILES)
    span = float(z["crit_borders"][-2] - z["crit_borders"][1])
    em = float(np.abs(full["mean"] - z["mean_mean"]).max())
    eq = float(np.abs(np.stack(full["quantiles"]) - z["mean_quantiles"]).max())
    report(f"regressor b100 {dtype}: mean |d| vs fp32 reference {em:.3e} ({em / span:.2e} of the span), quantiles "
           f"{eq:.3e} ({eq / span:.2e})")
    assert np.isfinite(full["mean"]).all() and all(np.isfinite(q).all() for q in full["quantiles"])
    assert math.isfinite(em) and math.isfinite(eq)
