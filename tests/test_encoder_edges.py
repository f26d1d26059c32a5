"""The CPU oracle's input encoders reproduce the reference on the encoder edge fixtures.

``tests/golden/encoder/*.npz`` (``make_encoder_golden.py``) are small tabular tables built around one edge each:
columns constant on the train rows only, an all-constant group, the zero padding column, NaN / inf placement, one
valid train value, values far outside the soft-clip bounds, ``nf > fpg`` padding, NaN / gapped / fractional
labels, one train row.  The oracle is what the GPU tests of the encoder kernels compare against
(``test_encoder_gpu.py``), so it is pinned here first: fp32 to 1e-6 of the stored ``embedded_input`` (measured 0:
bit-exact), fp64 and the logits to the oracle tolerance 1e-5, the reference's ``ValueError`` where it raises, and
the same discrete decisions (selected columns, used flags, label codes) in fp32 and fp64, so that no fixture sits on
a knife edge where a correct kernel could legitimately decide differently.
"""

import json

import numpy as np
import pytest
import torch

from helpers import GOLDEN, oracle_spec, rel_err, report, torch_sd
from oracle.forward import embed_inputs, oracle_forward

ENC = GOLDEN / "encoder"
ENC_CASES = sorted(p.stem for p in ENC.glob("*.npz"))
EXPECTED = {"train_const", "group_all_const", "odd_F", "nan_mix", "one_valid", "outliers", "fpg1", "ynan", "ygap",
            "ynan_frac", "n1", "inf_train", "n1_no_outlier"}


def load_encoder_case(name: str):
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    z = np.load(ENC / f"{name}.npz")
    meta = json.loads(str(z["meta"]))
    cfg = ModelConfig(**meta["cfg"])
    sd = synth_state_dict(state_dict_spec(cfg), meta["wseed"])
    return z, meta, cfg, sd


def test_every_encoder_fixture_is_present():
    assert set(ENC_CASES) == EXPECTED
    for name in ("n1", "inf_train"):
        assert load_encoder_case(name)[1]["expect_raise"]


@pytest.mark.parametrize("case", ENC_CASES)
def test_oracle_embedding_matches_reference_on_edges(case):
    z, meta, cfg, sd = load_encoder_case(case)
    spec, w = oracle_spec(cfg), torch_sd(sd)
    x, y = torch.from_numpy(z["x"]), torch.from_numpy(z["y_train"])
    assert len(y) == meta["N"]
    if meta["expect_raise"]:
        assert "embedded_input" not in z and "logits" not in z
        for dt in (torch.float32, torch.float64):
            with pytest.raises(ValueError, match="no NaNs in the encoded x and y"):
                embed_inputs(spec, w, x, None, y, dtype=dt)
            with pytest.raises(ValueError):
                oracle_forward(spec, w, x, None, y, dtype=dt)
        return
    t32, t64 = {}, {}
    X32 = embed_inputs(spec, w, x, None, y, dtype=torch.float32, taps=t32)
    X64 = embed_inputs(spec, w, x, None, y, dtype=torch.float64, taps=t64)
    e32, e64 = rel_err(X32.numpy(), z["embedded_input"]), rel_err(X64.numpy(), z["embedded_input"])
    out = oracle_forward(spec, w, x, None, y)
    out64 = oracle_forward(spec, w, x, None, y, dtype=torch.float64)
    el, el64 = rel_err(out.numpy(), z["logits"]), rel_err(out64.numpy(), z["logits"])
    report(f"oracle vs reference {case}: embedding fp32 {e32:.2e} fp64 {e64:.2e}, logits fp32 {el:.2e} fp64 {el64:.2e}")
    assert X32.shape == z["embedded_input"].shape and np.isfinite(z["embedded_input"]).all()
    assert e32 <= 1e-6
    assert e64 <= 1e-5
    assert el <= 1e-5 and el64 <= 1e-5
    for k in ("x_selected", "x_used", "y_codes"):
        assert torch.equal(t32[k].long(), t64[k].long()), k


def test_ynan_frac_label_fill_is_the_device_mean():
    """``ynan_frac``'s labels are chosen so that a float32 ``np.nanmean`` lies below the float32 rounding of the
    float64 mean, which is what the statistics kernel fills NaN labels with (``(float)(fp64 sum / count)``).
    ``engine.target_uniques`` must hold that same value: otherwise the filled rows compare greater than the host's
    mean in ``uniq`` and every NaN-label row -- every test row -- is coded one class too high.  (Failed before
    ``target_uniques`` took the float64 mean: 5 unique values with the fill one ulp low, codes 3 instead of 2.)"""
    from multimodalpfn_amd.engine import target_uniques

    z, meta, cfg, sd = load_encoder_case("ynan_frac")
    y = z["y_train"]
    ok = ~np.isnan(y)
    assert meta["N"] >= 100 and (~ok).sum() == 1
    dev = np.float32(y[ok].astype(np.float64).sum() / ok.sum())
    assert np.float32(np.nanmean(y)) < dev  # the fixture's premise
    uniq = target_uniques(y)
    assert dev in uniq
    codes = (np.where(ok, y, dev)[:, None] > uniq[None, :]).sum(1)
    t = {}
    embed_inputs(oracle_spec(cfg), torch_sd(sd), torch.from_numpy(z["x"]), None, torch.from_numpy(y), taps=t)
    assert np.array_equal(codes, t["y_codes"][: len(y)].long().numpy())
    assert int((dev > uniq).sum()) == int(t["y_codes"][-1])  # the test rows' code


def test_target_uniques_plain_labels_unchanged():
    from multimodalpfn_amd.engine import target_uniques

    assert np.array_equal(target_uniques(np.array([2, 0, 1, 1, 2], dtype=np.float32)), [0, 1, 2])
    u = target_uniques(np.array([2, np.nan, 0, 1], dtype=np.float32))
    assert np.array_equal(u, [0, 1, 2])  # the integer mean 1 is already a label
    assert u.dtype == np.float32
