"""Row embeddings on the host: the oracle's last layer against the reference's embeddings, and the checks of the
embeddings interface that need no GPU.

The reference's forward with ``only_return_standard_out=False`` returns the target token's final state of every row
(``transformer.py:850-864``); ``tests/golden/emb/<case>.npz`` (``make_embeddings_golden.py``) holds it for the eight
golden cases, from forwards whose logits are the committed goldens bit for bit.  The oracle's last layer tap at the
target token is the same quantity, held to the bound ``test_oracle_golden.py`` uses for layer states (1e-5; measured
3.2e-7 .. 8.0e-7 over the cases).
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import CASES, GOLDEN, load_case, oracle_spec, rel_err, torch_sd
from oracle.forward import oracle_forward

HEADER = Path(__file__).resolve().parent.parent / "include" / "mmpfn_hip.h"

ENTRY_POINTS = {  # name: the arguments mmpfn_forward's relative takes beyond it
    "mmpfn_forward_embed": ("mmpfn_forward", ("float* train_emb", "float* test_emb")),
    "mmpfn_forward_batch_embed": ("mmpfn_forward_batch", ("float* train_emb", "float* test_emb")),
    "mmpfn_cache_predict_embed": ("mmpfn_cache_predict", ("float* test_emb",)),
}


def load_embeddings(case):
    f = np.load(GOLDEN / "emb" / f"{case}.npz")
    return f["train_embeddings"], f["test_embeddings"]


@pytest.mark.parametrize("case", CASES)
def test_oracle_last_layer_target_token_is_the_reference_embedding(case):
    z, meta, cfg, sd = load_case(case)
    train, test = load_embeddings(case)
    N = len(z["y_train"])
    assert train.dtype == test.dtype == np.float32
    assert train.shape == (N, cfg.emsize) and test.shape == (len(z["logits"]), cfg.emsize)
    x = torch.from_numpy(z["x"]) if "x" in z else None
    im = torch.from_numpy(z["image"]) if "image" in z else None
    taps = {}
    out = oracle_forward(oracle_spec(cfg), torch_sd(sd), x, im, torch.from_numpy(z["y_train"]), taps=taps)
    assert rel_err(out.numpy(), z["logits"]) < 1e-5  # the forward the embeddings belong to
    emb = taps[f"layer{cfg.nlayers - 1}"][:, -1].numpy()
    e_train, e_test = rel_err(emb[:N], train), rel_err(emb[N:], test)
    print(f"oracle embeddings {case}: train {e_train:.2e}, test {e_test:.2e}")
    assert e_train < 1e-5 and e_test < 1e-5


def _classifier(**kw):
    from multimodalpfn_amd.classifier import MMPFNClassifier

    return MMPFNClassifier(mixer_type="MGM+CAP", mgm_heads=8, cap_heads=4, features_per_group=2, **kw)


def _regressor(**kw):
    from multimodalpfn_amd.regressor import MMPFNRegressor

    return MMPFNRegressor(mixer_type="MGM+CAP", mgm_heads=8, cap_heads=4, features_per_group=2, **kw)


@pytest.mark.parametrize("make", [_classifier, _regressor])
@pytest.mark.parametrize("method", ["get_embeddings", "get_embeddings_device"])
def test_unknown_data_source_is_refused_before_anything_runs(make, method):
    """An unfitted estimator has no model, executor or device: the refusal must come before any of them is touched."""
    est = make()
    for bad in ("valid", "Train", "both", None, 0):
        with pytest.raises(ValueError, match="data_source must be one of"):
            getattr(est, method)(np.zeros((3, 4)), None, data_source=bad)


@pytest.mark.parametrize("make", [_classifier, _regressor])
def test_cache_mode_refuses_train_embeddings(make):
    est = make(fit_mode="fit_with_cache")
    with pytest.raises(ValueError, match="fit_preprocessors.*low_memory"):
        est.get_embeddings(np.zeros((3, 4)), None, data_source="train")
    # "test" passes the source check and reaches the fitted-estimator check
    from sklearn.exceptions import NotFittedError

    with pytest.raises(NotFittedError):
        est.get_embeddings(np.zeros((3, 4)), None, data_source="test")


def test_cache_executor_refuses_train_embeddings_itself():
    """The executor's own member loop refuses too (``iter_outputs`` is what other callers reach), before it asks for
    the engine."""
    from multimodalpfn_amd.inference import InferenceEngineCacheKV, InferenceEngineCachePreprocessing

    ex = InferenceEngineCacheKV(save_peak_mem=False, dtype_byte_size=4)  # no model: touching the engine would raise
    with pytest.raises(ValueError, match="fit_preprocessors.*low_memory"):
        next(ex.iter_outputs(np.zeros((3, 4)), None, device=torch.device("cpu"), autocast=False, embeddings="train"))
    for cls in (InferenceEngineCacheKV, InferenceEngineCachePreprocessing):
        with pytest.raises(ValueError, match="data_source must be one of"):
            next(cls(save_peak_mem=False, dtype_byte_size=4).iter_outputs(
                np.zeros((3, 4)), None, device=torch.device("cpu"), autocast=False, embeddings="both"))


def _declaration(name):
    """The argument list of ``name``'s declaration in the header, whitespace collapsed."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER.read_text(), re.S)
    assert m, f"{name} is not declared in {HEADER.name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_header_declares_the_entry_point_as_its_relative_plus_the_embeddings(name):
    base, extra = ENTRY_POINTS[name]
    args, base_args = _declaration(name), _declaration(base)
    at = base_args.index("float* logits") + 1
    assert args == base_args[:at] + list(extra) + base_args[at:]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_binding_table_matches_the_header(name):
    from multimodalpfn_amd import _lib

    base, extra = ENTRY_POINTS[name]
    sig = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    res, args = sig[name]
    base_res, base_args = sig[base]
    assert res is ctypes.c_int and base_res is ctypes.c_int
    assert len(args) == len(_declaration(name)) == len(base_args) + len(extra)
    at = _declaration(base).index("float* logits") + 1
    assert list(args) == list(base_args[:at]) + [ctypes.c_void_p] * len(extra) + list(base_args[at:])


def test_library_exports_the_entry_points_and_refuses_a_null_context():
    from multimodalpfn_amd import _lib

    lib = _lib.load_library()
    assert lib.mmpfn_forward_embed(None, None, 0, 0, None, 0, None, 0, None, 0, None, None, None, None,
                                   0) == _lib.MMPFN_ERR_INVALID
    assert lib.mmpfn_forward_batch_embed(None, 1, None, 0, 0, None, 0, None, 0, None, None, None, None, None, None,
                                         0) == _lib.MMPFN_ERR_INVALID
    assert lib.mmpfn_cache_predict_embed(None, None, None, 0, 0, None, 0, None, None) == _lib.MMPFN_ERR_INVALID


def test_engine_refuses_an_unknown_embeddings_keyword_on_the_host():
    """``HipEngine``'s keyword is checked against one table; the check needs no context."""
    from multimodalpfn_amd.engine import HipEngine

    assert set(HipEngine.EMBEDDINGS) == {"test", "train", "both"}
    assert HipEngine.EMBEDDINGS["both"] == (True, True) and HipEngine.EMBEDDINGS["test"] == (False, True)
    with pytest.raises(ValueError, match="embeddings must be None or one of"):
        HipEngine._check_embeddings("all")
