"""Row embeddings from the forward: the target token's final state of the train and the test rows, from
the C ABI (``mmpfn_forward_embed`` and its batch and cache forms) up to ``get_embeddings`` of both estimators.

1. **Bitwise against the tested full path.**  A full last layer through the taps (``embed_state`` + ``run_layers`` +
   ``copy_state``) is the state the embeddings are rows of: ``forward(..., embeddings="both")`` must return its
   ``[:N, -1]`` and ``[N:, -1]`` with ``torch.equal`` -- the train rows through the last layer's column form, the test
   rows through the pruned form -- and the logits of the plain ``forward``.
2. **Entry-point consistency**: batched and laned members, ``"test"`` / ``"train"`` alone, the train-KV cache.
3. **Unchanged behaviour**: a plain ``forward`` before and after an embeddings call, the last layer pruned and in full.
4. **Parity** with the reference's embeddings (``tests/golden/emb``) in the fp32 mode, ``rel_err < 1e-4``: the
   project's bound for a layer state against the reference (``test_parity_gpu.py``) and for logits.  The 16-bit modes'
   figures are reported, not asserted (check 1 and the logits budgets bound them).
5. **Seam**: ``only_return_standard_out=False``.   6. **Estimators**: ``get_embeddings`` / ``get_embeddings_device``.

Shapes of checks 1-3: ``test_last_layer_gpu.py``'s -- N = 100 train rows (a partial 64-key tile; the test rows start
mid-way through a 256-query task), Q = 37 or 1, T = 4, 28, 36 and 55, a last layer that is also the first -- plus
N = 300, where the train rows span two 256-query tasks and the test rows start inside the second.
"""

import copy
import functools

import numpy as np
import pytest
import torch

from helpers import CASES as GOLDEN_CASES
from helpers import GOLDEN, load_case, rel_err, report, torch_sd

pytestmark = pytest.mark.gpu

SEED = 23
E = 192
# parity (split bf16), bf16, fp32-input MFMA, fp16, fp16 with the fp8 P.V (e4m3)
PRECS = {"f32": 0, "bf16": 1, "f32_mfma": 2, "f16": 5, "f16_f8": 6}
# name: (layers, train rows, test rows, mixer tokens?, features)
SHAPES = {"mixer_q37": (2, 100, 37, True, 5), "mixer_q1": (2, 100, 1, True, 5), "tabular_q37": (2, 100, 37, False, 5),
          "one_layer_q37": (1, 100, 37, True, 5), "t36_q37": (2, 100, 37, True, 21), "t55_q37": (1, 100, 37, True, 60),
          "n300_q37": (2, 300, 37, True, 5)}
TOKENS = {"mixer_q37": 28, "mixer_q1": 28, "tabular_q37": 4, "one_layer_q37": 28, "t36_q37": 36, "t55_q37": 55,
          "n300_q37": 28}


@functools.lru_cache(maxsize=None)
def _model(nlayers):
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec
    from multimodalpfn_amd.model.transformer import PerFeatureTransformer

    cfg = ModelConfig(nlayers=nlayers, mgm_heads=8, cap_heads=24)
    model = PerFeatureTransformer(cfg)
    model.load_state_dict(torch_sd(synth_state_dict(state_dict_spec(cfg), SEED)))
    return model.to("cuda"), cfg


@functools.lru_cache(maxsize=None)
def _inputs(N, Q, with_image, F):
    from synth import synth_image, synth_labels, synth_table

    S = N + Q
    x = torch.from_numpy(synth_table(S, F, SEED, n_cat=2, nan_frac=0.02)).cuda()
    im = torch.from_numpy(synth_image(S, 1, SEED)).cuda() if with_image else None
    return x, im, synth_labels(S, 4, SEED)[:N]


def _setup(shape, prec):
    nlayers, N, Q, with_image, F = SHAPES[shape]
    model, cfg = _model(nlayers)
    eng = model.engine()
    eng.full_last_layer = False
    x, im, y = _inputs(N, Q, with_image, F)
    tok = None if im is None else eng.mixer_tokens(im, PRECS[prec])
    return eng, cfg, x, tok, y, N, Q


# ------------------------------------------------------------------------------------------------ 1. bitwise


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_embeddings_are_bitwise_the_full_last_layers_target_token(prec, shape):
    code = PRECS[prec]
    with torch.inference_mode():
        eng, cfg, x, tok, y, N, Q = _setup(shape, prec)
        eng.embed_state(x, tok, y, code)
        state = eng.run_layers(0, cfg.nlayers)  # full layers, whatever the switch says
        assert state.shape == (N + Q, TOKENS[shape], E)
        plain = eng.forward(x, tok, y, code)
        logits, train, test = eng.forward(x, tok, y, code, embeddings="both")
    assert train.shape == (N, E) and test.shape == (Q, E) and train.dtype == test.dtype == torch.float32
    assert torch.isfinite(train).all() and torch.isfinite(test).all() and torch.isfinite(logits).all()
    assert torch.equal(train, state[:N, -1]), (train - state[:N, -1]).abs().max().item()
    assert torch.equal(test, state[N:, -1]), (test - state[N:, -1]).abs().max().item()
    assert torch.equal(logits, plain)


# ------------------------------------------------------------------------------------------------ 2. entry points


@pytest.mark.parametrize("shape", ["mixer_q37", "tabular_q37", "t55_q37", "n300_q37"])
@pytest.mark.parametrize("prec", PRECS)
def test_entry_points_agree(prec, shape):
    code = PRECS[prec]
    with torch.inference_mode():
        eng, cfg, x, tok, y, N, Q = _setup(shape, prec)
        # three members of one geometry: column rotations of the table, shifted labels
        items = [(torch.roll(x, k, dims=1), tok, (y + k) % 4) for k in range(3)]
        singles = [eng.forward(xi, ti, yi, code, embeddings="both") for xi, ti, yi in items]
        for lanes, batch in ((1, 3), (2, 1), (2, 2)):
            many = eng.forward_many(items, code, lanes=lanes, batch=batch, embeddings="both")
            eng.status()
            assert len(many) == 3
            for k, (one, got) in enumerate(zip(singles, many)):
                for name, a, b in zip(("logits", "train", "test"), one, got):
                    assert torch.equal(a, b), (lanes, batch, k, name)
        assert not torch.equal(singles[0][1], singles[1][1])  # (the members are different members)
        logits, train, test = singles[0]
        lg_te, none_tr, only_te = eng.forward(x, tok, y, code, embeddings="test")
        lg_tr, only_tr, none_te = eng.forward(x, tok, y, code, embeddings="train")
        assert none_tr is None and none_te is None
        assert torch.equal(only_te, test) and torch.equal(only_tr, train)
        assert torch.equal(lg_te, logits) and torch.equal(lg_tr, logits)
        for kw in ({}, {"lanes": 2}):  # "test" through the batching entry point: (logits, None, test) per member
            for one, got in zip(singles, eng.forward_many(items, code, embeddings="test", **kw)):
                assert got[1] is None and torch.equal(got[0], one[0]) and torch.equal(got[2], one[2])
        eng.status()
        # the train-KV cache: the decoder's input rows of that predict
        tt, tq = (None, None) if tok is None else (tok[:N], tok[N:])
        cache = eng.cache_build(x[:N], tt, y, code)
        try:
            plain = eng.cache_predict(cache, x[N:], tq)
            c_logits, c_none, c_test = eng.cache_predict(cache, x[N:], tq, embeddings="test")
            after = eng.copy_state()  # (a cache predict's state: Q rows, every one a test row)
            assert after.shape == (Q, TOKENS[shape], E)
            e_logits, _, e_test = eng.cache_predict(cache, x[N:N], None if tq is None else tq[:0], embeddings="test")
            assert e_logits.shape == (0, cfg.n_out) and e_test.shape == (0, E)  # no rows: nothing to launch
            many = eng.cache_predict_many([cache, cache], [x[N:], x[N:]], tq, lanes=2, embeddings="test")
            eng.status()
            with pytest.raises(ValueError, match="'test' only"):
                eng.cache_predict(cache, x[N:], tq, embeddings="both")
        finally:
            cache.free()
    assert c_none is None and c_test.shape == (Q, E)
    assert torch.equal(c_test, after[:, -1])
    assert torch.equal(c_logits, plain)
    for got in many:
        assert got[1] is None and torch.equal(got[0], plain) and torch.equal(got[2], c_test)


def test_engine_refuses_an_unknown_keyword_before_any_launch():
    with torch.inference_mode():
        eng, cfg, x, tok, y, N, Q = _setup("tabular_q37", "f32")
        for call in (lambda: eng.forward(x, tok, y, 0, embeddings="all"),
                     lambda: eng.forward_many([(x, tok, y)], 0, embeddings="all"),
                     lambda: eng.forward_batch([(x, tok, y)], 0, embeddings="all")):
            with pytest.raises(ValueError, match="embeddings must be None or one of"):
                call()
        eng.status()


def test_c_abi_null_outputs_and_alignment():
    """All three outputs NULL is MMPFN_ERR_INVALID; a NULL logits skips the decoder and still serves the embeddings;
    an embedding output that is not 16-byte aligned is refused."""
    from multimodalpfn_amd import _lib
    from multimodalpfn_amd.engine import _count, _ptr

    with torch.inference_mode():
        eng, cfg, x, tok, y, N, Q = _setup("tabular_q37", "f16")
        xd, td, yd, uniq, S, F, C, N_, G = eng._prepare(x, tok, y)
        pr = eng._pos(G + C)
        eng._bind_stream()

        def call(logits, train, test):
            return eng.lib.mmpfn_forward_embed(eng.ctx, _ptr(xd), S, F, _ptr(td), C, _ptr(yd), N, _ptr(uniq),
                                               _count(uniq), _ptr(pr), logits, train, test, 5)

        assert call(None, None, None) == _lib.MMPFN_ERR_INVALID
        _, train, test = eng.forward(x, tok, y, 5, embeddings="both")
        tr = torch.zeros((N, E), device="cuda")
        te = torch.zeros((Q, E), device="cuda")
        assert call(None, tr.data_ptr(), te.data_ptr()) == 0
        eng.status()
        assert torch.equal(tr, train) and torch.equal(te, test)
        odd = torch.zeros((N * E + 1,), device="cuda")[1:]
        assert call(None, odd.data_ptr(), None) == _lib.MMPFN_ERR_INVALID
        eng.status()
        assert float(odd.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 3. unchanged


@pytest.mark.parametrize("shape", ["mixer_q37", "n300_q37"])
@pytest.mark.parametrize("prec", PRECS)
def test_plain_forward_is_unchanged_around_an_embeddings_call(prec, shape):
    code = PRECS[prec]
    got = {}
    with torch.inference_mode():
        eng, cfg, x, tok, y, N, Q = _setup(shape, prec)
        for on in (False, True):
            eng.full_last_layer = on
            try:
                before = eng.forward(x, tok, y, code)
                got[on] = eng.forward(x, tok, y, code, embeddings="both")
                after = eng.forward(x, tok, y, code)
            finally:
                eng.full_last_layer = False
            assert torch.equal(before, after) and torch.equal(before, got[on][0]), on
    for a, b in zip(got[False], got[True]):  # the column form against the last layer in full
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 4. parity


def _golden_model(cfg, sd):
    from multimodalpfn_amd.model.transformer import PerFeatureTransformer

    model = PerFeatureTransformer(cfg)
    model.load_state_dict(torch_sd(sd))
    norm = next(e for e in model.encoder if "InputNormalizationEncoderStep" in str(e.__class__))
    norm.remove_outliers = cfg.remove_outliers_sigma is not None
    norm.remove_outliers_sigma = cfg.remove_outliers_sigma or 4.0
    return model.to("cuda")


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_embeddings_match_the_reference(case):
    from multimodalpfn_amd import _lib

    z, meta, cfg, sd = load_case(case)
    ref = np.load(GOLDEN / "emb" / f"{case}.npz")
    eng = _golden_model(cfg, sd).engine()
    x = torch.from_numpy(z["x"]).cuda() if "x" in z else None
    errs = {}
    with torch.inference_mode():
        for name, code in (("f32", _lib.PREC_F32), ("f16", _lib.PREC_F16), ("bf16", _lib.PREC_BF16)):
            tok = eng.mixer_tokens(torch.from_numpy(z["image"]).cuda(), code) if "image" in z else None
            _, train, test = eng.forward(x, tok, z["y_train"], code, embeddings="both")
            assert torch.isfinite(train).all() and torch.isfinite(test).all()
            errs[name] = (rel_err(train.cpu().numpy(), ref["train_embeddings"]),
                          rel_err(test.cpu().numpy(), ref["test_embeddings"]))
    report(f"embeddings vs reference {case} (train, test): " +
           ", ".join(f"{k} {a:.2e} {b:.2e}" for k, (a, b) in errs.items()))
    assert max(errs["f32"]) < 1e-4, errs["f32"]


# ------------------------------------------------------------------------------------------------ 5. seam


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_seam_returns_the_references_dict(prec):
    code = PRECS[prec]
    nlayers, N, Q, with_image, F = SHAPES["mixer_q37"]
    model, cfg = _model(nlayers)
    model.engine().full_last_layer = False
    x, im, y = _inputs(N, Q, with_image, F)
    yt = torch.from_numpy(y).cuda()
    with torch.inference_mode():
        std = model(None, x[:, None, :], im, yt, only_return_standard_out=True, single_eval_pos=N, precision=code)
        out = model(None, x[:, None, :], im, yt, only_return_standard_out=False, single_eval_pos=N, precision=code)
        assert sorted(out) == ["standard", "test_embeddings", "train_embeddings"]
        assert out["standard"].shape == (Q, 1, cfg.n_out) and torch.equal(out["standard"], std)
        assert out["train_embeddings"].shape == (N, 1, E) and out["test_embeddings"].shape == (Q, 1, E)
        _, train, test = model.engine().forward(x, model.engine().mixer_tokens(im, code), y, code, embeddings="both")
        assert torch.equal(out["train_embeddings"][:, 0], train) and torch.equal(out["test_embeddings"][:, 0], test)
        # a model that holds a train-KV cache: test rows only, no train rows' embeddings
        cached = copy.deepcopy(model)
        cached.cache_trainset_representation = True
        try:
            with pytest.raises(NotImplementedError, match="train-only cache-building call"):
                cached(None, x[:N, None, :], im[:N], yt, only_return_standard_out=False, single_eval_pos=N,
                       precision=code)
            built = cached(None, x[:N, None, :], im[:N], yt, single_eval_pos=N, precision=code)
            assert built.shape == (0, 1, cfg.n_out)
            c_std = cached(None, x[N:, None, :], im[N:], None, single_eval_pos=None, precision=code)
            c_out = cached(None, x[N:, None, :], im[N:], None, only_return_standard_out=False, single_eval_pos=None,
                           precision=code)
        finally:
            cached.empty_trainset_representation_cache()
        assert sorted(c_out) == ["standard", "test_embeddings", "train_embeddings"]
        assert c_out["train_embeddings"].shape == (0, 1, E) and c_out["train_embeddings"].dtype == torch.float32
        assert c_out["test_embeddings"].shape == (Q, 1, E) and torch.isfinite(c_out["test_embeddings"]).all()
        assert c_out["standard"].shape == (Q, 1, cfg.n_out) and torch.equal(c_out["standard"], c_std)


# ------------------------------------------------------------------------------------------------ 6. estimators


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _estimator_checks(make, d, image, predict):
    """``make(fit_mode)`` -> a fitted estimator with 4 members whose preprocessing is exact on the device; ``d``:
    its train / test tables; ``predict(est)``: the estimator's prediction, for the unchanged-behaviour check.

    The members rotate their features (``FEATURE_SHIFT_METHOD="rotate"``: the shift counts are part of the ensemble
    configs) so that the three fit modes hold the same members: a shuffling member draws its permutation from the
    member seed, which ``low_memory`` draws anew from a seed of its own (``test_regressor_fit_modes``), and its
    embeddings -- like its logits -- are then another member's."""
    est = make("fit_preprocessors")
    X, Xd = d["X_test"], _cuda(d["X_test"])
    N, Q = len(d["X_train"]), len(X)
    before = predict(est)
    test = est.get_embeddings(X, image, data_source="test")
    train = est.get_embeddings(X, image, data_source="train")
    assert isinstance(test, np.ndarray) and test.dtype == train.dtype == np.float32
    assert test.shape == (4, Q, E) and train.shape == (4, N, E)
    assert np.isfinite(test).all() and np.isfinite(train).all()
    assert not np.array_equal(test[0], test[1])  # the members differ (feature shifts)
    np.testing.assert_array_equal(est.get_embeddings(X, image), test)  # "test" is the default
    dev = est.get_embeddings_device(X, image, data_source="test")
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32
    np.testing.assert_array_equal(dev.cpu().numpy(), test)
    # a table on the GPU takes the members' device programs
    assert all(p is not None for p in est.executor_.device_programs), est.executor_.program_reasons
    np.testing.assert_array_equal(est.get_embeddings(Xd, image, data_source="test"), test)
    np.testing.assert_array_equal(est.get_embeddings(Xd, image, data_source="train"), train)
    # "train": X only rides along
    other = np.ascontiguousarray(X[::-1][: max(1, Q // 2)])
    other_image = None if image is None else np.ascontiguousarray(image[::-1][: len(other)])
    np.testing.assert_array_equal(est.get_embeddings(other, other_image, data_source="train"), train)
    np.testing.assert_array_equal(predict(est), before)
    low = make("low_memory")
    np.testing.assert_array_equal(low.get_embeddings(X, image, data_source="test"), test)
    np.testing.assert_array_equal(low.get_embeddings(X, image, data_source="train"), train)
    kv = make("fit_with_cache")
    kv_before = predict(kv)
    kv_test = kv.get_embeddings(X, image, data_source="test")
    assert kv_test.shape == (4, Q, E) and kv_test.dtype == np.float32 and np.isfinite(kv_test).all()
    np.testing.assert_array_equal(kv.get_embeddings(Xd, image, data_source="test"), kv_test)
    with pytest.raises(ValueError, match="fit_preprocessors.*low_memory"):
        kv.get_embeddings(X, image, data_source="train")
    with pytest.raises(ValueError, match="data_source must be one of"):
        kv.get_embeddings(X, image, data_source="valid")
    np.testing.assert_array_equal(predict(kv), kv_before)
    return test, kv_test


def test_classifier_get_embeddings(tmp_path):
    from test_api_host import _case, case_data, make_classifier, write_ckpt

    case = dict(_case("pad_none"))  # PreprocessorConfig("none"), FINGERPRINT_FEATURE=False, 4 members, image tokens
    assert case["interface"]["FINGERPRINT_FEATURE"] is False and case["clf"]["n_estimators"] == 4
    case["interface"] = dict(case["interface"], FEATURE_SHIFT_METHOD="rotate")
    d = case_data(case)
    ckpt = write_ckpt(case, tmp_path)

    def make(fit_mode):
        clf = make_classifier(case, ckpt, fit_mode=fit_mode)
        return clf.fit(d["X_train"], d["image_train"], d["y_train"])

    test, kv_test = _estimator_checks(make, d, d["image_test"], lambda clf: clf.predict_proba(d["X_test"], d["image_test"]))
    report(f"classifier get_embeddings: fit_with_cache vs fit_preprocessors test embeddings rel err "
           f"{rel_err(kv_test, test):.2e}")


def test_regressor_get_embeddings(tmp_path):
    import regression_oracle as ro
    from test_regression_host import api_case, write_ckpt

    from multimodalpfn_amd import MMPFNRegressor
    from multimodalpfn_amd.preprocessing import PreprocessorConfig

    case, _ = api_case("b100")
    d = ro.api_case_data(case)
    path, _, _ = write_ckpt(case, tmp_path)
    kw = ro.api_regressor_kwargs(case, case["variants"][0])
    kw["inference_config"] = {"FINGERPRINT_FEATURE": False, "PREPROCESS_TRANSFORMS": [PreprocessorConfig("none")],
                              "FEATURE_SHIFT_METHOD": "rotate"}

    def make(fit_mode):
        return MMPFNRegressor(model_path=str(path), fit_mode=fit_mode, **kw).fit(d["X_train"], None, d["y_train"])

    test, kv_test = _estimator_checks(make, d, None, lambda reg: reg.predict(d["X_test"], None))
    report(f"regressor get_embeddings: fit_with_cache vs fit_preprocessors test embeddings rel err "
           f"{rel_err(kv_test, test):.2e}")
