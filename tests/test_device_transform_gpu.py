"""Member preprocessing on the device: the kernel alone on the CPU cases' programs, then end to end.

The tap (``HipEngine.member_transform``) is held to ``test_device_transform.py``'s bounds against
``pipeline.transform(X).X``: bit equality for gathers, lookups, guarded scalers and fingerprints, 8 * 2^-53 for uniform
quantiles, ``2 (F + 2) 2^-53 sum |z| |c|`` for SVD columns; ``out32`` is ``float32(out64)`` bit for bit; what lies
outside the ``[Q, n_out]`` block of an output buffer keeps its bits.  End to end (fp32 mode) a CUDA tensor ``X`` is
compared with the same table as a numpy array.  Before the feature a CUDA tensor raises inside ``validate_X_predict``
and ``HipEngine`` has no ``member_transform``: every test here fails on the parent.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import device_transform_cases as C
import regression_oracle as ro
from helpers import rel_err, report
from multimodalpfn_amd import _lib
from multimodalpfn_amd import device_transform as D
from test_api_host import _case, case_data, make_classifier, write_ckpt
from test_regression_host import api_case
from test_regression_host import write_ckpt as write_reg_ckpt

pytestmark = pytest.mark.gpu

_ENGINE: list = []
GUARD32, GUARD64 = 0x7FC12345, 0x7FF8000000ABCDEF  # NaN patterns no kernel output has


def _engine():
    from synth import synth_state_dict

    from multimodalpfn_amd.engine import HipEngine
    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    if not _ENGINE:
        cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2)
        _ENGINE.append(HipEngine(cfg, synth_state_dict(state_dict_spec(cfg), 23), torch.device("cuda")))
    return _ENGINE[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# one case per config and layout that changes the program's shape: every op and map kind, the widest rows (7 rows
# per block instead of 8), the one-column table, the pure gather
TAP_CASES = [
    ("clf_default_0", "c21", 200, 460, "shuffle", False),
    ("clf_default_0", "w140", 200, 460, "rotate", False),
    ("clf_default_1", "c21", 200, 460, None, True),
    ("run_none", "c21", 30, 460, "shuffle", False),
    ("reg_default_0", "n2", 200, 460, "rotate", False),
    ("reg_default_0", "n1", 1838, 460, None, True),
    ("scaler", "c21", 200, 460, "rotate", True),
    ("subsample", "w140", 200, 460, "shuffle", True),
]


def _q_values(width: int) -> list[int]:
    r = D.rows_per_block(width)
    return sorted({1, r - 1, r, r + 1, 63, 64, 65, 460})


@pytest.mark.parametrize("case", TAP_CASES, ids=C.case_id)
def test_tap_matches_host_pipeline(case):
    """Q on both sides of a wave and of the kernel's rows per block, 1 and 460; float64 and float32 input, each with
    a padded leading dimension; outputs into NaN-filled buffers with guard rows and columns."""
    eng = _engine()
    config, layout, n_train, n_test, shift, fp = case
    pipe, X, T = C.fitted(config, layout, n_train, n_test, shift, fp)
    prog, why = D.compile_member(pipe, X.shape[1], probe=X)
    assert prog is not None, why
    F, n_out = prog.n_in, prog.n_out
    worst_q = worst_svd = 0.0
    same_as_restatement = True
    for dtype in (torch.float64, torch.float32):
        with np.errstate(invalid="ignore"):
            Th = np.array(T) if dtype == torch.float64 else np.array(T).astype(np.float32)
        T64 = Th.astype(np.float64)
        want = C.host_reference(pipe, T64)
        host64, _, bound = D.run_program_host(prog, T64, return_bound=True)
        padded = torch.full((len(Th), F + 3), 7.0, dtype=dtype, device="cuda")
        padded[:, :F] = torch.from_numpy(Th).cuda()
        for Q in _q_values(prog.width):
            buf32 = torch.full((Q + 2, n_out + 3), 0, dtype=torch.int32, device="cuda").fill_(GUARD32)
            buf64 = torch.full((Q + 2, n_out + 5), 0, dtype=torch.int64, device="cuda").fill_(GUARD64)
            out32, out64 = eng.member_transform(prog, padded[:Q, :F], out=buf32.view(torch.float32)[:Q],
                                                want64=buf64.view(torch.float64)[:Q])
            eng.status()
            g32, g64 = buf32.cpu().numpy(), buf64.cpu().numpy()
            assert (g32[Q:] == GUARD32).all() and (g32[:, n_out:] == GUARD32).all(), (Q, "float32 guards")
            assert (g64[Q:] == GUARD64).all() and (g64[:, n_out:] == GUARD64).all(), (Q, "float64 guards")
            got = np.ascontiguousarray(g64[:Q, :n_out]).view(np.float64)
            got32 = np.ascontiguousarray(g32[:Q, :n_out]).view(np.float32)
            bad = D.mismatch(got, want[:Q], bound[:Q])
            assert not bad.any(), (str(dtype), Q, np.argwhere(bad)[:5].tolist())
            with np.errstate(invalid="ignore", over="ignore"):
                assert np.array_equal(bits(got32), bits(got.astype(np.float32))), (str(dtype), Q)
            same_as_restatement &= bool(np.array_equal(bits(got), bits(host64[:Q])))
            with np.errstate(invalid="ignore"):
                err = np.nan_to_num(np.abs(got - want[:Q]))  # NaN only against NaN (mismatch above)
            qm, sm = bound[:Q] == D.QUANTILE_BOUND, (bound[:Q] > 0) & (bound[:Q] != D.QUANTILE_BOUND)
            if qm.any():
                worst_q = max(worst_q, float(err[qm].max()))
            if sm.any():
                worst_svd = max(worst_svd, float((err[sm] / bound[:Q][sm]).max()))
    report(f"member_transform {C.case_id(case)}: ops {prog.ops[:, 0].tolist()} width {prog.width}; worst quantile err "
           f"{worst_q:.2e} (bound {D.QUANTILE_BOUND:.2e}), worst SVD err {worst_svd:.2e} of its bound; "
           f"bit-equal to the numpy restatement: {same_as_restatement}")


def test_tap_width_limit_and_refusals():
    """A program at the width limit runs (one row per block, the whole 64 KiB of LDS); one past it does not reach
    the device; a damaged op list is refused where it is uploaded."""
    from multimodalpfn_amd.model.preprocessing import SequentialFeatureTransformer, ShuffleFeaturesStep

    eng = _engine()
    F = D.MAX_WIDTH
    pipe = SequentialFeatureTransformer([ShuffleFeaturesStep("shuffle", 0, 3)])
    X = np.random.default_rng(0).standard_normal((3, F))
    pipe.fit(X, [])
    prog, why = D.compile_member(pipe, F, probe=X)
    assert prog is not None and prog.width == F and D.rows_per_block(prog.width) == 1, why
    out, out64 = eng.member_transform(prog, torch.from_numpy(X).cuda(), want64=True)
    eng.status()
    assert np.array_equal(bits(out64.cpu().numpy()), bits(C.host_reference(pipe, X)))
    assert np.array_equal(bits(out.cpu().numpy()), bits(out64.cpu().numpy().astype(np.float32)))

    wide = D.MemberProgram(np.array([[D.OP_GATHER, F + 1, F + 1, 0, 0, 0, 0, 0]], np.int32),
                           np.arange(F + 1, dtype=np.int32), np.zeros(0), F + 1, F + 1, F + 1)
    with pytest.raises(_lib.EngineError, match="MMPFN_XFORM_MAX_WIDTH"):
        eng.xform_upload(wide)
    for ops, ints, what in [
        ([[9, 4, 4, 0, 0, 0, 0, 0]], [0, 1, 2, 3], "op code"),
        ([[D.OP_GATHER, 4, 4, 0, 0, 0, 0, 0]], [0, 1, 2, 4], "gather index"),
        ([[D.OP_GATHER, 4, 4, 0, 0, 0, 0, 0]], [0, 1, 2], "past the int blob"),
        ([[D.OP_GATHER, 3, 4, 0, 0, 0, 0, 0]], [0, 1, 2, 2], "predecessor"),
        ([[D.OP_MAP, 4, 1, 0, 0, 0, 0, 0]], [0, 7, 0, 0, 0], "map kind"),
        ([[D.OP_MAP, 4, 1, 0, 0, 0, 0, 0]], [0, D.K_QUANTILE, 0, 3, 0], "quantiles past"),
        ([[D.OP_SVD, 4, 3, 0, 0, 2, 2, 1]], [], "svd components"),
    ]:
        bad = D.MemberProgram(np.array(ops, np.int32), np.array(ints, np.int32), np.zeros(1), 4, 4, 4)
        with pytest.raises(_lib.EngineError, match=what):
            eng.xform_upload(bad)
    good = D.MemberProgram(np.array([[D.OP_GATHER, 4, 4, 0, 0, 0, 0, 0]], np.int32), np.array([3, 2, 1, 0], np.int32),
                           np.zeros(0), 4, 4, 4)
    x = torch.arange(8, dtype=torch.float32, device="cuda").reshape(2, 4)
    assert torch.equal(eng.member_transform(good, x), x.flip(1))
    with pytest.raises(ValueError, match="takes"):
        eng.member_transform(good, x[:, :3])
    with pytest.raises(TypeError):
        eng.member_transform(good, x.to(torch.int32))


def test_tap_infinity_raises_at_status_and_the_context_recovers():
    eng = _engine()
    pipe, X, T = C.fitted("subsample", "c21", 200, 65, "shuffle", True)
    prog, _ = D.compile_member(pipe, X.shape[1], probe=X)
    want = C.host_reference(pipe, T)
    for bad in (np.inf, -np.inf):
        Tb = np.array(T)
        Tb[40, 19] = bad
        eng.member_transform(prog, torch.from_numpy(Tb).cuda())
        with pytest.raises(ValueError, match="Input X contains infinity"):
            eng.status()
        eng.status()  # reported once
        _, got = eng.member_transform(prog, torch.from_numpy(np.array(T)).cuda(), want64=True)
        eng.status()
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))


# ----------------------------------------------------------------------------- end to end, fp32 mode


def _fit_clf(name, tmp_path, fingerprint=True, **over):
    case = dict(_case(name))
    if not fingerprint:
        case["interface"] = dict(case.get("interface", {}), FINGERPRINT_FEATURE=False)
    d = case_data(case)
    clf = make_classifier(case, write_ckpt(case, tmp_path), inference_precision=torch.float32, **over)
    clf.fit(d["X_train"], d["image_train"], d["y_train"])
    return clf, d


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_run_config_is_bit_equal(tmp_path):
    """run.py's config (no preprocessing, categorical columns through the front encoder): every op is exact, so the
    two routes give the same probabilities bit for bit; every member has a program."""
    clf, d = _fit_clf("pad_none", tmp_path)
    assert all(p is not None for p in clf.executor_.device_programs), clf.executor_.program_reasons
    host = clf.predict_proba_device(d["X_test"], d["image_test"])
    dev = clf.predict_proba_device(_cuda(d["X_test"]), d["image_test"])
    assert torch.equal(host, dev)
    dev32 = clf.predict_proba_device(_cuda(d["X_test"].astype(np.float32)), d["image_test"])
    assert torch.equal(clf.predict_proba_device(d["X_test"].astype(np.float32), d["image_test"]), dev32)
    np.testing.assert_array_equal(clf.predict(_cuda(d["X_test"]), d["image_test"]),
                                  clf.predict(d["X_test"], d["image_test"]))


@pytest.mark.parametrize("fingerprint", [True, False], ids=["fp", "nofp"])
@pytest.mark.parametrize("fit_mode", ["fit_preprocessors", "fit_with_cache"])
def test_default_classifier_preprocessing(fit_mode, fingerprint, tmp_path):
    """Default preprocessing (quantile + SVD + shuffled ordinal members, raw members): probabilities within 1e-5
    absolute -- the ensemble bound of DESIGN.md 3 -- and equal labels.  With the fingerprint (the default) the SVD
    members keep the host transform, by name, and the raw members run on the device; without it every member does."""
    clf, d = _fit_clf("tab_default", tmp_path, fingerprint=fingerprint, fit_mode=fit_mode)
    ex = clf.executor_
    on_device = [p is not None for p in ex.device_programs]
    svd = [c.preprocess_config.global_transformer_name == "svd" for c in ex.ensemble_configs]
    assert any(svd) and not all(svd)
    if fingerprint:
        assert on_device == [not s for s in svd], ex.program_reasons
        assert all("after TruncatedSVD" in why for why, s in zip(ex.program_reasons, svd) if s)
    else:
        assert all(on_device), ex.program_reasons
    host = clf.predict_proba(d["X_test"], d["image_test"])
    dev = clf.predict_proba(_cuda(d["X_test"]), d["image_test"])
    diff = float(np.abs(host - dev).max())
    report(f"default classifier, {fit_mode}, fingerprint {fingerprint}: max |p(device X) - p(numpy X)| = {diff:.2e}")
    assert diff <= 1e-5
    np.testing.assert_array_equal(host.argmax(1), dev.argmax(1))
    np.testing.assert_array_equal(clf.predict(_cuda(d["X_test"]), d["image_test"]),
                                  clf.predict(d["X_test"], d["image_test"]))


def test_low_memory_takes_the_host_route(tmp_path):
    clf, d = _fit_clf("tab_default", tmp_path, fit_mode="low_memory")
    assert not clf.executor_.device_programs
    host = clf.predict_proba_device(d["X_test"], d["image_test"])
    assert torch.equal(host, clf.predict_proba_device(_cuda(d["X_test"]), d["image_test"]))


def test_tensor_x_errors(tmp_path):
    """The host path's error types: width, rank, another device; infinity at status time, after which the same
    estimator predicts; an estimator whose front encoder has no numeric plan says so."""
    clf, d = _fit_clf("tab_default", tmp_path)
    X = _cuda(d["X_test"])
    with pytest.raises(ValueError, match="features"):
        clf.predict_proba(X[:, :-1], None)
    with pytest.raises(ValueError, match="2D"):
        clf.predict_proba(X[0], None)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="lives on"):
            clf.predict_proba(X.to("cuda:1"), None)
    want = clf.predict_proba(d["X_test"], None)
    Xi = X.clone()
    Xi[3, 2] = float("inf")
    with pytest.raises(ValueError, match="Input X contains infinity"):
        clf.predict_proba(Xi, None)
    assert np.abs(clf.predict_proba(X, None) - want).max() <= 1e-5
    ints = clf.predict_proba(_cuda(np.rint(d["X_test"]).astype(np.int64)), None)  # the host takes integer tables too
    assert np.abs(ints - clf.predict_proba(np.rint(d["X_test"]).astype(np.int64), None)).max() <= 1e-5
    clf._ordinal_plan_ = None
    with pytest.raises(TypeError, match="front encoder"):
        clf.predict_proba(X, None)


@pytest.mark.parametrize("fingerprint", [True, False], ids=["fp", "nofp"])
def test_default_regressor(fingerprint, tmp_path):
    """The default regressor's preprocessing.  Its ``safepower`` / ``onehot`` members have no device form and transform
    the host copy; the ``quantile_uni`` + SVD members run on the device without the fingerprint (half the members
    fall back) and keep the host transform with it (all do: the default).  Members' logits between the two routes
    within the fp32 logit band of DESIGN.md 3 (1e-4 of max(1, max|ref|)), mean and quantiles within 2.4e-6 of the span
    of the criterion's inner borders (twice the smallest move that band gives them there); ``sample`` with a fixed
    ``random_state`` bit-equal when the members' logits are, else within that bound."""
    from multimodalpfn_amd import MMPFNRegressor

    case, z = api_case("b100")
    data = ro.api_case_data(case)
    path, _, _ = write_reg_ckpt(case, tmp_path)
    kw = ro.api_regressor_kwargs(case, case["variants"][0])
    if not fingerprint:
        kw["inference_config"] = {"FINGERPRINT_FEATURE": False}
    reg = MMPFNRegressor(model_path=str(path), **kw)
    reg.fit(data["X_train"], None, data["y_train"])
    progs, reasons = reg.executor_.device_programs, reg.executor_.program_reasons
    names = [c.preprocess_config.name for c in reg.executor_.ensemble_configs]
    assert sorted(set(names)) == ["quantile_uni", "safepower"]
    for p, why, name in zip(progs, reasons, names):
        if name == "safepower":
            assert p is None and "safepower" in why
        elif fingerprint:
            assert p is None and "after TruncatedSVD" in why
        else:
            assert p is not None, why
    X, Xd = data["X_test"], _cuda(data["X_test"])
    levels = [0.1, 0.5, 0.9]
    host, dev = reg.predict_device(X, None, quantiles=levels), reg.predict_device(Xd, None, quantiles=levels)
    span = float(z["crit_borders"][-2] - z["crit_borders"][1])
    lg = rel_err(dev["member_logits"].cpu().numpy(), host["member_logits"].cpu().numpy())
    dm = float((dev["mean"] - host["mean"]).abs().max()) / span
    dq = float((dev["quantiles"] - host["quantiles"]).abs().max()) / span
    same = torch.equal(dev["member_logits"], host["member_logits"])
    report(f"default regressor, fingerprint {fingerprint}, device X vs numpy X: member logits rel err {lg:.2e}, mean {dm:.2e} and quantiles "
           f"{dq:.2e} of the span; bit-equal logits: {same}")
    assert lg <= 1e-4 and dm <= 2.4e-6 and dq <= 2.4e-6
    np.testing.assert_allclose(reg.predict(Xd, None), reg.predict(X, None), rtol=0, atol=2.4e-6 * span)
    a, b = reg.sample(X, None, 50, random_state=7), reg.sample(Xd, None, 50, random_state=7)
    if same:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    else:
        np.testing.assert_allclose(b, a, rtol=0, atol=2.4e-6 * span)
    y = data["y_test"]
    for got, ref in ((reg.score_samples(Xd, None, y), reg.score_samples(X, None, y)),
                     (reg.acquisition(Xd, None, 1.0), reg.acquisition(X, None, 1.0)),
                     (reg.sample_device(Xd, None, 3, random_state=1).cpu().numpy(),
                      reg.sample_device(X, None, 3, random_state=1).cpu().numpy())):
        assert got.shape == ref.shape
        if same:
            assert np.array_equal(got, ref)
