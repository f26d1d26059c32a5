"""The member-preprocessing compiler and its numpy restatement against the host pipeline (no GPU).

``compile_member`` turns a fitted ``SequentialFeatureTransformer`` into the op list the kernel runs;
``run_program_host`` is that kernel's restatement.  Here every case of ``device_transform_cases.grid()`` is held, per
element and on the float64 output, against ``pipeline.transform(X).X``:

    gather, ordinal, fingerprint, guarded scaler    bit equality, NaN positions (and bits) included
    uniform quantile (values in [0, 1])             |err| <= 8 * 2^-53: three roundings per interpolation on either
                                                    side, two interpolations halved, one final rounding -- more is a
                                                    tie or bounds-semantics bug, not rounding
    SVD columns                                     |err| <= 2 (F + 2) 2^-53 sum |z| |c|: the any-order float64
                                                    summation bound, doubled (``modality_kernel_cases.py``'s form)

and ``out32`` is ``float32(out64)`` bit for bit.  The sensitivity tests move the restatement and record by how much the
bounds are then missed.
"""

from __future__ import annotations

import warnings

import numpy as np
import pytest

import device_transform_cases as C
from multimodalpfn_amd import device_transform as D
from multimodalpfn_amd.preprocessing import PreprocessorConfig


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def compiled(case):
    config, layout, n_train, n_test, shift, fp = case
    pipe, X, T = C.fitted(config, layout, n_train, n_test, shift, fp)
    prog, why = D.compile_member(pipe, X.shape[1], probe=X)
    assert prog is not None, why
    return prog, pipe, X, T


@pytest.mark.parametrize("case", C.grid(), ids=C.case_id)
def test_program_matches_host_pipeline(case):
    if C.stays_on_host(case):  # the one combination of the grid without a device form, refused by name
        config, layout, n_train, n_test, shift, fp = case
        pipe, X, _ = C.fitted(config, layout, n_train, n_test, shift, fp)
        prog, why = D.compile_member(pipe, X.shape[1], probe=X)
        assert prog is None and "after TruncatedSVD" in why, why
        return
    prog, pipe, X, T = compiled(case)
    want = C.host_reference(pipe, T)
    got, got32, bound = D.run_program_host(prog, T, return_bound=True)
    assert got.shape == want.shape == (len(T), prog.n_out)
    bad = D.mismatch(got, want, bound)
    worst = float(np.nanmax(np.abs(got - want))) if np.isfinite(got - want).any() else 0.0
    assert not bad.any(), (np.argwhere(bad)[:5].tolist(), worst)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got32), bits(got.astype(np.float32)))
    assert prog.width <= D.MAX_WIDTH and prog.ops[0, 1] == X.shape[1] and prog.ops[-1, 2] == prog.n_out


def test_grid_covers_the_ops_and_cells():
    """The grid reaches every op and map kind, programs with and without folding room, and the test rows hold the
    cells the restatement can get wrong."""
    codes, kinds = set(), set()
    for case in C.grid():
        if C.stays_on_host(case):
            continue
        prog = compiled(case)[0]
        codes |= set(prog.ops[:, 0].tolist())
        for code, _, w_out, ioff, *_ in prog.ops.tolist():
            if code == D.OP_MAP:
                kinds |= set(prog.ints[ioff + 1: ioff + D.MAP_INTS * w_out: D.MAP_INTS].tolist())
    assert codes == {D.OP_GATHER, D.OP_MAP, D.OP_SVD, D.OP_FINGERPRINT}
    assert kinds == {D.K_PASS, D.K_LOOKUP, D.K_QUANTILE, D.K_SCALE}
    X, T, cat_ix = C.make_tables("c21", 200, 7, 3)
    assert np.isnan(X[:, 0]).any() and np.unique(X[:, 18]).size == 5 and np.unique(X[:, 20]).size == 1
    assert np.isnan(T[0]).all() and (T[1] < np.nanmin(X, 0)).all() and (T[2] > np.nanmax(X, 0)).all()
    assert np.array_equal(T[3], np.nanmin(X, 0)) and np.array_equal(T[4], np.nanmax(X, 0)) and T[5, 18] == 0.5


def test_adjacent_gathers_fold():
    """run.py's members (constant removal, select_cols_, column shuffle) are one gather; with the fingerprint, one on
    either side of it."""
    pipe, X, _ = C.fitted("run_none", "c21", 200, 7, "shuffle", False)
    prog, _ = D.compile_member(pipe, X.shape[1])
    assert prog.ops[:, 0].tolist() == [D.OP_GATHER]
    pipe, X, _ = C.fitted("run_none", "c21", 200, 7, "shuffle", True)
    prog, _ = D.compile_member(pipe, X.shape[1])
    assert prog.ops[:, 0].tolist() == [D.OP_GATHER, D.OP_FINGERPRINT, D.OP_GATHER]


def test_front_encoder_matches_the_fitted_ordinal_encoder():
    """The estimators' front encoder as a program: the fitted ColumnTransformer's table bit for bit -- unseen -> -1,
    missing -> NaN where NaN was a fitted category and -1 where it was not -- and ``with_front`` folds it in."""
    from multimodalpfn_amd.utils import _fix_dtypes, _get_ordinal_encoder

    X, T, _ = C.make_tables("c21", 200, 65, 5)
    cat = [0, 1, 2, 5]
    enc = _get_ordinal_encoder()
    Xe = enc.fit_transform(_fix_dtypes(np.array(X), cat_indices=cat))
    plan = D.plan_front_encoder(enc)
    assert plan is not None and plan[0] == cat and np.isnan(plan[2][0]) and plan[2][1] == -1.0
    want = np.asarray(enc.transform(_fix_dtypes(np.array(T), cat_indices=cat)), np.float64)
    front = D._Builder(21)
    front.add(D.front_map(plan, 21))
    got, _ = D.run_program_host(D._finish(front), T)
    assert np.array_equal(bits(got), bits(want))
    assert (want[:, :4] == -1).any() and np.isnan(want[:, 0]).any() and not np.isnan(want[:, 1:4]).any()

    from multimodalpfn_amd.preprocessing import ClassifierEnsembleConfig, fit_preprocessing_one

    cfg = ClassifierEnsembleConfig(preprocess_config=C.CONFIGS["subsample"], add_fingerprint_feature=True,
                                   polynomial_features="no", feature_shift_count=2, feature_shift_decoder="shuffle",
                                   subsample_ix=None, class_permutation=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, pipe, _, _, _ = fit_preprocessing_one(cfg, Xe, np.arange(200) % 3, 4, cat_ix=[0, 1, 2, 3])
    member, why = D.compile_member(pipe, 21, probe=Xe)
    assert member is not None, why
    whole = D.with_front(member, plan)
    # both encoders look the same columns up, so the front map stays an op of its own (it folds into a gather)
    assert len(whole.ops) == len(member.ops) + 1 and whole.n_in == 21
    got, _ = D.run_program_host(whole, T)
    assert np.array_equal(bits(got), bits(C.host_reference(pipe, want)))


@pytest.mark.parametrize("config, poly, names", [
    (PreprocessorConfig("safepower", categorical_name="onehot"), "no", ("safepower",)),
    (PreprocessorConfig("none", categorical_name="onehot"), "no", ("onehot",)),
    (PreprocessorConfig("none"), 5, ("NanHandlingPolynomialFeaturesStep",)),
    (PreprocessorConfig("quantile_norm"), "no", ("quantile_norm",)),
    (PreprocessorConfig("robust"), "no", ("robust",)),
])
def test_steps_without_a_device_form_are_refused_by_name(config, poly, names, monkeypatch):
    monkeypatch.setitem(C.CONFIGS, "refused", config)
    pipe, X, _ = C.fitted("refused", "c21", 200, 7, "shuffle", True, poly)
    C.fitted.cache_clear()
    prog, why = D.compile_member(pipe, X.shape[1], probe=X)
    assert prog is None and all(n in why for n in names), why


def test_width_limit():
    """A row of MAX_WIDTH doubles is the widest the kernel holds (two of them are a block's 64 KiB of LDS): a program
    at the limit compiles, one past it is refused."""
    from multimodalpfn_amd.model.preprocessing import SequentialFeatureTransformer, ShuffleFeaturesStep

    for F, ok in ((D.MAX_WIDTH, True), (D.MAX_WIDTH + 1, False)):
        pipe = SequentialFeatureTransformer([ShuffleFeaturesStep("shuffle", 0, 3)])
        X = np.random.default_rng(0).standard_normal((3, F))
        pipe.fit(X, [])
        prog, why = D.compile_member(pipe, F, probe=X)
        assert (prog is not None) == ok, why
        if not ok:
            assert str(D.MAX_WIDTH) in why
    assert D.rows_per_block(D.MAX_WIDTH) == 1 and D.rows_per_block(513) == 7 and D.rows_per_block(48) == D.MAX_ROWS


def _first_map_col(prog, kind):
    for code, _, w_out, ioff, *_ in prog.ops.tolist():
        if code == D.OP_MAP:
            for j in range(w_out):
                c = prog.ints[ioff + D.MAP_INTS * j: ioff + D.MAP_INTS * (j + 1)]
                if c[1] == kind and c[3] >= 3:
                    return c
    raise AssertionError("no such column")


def test_probe_check_rejects_damaged_programs():
    case = ("clf_default_0", "c21", 200, 7, "shuffle", False)
    prog, pipe, X, _ = compiled(case)
    assert D.probe_check(prog, pipe, X) == ""
    # two quantiles exchanged (a continuous column: distinct values)
    bad = D.MemberProgram(prog.ops, prog.ints, prog.doubles.copy(), prog.n_in, prog.n_out, prog.width)
    for code, _, w_out, ioff, *_ in prog.ops.tolist():
        if code != D.OP_MAP:
            continue
        for j in range(w_out):
            _, kind, off, n, _ = prog.ints[ioff + D.MAP_INTS * j: ioff + D.MAP_INTS * (j + 1)].tolist()
            if kind == D.K_QUANTILE and np.unique(prog.doubles[off: off + n]).size == n:
                bad.doubles[[off + n // 2, off + n // 2 + 1]] = bad.doubles[[off + n // 2 + 1, off + n // 2]]
                break
    assert not np.array_equal(bad.doubles, prog.doubles)
    assert "probe check" in D.probe_check(bad, pipe, X)
    # a category permutation shifted by one
    bad = D.MemberProgram(prog.ops, prog.ints, prog.doubles.copy(), prog.n_in, prog.n_out, prog.width)
    _, _, off, n, _ = _first_map_col(prog, D.K_LOOKUP).tolist()
    bad.doubles[off + 2 + n: off + 2 + 2 * n] = np.roll(prog.doubles[off + 2 + n: off + 2 + 2 * n], 1)
    assert "probe check" in D.probe_check(bad, pipe, X)


def test_a_disagreeing_program_is_dropped_with_a_warning(monkeypatch):
    """A scikit-learn whose fitted state means something else (here: an interpolation that is not np.interp's) leaves
    the member on the host, loudly."""
    pipe, X, _ = C.fitted("clf_default_0", "c21", 200, 7, "shuffle", False)
    real = D._quantile
    monkeypatch.setattr(D, "_quantile", lambda x, q, r, tie_first=False: real(x, q, r, tie_first) * (1 - 1e-9))
    with pytest.warns(RuntimeWarning, match="stays on the host"):
        prog, why = D.compile_member(pipe, X.shape[1], probe=X)
    assert prog is None and "probe check" in why


def test_host_adder_quiets_a_nan_and_keeps_its_bits():
    """What ``(X + salt) + salt`` makes of a NaN cell on the host, which the kernel writes out explicitly instead of
    trusting its adder: sign and payload kept, quiet bit set.  And float32 -> float64 of a NaN: the same, payload
    shifted up -- how a float32 device table's NaNs reach the hash."""
    pats = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FF4000000001234,
                     0xFFF0000000000001], dtype=np.uint64)
    x = np.tile(pats, 3).view(np.float64)
    with np.errstate(invalid="ignore"):
        y = (x + 40000) + 40000
    assert np.array_equal(bits(y), bits(x) | np.uint64(1 << 51))
    assert np.array_equal(bits(D.salted_twice(x, 40000.0)), bits(y))
    p32 = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFF801234], dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        w = p32.view(np.float32).astype(np.float64)
    want = ((p32.astype(np.uint64) >> np.uint64(31)) << np.uint64(63)) | np.uint64(0x7FF8000000000000) \
        | ((p32.astype(np.uint64) & np.uint64(0x7FFFFF)) << np.uint64(29))
    assert np.array_equal(bits(w), want)
    with np.errstate(invalid="ignore"):
        n32 = x.astype(np.float32)  # and back down, the final rounding of a NaN output
    want32 = ((bits(x) >> np.uint64(63)) << np.uint64(31)).astype(np.uint32) | np.uint32(0x7FC00000) \
        | ((bits(x) >> np.uint64(29)) & np.uint64(0x3FFFFF)).astype(np.uint32)
    assert np.array_equal(bits(n32), want32)


# ----------------------------------------------------------------------------- sensitivity: moves of the restatement


def test_sensitivity_tie_index():
    """The first instead of the last index of a tie run (np.interp takes the last): the few-valued column's exact hits
    land on the other end of their run.  Recorded: the largest miss is 0.1-0.4 of the unit interval, 1e14 bounds."""
    prog, pipe, X, T = compiled(("reg_default_0", "c21", 200, 7, None, False))
    want = C.host_reference(pipe, T)
    got, _, bound = D.run_program_host(prog, T, return_bound=True, variant="tie_first")
    q = bound == D.QUANTILE_BOUND
    miss = np.nanmax(np.abs(got - want)[q])
    print(f"tie_first: worst quantile miss {miss:.3g} = {miss / D.QUANTILE_BOUND:.3g} bounds")
    assert miss > 1e6 * D.QUANTILE_BOUND


def test_sensitivity_single_salt():
    """Hashing ``X + salt`` instead of ``(X + salt) + salt``: every row's fingerprint is another number of [0, 1)
    (bound: bit equality).  Recorded: all 64 rows with a number in them differ (the row of NaNs hashes the same bits
    either way), by 0.29 on average."""
    prog, pipe, X, T = compiled(("clf_default_1", "c21", 200, 65, None, True))
    want = C.host_reference(pipe, T)
    got, _ = D.run_program_host(prog, T, variant="single_salt")
    moved = bits(got) != bits(want)
    cols = np.where(moved.any(0))[0]
    print(f"single_salt: {moved.sum()} cells differ, columns {cols.tolist()}, mean |diff| "
          f"{np.abs(got - want)[moved].mean():.3g}")
    assert len(cols) == 1 and moved[1:, cols[0]].all() and np.abs(got - want)[moved].mean() > 0.05


def test_sensitivity_svd_components():
    """Two SVD components exchanged: their two output columns trade places.  Recorded: the largest miss is of the
    size of the projections themselves, 1e13 and more of its bound."""
    prog, pipe, X, T = compiled(("clf_default_0", "c21", 200, 65, None, False))
    want = C.host_reference(pipe, T)
    got, _, bound = D.run_program_host(prog, T, return_bound=True, variant="svd_swap")
    svd = (bound > 0) & (bound != D.QUANTILE_BOUND)
    ratio = np.max(np.abs(got - want)[svd] / bound[svd])
    print(f"svd_swap: worst miss {np.max(np.abs(got - want)[svd]):.3g} = {ratio:.3g} bounds")
    assert svd.any(0).sum() >= 2 and ratio > 1e6
