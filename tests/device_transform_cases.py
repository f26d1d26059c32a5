"""Seeded tables, member configs and fitted pipelines shared by ``test_device_transform.py`` (the compiler and its numpy
restatement against the host pipeline) and ``test_device_transform_gpu.py`` (the kernel on the same programs).

A case is (config, column layout, train rows, test rows).  The layouts: ``n1`` one numeric column (the SVD is skipped
for ``n_features < 2``), ``n2`` two numeric columns, ``c21`` config C's 21 columns of which 18 categorical, ``w140`` 140
columns of which 20 categorical.  Where the layout has room the train table holds a numeric column with 5 distinct
values (its fitted quantiles are runs of ties), a categorical column with NaN among its train values, and a column
constant on the train rows.  The test rows start with: a row of NaNs; a row of unseen categories and values below every
fitted minimum; one above every maximum; the column minima; the maxima; and a row of train values of the few-valued
column (exact hits on interior quantiles inside a tie run); random rows with NaNs sprinkled in follow.  With one test
row that row mixes those cells column by column.
"""

from __future__ import annotations

import functools
import warnings

import numpy as np

from multimodalpfn_amd.preprocessing import ClassifierEnsembleConfig, PreprocessorConfig, fit_preprocessing_one

LAYOUTS = {"n1": (1, 0), "n2": (2, 0), "c21": (21, 18), "w140": (140, 20)}  # name -> (columns, categorical)

CONFIGS = {
    "clf_default_0": PreprocessorConfig("quantile_uni_coarse", append_original=True,
                                        categorical_name="ordinal_very_common_categories_shuffled",
                                        global_transformer_name="svd"),
    "clf_default_1": PreprocessorConfig("none", categorical_name="numeric"),
    "run_none": PreprocessorConfig("none"),
    "reg_default_0": PreprocessorConfig("quantile_uni", append_original=True,
                                        categorical_name="ordinal_very_common_categories_shuffled",
                                        global_transformer_name="svd"),
    "scaler": PreprocessorConfig("none", categorical_name="ordinal", global_transformer_name="scaler"),
    "subsample": PreprocessorConfig("quantile_uni_fine", categorical_name="ordinal_shuffled", subsample_features=0.7),
}
SHIFTS = ["rotate", "shuffle", None]


def make_tables(layout: str, n_train: int, n_test: int, seed: int):
    """``(X_train, X_test, cat_ix)`` in the members' input space (categorical columns hold ordinal codes)."""
    F, n_cat = LAYOUTS[layout]
    g = np.random.default_rng(seed)
    X = g.standard_normal((n_train, F)) * (1.0 + np.arange(F) % 3)
    for c in range(n_cat):
        X[:, c] = g.integers(0, 2 + c % 5, n_train)
    few = const = None
    if F - n_cat >= 2:
        few = n_cat  # the first numeric column: 5 distinct values
        X[:, few] = g.integers(0, 5, n_train) * 0.5 - 1.0
    if n_cat:
        X[g.random(n_train) < 0.2, 0] = np.nan  # NaN is a fitted category of column 0
    if F >= 4:
        const = F - 1
        X[:, const] = 3.25
    lo, hi = np.nanmin(X, 0), np.nanmax(X, 0)
    special = np.stack([np.full(F, np.nan), lo - 7.5, hi + 7.5, lo, hi, X[n_train // 2]])
    if few is not None:
        special[5, few] = 0.5  # an interior value of the tie runs
    rows = g.standard_normal((max(n_test, 6), F)) * 2.0
    for c in range(n_cat):
        rows[:, c] = g.integers(-1, 3 + c % 5, len(rows))  # codes seen, the front encoder's -1, and one beyond
    rows[g.random(rows.shape) < 0.1] = np.nan
    if n_test == 1:
        T = np.array([special[c % 6, c] for c in range(F)])[None, :]
    else:
        T = np.concatenate([special[:min(6, n_test)], rows[:max(0, n_test - 6)]])
    return X, T, list(range(n_cat))


@functools.lru_cache(maxsize=None)
def fitted(config: str, layout: str, n_train: int, n_test: int, shift, fingerprint: bool, poly="no"):
    """``(pipeline, X_train, X_test)``: the member fitted as ``fit_preprocessing_one`` fits it.  Shared and read-only."""
    X, T, cat_ix = make_tables(layout, n_train, n_test, seed=n_train + 7 * n_test + len(layout))
    y = np.random.default_rng(1).integers(0, 3, n_train)
    cfg = ClassifierEnsembleConfig(preprocess_config=CONFIGS[config], add_fingerprint_feature=fingerprint,
                                   polynomial_features=poly, feature_shift_count=5, feature_shift_decoder=shift,
                                   subsample_ix=None, class_permutation=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # sklearn's n_quantiles > n_samples note on the 30-row tables
        _, pipe, _, _, _ = fit_preprocessing_one(cfg, X, y, 11, cat_ix=cat_ix)
    X.setflags(write=False)
    T.setflags(write=False)
    return pipe, X, T


def host_reference(pipe, T):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.ascontiguousarray(pipe.transform(np.array(T)).X, dtype=np.float64)


def grid():
    """The cases: every config on every layout, the train / test sizes, shifts and the fingerprint cycling so that
    each value meets each config; train rows 30 / 200 / 1838, test rows 1 / 7 / 65."""
    out = []
    k = 0
    for config in CONFIGS:
        for layout in LAYOUTS:
            for n_train in (30, 200, 1838):
                if n_train == 1838 and layout == "w140" and config not in ("clf_default_0", "run_none"):
                    continue  # the widest fits: once with every op, once as a pure gather
                out.append((config, layout, n_train, (1, 7, 65)[k % 3], SHIFTS[(k // 3) % 3], k % 2 == 0))
                k += 1
    return out


def stays_on_host(case) -> bool:
    """The fingerprint behind an SVD: the compiler refuses the member (``device_transform._Builder.add``).  One
    column has no SVD (``n_features < 2``)."""
    config, layout, _, _, _, fp = case
    return layout != "n1" and fp and CONFIGS[config].global_transformer_name == "svd"


def case_id(case) -> str:
    config, layout, n_train, n_test, shift, fp = case
    return f"{config}-{layout}-{n_train}x{n_test}-{shift}-{'fp' if fp else 'nofp'}"
