"""A fitted member pipeline as a small program the device can run (``mmpfn_member_transform``).

``compile_member`` reads the *fitted state* of a ``SequentialFeatureTransformer`` (``model/preprocessing.py``; the
steps ``preprocessing.py:416-473`` chains) and writes the test-row transform as a flat list of ops over one working
row, plus an int and a double parameter blob.  ``run_program_host`` interprets that list in plain numpy: it is the
kernel's restatement (``csrc/xform.hip`` runs the same ops in the same order of roundings) and what the CPU tests
hold against ``pipeline.transform``.  Nothing here needs a GPU.

Ops (``ops`` is ``int32 [n_ops, 8]``: code, width in, width out, int offset, double offset, a, b, c):

``OP_GATHER``       ``out[j] = in[ints[ioff + j]]``.  Constant removal, feature sub-sampling, ``select_cols_``, the
                    ColumnTransformers' column orders, ``append_original``, the FeatureUnion's concatenation and the
                    column shuffle are all gathers; adjacent ones are folded.
``OP_MAP``          ``out[j] = f_j(in[src_j])``, five ints per column (src, kind, double offset, n, aux):
                    ``K_PASS``; ``K_LOOKUP`` (doubles ``[unseen, miss, cats[n], values[n]]``: exact match in the sorted
                    categories -> its value, no match -> unseen, NaN -> miss; the estimators' front encoder and the
                    members' ordinal re-encoding with its shuffle); ``K_QUANTILE`` (doubles ``quantiles[n]``, aux the
                    offset of ``references[n]``: sklearn's uniform ``QuantileTransformer._transform_col``);
                    ``K_SCALE`` (doubles ``[pre, mean, scale, post]``: inf -> NaN -> pre, ``(x - mean) / scale``,
                    inf -> NaN -> post: ``make_standard_scaler_safe``).  A map whose source columns all come out
                    of a gather or pass through an earlier map is folded into it.
``OP_SVD``          ``out[:a] = in[:a]``; ``out[a + j] = sum_i in[a + i] * comps[j, i]``, ``i`` ascending from 0,
                    product and sum rounded separately (b inputs, c components, doubles ``comps[c, b]``).
``OP_FINGERPRINT``  ``out = [in, h]``: SipHash-2-4 (``_siphash.py``) of the row's float64 bytes of ``(in + salt) +
                    salt``, ``mod 10**12 / 10**12``.  A NaN cell keeps its sign and payload and gets the quiet bit,
                    which is what the host's adder makes of it (checked in ``tests/test_device_transform.py``).

The widest row of a program (input, output and every intermediate) may hold ``MAX_WIDTH`` = 4096 doubles: the kernel
keeps the working row of each of its rows in LDS twice (ping-pong), and two rows of 4096 doubles are the 64 KiB a
block gets without asking for more.  ``compile_member`` refuses wider programs.
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np

OP_GATHER, OP_MAP, OP_SVD, OP_FINGERPRINT = 1, 2, 3, 4
K_PASS, K_LOOKUP, K_QUANTILE, K_SCALE = 0, 1, 2, 3
OP_INTS = 8      # ints of one op header
MAP_INTS = 5     # ints of one OP_MAP column
MAX_WIDTH = 4096  # doubles of the widest row: 2 buffers x 4096 x 8 B = 64 KiB of LDS at one row per block
MAX_ROWS = 8     # rows per block at most (kXformMaxRows); rows_per_block() is the kernel's choice
_EPS = 2.0 ** -53
QUANTILE_BOUND = 8 * _EPS  # three roundings per interpolation, two interpolations halved, one final rounding
_FP_MOD = 10 ** 12
_QUIET = np.uint64(1 << 51)


def rows_per_block(width: int) -> int:
    """Rows one block of the kernel transforms: as many as fit two ``width``-double rows each into 64 KiB, 8 at most."""
    return max(1, min(MAX_ROWS, MAX_WIDTH // max(1, int(width))))


@dataclass
class MemberProgram:
    ops: np.ndarray      # int32 [n_ops, OP_INTS]
    ints: np.ndarray     # int32
    doubles: np.ndarray  # float64
    n_in: int
    n_out: int
    width: int           # the widest row
    _handles: dict = field(default_factory=dict, repr=False, compare=False)  # device copies, by engine serial
    _sym: list = field(default_factory=list, repr=False, compare=False)  # the ops before serialising (with_front)


# ----------------------------------------------------------------------------- symbolic ops


@dataclass
class _Col:
    src: int
    kind: int = K_PASS
    a: np.ndarray | None = None  # LOOKUP: cats; QUANTILE: quantiles; SCALE: [pre, mean, scale, post]
    b: np.ndarray | None = None  # LOOKUP: values; QUANTILE: references
    unseen: float = np.nan
    miss: float = np.nan


@dataclass
class _Map:
    cols: list


@dataclass
class _Svd:
    n_pass: int
    comps: np.ndarray  # [k, F]


@dataclass
class _Fingerprint:
    salt: float


class _NoDeviceForm(Exception):
    pass


def _gather(idx) -> _Map:
    return _Map([_Col(int(i)) for i in np.asarray(idx).reshape(-1)])


def _fold(a: _Map, b: _Map) -> _Map | None:
    """``b`` after ``a`` as one map, if no column is transformed by both."""
    cols = []
    for cb in b.cols:
        ca = a.cols[cb.src]
        if cb.kind == K_PASS:
            cols.append(ca)
        elif ca.kind == K_PASS:
            cols.append(_Col(ca.src, cb.kind, cb.a, cb.b, cb.unseen, cb.miss))
        else:
            return None
    return _Map(cols)


class _Builder:
    def __init__(self, n_in: int):
        self.n_in = int(n_in)
        self.width = int(n_in)
        self.ops: list = []

    def add(self, op) -> None:
        if isinstance(op, _Map):
            for c in op.cols:
                if not 0 <= c.src < self.width:
                    raise _NoDeviceForm(f"a column index {c.src} outside the {self.width} columns of its input")
            if self.ops and isinstance(self.ops[-1], _Map):
                folded = _fold(self.ops[-1], op)
                if folded is not None:
                    self.ops[-1] = folded
                    self.width = len(op.cols)
                    return
            self.width = len(op.cols)
        elif isinstance(op, _Svd):
            if op.n_pass + op.comps.shape[1] != self.width:
                raise _NoDeviceForm("TruncatedSVD: components_ do not fit the scaled table")
            self.width = op.n_pass + op.comps.shape[0]
        else:
            # the hash reads every bit of the row, and the host's projection z @ components_.T has no restatement
            # to the bit: numpy sums it in its own loop (the SVD op's order) or hands it to BLAS, by the operands'
            # shapes and strides, and one last bit of one SVD column is another fingerprint.  Within the SVD bound
            # that is nothing; behind the hash the member keeps the host transform.
            if any(isinstance(o, _Svd) for o in self.ops):
                raise _NoDeviceForm("AddFingerprintFeaturesStep after TruncatedSVD (the hash reads every bit of a "
                                    "projection whose summation order on the host depends on BLAS)")
            self.width += 1
        self.ops.append(op)


# ----------------------------------------------------------------------------- reading the fitted state


def _is_passthrough(t) -> bool:
    from sklearn.preprocessing import FunctionTransformer

    from multimodalpfn_amd.model.preprocessing import _identity

    if isinstance(t, str):
        return t == "passthrough"
    return isinstance(t, FunctionTransformer) and (t.func is None or t.func is _identity)


def _guarded_scaler_cols(pipe, n: int, src0: int) -> list:
    """``make_standard_scaler_safe``'s five fitted steps over columns ``src0 .. src0 + n`` as K_SCALE columns."""
    from sklearn.impute import SimpleImputer
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import FunctionTransformer, StandardScaler

    from multimodalpfn_amd.model.preprocessing import _inf_to_nan_func

    steps = [s for _, s in pipe.steps] if isinstance(pipe, Pipeline) else []
    kinds = (FunctionTransformer, SimpleImputer, StandardScaler, FunctionTransformer, SimpleImputer)
    if len(steps) != 5 or not all(isinstance(s, k) for s, k in zip(steps, kinds)) \
            or steps[0].func is not _inf_to_nan_func or steps[3].func is not _inf_to_nan_func:
        raise _NoDeviceForm(f"{type(pipe).__name__}: not the guarded scaler")
    pre_i, sc, post_i = steps[1], steps[2], steps[4]
    if pre_i.strategy != "mean" or post_i.strategy != "mean" or not sc.with_std:
        raise _NoDeviceForm("guarded scaler: an imputer or scaler setting without a device form")
    pre = np.asarray(pre_i.statistics_, np.float64)
    post = np.asarray(post_i.statistics_, np.float64)
    scale = np.asarray(sc.scale_, np.float64)
    mean = np.asarray(sc.mean_, np.float64) if sc.with_mean else np.zeros(n)
    if not (len(pre) == len(post) == len(scale) == len(mean) == n):
        raise _NoDeviceForm("guarded scaler: fitted state of another width")
    return [_Col(src0 + j, K_SCALE, np.array([pre[j], mean[j], scale[j], post[j]])) for j in range(n)]


def _column_transformer_map(ct, width: int, per_transformer) -> _Map:
    """The fitted ColumnTransformer's output columns: ``per_transformer(name, trans, cols)`` gives the _Col list of
    one entry, placed at ``output_indices_[name]``."""
    n_out = max((s.stop for s in ct.output_indices_.values()), default=0)
    out: list = [None] * n_out
    for name, trans, cols in ct.transformers_:
        sl = ct.output_indices_[name]
        if sl.stop - sl.start == 0:
            continue
        cols = [int(c) for c in np.atleast_1d(np.asarray(cols))] if not isinstance(cols, slice) \
            else list(range(width))[cols]
        if isinstance(trans, str) and trans == "drop":
            raise _NoDeviceForm("ColumnTransformer: a dropped entry with output columns")
        made = per_transformer(name, trans, cols)
        if len(made) != sl.stop - sl.start:
            raise _NoDeviceForm(f"{type(trans).__name__}: changes the number of columns")
        out[sl] = made
    if any(c is None for c in out):
        raise _NoDeviceForm("ColumnTransformer: output columns without a transformer")
    return _Map(out)


def _reshape_step(b: _Builder, step) -> None:
    from sklearn.compose import ColumnTransformer
    from sklearn.decomposition import TruncatedSVD
    from sklearn.pipeline import FeatureUnion, Pipeline
    from sklearn.preprocessing import QuantileTransformer

    sel = getattr(step, "select_cols_", None)
    if sel is not None:
        b.add(_gather(sel))
        return
    b.add(_gather(step.subsampled_features_))
    tf = step.transformer_
    ct, glob = (tf.steps[0][1], tf.steps[1][1]) if isinstance(tf, Pipeline) else (tf, None)
    if not isinstance(ct, ColumnTransformer):
        raise _NoDeviceForm(f"{type(ct).__name__} in place of the ColumnTransformer")

    def per(name, trans, cols):
        if _is_passthrough(trans):
            return [_Col(c) for c in cols]
        if isinstance(trans, QuantileTransformer) and trans.output_distribution == "uniform":
            q = np.asarray(trans.quantiles_, np.float64)
            refs = np.asarray(trans.references_, np.float64)
            if q.shape != (len(refs), len(cols)) or len(refs) < 1:
                raise _NoDeviceForm("QuantileTransformer: fitted state of another shape")
            return [_Col(c, K_QUANTILE, np.ascontiguousarray(q[:, k]), refs) for k, c in enumerate(cols)]
        raise _NoDeviceForm(f"{step.transform_name} ({type(trans).__name__})")

    b.add(_column_transformer_map(ct, b.width, per))
    if glob is None:
        return
    w = b.width
    if isinstance(glob, FeatureUnion):
        parts = [t for _, t in glob.transformer_list]
        if len(parts) != 2 or not _is_passthrough(parts[0]) or not isinstance(parts[1], Pipeline) \
                or len(parts[1].steps) != 2 or not isinstance(parts[1].steps[1][1], TruncatedSVD):
            raise _NoDeviceForm("FeatureUnion: not passthrough + scaled TruncatedSVD")
        b.add(_Map([_Col(j) for j in range(w)] + _guarded_scaler_cols(parts[1].steps[0][1], w, 0)))
        b.add(_Svd(w, np.ascontiguousarray(parts[1].steps[1][1].components_, dtype=np.float64)))
    else:
        b.add(_Map(_guarded_scaler_cols(glob, w, 0)))


def _encode_step(b: _Builder, step) -> None:
    from sklearn.preprocessing import OrdinalEncoder

    ct = step.categorical_transformer_
    if ct is None:
        return
    name = step.categorical_transform_name
    if not name.startswith("ordinal"):
        raise _NoDeviceForm(name)
    maps = getattr(step, "random_mappings_", {}) if name.endswith("_shuffled") else {}

    def per(tname, trans, cols):
        if _is_passthrough(trans):
            return [_Col(c) for c in cols]
        if not isinstance(trans, OrdinalEncoder) or trans.handle_unknown != "use_encoded_value":
            raise _NoDeviceForm(f"{name} ({type(trans).__name__})")
        made = []
        for k, c in enumerate(cols):
            cats = np.asarray(trans.categories_[k], np.float64)
            values = np.arange(len(cats), dtype=np.float64)
            if k in maps:
                values = np.asarray(maps[k], np.float64)[: len(cats)]
            keep = ~np.isnan(cats)  # a fitted NaN category sits last; a NaN cell encodes as NaN either way
            cats, values = cats[keep], values[keep]
            if np.any(np.diff(cats) <= 0):
                raise _NoDeviceForm("OrdinalEncoder: categories_ not sorted")
            made.append(_Col(c, K_LOOKUP, cats, values, float(trans.unknown_value),
                             float(trans.encoded_missing_value)))
        return made

    b.add(_column_transformer_map(ct, b.width, per))


def front_map(plan, n_in: int) -> _Map:
    """The estimators' front encoder (``_encode_predict_X``'s ``_ordinal_plan_``) as one map: encoded columns
    first (unseen -> -1, missing -> NaN if it was a fitted category, else -1), then the remainder in order."""
    cols, cats, miss, _lut, rem = plan
    made = [_Col(int(c), K_LOOKUP, np.asarray(cat, np.float64), np.arange(len(cat), dtype=np.float64), -1.0, float(m))
            for c, cat, m in zip(cols, cats, miss)]
    made += [_Col(int(c)) for c in rem]
    if any(not 0 <= c.src < n_in for c in made):
        raise _NoDeviceForm("front encoder: a column outside the table")
    return _Map(made)


def plan_front_encoder(enc):
    """The fitted front encoder's column plan ``(cols, cats, miss, None, rem)`` for numeric tables, or None."""
    ts = [(n, t, c) for n, t, c in enc.transformers_ if not (n == "remainder" and isinstance(t, str) and t == "drop")]
    if not ts or ts[0][0] != "encoder" or any(n not in ("encoder", "remainder") for n, _, _ in ts):
        return None
    cols = [int(c) for c in ts[0][2]]
    oe = ts[0][1]
    if len(cols) and not hasattr(oe, "categories_"):
        return None
    cats, miss = [], []
    for c in (oe.categories_ if len(cols) else []):
        c = np.asarray(c)
        if c.dtype.kind not in "biuf":
            return None
        c = c.astype(np.float64)
        miss.append(np.nan if np.isnan(c).any() else -1.0)
        cats.append(np.sort(c[~np.isnan(c)]))
    rem = [int(c) for c in ts[1][2]] if len(ts) > 1 else []
    return cols, cats, np.asarray(miss, np.float64), None, rem


# ----------------------------------------------------------------------------- serialising


def _serialise(b: _Builder) -> MemberProgram:
    ops, ints, dbl = [], [], []
    n_d = 0
    shared: dict = {}

    def put(a) -> int:
        nonlocal n_d
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        off = n_d
        dbl.append(a)
        n_d += a.size
        return off

    width, widest = b.n_in, b.n_in
    for op in b.ops:
        ioff, doff = len(ints), n_d
        if isinstance(op, _Map):
            w_out = len(op.cols)
            if all(c.kind == K_PASS for c in op.cols):
                ints += [c.src for c in op.cols]
                ops.append([OP_GATHER, width, w_out, ioff, doff, 0, 0, 0])
            else:
                for c in op.cols:
                    if c.kind == K_PASS:
                        ints += [c.src, K_PASS, 0, 0, 0]
                    elif c.kind == K_LOOKUP:
                        off = put(np.concatenate([[c.unseen, c.miss], c.a, c.b]))
                        ints += [c.src, K_LOOKUP, off, len(c.a), 0]
                    elif c.kind == K_QUANTILE:
                        if id(c.b) not in shared:
                            shared[id(c.b)] = put(c.b)
                        ints += [c.src, K_QUANTILE, put(c.a), len(c.a), shared[id(c.b)]]
                    else:
                        ints += [c.src, K_SCALE, put(c.a), 4, 0]
                ops.append([OP_MAP, width, w_out, ioff, doff, 0, 0, 0])
        elif isinstance(op, _Svd):
            k, f = op.comps.shape
            w_out = op.n_pass + k
            ops.append([OP_SVD, width, w_out, ioff, put(op.comps), op.n_pass, f, k])
        else:
            w_out = width + 1
            ops.append([OP_FINGERPRINT, width, w_out, ioff, put([op.salt]), 0, 0, 0])
        width = w_out
        widest = max(widest, width)
    return MemberProgram(ops=np.asarray(ops, np.int32).reshape(-1, OP_INTS), ints=np.asarray(ints, np.int32),
                         doubles=np.concatenate(dbl) if dbl else np.zeros(0), n_in=b.n_in, n_out=width, width=widest)


# ----------------------------------------------------------------------------- the compiler


def compile_member(pipeline, n_in: int, *, front=None, probe=None):
    """``(program, "")``, or ``(None, reason)`` when a fitted step has no device form.

    ``pipeline``: a fitted ``SequentialFeatureTransformer`` over ``n_in`` columns.  ``front``: the estimator's
    ``_ordinal_plan_``, prepended (the program then takes the raw table).  ``probe``: train rows in the pipeline's
    input space; the program's member part is run on their first rows, a row of NaNs and two rows of unseen /
    out-of-range values and held against ``pipeline.transform`` under ``run_program_host``'s bounds -- a program
    that disagrees is dropped with a ``RuntimeWarning`` (a scikit-learn whose fitted state means something else
    must not produce wrong tables silently)."""
    from multimodalpfn_amd.model import preprocessing as P

    try:
        member = _Builder(n_in)
        for step in pipeline:
            if isinstance(step, P.RemoveConstantFeaturesStep):
                member.add(_gather(np.where(np.asarray(step.sel_, bool))[0]))
            elif isinstance(step, P.ReshapeFeatureDistributionsStep):
                _reshape_step(member, step)
            elif isinstance(step, P.EncodeCategoricalFeaturesStep):
                _encode_step(member, step)
            elif isinstance(step, P.AddFingerprintFeaturesStep):
                member.add(_Fingerprint(float(step.rnd_salt_)))
            elif isinstance(step, P.ShuffleFeaturesStep):
                member.add(_gather(step.index_permutation_))
            else:
                raise _NoDeviceForm(type(step).__name__)
        prog = _finish(member)
        if probe is not None:
            why = probe_check(prog, pipeline, probe)
            if why:
                warnings.warn(f"member preprocessing stays on the host: {why}", RuntimeWarning, stacklevel=2)
                return None, why
        if front is not None:
            prog = with_front(prog, front)
        return prog, ""
    except _NoDeviceForm as e:
        return None, str(e)
    except (AttributeError, IndexError, KeyError, TypeError, ValueError) as e:  # fitted state of an unknown layout
        return None, f"{type(e).__name__}: {e}"


def _finish(b: _Builder) -> MemberProgram:
    prog = _serialise(b)
    if prog.width > MAX_WIDTH:
        raise _NoDeviceForm(f"a row of {prog.width} columns: the kernel holds {MAX_WIDTH} per row")
    prog._sym = list(b.ops)
    return prog


def with_front(prog: MemberProgram, front) -> MemberProgram:
    """``prog`` (a member's, from ``compile_member``) behind the estimator's front encoder: the program of the raw
    table.  Raises ``ValueError`` where the two do not fit or the result is too wide."""
    try:
        whole = _Builder(len(front[0]) + len(front[4]))
        whole.add(front_map(front, whole.n_in))
        if whole.width != prog.n_in:
            raise _NoDeviceForm("front encoder: another width than the members' input")
        for op in prog._sym:
            whole.add(op)
        return _finish(whole)
    except _NoDeviceForm as e:
        raise ValueError(str(e)) from None


class DeviceTable:
    """A predict's ``X`` that lives on the GPU, as the estimators hand it to their executor: the tensor for the
    members that have a program, and the host route's table (copied back, validated and front-encoded once, on
    first use) for those that do not."""

    def __init__(self, tensor, host_encode):
        self.tensor = tensor
        self._host_encode = host_encode
        self._host = None

    def __len__(self) -> int:
        return int(self.tensor.shape[0])

    def host(self) -> np.ndarray:
        if self._host is None:
            self._host = self._host_encode(self.tensor.detach().cpu().numpy())
        return self._host


def device_table(estimator, X, device, host_encode) -> DeviceTable:
    """A CUDA tensor ``X`` given to ``predict`` and its kin, checked as ``validate_X_predict`` checks an array and
    with its error types: ``ValueError`` for a rank other than 2, no rows, a width other than ``n_features_in_``,
    complex data or a tensor on another device than the estimator's; integer, boolean and 16-bit tables become
    float64 (the host takes them too).  ``TypeError`` if the fitted front encoder has no numeric plan (string
    categories): such an estimator cannot encode on the device.  Infinities are found by the kernel
    (``HipEngine.status``), NaN is data."""
    import torch

    name = type(estimator).__name__
    if X.dim() != 2:
        raise ValueError(f"Expected 2D array, got {X.dim()}D tensor instead: shape={tuple(X.shape)}.")
    if X.shape[0] < 1:
        raise ValueError(f"Found array with 0 sample(s) (shape={tuple(X.shape)}) while a minimum of 1 is required.")
    if X.shape[1] != estimator.n_features_in_:
        raise ValueError(f"X has {X.shape[1]} features, but {name} is expecting {estimator.n_features_in_} features "
                         "as input.")
    if X.is_complex():
        raise ValueError("Complex data not supported")
    want = torch.device(device)
    index = want.index if want.index is not None else torch.cuda.current_device()
    if want.type != "cuda" or X.device.index != index:
        raise ValueError(f"X lives on {X.device}, {name} runs on {want}: move X there or pass a host array")
    if getattr(estimator, "_ordinal_plan_", None) is None:
        raise TypeError(f"{name} was fitted on a table whose categories are not numbers: its front encoder has no "
                        "device form, so a CUDA tensor X cannot be encoded; pass X as a host array")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.to(torch.float64)
    return DeviceTable(X, host_encode)


def probe_rows(X_train: np.ndarray, n_first: int = 32) -> np.ndarray:
    X = np.asarray(X_train, np.float64)
    first = X[:n_first]
    with np.errstate(invalid="ignore"):
        top = np.nan_to_num(np.nanmax(np.where(np.isfinite(X), X, np.nan), axis=0), nan=0.0)
        bot = np.nan_to_num(np.nanmin(np.where(np.isfinite(X), X, np.nan), axis=0), nan=0.0)
    extra = np.stack([np.full(X.shape[1], np.nan), top + 1000.5, bot - 1000.5])
    return np.concatenate([first, extra], 0)


def probe_check(prog: MemberProgram, pipeline, X_train) -> str:
    """"" if the program and ``pipeline.transform`` agree on the probe rows, else what differs."""
    rows = probe_rows(X_train)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = np.asarray(pipeline.transform(rows.copy()).X, np.float64)
    got, _, bound = run_program_host(prog, rows, return_bound=True)
    if got.shape != want.shape:
        return f"probe check: shape {got.shape} != {want.shape}"
    bad = mismatch(got, want, bound)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        return f"probe check: output [{r}, {c}] is {got[r, c]!r}, the host pipeline gives {want[r, c]!r}"
    return ""


def mismatch(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """Elements outside their bound: bit equality where the bound is 0 (NaN positions and payloads included),
    ``|got - want| <= bound`` elsewhere (NaN only against NaN)."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    same = got.view(np.uint64) == want.view(np.uint64)
    with np.errstate(invalid="ignore"):
        near = (bound > 0) & (np.abs(got - want) <= bound)
    return ~(same | near)


# ----------------------------------------------------------------------------- the host interpreter


def _interp(x, xp, fp, tie_first=False):
    """``np.interp`` restated (numpy's ``arr_interp``): j the LAST index with ``xp[j] <= x``."""
    n = len(xp)
    j = np.searchsorted(xp, x, side="left" if tie_first else "right") - (0 if tie_first else 1)
    j = np.clip(j, 0, n - 1)
    j1 = np.minimum(j + 1, n - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        slope = (fp[j1] - fp[j]) / (xp[j1] - xp[j])
        r = slope * (x - xp[j]) + fp[j]
        r2 = slope * (x - xp[j1]) + fp[j1]
        r = np.where(np.isnan(r), np.where(np.isnan(r2) & (fp[j] == fp[j1]), fp[j], r2), r)
    r = np.where((j == n - 1) | (xp[j] == x), fp[j], r)
    r = np.where(x > xp[n - 1], fp[n - 1], r)
    return np.where(x < xp[0], fp[0], r)


def _quantile(x, q, refs, tie_first=False):
    out = x.copy()
    ok = ~np.isnan(x)
    xf = x[ok]
    out[ok] = 0.5 * (_interp(xf, q, refs, tie_first) - _interp(-xf, -q[::-1], -refs[::-1], tie_first))
    out[x == q[-1]] = 1.0
    out[x == q[0]] = 0.0
    return out


def salted_twice(x: np.ndarray, salt: float) -> np.ndarray:
    """``(x + salt) + salt`` with a NaN cell's bits carried through explicitly: sign and payload kept, quiet bit set."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x + salt) + salt
    nan = np.isnan(x)
    yb = y.view(np.uint64).copy()
    yb[nan] = x.view(np.uint64)[nan] | _QUIET
    return yb.view(np.float64)


def fingerprint(x: np.ndarray, salt: float, single_salt: bool = False) -> np.ndarray:
    from multimodalpfn_amd.model._siphash import siphash24_rows_numpy

    x = np.ascontiguousarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = x + salt if single_salt else salted_twice(x, salt)
    return np.mod(siphash24_rows_numpy(np.ascontiguousarray(rows)), _FP_MOD) / _FP_MOD


def _svd_chain(z: np.ndarray, comps: np.ndarray) -> np.ndarray:
    """``sum_i z[:, i] * comps[j, i]``, i ascending from 0, the product and the sum rounded separately: what
    numpy's own matmul loop gives for ``z @ components_.T`` (``components_`` comes out of ARPACK row-reversed, a
    view BLAS does not take), bit for bit."""
    acc = np.zeros((z.shape[0], comps.shape[0]))
    for i in range(z.shape[1]):
        acc = acc + z[:, i:i + 1] * comps[None, :, i]
    return acc


def run_program_host(prog: MemberProgram, X64, *, return_bound: bool = False, variant: str | None = None):
    """``(out64, out32)`` of ``X64`` ``[Q, n_in]``: the op list in plain numpy, ``out32 = out64.astype(float32)``
    (round to nearest even).  With ``return_bound`` a third array gives each element's bound against the host
    pipeline: 0 (bit equality) for gathers, lookups, guarded scalers and fingerprints; ``QUANTILE_BOUND`` for
    uniform quantiles; ``2 (F + 2) 2^-53 sum |z| |c|`` for SVD columns (the any-order float64 summation bound,
    doubled).  A column that is only moved keeps its bound; nothing is widened for an inexact input, so a scaler,
    SVD or fingerprint fed by a quantile that is off by a rounding fails its bound (and the probe check).  ``variant`` names one deliberate mistake for the sensitivity
    tests: ``"tie_first"`` (the first index of a tie run), ``"single_salt"`` (hash ``X + salt``) or ``"svd_swap"``
    (the first two components exchanged)."""
    cur = np.array(X64, dtype=np.float64, ndmin=2)
    if cur.shape[1] != prog.n_in:
        raise ValueError(f"X has {cur.shape[1]} columns, the program takes {prog.n_in}")
    bnd = np.zeros_like(cur)
    ints, d = prog.ints, prog.doubles
    for code, w_in, w_out, ioff, doff, a, b, c in prog.ops.tolist():
        assert cur.shape[1] == w_in
        if code == OP_GATHER:
            idx = ints[ioff:ioff + w_out]
            cur, bnd = cur[:, idx], bnd[:, idx]
        elif code == OP_MAP:
            nxt, nb = np.empty((len(cur), w_out)), np.zeros((len(cur), w_out))
            for j in range(w_out):
                src, kind, off, n, aux = ints[ioff + MAP_INTS * j: ioff + MAP_INTS * (j + 1)].tolist()
                x = cur[:, src]
                if kind == K_PASS:
                    nxt[:, j], nb[:, j] = x, bnd[:, src]
                elif kind == K_LOOKUP:
                    unseen, miss = d[off], d[off + 1]
                    cats, vals = d[off + 2: off + 2 + n], d[off + 2 + n: off + 2 + 2 * n]
                    i = np.minimum(np.searchsorted(cats, x), max(n - 1, 0))
                    hit = cats[i] == x if n else np.zeros(len(x), bool)
                    nxt[:, j] = np.where(np.isnan(x), miss, np.where(hit, vals[i] if n else unseen, unseen))
                elif kind == K_QUANTILE:
                    nxt[:, j] = _quantile(x, d[off: off + n], d[aux: aux + n], tie_first=variant == "tie_first")
                    nb[:, j] = QUANTILE_BOUND
                else:
                    pre, mean, scale, post = d[off: off + 4]
                    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                        y = np.where(np.isinf(x), np.nan, x)
                        y = (np.where(np.isnan(y), pre, y) - mean) / scale
                        y = np.where(np.isinf(y), np.nan, y)
                        y = np.where(np.isnan(y), post, y)
                    nxt[:, j] = y
            cur, bnd = nxt, nb
        elif code == OP_SVD:
            comps = d[doff: doff + b * c].reshape(c, b)
            if variant == "svd_swap" and c >= 2:
                comps = comps[[1, 0] + list(range(2, c))]
            z = cur[:, a:]
            red = _svd_chain(z, comps)
            rb = 2 * (b + 2) * _EPS * (np.abs(z) @ np.abs(comps).T)
            cur, bnd = np.concatenate([cur[:, :a], red], 1), np.concatenate([bnd[:, :a], rb], 1)
        elif code == OP_FINGERPRINT:
            fp = fingerprint(cur, d[doff], single_salt=variant == "single_salt")
            cur, bnd = np.concatenate([cur, fp[:, None]], 1), np.concatenate([bnd, np.zeros((len(cur), 1))], 1)
        else:
            raise ValueError(f"op code {code}")
    cur = np.ascontiguousarray(cur)
    with np.errstate(over="ignore", invalid="ignore"):
        out32 = cur.astype(np.float32)
    return (cur, out32, np.ascontiguousarray(bnd)) if return_bound else (cur, out32)
