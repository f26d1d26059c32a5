"""CPU: what the bounds of tests/feat_block_cases.py catch, and what ties its restatement to the oracle.

* Modes 0 and 2 of ``feat_block`` equal ``oracle.forward.feat_sublayer`` to 1e-12 (normal data, every path's T).
* Each fault of ``feat_block_cases.FAULTS`` is a mistake ``feat_rows_kernel`` (featrow.hip), its weight packing
  (weight_pack.h ``pack_feat_rows``) or its host could make, applied to the float64 restatement itself; in modes 1 and 5
  each must drive the ratio result / bound of at least one case of tests/test_feat_block_gpu.py above 1 (``no_res_perm``
  exists in mode 5 only).  The worst ratio per fault and case kind is printed.
* The tap tests' own measure (tests/test_taps_gpu.py: max error over max(1, max|ref|), 2e-2 in bf16 and 1e-2 in fp16,
  its ragged shapes, weights and seeds) lets the first fault pass before any rounding is added: asserted here about
  that tolerance, 1.5e-2 at T = 16 down to 2.5e-3 at T = 49.
* The selection case's 40-unit margin, over every shape the GPU module uses.
"""

import pytest
import torch

import feat_block_cases as F
import layer_tail_cases as L
import oracle.forward as ofw
from helpers import oracle_spec, rel_err, torch_sd
from synth import synth_state_dict
from test_taps_gpu import TOL

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

SHAPES = ((1, 2, 17), (1, 2, 36), (2, 3, 36), (1, 2, 49))  # (M, S, T): two, three (parked) and four tiles, two members
_CACHE: dict = {}


def _weights(kind: str) -> dict:
    if kind not in _CACHE:
        _CACHE[kind] = F.WEIGHTS[kind]()
    return _CACHE[kind]


def _ref(kind: str, shape, mode: int):
    """(state, restatement, bounds) of a case: a per-element bound (integer cases) or normal_bounds' dict."""
    key = (kind, shape, mode)
    if key not in _CACHE:
        W, c = _weights(kind), F.STATES[kind](*shape)
        r = F.feat_block(mode, c["X"], W)
        if kind == "normal":
            b = F.normal_bounds(mode, r, F.feat_block(mode, c["X"], W, exact=True), TOL)
        else:
            F.INT_CHECK[kind](mode, W, c, r)
            b = F.INT_BOUND[kind](mode, W, r)
        _CACHE[key] = (c, r, b)
    return _CACHE[key]


def _ratio(kind: str, shape, mode: int, fault: str | None) -> float:
    c, r, b = _ref(kind, shape, mode)
    got = F.feat_block(mode, c["X"], _weights(kind), fault=fault)["out"]  # what a kernel with the fault would store
    if kind == "normal":
        mx, rms = L.normal_ratios(mode, got, r, b)
        return max(mx, rms or 0.0)
    return F.int_ratio(got, r, b)


def test_restatement_is_the_oracle_in_the_fp32_modes():
    W = _weights("normal")
    cfg = ModelConfig(nlayers=1, mixer_type=None)
    w = {k: v.double() for k, v in torch_sd(F.state_dict_with(synth_state_dict(state_dict_spec(cfg), 71), W)).items()}
    for T in (1, 17, 36, 64, 65, 129):
        X = F.normal_state(2, 3, T)["X"]
        for mode in (0, 2):
            got = F.feat_block(mode, X, W)["out"]
            for m in range(2):
                want = ofw.feat_sublayer(oracle_spec(cfg), w, 0, X[m].transpose(0, 1))  # [S][T][E]
                assert float((got[m].transpose(0, 1) - want).abs().max()) <= 1e-12, (T, mode)


@pytest.mark.parametrize("mode", [1, 5])
def test_no_fault_passes(mode):
    """The stored restatement itself is within every bound (mode 5: its store's half ulp, the rest: zero)."""
    for kind in F.STATES:
        for shape in SHAPES:
            assert _ratio(kind, shape, mode, None) <= 1.0, (kind, shape)


# (the out-projection's rows are permuted in the fp16 form only)
@pytest.mark.parametrize("fault,mode", [(f, m) for f in F.FAULTS for m in (1, 5) if (f, m) != ("no_res_perm", 1)])
def test_fault_is_caught(fault, mode):
    worst = {kind: max(_ratio(kind, shape, mode, fault) for shape in SHAPES) for kind in F.STATES}
    print(f"{fault} mode {mode}: worst result / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) > 1.0, (fault, mode, worst)


def test_the_taps_measure_lets_a_joining_padding_key_pass():
    """tests/test_taps_gpu.py ``test_taps_ragged_shapes``: its model, weights, states and measure, on the fp64 oracle
    (mode 0's restatement).  One zero padding key in the softmax stays inside the bf16 tolerance at every shape and
    inside the fp16 one from T = 33 on, before a kernel's own rounding is added."""
    cfg = ModelConfig(nlayers=1, mgm_heads=8, cap_heads=4)
    sd = torch_sd(synth_state_dict(state_dict_spec(cfg), 3))
    qkv = sd[F.LAYER0 + "_w_qkv"].double()
    W = dict(Wq=qkv[0], Wk=qkv[1], Wv=qkv[2], Wout=L.wout_matrix(sd[F.LAYER0 + "_w_out"].double()))
    for S, T in [(5, 16), (130, 17), (7, 33), (9, 36), (66, 48), (3, 49)]:
        X = torch.randn(S, T, 192, generator=torch.Generator().manual_seed(S * 131 + T)).double()
        X = X.transpose(0, 1).unsqueeze(0)  # [1][T][S][E]
        ref = F.feat_block(0, X, W)["out"]
        err = rel_err(F.feat_block(0, X, W, fault="pad_joins")["out"].numpy(), ref.numpy())
        print(f"S {S} T {T}: a joining padding key moves the tap's measure by {err:.2e}")
        assert 1e-3 < err <= TOL[1] and (T < 33 or err <= TOL[5]), (S, T, err)


def test_selection_margin():
    W = _weights("selection")
    shapes = [(1, S, T) for T in F.T_EDGES for S in F.S_EDGES] + [(M, S, T) for M, S in F.MS for T in (17, 36, 48)] \
        + [(2, 3, T) for T in (1, 16, 17, 33, 36, 48, 49, 64)]
    for mode in F.MODES:
        lead = min(F.selection_margin(F.feat_block(mode, c["X"], W), c)
                   for c in (F.selection_state(*s) for s in shapes))
        print(f"mode {mode}: the target key leads by {lead:.1f} log2 units")
        assert lead >= F.MARGIN
