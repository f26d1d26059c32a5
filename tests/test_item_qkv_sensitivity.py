"""CPU: what the checks of tests/item_qkv_cases.py catch, and what ties its restatement to the oracle.

* Modes 0 and 2 of ``project`` on normal data equal the Q, K and V that ``oracle.forward.item_sublayer`` hands its
  attention (taken at its ``_attn`` calls) within the taps' tolerance (tests/test_taps_gpu.py ``TOL``; mode 2 to 1e-12),
  on a ``two_sets_of_queries`` model and on a plain one.
* The address case rests on properties of its weights, asserted by ``check_address_weights``.
* Each fault of ``item_qkv_cases.FAULTS`` is a mistake a projection kernel or ``item_project`` could make, applied to the
  float64 restatement itself.  In every mode it applies to, the address case's bitwise comparison must fail -- for
  ``drop_lo_hi``, which one-hot rows cannot show (they have no lo part), the normal case's result / bound must exceed 1.
* The unfaulted restatement passes both: its own bits, and every normal-case ratio at most 1 (the 16-bit modes' ratios
  are close to 1: the store's half ulp is most of their bound).
"""

import pytest
import torch

import item_qkv_cases as C
import oracle.forward as ofw
from helpers import oracle_spec, rel_err, torch_sd
from synth import synth_state_dict
from test_taps_gpu import TOL

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

SHAPE = (2, 3, 70, 33)  # (M, T, S, N): two members, three columns, N % 8 != 0, test rows
_CACHE: dict = {}


def _ref(kind: str, mode: int, two: bool, last: bool):
    key = (kind, mode, two, last)
    if key not in _CACHE:
        M, T, S, N = SHAPE
        if kind == "address":
            _CACHE[key] = C.project(mode, C.address_state(M, T, S), C.address_weights(two), N, last=last)
        else:
            _CACHE[key] = C.project(mode, C.normal_state(M, T, S), C.normal_weights(two), N, last=last, want_mag=True)
    return _CACHE[key]


def _faulted(kind: str, mode: int, two: bool, last: bool, fault: str):
    M, T, S, N = SHAPE
    X, W = ((C.address_state(M, T, S), C.address_weights(two)) if kind == "address"
            else (C.normal_state(M, T, S), C.normal_weights(two)))
    return C.project(mode, X, W, N, last=last, fault=fault)


@pytest.mark.parametrize("two", [False, True])
def test_address_weights_hold_their_properties(two):
    C.check_address_weights(C.address_weights(two))


@pytest.mark.parametrize("two", [False, True])
def test_restatement_is_the_oracle_in_the_fp32_modes(two, monkeypatch):
    cfg = ModelConfig(nlayers=1, mixer_type=None, two_sets_of_queries=two)
    W = C.normal_weights(two)
    w = {k: v.double() for k, v in torch_sd(C.state_dict_with(synth_state_dict(state_dict_spec(cfg), 71), W)).items()}
    seen = []
    attn = ofw._attn
    monkeypatch.setattr(ofw, "_attn", lambda q, k, v, *a: (seen.append((q, k, v)), attn(q, k, v, *a))[1])
    M, T, S, N = SHAPE
    X = C.normal_state(M, T, S)
    proj = {mode: C.project(mode, X, W, N) for mode in (0, 2)}
    for m in range(M):
        seen.clear()
        ofw.item_sublayer(oracle_spec(cfg), w, 0, X[m].transpose(0, 1), N)  # [S][T][E]
        (qtr, k, v), (qte, k0, v0) = seen  # [T][H][rows][32]; the test rows' k0 / v0: head 0's, broadcast
        assert torch.equal(k0, k[:, :1].expand_as(k)) and torch.equal(v0, v[:, :1].expand_as(v))
        # the stored result within the taps' tolerance; mode 2 rounds nothing in front of its store
        for mode, key, tol in ((0, "out", TOL[0]), (2, "out", TOL[2]), (2, "pre", 1e-12)):
            got = {o: t[m * T:(m + 1) * T].double() for o, t in proj[mode][key].items()}
            for name, a, b in (("q train", got["q"][:, :, :N], qtr), ("q test", got["q"][:, :, N:], qte),
                               ("k", got["k"][:, :, :N], k), ("vt", got["vt"][:, :, :, :N], v.transpose(2, 3))):
                err = rel_err(a.numpy(), b.numpy())
                assert err <= tol, (two, mode, key, name, err)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("two", [False, True])
def test_no_fault_passes(mode, two):
    for last in (False, True):
        r = _ref("address", mode, two, last)
        for o in r["pre"]:  # one product per element: the store is exact, but for mode 5's fp16 operand going to bf16
            d = (r["out"][o].double() - r["pre"][o]).abs()
            assert bool((d <= (2.0 ** -8 if mode == 5 else 0.0) * r["pre"][o].abs()).all()), (mode, o)
            assert bool((r["pre"][o] != 0)[r["written"][o]].all())
        n = _ref("normal", mode, two, last)
        worst = C.ratios(n["out"], n)
        print(f"mode {mode} two {two} last {last}: the stored restatement / bound", worst)
        assert max(worst.values()) <= 1.0, (mode, two, last, worst)


@pytest.mark.parametrize("fault,mode", [(f, m) for f in C.FAULTS for m in C.MODES if C.applies(f, m, True)])
def test_fault_is_caught(fault, mode):
    two = True  # (the model on which every fault is one)
    for last in (False, True):
        if fault == "last_wrong_col" and not last:
            continue
        if fault == "drop_lo_hi":
            n = _ref("normal", mode, two, last)
            worst = C.ratios(_faulted("normal", mode, two, last, fault)["out"], n)
            print(f"{fault} mode {mode} last {last}: result / bound", worst)
            assert min(worst.values()) > 1.0, (fault, mode, last, worst)
            # one-hot rows have no lo part: the address case cannot see this one
            assert C.same_bits(C.bits(_faulted("address", mode, two, last, fault)), C.bits(_ref("address", mode, two, last)))
        else:
            got, ref = C.bits(_faulted("address", mode, two, last, fault)), C.bits(_ref("address", mode, two, last))
            assert not C.same_bits(got, ref), (fault, mode, last)
            bad = {o: int((got[o] != ref[o]).sum()) for o in got}
            print(f"{fault} mode {mode} last {last}: elements that differ", bad)


def test_faults_on_a_plain_model():
    """On a model with one set of queries ``test_q_from_train`` is no fault; every other one is caught there too."""
    for mode in C.MODES:
        ref = C.bits(_ref("address", mode, False, False))
        assert C.same_bits(C.bits(_faulted("address", mode, False, False, "test_q_from_train")), ref)
        for fault in C.FAULTS:
            if C.applies(fault, mode, False) and fault not in ("last_wrong_col", "drop_lo_hi"):
                assert not C.same_bits(C.bits(_faulted("address", mode, False, False, fault)), ref), (fault, mode)


def test_every_count_occurs():
    qs = {q for i in range(len(C.N_EDGES)) for q in C.q_pairs(i)}
    assert qs == set(C.Q_EDGES)
