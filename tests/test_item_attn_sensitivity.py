"""CPU: what the checks of tests/item_attn_cases.py catch, and what ties its restatement to the oracle.

* The selection case rests on properties of its operands, asserted by ``check_selection_operands`` for every way, with
  and without the per-query shifts; its unfaulted restatement stores V[pi] itself, bit for bit in the 16-bit ways.
* Modes 0 and 2 of ``attend`` on the spread case equal ``oracle.forward._attn`` within the taps' tolerance
  (tests/test_taps_gpu.py ``TOL``).
* The unfaulted restatement passes its own checks: its bits, and every spread-case |out - exact| / bound at most 1, in
  all three spread states.
* Each fault of ``item_attn_cases.FAULTS`` is a mistake the kernels or ``item_attn_args`` could make, applied to the
  restatement.  Wherever it applies, the selection case's comparison must fail -- but for ``last_key_dropped`` and
  ``pad_key_counted`` where the dropped key is no query's choice (a one-hot softmax does not see the others), and for
  the prescale faults, which scale every score of a query alike: these must push a spread-case result / bound above 1.
* ``p_not_rounded`` is invisible, as the module says: the bound contains P's half ulp.  It is asserted to be unseen, so
  that a bound tightened enough to see it would show up here.
"""

import pytest
import torch

import item_attn_cases as C
import oracle.forward as ofw
from helpers import rel_err
from test_taps_gpu import TOL

# three columns, five full key tiles and one key, a0 = 256 and 65 own rows in form 1, 54 test rows: 6 * 54 >= N queries on
# head 0's K / V, so every key is some query's choice in every form
T, S, N = 3, 375, 321
WAYS = dict(fwd0=C.forward_way(0), fwd1=C.forward_way(1), fwd2=C.forward_way(2), fwd5=C.forward_way(5),
            old_bf16=C.OLD_BF16, old_f16=C.OLD_F16)
FORMS = {name: ((0, 1, 2) if name.startswith("fwd") else (0, 2) if name == "old_bf16" else (0,)) for name in WAYS}
SPREAD_ONLY = ("no_prescale", "double_prescale", "p_not_rounded")
_CACHE: dict = {}


def _case(kind: str, prescaled: bool, state: int = 0) -> dict:
    key = (kind, prescaled, state)
    if key not in _CACHE:
        _CACHE[key] = (C.selection_case(T, S, N, prescaled, shifted=bool(state)) if kind == "selection"
                       else C.spread_case(T, S, N, prescaled, state))
    return _CACHE[key]


def _run(kind: str, name: str, form: int, fault=None, state: int = 0) -> dict:
    key = (kind, name, form, fault, state)
    if key not in _CACHE:
        way = WAYS[name]
        c = _case(kind, way.prescaled, state)
        if kind == "spread":
            c = C.stored(way, c)
        if form == 2:
            c = C.cached_operands(c)
        _CACHE[key] = C.attend(way, form, c["q"], c["k"], c["vt"], N, fault=fault, want_mag=kind == "spread")
    return _CACHE[key]


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", WAYS)
def test_selection_operands_hold_their_properties(name, shifted):
    C.check_selection_operands(_case("selection", WAYS[name].prescaled, int(shifted)), WAYS[name])
    for nk in (1, 2, 64, 65, 705):  # the smallest, one tile, the largest of the GPU suite
        C.check_selection_operands(C.selection_case(1, nk + 3, nk, WAYS[name].prescaled, shifted), WAYS[name])


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", WAYS)
def test_selection_restatement_stores_the_chosen_vector(name, shifted):
    way = WAYS[name]
    c = _case("selection", way.prescaled, int(shifted))
    v = c["vt"].permute(0, 1, 3, 2)  # [T][H][Npad][32]
    own = (torch.arange(S) < N)[None, :, None].expand(T, S, C.H)
    pi = c["pi"].permute(0, 2, 1)  # [T][S][H]
    b = torch.arange(T)[:, None, None].expand(T, S, C.H)
    g = torch.where(own, torch.arange(C.H)[None, None, :].expand(T, S, C.H), torch.zeros(T, S, C.H, dtype=torch.long))
    want = v[b, g, pi].reshape(T, S, C.H * C.HD)
    for form in FORMS[name]:
        r = _run("selection", name, form, state=int(shifted))
        assert C.selection_passes(C.bits(r), r)
        w = want[:, N:] if form == 2 else want
        if C.is16(way):
            assert torch.equal(r["out"].double()[r["written"]], w[r["written"]]), (name, form)
        else:
            assert bool(((r["out"].double() - w).abs() <= 4 * C.U * w.abs())[r["written"]].all()), (name, form)
        a0, na = C.own_rows(form, S, N)
        nwritten = int(r["written"].sum()) // (C.H * C.HD) // T
        assert nwritten == (S - N if form == 2 else S - a0), (name, form, nwritten)


@pytest.mark.parametrize("mode", [0, 2])
def test_restatement_is_the_oracle_in_the_fp32_modes(mode):
    way = C.forward_way(mode)
    c = C.stored(way, _case("spread", False))
    r = _run("spread", f"fwd{mode}", 0)
    k, v = c["k"][:, :, :N], c["vt"][:, :, :, :N].transpose(2, 3)
    ref_tr = ofw._attn(c["q"][:, :, :N], k, v)
    ref_te = ofw._attn(c["q"][:, :, N:], k[:, :1].expand_as(k), v[:, :1].expand_as(v))
    ref = torch.cat([ref_tr, ref_te], 2).permute(0, 2, 1, 3).reshape(T, S, C.H * C.HD)
    for key in ("exact", "out"):
        err = rel_err(r[key].double().numpy(), ref.numpy())
        print(f"mode {mode} {key}: restatement against the oracle {err:.3e}")
        assert err <= TOL[mode], (mode, key, err)


@pytest.mark.parametrize("name,state", [(n, s) for n in WAYS for s in (0, 1, 2)])
def test_no_fault_passes_the_spread_bound(name, state):
    for form in FORMS[name]:
        r = _run("spread", name, form, state=state)
        worst = C.ratio(r["out"], r)
        print(f"{name} form {form} state {state}: the stored restatement / bound {worst:.3f}")
        assert worst <= 1.0, (name, form, state, worst)
        bound = C.elem_bound(r)[r["written"]]
        assert bool(torch.isfinite(bound).all()) and float(bound.min()) > 0.0


def test_shifted_states_reach_the_rerun_the_backstop_and_small_row_sums():
    """What states 1 and 2 are for, read off the restatement: row sums at reference 0 past both ends of the kept pass's
    range [2^-60, 2^100), row sums between the padded tile's threshold 2^-12 npad and 1, and (state 2) queries whose
    later tiles lead the first tile's max by more than 100 log2 units, which the re-run's reference cannot hold."""
    way = WAYS["fwd1"]
    plain, r = _run("spread", "fwd1", 0, state=0), _run("spread", "fwd1", 0, state=2)
    npad = r["npad"]
    assert npad == 63
    l0 = r["log2L0"]
    assert float(plain["log2L0"].min()) > 0.0 and float(plain["log2L0"].max()) < 30.0  # state 0: every wave keeps its pass
    assert int((l0 >= 100).sum()) > 0 and int((l0 < -60).sum()) > 0
    assert int(((l0 > -12 + torch.log2(torch.tensor(float(npad)))) & (l0 < 0)).sum()) > 0
    c = C.stored(way, _case("spread", True, 2))
    s = torch.einsum("thsd,thkd->thsk", C.q_operand(way, c["q"][:, :, :N]), c["k"][:, :, :N])
    lead = s[..., C.KT:].max(-1).values - s[..., :C.KT].max(-1).values
    assert int((lead > 100).sum()) > 0
    # every wave of 64 consecutive queries holds shifted and plain ones
    shifted = (c["q"][0, 0, :, 30] != 0) | (c["q"][0, 0, :, 31] != 0)
    for j in range(0, S - 63, 64):
        assert 0 < int(shifted[j:j + 64].sum()) < 64


CASES = [(f, name, form) for f in C.FAULTS for name in WAYS for form in FORMS[name]
         if C.applies(f, WAYS[name], form, T, S - N if form == 2 else S, N)]


@pytest.mark.parametrize("fault,name,form", CASES)
def test_fault_is_caught(fault, name, form):
    way = WAYS[name]
    seen_sel = []
    for shifted in (0, 1):
        ref = _run("selection", name, form, state=shifted)
        bad = _run("selection", name, form, fault=fault, state=shifted)
        seen_sel.append(not C.selection_passes(C.bits(bad), ref))
    if fault == "p_not_rounded":
        assert not any(seen_sel)
        for state in (0, 1):
            r = _run("spread", name, form, state=state)
            assert C.ratio(_run("spread", name, form, fault=fault, state=state)["out"], r) <= 1.0
        return
    if fault not in SPREAD_ONLY:
        assert all(seen_sel), (fault, name, form, seen_sel)
    if fault in ("last_key_dropped", "pad_key_counted") or (fault in SPREAD_ONLY and not all(seen_sel)):
        for state in (0, 1):
            if fault == "pad_key_counted" and state == 0:
                continue  # (a row sum of hundreds hides one more: state 1's small row sums are where it shows)
            r = _run("spread", name, form, state=state)
            worst = C.ratio(_run("spread", name, form, fault=fault, state=state)["out"], r)
            print(f"{fault} {name} form {form} state {state}: result / bound {worst:.2f}")
            assert worst > 1.0, (fault, name, form, state, worst)


def test_every_fault_applies_somewhere():
    assert {f for f, _, _ in CASES} == set(C.FAULTS)
    assert {q for i in range(len(C.N_FULL)) for q in C.q_pairs(i)} == set(C.Q_EDGES)
