"""GPU: the CAP, MGM and MoE mixers alone against the fp64 oracle, over the reference's head grid and at the
kernels' tile edges.

Every engine is an ``nlayers=1`` model with synthetic weights; the reference is always ``oracle_cap`` /
``oracle_mgm`` / ``oracle_mixer`` in float64 on the CPU with float64 weights, computed once per input and shared by
the precision modes.  The metric is ``helpers.rel_err``; the bounds are the project's: 1e-4 for the fp32 modes (0, 2),
2e-2 for the bf16 mode (1), 1e-2 for the fp16 mode's (5) MGM head bank.  Where mode 5 runs the bf16 mode's kernels --
the pooler, the MoE, an MGM head bank without the fp16 form (``mgm_heads * nhid % 256 != 0``) -- its result must be
``torch.equal`` to mode 1's.  tests/test_mixer_oracle_sensitivity.py shows that the mistakes these kernels can make
move the oracle by five times the widest bound or more.

What the shapes reach:

* CAP tap: every ``cap_heads`` that ``mmpfn_set_model`` accepts on the reference's grid (head dims 96 .. 1; 3 and 6
  are head dims 64 and 32), ``cap_heads`` 48 and up loop over the (head, query) pairs (cap^2 > 1024; 192: 36 times);
  M = 1, a last LDS chunk of one key (65) and a third one of two (130), a 32-key sub-chunk of one key (33); for
  24 heads the MFMA kernel's MB = 1 .. 4 (M = 32, 64, 96, 128) and its fall-back (M = 160, 256, and M % 32 != 0);
  S % 4 != 0.
* MGM tap: the GLU GEMM's 256-row and the remap GEMM's 320-row tile edges, the latter between the modalities of one
  sample (n_mod = 3: row 320 is modality 2 of sample 106); the generic 16-bit GLU path (nhid = 384).
* Whole mixer: the 16-bit token hand-over from MGM to CAP, M = mgm_heads * n_mod up to 160.
* MoE: 1 .. 16 experts, the modality-0 gather (n_mod > 1), the generic GEMM's 64-row tile edges, a peaked gate.
"""

import ctypes

import pytest
import torch

from helpers import oracle_spec, rel_err, report, torch_sd
from oracle.forward import oracle_cap, oracle_mgm, oracle_mixer
from synth import synth_state_dict

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

pytestmark = pytest.mark.gpu

BOUND = {0: 1e-4, 1: 2e-2, 2: 1e-4, 5: 1e-2}
PRECS = [0, 1, 2, 5]
E = 192

_ENGINES: dict = {}  # config key -> (engine, oracle spec, float64 weights)
_REFS: dict = {}  # input key -> (input, float64 reference)
_OUT16: dict = {}  # (input key, tap) -> mode 1's output, for mode 5's torch.equal
_WORST: dict = {}  # (group, precision) -> (error, case)


@pytest.fixture(scope="module", autouse=True)
def _engines_closed_at_teardown():
    yield
    for grp in sorted({g for g, _ in _WORST}):
        report(f"mixer {grp}: worst rel err " + ", ".join(
            f"prec {p} {_WORST[grp, p][0]:.2e} ({_WORST[grp, p][1]})" for p in PRECS if (grp, p) in _WORST))
    for eng, _, _ in _ENGINES.values():
        eng.close()
    _ENGINES.clear(), _REFS.clear(), _OUT16.clear(), _WORST.clear()


def _model(**kw):
    """One engine per config (module-wide), with its oracle spec and float64 weights."""
    from multimodalpfn_amd.engine import HipEngine

    key = tuple(sorted(kw.items()))
    if key not in _ENGINES:
        cfg = ModelConfig(nlayers=1, **kw)
        sd = synth_state_dict(state_dict_spec(cfg), 61)
        eng = HipEngine(cfg, sd, torch.device("cuda", 0))
        _ENGINES[key] = (eng, oracle_spec(cfg), {k: v.double() for k, v in torch_sd(sd).items()})
    return (key,) + _ENGINES[key]


def _ref(key, make_input, oracle):
    if key not in _REFS:
        x = make_input()
        _REFS[key] = (x, oracle(x.double()))
    return _REFS[key]


def _check(misses, group, case, prec, got, ref, bound, same_as_bf16=None):
    """Print the error and keep the group's worst; a case over its bound (or, where mode 5 runs the bf16 mode, not
    equal to mode 1's output) goes to ``misses``, which the test asserts empty after its last case."""
    got = got.cpu()
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    err = rel_err(got.numpy(), ref.numpy())
    print(f"{group} {case} prec {prec}: rel err {err:.2e}")
    if not err <= _WORST.get((group, prec), (-1.0, ""))[0]:
        _WORST[group, prec] = (err, case)
    if same_as_bf16 is not None and not torch.equal(got, same_as_bf16):
        misses.append((case, "differs from mode 1, whose kernels mode 5 runs here"))
    if not err <= bound:  # (a NaN misses too)
        misses.append((case, err, bound))
    return got


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ CAP tap
CAP_HEADS = [2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 192]
CAP_M = [1, 33, 64, 65, 130]
CAP_M_24 = [32, 96, 128, 160, 256]  # the MFMA kernel's MB = 1, 3, 4 (2 is M = 64) and two fall-backs


def _cap_inputs(cap):
    """(S, M, scaled): S in {5, 9} at every M, S = 1 once, one input with per-token scales 0.1 .. 10."""
    ms = CAP_M + (CAP_M_24 if cap == 24 else [])
    cases = [(S, M, False) for M in ms for S in (5, 9)]
    cases += [(1, 65, False), (5, 64, True)]
    return cases


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cap", CAP_HEADS)
def test_cap_tap_matches_oracle(cap, prec):
    mkey, eng, spec, w = _model(mgm_heads=1, cap_heads=cap)
    misses = []
    for S, M, scaled in _cap_inputs(cap):
        def tokens():
            t = _randn((S, M, E), 1000 * cap + 10 * M + S)
            return t * torch.logspace(-1, 1, M)[None, :, None] if scaled else t

        key = (mkey, S, M, scaled)
        tok, ref = _ref(key, tokens, lambda t: oracle_cap(spec, w, t))
        with torch.inference_mode():
            got = eng.cap(tok, prec)
        case = f"cap_heads {cap} S {S} M {M}" + (" scaled" if scaled else "")
        got = _check(misses, "CAP", case, prec, got, ref, BOUND[1 if prec == 5 else prec],
                     same_as_bf16=_bf16_output(key, "cap", prec, lambda: eng.cap(tok, 1)))
        if prec == 1:
            _OUT16[key, "cap"] = got
    assert not misses, misses


def _bf16_output(key, tap, prec, run):
    """Mode 1's output for the same input (None unless prec is 5): kept by the mode 1 test, else computed here."""
    if prec != 5:
        return None
    if (key, tap) not in _OUT16:
        with torch.inference_mode():
            _OUT16[key, tap] = run().cpu()
    return _OUT16[key, tap]


# ------------------------------------------------------------------------------------------------ MGM tap
MGM_MODELS = [(2, 4), (3, 4), (1, 2), (3, 2)]  # (mgm_heads, nhid_factor); nhid_factor 2: no fp16 head bank
MGM_ROWS = [(1, 255), (1, 256), (1, 257), (1, 320), (1, 321), (3, 107), (3, 214)]  # (n_mod, S)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("heads,fac", MGM_MODELS)
def test_mgm_tap_matches_oracle(heads, fac, prec):
    mkey, eng, spec, w = _model(mixer_type="MGM", mgm_heads=heads, nhid_factor=fac)
    f16_bank = (heads * eng.cfg.nhid) % 256 == 0
    misses = []
    for n_mod, S in MGM_ROWS:
        key = (mkey, n_mod, S)
        im, ref = _ref(key, lambda: _randn((S, n_mod, eng.cfg.nhid), 7000 + 10 * S + n_mod),
                       lambda x: oracle_mgm(spec, w, x))
        with torch.inference_mode():
            got = eng.mgm(im, prec)
        same = None if f16_bank else _bf16_output(key, "mgm", prec, lambda: eng.mgm(im, 1))
        got = _check(misses, "MGM" if f16_bank else "MGM (no fp16 bank)",
                     f"heads {heads} nhid {eng.cfg.nhid} n_mod {n_mod} S {S}", prec, got, ref,
                     BOUND[prec] if f16_bank or prec != 5 else BOUND[1], same_as_bf16=same)
        if prec == 1:
            _OUT16[key, "mgm"] = got
    assert not misses, misses


# ------------------------------------------------------------------------------------------------ whole MGM+CAP mixer
MIXER_MODELS = [(32, 24, 1), (32, 24, 3), (32, 24, 5), (16, 12, 1), (8, 8, 2), (32, 32, 1), (2, 2, 1)]


@pytest.mark.parametrize("prec", [0, 1, 5])
@pytest.mark.parametrize("mgm,cap,n_mod", MIXER_MODELS)
def test_whole_mixer_matches_oracle(mgm, cap, n_mod, prec):
    mkey, eng, spec, w = _model(mgm_heads=mgm, cap_heads=cap)
    S, misses = 9, []
    im, ref = _ref((mkey, "mixer", n_mod), lambda: _randn((S, n_mod, eng.cfg.nhid), 9000 + 100 * mgm + n_mod),
                   lambda x: oracle_mixer(spec, w, x))
    with torch.inference_mode():
        got = eng.mixer_tokens(im, prec)
    _check(misses, "MGM+CAP", f"mgm {mgm} cap {cap} n_mod {n_mod} S {S}", prec, got, ref,
           BOUND[1 if prec == 5 else prec])
    assert not misses, misses


# ------------------------------------------------------------------------------------------------ MoE
MOE_S = [1, 5, 63, 64, 65, 130]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_exp", [1, 3, 4, 16])
def test_moe_matches_oracle(n_exp, prec):
    mkey, eng, spec, w = _model(mixer_type="MoE", mgm_heads=n_exp)
    cases = [(n_mod, S, 1.0) for n_mod in (1, 2, 3) for S in MOE_S]
    if n_exp == 4:
        cases.append((2, 65, 8.0))  # the image scaled by 8: the experts normalise it, the gate does not
    misses = []
    for n_mod, S, scale in cases:
        key = (mkey, n_mod, S, scale)
        im, ref = _ref(key, lambda: scale * _randn((S, n_mod, eng.cfg.nhid), 5000 + 10 * S + n_mod),
                       lambda x: oracle_mixer(spec, w, x))
        with torch.inference_mode():
            got = eng.mixer_tokens(im, prec)
        case = f"experts {n_exp} n_mod {n_mod} S {S}" + (" peaked gate" if scale != 1.0 else "")
        got = _check(misses, "MoE", case, prec, got, ref, BOUND[1 if prec == 5 else prec],
                     same_as_bf16=_bf16_output(key, "moe", prec, lambda: eng.mixer_tokens(im, 1)))
        if prec == 1:
            _OUT16[key, "moe"] = got
    assert not misses, misses


def test_peaked_gate_input_is_peaked():
    """The scaled MoE case does reach a peaked softmax: the oracle's largest gate probability averages above 0.9
    (0.3 - 0.6 for the unscaled image)."""
    mkey, eng, spec, w = _model(mixer_type="MoE", mgm_heads=4)
    im = 8.0 * _randn((65, 2, eng.cfg.nhid), 5000 + 10 * 65 + 2)
    gate = torch.softmax(im[:, 0].double() @ w["moe.gate.weight"].T + w["moe.gate.bias"], -1)
    print(f"peaked gate: mean of the largest probability {float(gate.max(-1).values.mean()):.3f}")
    assert float(gate.max(-1).values.mean()) > 0.9


# ------------------------------------------------------------------------------------------------ model contract
REFUSED = [
    ("cap_heads", dict(mgm_heads=1, cap_heads=1)),  # head dim 192: no cap_attn_kernel
    ("nhid", dict(mixer_type="MGM", mgm_heads=2, nhid_factor=1)),  # nhid / 2 = 96
    ("nhid", dict(mixer_type="MGM", mgm_heads=2, nhid_factor=3)),  # nhid / 2 = 288
    ("nhid", dict(mgm_heads=2, cap_heads=2, nhid_factor=1)),
    ("nhid", dict(mgm_heads=2, cap_heads=2, nhid_factor=3)),
    ("nhid", dict(mixer_type="MoE", mgm_heads=2, nhid_factor=1)),
    ("nhid", dict(mixer_type="MoE", mgm_heads=2, nhid_factor=3)),
]


@pytest.mark.parametrize("field,kw", REFUSED, ids=[f"{f}-{'-'.join(map(str, kw.values()))}" for f, kw in REFUSED])
def test_set_model_refuses_geometry_no_kernel_runs(field, kw):
    """``mmpfn_set_model`` is the one place that checks the model: a geometry some kernel behind it cannot run is
    refused there with MMPFN_ERR_INVALID and a message naming the field, not by a launch in the forward."""
    from multimodalpfn_amd import _lib
    from multimodalpfn_amd.engine import HipEngine, model_desc

    cfg = ModelConfig(nlayers=1, **kw)
    lib = _lib.load_library()
    ctx = lib.mmpfn_create(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert ctx
    try:
        desc = model_desc(cfg)
        assert lib.mmpfn_set_model(ctx, ctypes.byref(desc)) == _lib.MMPFN_ERR_INVALID
        assert field in lib.mmpfn_last_error(ctx).decode()
    finally:
        lib.mmpfn_destroy(ctx)
    with pytest.raises(_lib.EngineError, match=field):
        HipEngine(cfg, {}, torch.device("cuda", 0))


@pytest.mark.parametrize("cap", [c for c in range(1, E + 1) if E % c == 0 and c > 1])
def test_set_model_accepts_every_cap_heads_the_cap_test_runs(cap):
    """Every divisor of 192 but 1 is accepted, and is one of the ``cap_heads`` of the CAP tap test above."""
    from multimodalpfn_amd import _lib
    from multimodalpfn_amd.engine import model_desc

    assert cap in CAP_HEADS
    lib = _lib.load_library()
    ctx = lib.mmpfn_create(0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert ctx
    try:
        desc = model_desc(ModelConfig(nlayers=1, mgm_heads=1, cap_heads=cap))
        assert lib.mmpfn_set_model(ctx, ctypes.byref(desc)) == _lib.MMPFN_OK
    finally:
        lib.mmpfn_destroy(ctx)
