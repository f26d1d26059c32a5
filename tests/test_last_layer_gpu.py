"""The pruned last layer of the forward entry points against the same layer run in full.

After the last layer the decoder reads the target token's test rows only, so ``mmpfn_forward``,
``mmpfn_forward_batch``, ``mmpfn_cache_build`` and ``mmpfn_cache_predict`` compute just those there.  Every kernel
computes a state row from that row's own inputs, so the logits must be **bitwise** those of a full last layer
(``HipEngine.full_last_layer = True``, ``mmpfn_set_full_last_layer``): ``torch.equal``, no tolerance.

Shapes: the smallest at which the pruning can go wrong -- N = 100 train rows (a partial 64-key tile; the test rows
start mid-way through a 256-query attention task), Q = 37 test rows (a partial 32-row wave and 64-query group) or
Q = 1; F = 5 features in groups of two plus a 24-token mixer, so the target token T-1 = 27 is no multiple of the
feature block's 16-token tile; a tabular-only table (C = 0, T = 4); a last layer that is also the first; and F = 21
and F = 60 (T = 36 and 55), the feature block's three- and four-tile forms, whose last-layer variant computes
token T-1 alone.
"""

import ctypes
import functools

import pytest
import torch

from helpers import torch_sd

pytestmark = pytest.mark.gpu

N_TRAIN = 100
SEED = 23
# parity (split bf16), bf16, fp32-input MFMA, fp16, fp16 with the fp8 P.V (e4m3)
PRECS = {"f32": 0, "bf16": 1, "f32_mfma": 2, "f16": 5, "f16_f8": 6}
# name: (layers, test rows, mixer tokens?, features)
CASES = {"mixer_q37": (2, 37, True, 5), "mixer_q1": (2, 1, True, 5), "tabular_q37": (2, 37, False, 5),
         "one_layer_q37": (1, 37, True, 5), "t36_q37": (2, 37, True, 21), "t55_q37": (1, 37, True, 60)}


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
def _inputs(Q, with_image, F=5):
    from synth import synth_image, synth_labels, synth_table

    S = N_TRAIN + Q
    x = torch.from_numpy(synth_table(S, F, SEED, n_cat=2, nan_frac=0.02)).cuda()
    im = torch.from_numpy(synth_image(S, 1, SEED)).cuda() if with_image else None
    return x, im, synth_labels(S, 4, SEED)[:N_TRAIN]


def _entry_points(eng, x, tok, y, prec):
    """Logits of forward, a batch-3 forward_many and cache_build + cache_predict, at the engine's current switch."""
    N = len(y)
    tt = None if tok is None else tok[:N]
    tq = None if tok is None else tok[N:]
    # three members of one geometry: column permutations of the table, shifted labels
    items = [(torch.roll(x, k, dims=1), tok, (y + k) % 4) for k in range(3)]
    out = {"forward": eng.forward(x, tok, y, prec)}
    out["forward_many"] = torch.stack(eng.forward_many(items, prec, lanes=1, batch=3))
    cache = eng.cache_build(x[:N], tt, y, prec)
    out["cache"] = eng.cache_predict(cache, x[N:], tq)
    eng.status()
    cache.free()
    return out


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("prec", PRECS)
def test_pruned_last_layer_is_bitwise_the_full_one(prec, case):
    nlayers, Q, with_image, F = CASES[case]
    model, cfg = _model(nlayers)
    eng = model.engine()
    x, im, y = _inputs(Q, with_image, F)
    code = PRECS[prec]
    eng.full_last_layer = False  # the default, unless MMPFN_FULL_LAST_LAYER=1 is set
    assert eng.full_last_layer is False
    with torch.inference_mode():
        tok = None if im is None else eng.mixer_tokens(im, code)
        assert (0 if tok is None else tok.shape[1]) == (24 if with_image else 0)
        pruned = _entry_points(eng, x, tok, y, code)
        eng.full_last_layer = True
        try:
            full = _entry_points(eng, x, tok, y, code)
        finally:
            eng.full_last_layer = False
    for name, ref in full.items():
        assert ref.shape[-2:] == (Q, cfg.n_out)
        assert torch.isfinite(ref).all(), name
        assert torch.equal(pruned[name], ref), (name, (pruned[name] - ref).abs().max().item())
    assert torch.equal(full["forward_many"][0], full["forward"])  # member 0 of the batch is the single forward


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_run_layers_state_is_whole_with_either_switch(prec):
    """The tap path runs full layers whatever the switch says: run_layers(0, L) + copy_state is the whole state (its
    decoder output is the forward's logits), and a pruned forward leaves that state at the target token's test rows."""
    model, cfg = _model(2)
    eng = model.engine()
    x, im, y = _inputs(37, True)
    code = PRECS[prec]
    states = {}
    with torch.inference_mode():
        tok = eng.mixer_tokens(im, code)
        for on in (False, True):
            eng.full_last_layer = on
            try:
                eng.embed_state(x, tok, y, code)
                states[on] = eng.run_layers(0, cfg.nlayers)
                logits = eng.decode(37)
                fwd = eng.forward(x, tok, y, code)
                after_forward = eng.copy_state()
            finally:
                eng.full_last_layer = False
            assert torch.equal(logits, fwd)
            assert torch.equal(after_forward[N_TRAIN:, -1], states[on][N_TRAIN:, -1])
            if on:
                assert torch.equal(after_forward, states[on])
            elif prec == "f16":
                # the feature block's last-layer form: token T-1 of every row (the train rows' is what the pruned
                # layer leaves there) bitwise the full kernel's, the other tokens not written
                eng.embed_state(x, tok, y, code)
                prev = eng.run_layers(0, cfg.nlayers - 1)
                feat = eng.feature_attention(cfg.nlayers - 1, prev, code)
                assert torch.equal(after_forward[:N_TRAIN, -1], feat[:N_TRAIN, -1])
                assert torch.equal(after_forward[:, :-1], prev[:, :-1])
    assert torch.isfinite(states[True]).all()
    assert torch.equal(states[False], states[True])


def test_kernel_timing_counts_the_full_shape_launches_only():
    """mmpfn_kernel_timing brackets the full layers' attention launches: nlayers - 1 of a pruned forward, each of
    exactly 4 T S N E flops (what bench.py's roofline leg requires of every timed launch)."""
    model, cfg = _model(2)
    eng = model.engine()
    x, im, y = _inputs(37, True)
    code = PRECS["f16"]
    S, T, E = x.shape[0], 3 + 24 + 1, cfg.emsize
    ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    with torch.inference_mode():
        tok = eng.mixer_tokens(im, code)
        for on, launches in ((False, cfg.nlayers - 1), (True, cfg.nlayers)):
            eng.full_last_layer = on
            try:
                assert eng.lib.mmpfn_kernel_timing(eng.ctx, 1) == 0
                eng.forward(x, tok, y, code)
                assert eng.lib.mmpfn_kernel_timing(eng.ctx, 0) == 0
            finally:
                eng.full_last_layer = False
            assert eng.lib.mmpfn_kernel_timing_read(eng.ctx, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)) == 0
            assert n.value == launches
            assert fl.value == launches * 4.0 * T * S * N_TRAIN * E
            assert ms.value > 0.0
