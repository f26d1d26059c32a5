"""CPU: the mixer tests' bounds would catch a mixer that is subtly wrong.

tests/test_mixer_gpu.py accepts a 16-bit mode within 2e-2 of the fp64 oracle (``helpers.rel_err``).  That bound only
means something if the mistakes a mixer kernel can make move the result by much more.  Each test here applies one such
mistake to the oracle itself, in float64, and requires the oracle to move by at least five times the bf16 bound:

* two CAP queries swapped (a (head, query) pair mix-up), at every ``cap_heads`` of the GPU test;
* the last key dropped at M = 33 (an off-by-one in the key loop or the last LDS chunk);
* the MoE reading modality 1 instead of modality 0 (the ``n_mod > 1`` gather);
* the MGM tokens in modality-major instead of head-major order (the remap GEMM's row map);
* two experts' tokens swapped (the expert / gate pairing).
"""

import pytest
import torch

from helpers import oracle_spec, rel_err, torch_sd
from oracle.forward import oracle_cap, oracle_mgm, oracle_mixer
from synth import synth_image, synth_state_dict

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

BF16_BOUND = 2e-2
MIN_MOVE = 5 * BF16_BOUND
CAP_HEADS = [2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 192]


def _weights(cfg, seed):
    return {k: v.double() for k, v in torch_sd(synth_state_dict(state_dict_spec(cfg), seed)).items()}


def _cap_case(cap):
    cfg = ModelConfig(nlayers=1, mgm_heads=1, cap_heads=cap)
    g = torch.Generator().manual_seed(cap)
    tok = torch.randn(5, 33, 192, generator=g).double()
    w = _weights(cfg, 41)
    return oracle_spec(cfg), w, tok, oracle_cap(oracle_spec(cfg), w, tok)


@pytest.mark.parametrize("cap", CAP_HEADS)
def test_cap_query_swap_moves_the_oracle(cap):
    spec, w, tok, ref = _cap_case(cap)
    w2 = dict(w)
    q = w["cap.queries"].clone()
    q[[0, 1]] = q[[1, 0]]
    w2["cap.queries"] = q
    move = rel_err(oracle_cap(spec, w2, tok).numpy(), ref.numpy())
    print(f"cap_heads {cap}: query swap moves the oracle by {move:.3f}")
    assert move >= MIN_MOVE


@pytest.mark.parametrize("cap", CAP_HEADS)
def test_cap_dropped_last_key_moves_the_oracle(cap):
    spec, w, tok, ref = _cap_case(cap)
    move = rel_err(oracle_cap(spec, w, tok[:, :-1]).numpy(), ref.numpy())
    print(f"cap_heads {cap}: dropping key 33 of 33 moves the oracle by {move:.3f}")
    assert move >= MIN_MOVE


def _moe_case(n_exp, n_mod):
    cfg = ModelConfig(nlayers=1, mixer_type="MoE", mgm_heads=n_exp, cap_heads=2)
    im = torch.from_numpy(synth_image(7, n_mod, 3, dim=cfg.nhid)).double()
    w = _weights(cfg, 42)
    return oracle_spec(cfg), w, im, oracle_mixer(oracle_spec(cfg), w, im)


def test_moe_wrong_modality_moves_the_oracle():
    spec, w, im, ref = _moe_case(4, 2)
    im2 = im.clone()
    im2[:, 0], im2[:, 1] = im[:, 1], im[:, 0]
    move = rel_err(oracle_mixer(spec, w, im2).numpy(), ref.numpy())
    print(f"MoE on modality 1 instead of 0 moves the oracle by {move:.3f}")
    assert move >= MIN_MOVE


def test_moe_expert_swap_moves_the_oracle():
    spec, w, im, ref = _moe_case(4, 2)
    swapped = ref.clone()
    swapped[:, [0, 1]] = ref[:, [1, 0]]
    move = rel_err(swapped.numpy(), ref.numpy())
    print(f"MoE experts 0 and 1 swapped moves the oracle by {move:.3f}")
    assert move >= MIN_MOVE
    # the experts under each other's gate probability (weights swapped, gate rows left in place)
    w2 = dict(w)
    for k in list(w):
        if k.startswith("moe.experts.0."):
            k1 = k.replace("moe.experts.0.", "moe.experts.1.")
            w2[k], w2[k1] = w[k1], w[k]
    move = rel_err(oracle_mixer(spec, w2, im).numpy(), ref.numpy())
    print(f"MoE experts 0 and 1 under each other's gate moves the oracle by {move:.3f}")
    assert move >= MIN_MOVE


@pytest.mark.parametrize("fac,heads,n_mod", [(4, 2, 3), (4, 3, 3), (2, 3, 3), (4, 3, 2)])
def test_mgm_token_order_moves_the_oracle(fac, heads, n_mod):
    cfg = ModelConfig(nlayers=1, nhid_factor=fac, mixer_type="MGM", mgm_heads=heads)
    spec, w = oracle_spec(cfg), _weights(cfg, 43)
    im = torch.from_numpy(synth_image(7, n_mod, 3, dim=cfg.nhid)).double()
    ref = oracle_mgm(spec, w, im)  # [S, heads * n_mod, E], token h * n_mod + m
    wrong = ref.reshape(7, heads, n_mod, -1).transpose(1, 2).reshape(ref.shape)  # token m * heads + h
    move = rel_err(wrong.numpy(), ref.numpy())
    print(f"nhid {cfg.nhid} heads {heads} n_mod {n_mod}: modality-major tokens move the oracle by {move:.3f}")
    assert move >= MIN_MOVE
