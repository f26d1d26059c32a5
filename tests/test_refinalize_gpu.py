"""A context finalised a second time, for another model, computes what a fresh context for that model computes.

``mmpfn_finalize_weights`` builds a whole new weight set and drops the previous one, so nothing of the first model
can reach the second one's forwards.  The case that can go wrong is a weight form the first model has and the second
lacks, since the dispatch branches on a form's presence:

* model A has both optional forms: the 16-bit MFMA decoder (``n_out <= 16 and nhid % 128 == 0``: n_out = 10,
  nhid = 768) and the fp16 MGM head bank (``mgm_heads * nhid % 256 == 0``: 4 heads);
* model B has neither: n_out = 17, and one MGM head of nhid = 384 (384 % 256 != 0).  (nhid = 192 would lose the
  decoder form too, but ``mmpfn_set_model`` refuses a mixer model of that width: the head bank's down-projection
  then has K = 96, not a multiple of 64; tests/test_mixer_gpu.py.)

Mixer tokens and logits of B on the re-finalised context must be ``torch.equal`` to a fresh engine's, in every base
precision mode.  Two engines, one process; S = 48, N = 32, F = 4, one modality.
"""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 31
S, N, F = 48, 32, 4
PRECS = {"f16": 5, "bf16": 1, "f32": 0, "f32_mfma": 2}


def _cfg(which):
    from multimodalpfn_amd.model.spec import ModelConfig

    if which == "A":
        return ModelConfig(nlayers=1, mixer_type="MGM", mgm_heads=4)
    return ModelConfig(nlayers=1, nhid_factor=2, max_num_classes=17, mixer_type="MGM", mgm_heads=1)


def _state_dict(cfg):
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import state_dict_spec

    return synth_state_dict(state_dict_spec(cfg), SEED)


def _refinalize(eng, cfg, sd):
    """set_model + load_weight + finalize_weights on the engine's existing context, as HipEngine.__init__ does."""
    from multimodalpfn_amd.engine import model_desc

    eng.cfg, eng.desc = cfg, model_desc(cfg)
    eng._check(eng.lib.mmpfn_set_model(eng.ctx, ctypes.byref(eng.desc)), "mmpfn_set_model")
    for name, w in sd.items():
        a = np.ascontiguousarray(w, dtype=np.float32)
        eng._check(eng.lib.mmpfn_load_weight(eng.ctx, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size),
                   f"mmpfn_load_weight({name})")
    eng._check(eng.lib.mmpfn_finalize_weights(eng.ctx), "mmpfn_finalize_weights")


@pytest.fixture(scope="module")
def engines():
    from multimodalpfn_amd.engine import HipEngine

    dev = torch.device("cuda", 0)
    cfg_a, cfg_b = _cfg("A"), _cfg("B")
    sd_b = _state_dict(cfg_b)
    reused = HipEngine(cfg_a, _state_dict(cfg_a), dev)
    _forward(reused, cfg_a, PRECS["f16"])  # A's forms have been in use before B arrives
    _refinalize(reused, cfg_b, sd_b)
    fresh = HipEngine(cfg_b, sd_b, dev)
    yield reused, fresh, cfg_b
    reused.close()
    fresh.close()


def _forward(eng, cfg, prec):
    from synth import synth_image, synth_labels, synth_table

    x = torch.from_numpy(synth_table(S, F, SEED, n_cat=1)).cuda()
    im = torch.from_numpy(synth_image(S, 1, SEED, dim=cfg.nhid)).cuda()
    y = synth_labels(S, 3, SEED)[:N]
    with torch.inference_mode():
        tok = eng.mixer_tokens(im, prec)
        return tok, eng.forward(x, tok, y, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_refinalized_context_matches_a_fresh_one(engines, prec):
    reused, fresh, cfg = engines
    tok_r, out_r = _forward(reused, cfg, PRECS[prec])
    tok_f, out_f = _forward(fresh, cfg, PRECS[prec])
    assert out_f.shape == (S - N, 17) and bool(torch.isfinite(out_f).all())
    assert torch.equal(tok_r, tok_f)
    assert torch.equal(out_r, out_f)
