"""Bit fixtures of the feature block and its neighbours, recorded from THIS project's own GPU build.

Run from the repo root on a machine with the GPU, at the commit whose bits are to be pinned:

    python tests/golden/make_featrow_bits.py

Writes ``tests/golden/featrow/featrow_bits.npz`` (a directory of its own: ``helpers.CASES`` takes every
``tests/golden/*.npz`` for a model case).  tests/test_featrow_bits_gpu.py recomputes every case with the build under
test and asks for the same bits, so a change to ``feat_rows_kernel``, ``rowgemm_qkv2_kernel`` or
``rowgemm_ln_store_kernel`` that is meant to move data differently and compute the same (where fragments wait, which
LDS address a staging tile uses) is held to that.

The cases (``cases()``): inputs are seeded CPU ``randn`` states, weights ``synth_state_dict``.

``feat``  ``HipEngine.feature_attention`` at T in {1, 16, 17, 32, 33, 36, 47, 48, 49, 64} (every tile count of
          ``feat_rows_kernel<NT>``, both edges of each tile, the workload's T = 36) x S in {1, 5, 9} (a block with
          one live wave; three waves past the last row) x PREC_F16, PREC_BF16.
``item``  ``HipEngine.item_attention_block`` at T = 36, S = 130, N = 100 (more than one 128-row block of the q | k | v
          projection, a partial wave, Npad > N), both 16-bit modes.
``cap``   ``HipEngine.cap`` of the MGM 64 + CAP 24 mixer's pooler at S = 9, M = 64 (K | V^T through
          ``rowgemm_ln_store_kernel``, S % 4 != 0), both 16-bit modes.

What is stored.  All outputs together are 11 MB, ten times what one committed file may hold, so every case stores the
SHA-256 of its output's bytes (``sha_<case>``, 32 bytes: equal digests are equal bits), and the S = 1 feature cases
also store the output itself (``out_<case>``; the fp16 mode's as float16, which holds its fp16 state exactly), so that
a mismatch there can be looked at element by element.
"""

from __future__ import annotations

import hashlib
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(HERE))

OUT = HERE / "featrow" / "featrow_bits.npz"
PREC_BF16, PREC_F16 = 1, 5  # multimodalpfn_amd._lib.PREC_BF16 / PREC_F16
FEAT_T = [1, 16, 17, 32, 33, 36, 47, 48, 49, 64]
FEAT_S = [1, 5, 9]
ITEM_SHAPE = dict(T=36, S=130, N=100)
CAP_SHAPE = dict(S=9, M=64)
E = 192


def cases() -> list[tuple[str, str, dict]]:
    """(name, kind, arguments) of every case, in the order they run."""
    out = []
    for prec in (PREC_F16, PREC_BF16):
        for T in FEAT_T:
            for S in FEAT_S:
                out.append((f"feat_p{prec}_T{T}_S{S}", "feat", dict(T=T, S=S, prec=prec)))
        out.append((f"item_p{prec}", "item", dict(prec=prec, **ITEM_SHAPE)))
        out.append((f"cap_p{prec}", "cap", dict(prec=prec, **CAP_SHAPE)))
    return out


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def make_engines():
    """The layer model (8 MGM / 4 CAP heads, one layer) and the config-C mixer model (MGM 64 + CAP 24)."""
    from synth import synth_state_dict

    from multimodalpfn_amd.engine import HipEngine
    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    engines = {}
    for key, kw, seed in (("layer", dict(mgm_heads=8, cap_heads=4), 3), ("mixer", dict(mgm_heads=64, cap_heads=24), 4)):
        cfg = ModelConfig(nlayers=1, **kw)
        engines[key] = HipEngine(cfg, synth_state_dict(state_dict_spec(cfg), seed), torch.device("cuda", 0))
    return engines


def run_case(engines: dict, kind: str, a: dict) -> np.ndarray:
    """One case's output on the GPU build that ``multimodalpfn_amd`` loads, as a contiguous float32 array."""
    with torch.inference_mode():
        if kind == "feat":
            X = _randn((a["S"], a["T"], E), 7000 + 131 * a["S"] + a["T"])
            got = engines["layer"].feature_attention(0, X, a["prec"])
        elif kind == "item":
            X = _randn((a["S"], a["T"], E), 7100)
            got = engines["layer"].item_attention_block(0, X, a["N"], a["prec"])
        else:
            tok = _randn((a["S"], a["M"], E), 7200)
            got = engines["mixer"].cap(tok, a["prec"])
    return np.ascontiguousarray(got.float().cpu().numpy())


def digest(a: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def stored_output(kind: str, a: dict, out: np.ndarray):
    """The array kept beside the digest (S = 1 feature cases), or None."""
    if kind != "feat" or a["S"] != 1:
        return None
    if a["prec"] == PREC_F16:
        h = out.astype(np.float16)
        assert np.array_equal(h.astype(np.float32), out)  # the fp16 state, widened: float16 holds it exactly
        return h
    return out


def main():
    engines = make_engines()
    res = {}
    for name, kind, a in cases():
        out = run_case(engines, kind, a)
        assert np.isfinite(out).all(), name
        res[f"sha_{name}"] = digest(out)
        keep = stored_output(kind, a, out)
        if keep is not None:
            res[f"out_{name}"] = keep
    OUT.parent.mkdir(exist_ok=True)
    np.savez_compressed(OUT, **res)
    print(f"{len(cases())} cases -> {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
