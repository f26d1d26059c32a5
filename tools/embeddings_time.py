"""Timing of the last layer's three forms on one member of config C's shape (1838 train rows, 460 test rows, 21
features, MGM 64 + CAP 24, 12 layers) in the fp16 mode:

* ``forward(..., embeddings="both")``: the column form plus the two gather kernels;
* ``forward``: the pruned form (the default);
* ``forward`` with ``full_last_layer = True``: the last layer in full.

Device events around ``reps`` back-to-back calls after a warm-up; the three are alternated window by window, five
windows each, so drift shows up as spread and not as a difference.
    python tools/embeddings_time.py [out.txt]
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "golden")]

from synth import synth_image, synth_labels, synth_state_dict, synth_table  # noqa: E402

from multimodalpfn_amd import _lib  # noqa: E402
from multimodalpfn_amd.engine import HipEngine  # noqa: E402
from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec  # noqa: E402

S, N, F, REPS, WINDOWS = 2298, 1838, 21, 40, 5


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    cfg = ModelConfig(mgm_heads=64, cap_heads=24)
    eng = HipEngine(cfg, synth_state_dict(state_dict_spec(cfg), 2), torch.device("cuda"))
    x = torch.from_numpy(synth_table(S, F, 2, n_cat=18)).cuda()
    y = synth_labels(S, 6, 2)[:N]
    prec = _lib.PREC_F16
    tok = eng.mixer_tokens(torch.from_numpy(synth_image(S, 1, 2)).cuda(), prec)

    def full():
        eng.full_last_layer = True
        try:
            eng.forward(x, tok, y, prec, check_nan=False)
        finally:
            eng.full_last_layer = False

    forms = {
        'forward(embeddings="both"), column form': lambda: eng.forward(x, tok, y, prec, check_nan=False,
                                                                        embeddings="both"),
        "forward, pruned last layer": lambda: eng.forward(x, tok, y, prec, check_nan=False),
        "forward, full last layer": full,
    }
    with torch.inference_mode():
        for fn in forms.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(WINDOWS):
            for k, fn in forms.items():
                times[k].append(window(fn))
        eng.status()
    T = (F + 1) // 2 + tok.shape[1] + 1
    lines = [f"one member, S = {S}, N = {N}, T = {T}, {cfg.nlayers} layers, fp16 mode; ms per forward, best of "
             f"{WINDOWS} windows of {REPS} (all windows)"]
    for k, t in times.items():
        lines.append(f"  {k}: {min(t):.3f} ({', '.join(f'{v:.3f}' for v in t)})")
    print("\n".join(lines))
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
