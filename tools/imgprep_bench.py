"""Measures the image front end (csrc/imgprep.hip) on the device; reported in DESIGN.md §3, not asserted anywhere.

    python tools/imgprep_bench.py [--batch 128] [--rounds 5] [--out profiles/r12/imgprep_bench.json]

1. Tower rate, device-resident input: ViT-B/14 (seeded weights), bf16 mode, ``mmpfn_vit_forward_rgb`` from 450 x 600
   and 1500 x 2000 sources against ``mmpfn_vit_forward`` on pre-resized fp32 336 x 336 images, alternated within each
   round so that all three see the same machine state; images/s, median and spread over the rounds.
2. The front end alone (``mmpfn_image_patches_rgb``, A operand only): time per image next to the bytes it has to
   move (source read once + A written).
3. End to end from host memory: ``embed_raw_images`` from numpy arrays against Pillow on 16 threads feeding
   ``embed_images`` (the host path a user has without the front end).

Times are device events around several calls after a warm-up of every shape (1, 2) or a host clock around work that
ends in the device-to-host copy of the embeddings (3).  Without a GPU the tool fails; there is no CPU path.
"""

from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from multimodalpfn_amd import _lib  # noqa: E402
from multimodalpfn_amd.modality import embed_images, embed_raw_images, vit_base  # noqa: E402

IMG = 14 * 24
SOURCES = [(450, 600), (1500, 2000)]


def seeded_vit_base():
    m = vit_base(patch_size=14, img_size=518, init_values=1.0, num_register_tokens=0, block_chunks=0, precision="bf16")
    g = torch.Generator().manual_seed(7)
    sd = {}
    for k, v in m.state_dict().items():
        if k.endswith("norm1.weight") or k.endswith("norm2.weight") or k == "norm.weight":
            sd[k] = torch.ones_like(v)
        elif k.endswith("gamma"):
            sd[k] = torch.full_like(v, 0.5)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.02
    m.load_state_dict(sd)
    return m


def device_time(fn, calls: int) -> float:
    """Seconds per call: device events around ``calls`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def packed(B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, device="cuda", generator=g)
    offsets = (np.arange(B, dtype=np.int64) * (H * W * 3))
    sizes = np.tile(np.array([[H, W]], np.int32), (B, 1))
    return buf, offsets, sizes


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--host-images", type=int, default=512)
    ap.add_argument("--sections", default="tower,front,host", help="which of the three measurements to take")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("imgprep_bench needs a ROCm GPU")
    B = args.batch
    m = seeded_vit_base()
    ctx = m.context()
    lib, enc = ctx.lib, ctx.enc
    ctx.bind()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "rounds": args.rounds, "calls_per_round": args.calls}

    # ---- 1. tower rate, device-resident input
    x = torch.rand(B, 3, IMG, IMG, device="cuda")
    cls = torch.empty(B, 768, device="cuda")
    src = {hw: packed(B, *hw, seed=hw[0]) for hw in SOURCES}

    def run_f32():
        ctx._check(lib.mmpfn_vit_forward(enc, x.data_ptr(), B, IMG, IMG, cls.data_ptr(), None, _lib.PREC_BF16), "fwd")

    def run_rgb(hw):
        buf, off, sz = src[hw]
        return lambda: ctx._check(lib.mmpfn_vit_forward_rgb(enc, buf.data_ptr(), vp(off), vp(sz), B, IMG, IMG,
                                                            cls.data_ptr(), None, _lib.PREC_BF16), "fwd_rgb")

    modes = {"fp32_336x336": run_f32}
    modes.update({f"rgb_{h}x{w}": run_rgb((h, w)) for h, w in SOURCES})
    if "tower" not in args.sections:
        modes = {}
    for fn in modes.values():  # warm every shape
        fn()
        fn()
    torch.cuda.synchronize()
    rates = {k: [] for k in modes}
    for _ in range(args.rounds):
        for k, fn in modes.items():
            rates[k].append(B / device_time(fn, args.calls))
    res["tower_images_per_s"] = {k: summary(v) for k, v in rates.items()}

    # ---- 2. the front end alone
    rows = B * (IMG // 14) ** 2
    A = torch.empty(rows, 640, device="cuda", dtype=torch.bfloat16)
    front = {}
    for hw in SOURCES if "front" in args.sections else []:
        buf, off, sz = src[hw]

        def tap():
            ctx._check(lib.mmpfn_image_patches_rgb(enc, buf.data_ptr(), vp(off), vp(sz), B, IMG, IMG, 14, 640, None,
                                                   A.data_ptr(), _lib.PREC_BF16), "tap")

        tap()
        torch.cuda.synchronize()
        ts = [device_time(tap, 10) for _ in range(args.rounds)]
        nbytes = buf.numel() + A.numel() * 2
        t = statistics.median(ts)
        front[f"{hw[0]}x{hw[1]}"] = {"us_per_image": summary([v / B * 1e6 for v in ts]), "bytes_per_image": nbytes // B,
                                     "GB_per_s": nbytes / t * 1e-9}
    res["front_end_alone"] = front

    # ---- 3. end to end from host memory
    N = args.host_images
    r = np.random.default_rng(3)
    host = [r.integers(0, 256, (450, 600, 3), dtype=np.uint8) for _ in range(16)]
    rows_raw = [[host[i % 16]] for i in range(N)]
    if "host" in args.sections:
        embed_raw_images(m, rows_raw[:B], IMG, batch_size=B)
    e2e = {"raw": [], "pillow16": []}
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def pil_one(a):
        return np.array(Image.fromarray(a, "RGB").resize((IMG, IMG), Image.BILINEAR), dtype=np.float32)

    for _ in range(max(2, args.rounds // 2) if "host" in args.sections else 0):
        t0 = time.perf_counter()
        out = embed_raw_images(m, rows_raw, IMG, batch_size=B)
        e2e["raw"].append(N / (time.perf_counter() - t0))
        if Image is not None:
            t0 = time.perf_counter()
            with ThreadPoolExecutor(16) as pool:
                arr = np.stack(list(pool.map(pil_one, [row[0] for row in rows_raw])))
            arr /= 255.0
            arr = np.ascontiguousarray(arr.transpose(0, 3, 1, 2))[:, None]
            ref = embed_images(m, arr, batch_size=B)
            e2e["pillow16"].append(N / (time.perf_counter() - t0))
            res["host_paths_equal"] = bool(torch.equal(out, ref))
    res["end_to_end_images_per_s"] = {k: (summary(v) if v else "not measured") for k, v in e2e.items()}
    res["host_images"] = N
    line = json.dumps(res)
    print(line)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(res, indent=1) + "\n")
    m._drop_contexts()


if __name__ == "__main__":
    main()
