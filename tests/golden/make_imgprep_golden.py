"""Writes tests/golden/imgprep/: Pillow's own ``resize(..., Image.BILINEAR)`` of every case of tests/imgprep_cases.py.

Needs only Pillow and numpy (the case list and the seeded inputs come from imgprep_cases.py, which is numpy alone):

    python tests/golden/make_imgprep_golden.py

Per case one ``imgprep_<H>x<W>_to_<oh>x<ow>.npz``: ``out_<kind>`` = Pillow's uint8 [oh][ow][3] for the random, all-255
and all-0 input, ``in_random`` = the random input -- or, where input and output together would pass 1 MB,
``sha_random`` = its SHA-256 (the input is regenerated from the case's seed and checked against it) -- and
``pil_version``.  The constant inputs are never stored.
"""

import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from imgprep_cases import CASES, GOLDEN_DIR, KINDS, case_data, case_name, digest  # noqa: E402

LIMIT = 1 << 20


def pillow_resize(a: np.ndarray, oh: int, ow: int) -> np.ndarray:
    return np.array(Image.fromarray(a, "RGB").resize((ow, oh), Image.BILINEAR), dtype=np.uint8)


def main() -> None:
    GOLDEN_DIR.mkdir(parents=True, exist_ok=True)
    total = 0
    for case in CASES:
        _, _, oh, ow = case
        rec = {"pil_version": np.array(PIL.__version__)}
        for kind in KINDS:
            src = case_data(case, kind)
            out = pillow_resize(src, oh, ow)
            rec[f"out_{kind}"] = out
            if kind == "random" and src.nbytes + out.nbytes <= LIMIT:
                rec[f"in_{kind}"] = src
            else:
                rec[f"sha_{kind}"] = np.array(digest(src))
        path = GOLDEN_DIR / f"imgprep_{case_name(case)}.npz"
        np.savez_compressed(path, **rec)
        total += path.stat().st_size
        print(f"{path.name}: {path.stat().st_size} bytes")
    print(f"Pillow {PIL.__version__}; {total} bytes in all")
    assert total < 2 << 20


if __name__ == "__main__":
    main()
