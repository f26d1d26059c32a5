"""The image front end's contract, restated in numpy, and its cases (tests/test_imgprep_host.py,
tests/test_imgprep_gpu.py, tests/golden/make_imgprep_golden.py).

The reference resizes every decoded picture with Pillow in front of its image tower
(mmpfn/datasets/pad_ufes_20.py:53-61, cbis_ddsm.py:71-81, petfinder.py:85-95):

    img = np.array(img.convert("RGB").resize((img_size, img_size), Image.BILINEAR), dtype=np.float32); images /= 255.0

Pillow's 8-bit resize is integer arithmetic on 22-bit fixed-point coefficients (libImaging/Resample.c), so it can be
restated exactly.  ``resize`` below is that restatement: the yardstick of the GPU tests, itself pinned bit for bit to
Pillow's recorded outputs under tests/golden/imgprep/.  Per axis, ``inS -> outS``, all in IEEE double in this order:

    scale = inS / outS; fs = max(scale, 1.0); support = 1.0 * fs; ksize = (int)ceil(support) * 2 + 1
    center = (xx + 0.5) * scale; ss = 1.0 / fs
    xmin = max((int)(center - support + 0.5), 0); xmax = min((int)(center + support + 0.5), inS) - xmin
    w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|), x < xmax; ww = left-to-right sum; w[x] /= ww if ww != 0
    k[x] = (int)(0.5 + w[x] * 2^22)
    out = clamp((2^21 + sum pixel[xmin + x] * k[x]) >> 22, 0, 255)

The horizontal pass runs first, the vertical pass on its uint8 result; a pass whose sizes are equal is skipped.  The
tower is handed ``float32(u8) / float32(255)``.  Images with H > 100 * W are outside the contract (Pillow's result
there equals the vertical-first order) and the device path refuses them.
"""

from __future__ import annotations

import hashlib
import math
from pathlib import Path

import numpy as np

GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "imgprep"
PRECISION_BITS = 22
MAX_SIDE = 16384

# (source H, source W, output oh, output ow)
CASES = [
    (1, 1, 28, 28),
    (2, 3, 28, 14),
    (13, 29, 28, 28),
    (28, 28, 28, 28),       # both passes skipped
    (336, 100, 28, 28),
    (100, 336, 42, 28),
    (29, 27, 28, 28),
    (57, 55, 28, 28),
    (3, 500, 14, 28),
    (1000, 10, 14, 14),     # the last accepted aspect
    (450, 600, 336, 336),
    (767, 1023, 336, 336),
]
KINDS = ("random", "ones", "zeros")
# (in, out) pairs whose tables the library must reproduce, beyond those of CASES
EXTRA_PAIRS = [(MAX_SIDE, 14), (14, MAX_SIDE)]


def case_name(case) -> str:
    H, W, oh, ow = case
    return f"{H}x{W}_to_{oh}x{ow}"


def case_seed(case) -> int:
    H, W, oh, ow = case
    return 7000003 + H * 40009 + W * 131 + oh * 7 + ow


def case_data(case, kind: str) -> np.ndarray:
    """uint8 [H][W][3]: uniform random bytes whose upper half of the rows is 0 / 255 at random per pixel (the clip and
    the rounding at one half), or all 255, or all 0."""
    H, W, _, _ = case
    if kind == "ones":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "zeros":
        return np.zeros((H, W, 3), np.uint8)
    r = np.random.default_rng(case_seed(case))
    a = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    half = H // 2
    if half:
        a[:half] = r.integers(0, 2, (half, W, 1), dtype=np.uint8) * np.uint8(255)
    return a


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------ coefficient tables
def coeffs(in_size: int, out_size: int, *, scaled_support: bool = True):
    """(k int32 [out][ksize], bounds int32 [out][2] = (xmin, xmax), weights float64 [out][ksize]) of one axis.
    ``scaled_support=False`` is the sensitivity variant whose support ignores the shrink factor."""
    scale = in_size / out_size
    fs = max(scale, 1.0) if scaled_support else 1.0
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    k = np.zeros((out_size, ksize), np.int32)
    wd = np.zeros((out_size, ksize), np.float64)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss))
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x in range(xmax):
            k[xx, x] = int(0.5 + w[x] * (1 << PRECISION_BITS))
            wd[xx, x] = w[x]
        bounds[xx] = (xmin, xmax)
    return k, bounds, wd


def _gather(a: np.ndarray, bounds: np.ndarray, ksize: int) -> np.ndarray:
    """a [in][...] -> [out][ksize][...]: the taps of every output index (indices past the count are clamped; their
    coefficients are zero)."""
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(ksize)[None, :], a.shape[0] - 1)
    return a[idx]


def _pass_u8(a: np.ndarray, out_size: int, **kw) -> np.ndarray:
    """One pass along axis 0 of uint8 ``a``: Pillow's integers."""
    k, bounds, _ = coeffs(a.shape[0], out_size, **kw)
    taps = _gather(a, bounds, k.shape[1]).astype(np.int64)
    acc = (taps * k.astype(np.int64).reshape(k.shape + (1,) * (a.ndim - 1))).sum(1) + (1 << (PRECISION_BITS - 1))
    assert int(acc.max()) < 2 ** 31  # Pillow's accumulator is an int32
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass_real(a: np.ndarray, out_size: int, *, integer_k: bool) -> np.ndarray:
    """One pass along axis 0 in float64, unrounded: with the integer coefficients / 2^22 or the double weights."""
    k, bounds, wd = coeffs(a.shape[0], out_size)
    w = k.astype(np.float64) / (1 << PRECISION_BITS) if integer_k else wd
    taps = _gather(a, bounds, k.shape[1]).astype(np.float64)
    return (taps * w.reshape(w.shape + (1,) * (a.ndim - 1))).sum(1)


def _round_u8(x: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)


def resize(img: np.ndarray, oh: int, ow: int, variant: str | None = None) -> np.ndarray:
    """Pillow's ``resize((ow, oh), BILINEAR)`` of uint8 [H][W][3] -> uint8 [oh][ow][3].  ``variant`` selects one of the
    deliberately wrong forms of the sensitivity test (None: the contract)."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W, _ = img.shape
    if variant == "double_weights":  # weights left in double, rounded once per pass
        a = img
        if W != ow:
            a = _round_u8(_pass_real(a.transpose(1, 0, 2), ow, integer_k=False)).transpose(1, 0, 2)
        return _round_u8(_pass_real(a, oh, integer_k=False)) if H != oh else a
    if variant == "no_rounding_between":  # the horizontal pass's result kept unrounded
        a = _pass_real(img.transpose(1, 0, 2), ow, integer_k=True).transpose(1, 0, 2)
        return _round_u8(_pass_real(a, oh, integer_k=True))
    kw = {"scaled_support": False} if variant == "unscaled_support" else {}
    assert variant in (None, "vertical_first", "unscaled_support"), variant

    def horiz(a):
        return a if a.shape[1] == ow else _pass_u8(a.transpose(1, 0, 2), ow, **kw).transpose(1, 0, 2)

    def vert(a):
        return a if a.shape[0] == oh else _pass_u8(a, oh, **kw)

    return horiz(vert(img)) if variant == "vertical_first" else vert(horiz(img))


def scale_table() -> np.ndarray:
    """What a byte becomes: float32(v) / float32(255), one correctly rounded fp32 division."""
    return np.arange(256, dtype=np.float32) / np.float32(255)


def to_float_image(u8: np.ndarray) -> np.ndarray:
    """uint8 [..., H, W, 3] -> the tower's fp32 [..., 3, H, W] input."""
    return np.ascontiguousarray(np.moveaxis(scale_table()[u8], -1, -3))


def im2col(x: np.ndarray, patch: int, kpad: int) -> np.ndarray:
    """fp32 [B][3][H][W] -> the patch GEMM's A operand [B * gh * gw][kpad]: row (b, py, px), column
    c * P * P + ky * P + kx, zero past 3 * P * P."""
    B, C, H, W = x.shape
    gh, gw = H // patch, W // patch
    p = x.reshape(B, C, gh, patch, gw, patch).transpose(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * patch * patch)
    out = np.zeros((B * gh * gw, kpad), np.float32)
    out[:, :p.shape[1]] = p
    return out


def pack(images):
    """A ragged batch as the C-ABI takes it: (bytes uint8 [total], offsets int64 [B], sizes int32 [B][2])."""
    sizes = np.array([im.shape[:2] for im in images], np.int32).reshape(-1, 2)
    lens = np.array([im.size for im in images], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    buf = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images]) if len(images) else np.zeros(0, np.uint8)
    return buf, offsets, sizes


def load_fixture(case):
    """The recorded fixture of a case: {kind: (input, Pillow's output)} and the Pillow version that wrote it."""
    z = np.load(GOLDEN_DIR / f"imgprep_{case_name(case)}.npz")
    out = {}
    for kind in KINDS:
        if f"in_{kind}" in z.files:
            src = z[f"in_{kind}"]
        else:  # regenerated from the seed; the recorded digest pins the generator
            src = case_data(case, kind)
            assert digest(src) == str(z[f"sha_{kind}"]), "the input generator no longer gives the recorded bytes"
        out[kind] = (src, z[f"out_{kind}"])
    return out, str(z["pil_version"])
