"""Image front end (SURVEY.md §8(f)4'), CPU side: the numpy restatement of Pillow's 8-bit bilinear resize
(tests/imgprep_cases.py) against Pillow's recorded outputs and Pillow itself, the library's host-built coefficient
tables against the restatement's, the scaled pixel values, the C-ABI table, and what bit equality catches."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import imgprep_cases as ic
from helpers import report
from multimodalpfn_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "mmpfn_modality.h"
NEW_SYMBOLS = ["mmpfn_resize_coeffs", "mmpfn_pixel_scale_table", "mmpfn_image_patches_rgb", "mmpfn_vit_forward_rgb"]

_IDS = [ic.case_name(c) for c in ic.CASES]


@pytest.mark.parametrize("case", ic.CASES, ids=_IDS)
def test_restatement_equals_pillow_fixture(case):
    fx, version = ic.load_fixture(case)
    _, _, oh, ow = case
    for kind, (src, want) in fx.items():
        assert src.shape == (case[0], case[1], 3) and want.shape == (oh, ow, 3)
        got = ic.resize(src, oh, ow)
        assert np.array_equal(got, want), (kind, version, int((got != want).sum()))


@pytest.mark.parametrize("case", ic.CASES, ids=_IDS)
def test_restatement_equals_installed_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    _, _, oh, ow = case
    for kind in ic.KINDS:
        src = ic.case_data(case, kind)
        want = np.array(Image.fromarray(src, "RGB").resize((ow, oh), Image.BILINEAR), dtype=np.uint8)
        got = ic.resize(src, oh, ow)
        assert np.array_equal(got, want), (kind, int((got != want).sum()))


def _pairs():
    p = set(ic.EXTRA_PAIRS)
    for H, W, oh, ow in ic.CASES:
        p.add((H, oh))
        p.add((W, ow))
    return sorted(p)


@pytest.mark.parametrize("pair", _pairs(), ids=lambda p: f"{p[0]}to{p[1]}")
def test_library_tables_equal_the_restatement(pair):
    lib = _lib.load_library()
    in_size, out_size = pair
    k, bounds, _ = ic.coeffs(in_size, out_size)
    ks = ctypes.c_int(-1)
    assert lib.mmpfn_resize_coeffs(in_size, out_size, None, None, ctypes.byref(ks)) == 0  # k == NULL: ksize alone
    assert ks.value == k.shape[1]
    GUARD = 64
    gk = np.full(k.size + GUARD, -7, np.int32)
    gb = np.full(bounds.size + GUARD, -7, np.int32)
    ks2 = ctypes.c_int(-1)
    assert lib.mmpfn_resize_coeffs(in_size, out_size, gk.ctypes.data_as(ctypes.c_void_p),
                                   gb.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ks2)) == 0
    assert ks2.value == k.shape[1]
    assert np.array_equal(gk[:k.size].reshape(k.shape), k)
    assert np.array_equal(gb[:bounds.size].reshape(bounds.shape), bounds)
    assert (gk[k.size:] == -7).all() and (gb[bounds.size:] == -7).all()
    sums = k.astype(np.int64).sum(1)
    assert int(np.abs(sums - (1 << ic.PRECISION_BITS)).max()) <= 2  # 2^22 +- 2, not renormalised


def test_library_refuses_sizes_outside_the_contract():
    lib = _lib.load_library()
    ks = ctypes.c_int(0)
    for a, b in [(0, 14), (14, 0), (ic.MAX_SIDE + 1, 14), (14, ic.MAX_SIDE + 1), (-1, 14)]:
        assert lib.mmpfn_resize_coeffs(a, b, None, None, ctypes.byref(ks)) == _lib.MMPFN_ERR_INVALID
    assert lib.mmpfn_resize_coeffs(10, 14, None, None, None) == _lib.MMPFN_ERR_INVALID
    one = np.zeros(64, np.int32)
    assert lib.mmpfn_resize_coeffs(10, 14, one.ctypes.data_as(ctypes.c_void_p), None,
                                   ctypes.byref(ks)) == _lib.MMPFN_ERR_INVALID  # k without bounds


def test_scaled_pixel_values_are_the_correctly_rounded_division():
    lib = _lib.load_library()
    got = np.full(256 + 8, -1.0, np.float32)
    assert lib.mmpfn_pixel_scale_table(got.ctypes.data_as(ctypes.c_void_p)) == 0
    want = np.array([np.float32(v) / np.float32(255) for v in range(256)], np.float32)
    assert np.array_equal(got[:256].view(np.uint32), want.view(np.uint32))
    assert (got[256:] == -1.0).all()
    assert np.array_equal(ic.scale_table().view(np.uint32), want.view(np.uint32))
    exact = np.array([float(np.float64(v) / 255.0) for v in range(256)])  # correctly rounded: nearest fp32 of v / 255
    assert np.array_equal(want, exact.astype(np.float32))
    assert lib.mmpfn_pixel_scale_table(None) == _lib.MMPFN_ERR_INVALID


def test_new_symbols_are_in_the_header_and_the_binding_table():
    syms = set(re.findall(r"\b(mmpfn_[a-z_]+)\s*\(", HEADER.read_text()))
    names = {n for n, _, _ in _lib.MODALITY_SIGNATURES}
    lib = _lib.load_library()
    for s in NEW_SYMBOLS:
        assert s in syms, s
        assert s in names, s
        assert hasattr(lib, s), s
    assert lib.mmpfn_image_patches_rgb(None, None, None, None, 1, 14, 14, 14, 608, None, None, 0) == _lib.MMPFN_ERR_INVALID
    assert lib.mmpfn_vit_forward_rgb(None, None, None, None, 1, 14, 14, None, None, 0) == _lib.MMPFN_ERR_INVALID
    text = HEADER.read_text()
    for cite in ("pad_ufes_20.py:53-61", "cbis_ddsm.py:71-81", "petfinder.py:85-95"):
        assert cite in text, cite


SENS_CASE = (450, 600, 336, 336)


@pytest.mark.parametrize("variant", ["double_weights", "no_rounding_between", "vertical_first", "unscaled_support"])
def test_bit_equality_catches_a_wrong_resize(variant):
    """Each deliberately wrong form changes output bytes of the 450 x 600 case: an exact comparison sees it."""
    src = ic.case_data(SENS_CASE, "random")
    good = ic.resize(src, 336, 336)
    bad = ic.resize(src, 336, 336, variant=variant)
    n = int((good != bad).sum())
    step = int(np.abs(good.astype(int) - bad.astype(int)).max())
    report(f"imgprep sensitivity {variant}: {n} of {good.size} bytes differ (largest step {step})")
    assert n >= 1


def test_bit_equality_catches_a_reciprocal_multiply():
    """u8 * (1 / 255.f) instead of u8 / 255.f changes some of the values the tower is handed."""
    u8 = ic.resize(ic.case_data(SENS_CASE, "random"), 336, 336)
    good = ic.to_float_image(u8)
    bad = np.ascontiguousarray(np.moveaxis(u8.astype(np.float32) * (np.float32(1) / np.float32(255)), -1, -3))
    n = int((good.view(np.uint32) != bad.view(np.uint32)).sum())
    nv = int((ic.scale_table() != np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))).sum())
    report(f"imgprep sensitivity reciprocal: {n} of {good.size} values differ ({nv} of the 256 byte values)")
    assert n >= 1


def test_im2col_restatement_matches_conv_weight_flattening():
    """ic.im2col's column order is Conv2d's weight flattening: A . W^T equals the strided convolution."""
    torch = pytest.importorskip("torch")
    r = np.random.default_rng(5)
    x = r.integers(0, 8, (2, 3, 28, 42)).astype(np.float32)
    w = r.integers(-3, 4, (5, 3, 14, 14)).astype(np.float32)
    a = ic.im2col(x, 14, 608)
    assert a.shape == (2 * 2 * 3, 608) and not a[:, 588:].any()
    got = a[:, :588] @ w.reshape(5, -1).T
    want = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), stride=14).permute(0, 2, 3, 1).reshape(-1, 5)
    assert np.array_equal(got, want.numpy())
