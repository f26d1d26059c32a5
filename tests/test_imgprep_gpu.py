"""The image front end on the device (csrc/imgprep.hip behind include/mmpfn_modality.h) against the numpy restatement
of Pillow's 8-bit bilinear resize (tests/imgprep_cases.py; tests/test_imgprep_host.py pins that restatement to Pillow
bit for bit).  Everything here is compared with ``torch.equal``: the resize is integer arithmetic on host-built
tables, the scaling one table lookup, the bf16 rounding torch's own, and the tower behind the front end is fed the
same operand bits by both entry points -- so there is no tolerance to choose.

* the tap ``mmpfn_image_patches_rgb``, each case alone: ``resized`` and ``patches`` (fp32 and bf16, kpad 608 and 640),
  with guard rows past the end that must keep their bits;
* the tap on all cases of one output size in one ragged call, in two orders, against the single calls;
* geometry beyond the case list where the kernel takes another path: several column tiles, the widest accepted row
  (one source row per LDS chunk, taps too many for LDS), patch 8 and 16;
* the whole tower from pixels against the tower fed the restatement's fp32 images; the Python API; the refusals.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import imgprep_cases as ic
from multimodalpfn_amd import _lib
from multimodalpfn_amd.modality import DinoVisionTransformer, embed_images, embed_raw_images
from test_modality_kernels_gpu import _vit_state

pytestmark = pytest.mark.gpu

GUARD = 8                            # rows of A past the end that no call may touch
PAT16, PAT32, PAT8 = 0x7A5B, 0x7FA55AA5, 0xA5
_IDS = [ic.case_name(c) for c in ic.CASES]


@pytest.fixture(scope="module")
def tap():
    lib = _lib.load_library()
    enc = lib.mmpfn_enc_create(0, None)
    assert enc
    yield lib, enc
    lib.mmpfn_enc_destroy(enc)


@functools.lru_cache(maxsize=None)
def _ref(case, kind):
    """(input, the restatement's resize) of a case: computed once, shared, never modified."""
    src = ic.case_data(case, kind)
    out = ic.resize(src, case[2], case[3])
    src.setflags(write=False)
    out.setflags(write=False)
    return src, out


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _call(tap, images, oh, ow, patch, kpad, prec, want_rc=0):
    """One mmpfn_image_patches_rgb call -> (resized [B][oh][ow][3], patches [rows][kpad]) on the host; asserts that
    the guard bytes / rows kept their bits."""
    lib, enc = tap
    buf, offsets, sizes = ic.pack(images)
    dbuf = torch.from_numpy(buf).cuda()
    B = len(images)
    rows = B * (oh // patch) * (ow // patch)
    nres = B * oh * ow * 3
    resized = torch.full((nres + 4096,), PAT8, device="cuda", dtype=torch.uint8)
    bf = prec == _lib.PREC_BF16
    patches = torch.empty(rows + GUARD, kpad, device="cuda", dtype=torch.bfloat16 if bf else torch.float32)
    bits = patches.view(torch.int16 if bf else torch.int32)
    bits.fill_(PAT16 if bf else PAT32)
    rc = lib.mmpfn_image_patches_rgb(enc, dbuf.data_ptr(), _vp(offsets), _vp(sizes), B, oh, ow, patch, kpad,
                                     resized.data_ptr(), patches.data_ptr(), prec)
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, lib.mmpfn_enc_last_error(enc))
    assert bool((resized[nres:] == PAT8).all()), "bytes past the resized images were written"
    assert bool((bits[rows:] == (PAT16 if bf else PAT32)).all()), "rows past the end of A were written"
    if rc != 0:
        assert bool((resized == PAT8).all()) and bool((bits == (PAT16 if bf else PAT32)).all()), "a refused call wrote"
        return None, None
    return resized[:nres].reshape(B, oh, ow, 3).cpu(), patches[:rows].cpu()


def _expected_patches(resized_u8, patch, kpad, prec):
    a = torch.from_numpy(ic.im2col(ic.to_float_image(resized_u8), patch, kpad))
    return a.bfloat16() if prec == _lib.PREC_BF16 else a


def _assert_tap(tap, images, want, oh, ow, patch, kpads):
    want = np.stack(want)
    for prec in (_lib.PREC_F32, _lib.PREC_BF16):
        for kpad in kpads:
            resized, patches = _call(tap, images, oh, ow, patch, kpad, prec)
            assert torch.equal(resized, torch.from_numpy(want)), ("resized", prec, kpad,
                                                                  int((resized.numpy() != want).sum()))
            exp = _expected_patches(want, patch, kpad, prec)
            assert patches.dtype == exp.dtype and torch.equal(patches, exp), ("patches", prec, kpad)


@pytest.mark.parametrize("case", ic.CASES, ids=_IDS)
def test_tap_each_case_alone(tap, case):
    for kind in ic.KINDS:
        src, want = _ref(case, kind)
        _assert_tap(tap, [src], [want], case[2], case[3], 14, (608, 640))


def _groups():
    g = {}
    for c in ic.CASES:
        g.setdefault((c[2], c[3]), []).append(c)
    return {k: v for k, v in g.items() if len(v) > 1}


@pytest.mark.parametrize("size", sorted(_groups()), ids=lambda s: f"{s[0]}x{s[1]}")
def test_tap_ragged_batch_equals_single_calls(tap, size):
    """All cases of one output size in one call, in two orders: image b's rows equal its own single call's, so an
    offset, a table or an output row taken from a neighbour cannot hide."""
    oh, ow = size
    items = [(c, k) for c in _groups()[size] for k in (("random", "ones") if oh < 100 else ("random",))]
    single = {}
    for it in items:
        single[it] = _call(tap, [_ref(*it)[0]], oh, ow, 14, 640, _lib.PREC_BF16)
        assert torch.equal(single[it][0][0], torch.from_numpy(_ref(*it)[1].copy()))
    n = len(items)
    for order in (list(range(n)), [(5 * i + 3) % n for i in range(n)] if n % 5 else list(range(n))[::-1]):
        assert sorted(order) == list(range(n))
        batch = [items[i] for i in order]
        resized, patches = _call(tap, [_ref(*it)[0] for it in batch], oh, ow, 14, 640, _lib.PREC_BF16)
        per = patches.reshape(n, -1, 640)
        for b, it in enumerate(batch):
            assert torch.equal(resized[b], single[it][0][0]), (order, b, it)
            assert torch.equal(per[b], single[it][1]), (order, b, it)


# (source H, W, oh, ow, patch, kpad): the paths the case list does not reach
EXTRA = {
    "three_column_tiles": (20, 30, 14, 840, 14, 608),     # 60 patches across: tiles of 27, 27, 6
    "two_tiles_shrinking": (40, 3000, 28, 392, 14, 640),  # 28 patches: 27 + 1; 17 taps per pixel, held in LDS
    "widest_row": (2, 16384, 14, 28, 14, 608),            # one source row per chunk, 1173 taps read from the table
    "tallest_column": (16384, 164, 14, 14, 14, 608),      # 16384 source rows into one band (H = 99.9 W)
    "patch_16": (29, 27, 32, 48, 16, 768),
    "patch_8": (57, 55, 24, 16, 8, 192),
    "upscale_large": (5, 4, 70, 56, 14, 608),             # every source row feeds a whole band
}


@pytest.mark.parametrize("name", sorted(EXTRA))
def test_tap_other_paths(tap, name):
    H, W, oh, ow, patch, kpad = EXTRA[name]
    case = (H, W, oh, ow)
    src = ic.case_data(case, "random")
    _assert_tap(tap, [src], [ic.resize(src, oh, ow)], oh, ow, patch, (kpad,))


def test_tap_serves_either_output_alone(tap):
    lib, enc = tap
    case = ic.CASES[2]
    src, want = _ref(case, "random")
    buf, offsets, sizes = ic.pack([src])
    dbuf = torch.from_numpy(buf).cuda()
    resized = torch.zeros(28, 28, 3, device="cuda", dtype=torch.uint8)
    patches = torch.zeros(4, 608, device="cuda", dtype=torch.float32)
    args = (enc, dbuf.data_ptr(), _vp(offsets), _vp(sizes), 1, 28, 28, 14, 608)
    assert lib.mmpfn_image_patches_rgb(*args, resized.data_ptr(), None, _lib.PREC_F32) == 0
    assert lib.mmpfn_image_patches_rgb(*args, None, patches.data_ptr(), _lib.PREC_F32) == 0
    torch.cuda.synchronize()
    assert torch.equal(resized.cpu(), torch.from_numpy(want.copy()))
    assert torch.equal(patches.cpu(), _expected_patches(want[None], 14, 608, _lib.PREC_F32))
    assert lib.mmpfn_image_patches_rgb(*args, None, None, _lib.PREC_F32) == _lib.MMPFN_ERR_INVALID


# ------------------------------------------------------------------------------------------------ whole tower
TOWER_SIZES = [(13, 29), (57, 55), (100, 336), (28, 42), (200, 31)]  # five ragged images -> 28 x 42


def _tower(dim, heads, hidden, prec, chans=3, seed=61):
    c = dict(dim=dim, heads=heads, hidden=hidden, patch=14, chans=chans, grid=37, depth=1, init_values=1.0, offset=0.1,
             seed=seed)
    m = DinoVisionTransformer(img_size=37 * 14, patch_size=14, in_chans=chans, embed_dim=dim, depth=1, num_heads=heads,
                              mlp_ratio=hidden / dim, init_values=1.0, block_chunks=0, interpolate_offset=0.1,
                              precision=prec)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _vit_state(c).items()})
    return m


def _tower_images(oh, ow):
    imgs = [ic.case_data((H, W, oh, ow), "random") for H, W in TOWER_SIZES]
    x = torch.from_numpy(ic.to_float_image(np.stack([ic.resize(a, oh, ow) for a in imgs])))
    return imgs, x


@pytest.mark.parametrize("geom", [(256, 4, 768, "bf16"), (768, 12, 3072, "f32")], ids=["d256_bf16", "d768_f32"])
def test_tower_from_pixels_equals_tower_from_resized_images(geom):
    """mmpfn_vit_forward_rgb against mmpfn_vit_forward fed the restatement's fp32 images: the same operand bits reach
    the same kernels, so cls and every token are equal, on the all-token path and on the CLS-only path."""
    dim, heads, hidden, prec = geom
    imgs, x = _tower_images(28, 42)
    m = _tower(dim, heads, hidden, prec)
    try:
        want = m.forward_features(x.cuda())
        got = m.forward_features_from_pixels(imgs, (28, 42))
        want_cls = m.cls_embeddings(x.cuda())
        got_cls = m.cls_embeddings_from_pixels(imgs, (28, 42))
        torch.cuda.synchronize()
        assert got["x_norm_patchtokens"].shape == (5, 6, dim)
        assert bool(torch.isfinite(want["x_norm_clstoken"]).all())
        for key in ("x_norm_clstoken", "x_norm_patchtokens"):
            assert torch.equal(got[key], want[key]), key
        assert torch.equal(got_cls, want_cls)
    finally:
        m._drop_contexts()


def test_embed_raw_images_equals_embed_images():
    """Three rows of two images of six sizes: the raw-pixel helper equals embed_images on the host-prepared array."""
    shapes = [(13, 29), (57, 55), (100, 336), (28, 28), (200, 31), (1, 1)]
    raw = [ic.case_data((H, W, 28, 28), "random") for H, W in shapes]
    rows = [[raw[0], raw[1]], [torch.from_numpy(raw[2]), raw[3]], [raw[4], raw[5]]]
    host = ic.to_float_image(np.stack([ic.resize(a, 28, 28) for a in raw])).reshape(3, 2, 3, 28, 28)
    m = _tower(256, 4, 768, "bf16")
    try:
        want = embed_images(m, host)
        got = embed_raw_images(m, rows, img_size=28)
        assert got.shape == (3, 2, 256) and got.device.type == "cpu"
        assert torch.equal(got, want)
        one = embed_raw_images(m, rows, img_size=28, batch_size=1)  # a batch per row
        assert one.shape == (3, 2, 256) and bool(torch.isfinite(one).all())
    finally:
        m._drop_contexts()


# ------------------------------------------------------------------------------------------------ refusals
def test_tap_refusals_leave_the_context_usable(tap):
    lib, enc = tap
    good = ic.case_data((13, 29, 28, 28), "random")
    want = ic.resize(good, 28, 28)

    def serves():
        resized, _ = _call(tap, [good], 28, 28, 14, 608, _lib.PREC_F32)
        assert torch.equal(resized[0], torch.from_numpy(want))

    serves()
    tall = np.zeros((1001, 10, 3), np.uint8)  # H > 100 * W (1000 x 10 is the last accepted aspect: a case above)
    _call(tap, [good, tall], 28, 28, 14, 608, _lib.PREC_F32, want_rc=_lib.MMPFN_ERR_INVALID)
    assert b"100" in lib.mmpfn_enc_last_error(enc)
    serves()
    for empty in (np.zeros((0, 5, 3), np.uint8), np.zeros((5, 0, 3), np.uint8)):  # a zero side
        _call(tap, [good, empty], 28, 28, 14, 608, _lib.PREC_F32, want_rc=_lib.MMPFN_ERR_INVALID)
        assert b"empty" in lib.mmpfn_enc_last_error(enc)
        serves()
    _call(tap, [good], 30, 28, 14, 608, _lib.PREC_F32, want_rc=_lib.MMPFN_ERR_INVALID)   # oh not a multiple of the patch
    serves()
    _call(tap, [good], 28, 30, 14, 608, _lib.PREC_F32, want_rc=_lib.MMPFN_ERR_INVALID)
    serves()
    _call(tap, [good], 28, 28, 14, 576, _lib.PREC_F32, want_rc=_lib.MMPFN_ERR_INVALID)   # kpad < 3 * 14 * 14 = 588
    serves()
    _call(tap, [good], 28, 28, 14, 600, _lib.PREC_F32, want_rc=_lib.MMPFN_ERR_INVALID)   # kpad not a multiple of 32
    serves()
    _call(tap, [good], 34, 34, 17, 896, _lib.PREC_F32, want_rc=_lib.MMPFN_ERR_INVALID)   # patch over 16
    serves()
    _call(tap, [good], 28, 28, 14, 608, 7, want_rc=_lib.MMPFN_ERR_INVALID)               # unknown precision
    serves()


def test_tower_refusals_leave_the_context_usable():
    imgs, x = _tower_images(28, 42)
    m = _tower(256, 4, 768, "bf16")
    try:
        want = m.cls_embeddings(x.cuda())
        with pytest.raises(ValueError, match="100"):
            m.cls_embeddings_from_pixels(imgs + [np.zeros((1001, 10, 3), np.uint8)], (28, 42))
        with pytest.raises(ValueError, match="empty"):
            m.cls_embeddings_from_pixels(imgs + [np.zeros((0, 4, 3), np.uint8)], (28, 42))
        with pytest.raises(ValueError, match="patch"):
            m.cls_embeddings_from_pixels(imgs, (30, 42))
        with pytest.raises(ValueError):
            m.cls_embeddings_from_pixels([np.zeros((4, 4, 4), np.uint8)], (28, 42))
        assert torch.equal(m.cls_embeddings_from_pixels(imgs, (28, 42)), want)
    finally:
        m._drop_contexts()
    g = _tower(256, 4, 768, "bf16", chans=1, seed=62)  # in_chans != 3
    try:
        x1 = x[:, :1].contiguous().cuda()
        want = g.cls_embeddings(x1)
        with pytest.raises(ValueError, match="in_chans"):
            g.cls_embeddings_from_pixels(imgs, (28, 42))
        assert torch.equal(g.cls_embeddings(x1), want)
    finally:
        g._drop_contexts()
