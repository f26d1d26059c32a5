"""GPU: the feature block, the item q | k | v projection and the CAP K | V projection give the bits they gave before
the feature block's data movement changed.

``feat_rows_kernel`` keeps the finished O^T fragments of a three-tile row's last tile in LDS instead of in (spilled)
registers, moves its weight images through a ring of 13-KB slots and runs the out-projection on two token tiles per
weight fragment.  None of that touches an MFMA chain, its order or its operands, so every output must equal, bit for
bit, what the build before the change produced: tests/golden/featrow/featrow_bits.npz, recorded from that build by
tests/golden/make_featrow_bits.py (which also defines the cases and what is stored: a SHA-256 of every output, since
the outputs themselves are ten times a committed file's limit, and the S = 1 feature outputs in full).  The item
block and the CAP pooler are pinned with it: their projections (``rowgemm_qkv2_kernel``, ``rowgemm_ln_store_kernel``)
stage output tiles through LDS, and a change of that staging's addressing has to leave these bits alone.
"""

import numpy as np
import pytest

import make_featrow_bits as fb

pytestmark = pytest.mark.gpu

CASES = fb.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(fb.OUT)


@pytest.fixture(scope="module")
def engines():
    engs = fb.make_engines()
    yield engs
    for e in engs.values():
        e.close()


def test_fixture_holds_every_case(golden):
    assert {f"sha_{name}" for name, _, _ in CASES} <= set(golden.files)


@pytest.mark.parametrize("name,kind,args", CASES, ids=[c[0] for c in CASES])
def test_same_bits_as_recorded(golden, engines, name, kind, args):
    out = fb.run_case(engines, kind, args)
    keep = fb.stored_output(kind, args, out)
    if keep is not None:  # element by element first: says where
        want = golden[f"out_{name}"]
        assert keep.dtype == want.dtype and keep.shape == want.shape
        diff = np.flatnonzero(keep.view(np.uint16 if keep.dtype == np.float16 else np.uint32).ravel()
                              != want.view(np.uint16 if want.dtype == np.float16 else np.uint32).ravel())
        assert diff.size == 0, (name, diff.size, diff[:8])
    assert np.array_equal(fb.digest(out), golden[f"sha_{name}"]), name
