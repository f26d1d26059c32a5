"""Codegen guard for the feature block's last-layer form (CPU: hipcc cross-compiles gfx950 here).

``feat_rows_kernel<NT, F16, LAST = true>`` (featrow.hip) runs in a forward's pruned last layer and computes token T-1
alone.  The kernel is register-bound (the full three-tile forms spill, pinned in test_codegen.py), so the variant
must spill no more than the limit pinned for the full instantiation of the same tile count and state type."""

from pathlib import Path

import pytest

from test_codegen import HIPCC, _resources

pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

# the full forms' limits of test_codegen.test_layer_kernels_spills (bf16 / fp32 state, fp16 state)
FULL_LIMIT = {"Lb0E": 16, "Lb1E": 32}


@pytest.fixture(scope="module")
def featrow_spills():
    return _resources("featrow.hip", ["-fno-honor-nans"])


@pytest.mark.parametrize("f16", ["Lb0E", "Lb1E"])
def test_last_layer_form_spills_no_more_than_the_full_one(featrow_spills, f16):
    last = {k: v for k, v in featrow_spills.items() if f"feat_rows_kernelILi3E{f16}Lb1E" in k}
    full = {k: v for k, v in featrow_spills.items() if f"feat_rows_kernelILi3E{f16}Lb0E" in k}
    assert len(last) == 1 and len(full) == 1, list(featrow_spills)
    assert max(last.values()) <= FULL_LIMIT[f16], last
    assert max(last.values()) <= max(full.values()), (last, full)
