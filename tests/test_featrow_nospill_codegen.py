"""Codegen guard: the feature block keeps nothing in scratch (CPU: hipcc cross-compiles gfx950 here).

``feat_rows_kernel<3, F16, LAST = false>`` (featrow.hip) once spilled 32 (fp16) / 16 (bf16) VGPRs -- finished heads'
O^T fragments -- to scratch, and the kernel moved 1.55x the bytes its algorithm needs because of them.  The fragments
of the row's last tile now wait in LDS, so every form of up to three tiles must compile to

* 0 spilled VGPRs and 0 bytes of scratch,
* at most 256 VGPRs (two waves per SIMD) and at most 81 920 B of static LDS (two blocks per CU).

The four-tile forms keep their shape (one token tile per out-projection pass, the full forms at one wave per SIMD)
and must be no worse off than before the change.  What they were, from a cross-compile of the commit before it
(VGPRs + AGPRs, spills, scratch, waves per SIMD, LDS):

    <4, fp16, full>  256 + 124, 0, 0, 1, 79 872        <4, fp16, LAST>  210 + 0, 0, 0, 2, 79 872
    <4, bf16, full>  256 + 102, 0, 0, 1, 79 872        <4, bf16, LAST>  220 + 0, 0, 0, 2, 79 872

Every one of these figures is held: registers, spills, scratch and LDS at most the parent's, occupancy at least.

``rowgemm_qkv2_kernel`` stays at 0 spills and no scratch.
"""

import re
import subprocess
from pathlib import Path

import pytest

from test_codegen import CSRC, FLAGS, HIPCC

pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

FIELDS = {"vgprs": r"\bVGPRs: (\d+)", "agprs": r"AGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
          "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)", "spill": r"VGPRs Spill: (\d+)",
          "lds": r"LDS Size \[bytes/block\]: (\d+)"}

# (VGPRs + AGPRs, spills, scratch, waves per SIMD, LDS) of the four-tile forms before the change; key: F16, LAST
PARENT_NT4 = {(1, 0): (256 + 124, 0, 0, 1, 79872), (0, 0): (256 + 102, 0, 0, 1, 79872),
              (1, 1): (210, 0, 0, 2, 79872), (0, 1): (220, 0, 0, 2, 79872)}


def _usage(src: str, extra=()) -> dict:
    """kernel name -> resource fields of the compiler's kernel-resource-usage remarks."""
    out = subprocess.run([HIPCC, *FLAGS, *extra, "-x", "hip", "-c", str(CSRC / src), "-o", "/dev/null",
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True,
                         timeout=600)
    res, name = {}, None
    for ln in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, pat in FIELDS.items():
            m = re.search(pat, ln)
            if m and name:
                res[name][key] = int(m.group(1))
    return res


@pytest.fixture(scope="module")
def featrow():
    return _usage("featrow.hip", ["-fno-honor-nans"])


def _kernel(usage: dict, nt: int, f16: int, last: int) -> dict:
    hits = [v for k, v in usage.items() if f"feat_rows_kernelILi{nt}ELb{f16}ELb{last}E" in k]
    assert len(hits) == 1, (nt, f16, last, list(usage))
    assert set(hits[0]) == set(FIELDS), hits[0]
    return hits[0]


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("nt", [1, 2, 3])
def test_up_to_three_tiles_no_scratch_two_blocks_per_cu(featrow, nt, f16, last):
    r = _kernel(featrow, nt, f16, last)
    print(nt, f16, last, r)
    assert r["spill"] == 0 and r["scratch"] == 0, r
    assert r["vgprs"] + r["agprs"] <= 256 and r["occupancy"] >= 2, r
    assert r["lds"] <= 81920, r


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("f16", [0, 1])
def test_four_tiles_no_worse_than_before(featrow, f16, last):
    r = _kernel(featrow, 4, f16, last)
    print(4, f16, last, r)
    regs, spill, scratch, occupancy, lds = PARENT_NT4[f16, last]
    assert r["vgprs"] + r["agprs"] <= regs, r
    assert r["spill"] <= spill and r["scratch"] <= scratch, r
    assert r["occupancy"] >= occupancy and r["lds"] <= lds, r


def test_item_qkv_projection_keeps_no_scratch():
    hits = {k: v for k, v in _usage("rowgemm.hip").items() if "rowgemm_qkv2_kernel" in k}
    assert len(hits) == 2, list(hits)  # the fp32 and the fp16 state's forms (Q / K bf16 in both)
    for k, r in hits.items():
        assert r["spill"] == 0 and r["scratch"] == 0, (k, r)
