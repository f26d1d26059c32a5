"""Bar-distribution scoring golden vectors from the REFERENCE (build container only).

Run from the repo root:   python tests/golden/make_bar_score_golden.py

Imports ``/root/reference`` read-only, as ``make_regression_golden.py`` does, runs its
``FullSupportBarDistribution`` on the CPU in fp32 under ``regression_oracle.FIXTURE_THREADS`` and writes
``tests/golden/bar_score/score_B<bars>.npz``.  Inputs are rebuilt from seeds by the tests
(``tests/bar_score_cases.py``); only the reference's float32 outputs are stored, per case ``<name>_<kind>``:

``nll`` ``[3, 9]`` ``forward(logits, ys[:, j])`` per target column (0 at the NaN target), ``pdf`` likewise;
``cdf`` / ``pi`` / ``ei`` ``[3, 8]`` for the targets after the NaN one (``cdf`` asserts on a NaN, ``pi`` / ``ei`` have no
rule for one), ``pi`` / ``ei`` with the target column as ``best_f``;
``mean_of_square`` / ``variance`` ``[3]``; ``sample`` ``[3]`` drawn after ``torch.manual_seed(SAMPLE_SEED)`` at
temperature ``SAMPLE_T``.
"""

from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / "bar_score"
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import bar_score_cases as bc  # noqa: E402
import regression_oracle as ro  # noqa: E402


def _reference_class():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    sys.path.insert(0, "/root/reference")
    from mmpfn.models.mmpfn.model.bar_distribution import FullSupportBarDistribution

    return FullSupportBarDistribution


def reference_scores(case: dict) -> dict:
    crit = _reference_class()(torch.from_numpy(case["borders"]))
    logits = case["logits"] if case["temperature"] == 1 else case["logits"] / case["temperature"]
    ys = case["ys"]
    real = ys[:, 1:].contiguous()
    cols = range(real.shape[1])
    res = {
        "nll": torch.stack([crit(logits, ys[:, j]) for j in range(ys.shape[1])], -1),
        "pdf": torch.stack([crit.pdf(logits, ys[:, j]) for j in range(ys.shape[1])], -1),
        "cdf": crit.cdf(logits, real),
        "pi": torch.stack([crit.pi(logits, real[:, j].contiguous()) for j in cols], -1),
        "ei": torch.stack([crit.ei(logits, real[:, j].contiguous()) for j in cols], -1),
        "mean_of_square": crit.mean_of_square(logits),
        "variance": crit.variance(logits),
    }
    torch.manual_seed(bc.SAMPLE_SEED)
    res["sample"] = crit.sample(logits, bc.SAMPLE_T)
    res = {k: v.detach().numpy().astype(np.float32) for k, v in res.items()}
    assert (res["nll"][:, 0] == 0).all()
    for k in ("cdf", "pi", "mean_of_square", "variance", "sample"):
        assert np.isfinite(res[k]).all(), (case["B"], case["name"], k)
    # an empty interior bucket makes the reference's expected improvement 0 / 0 for every row
    assert np.isnan(res["ei"]).all() if case["name"] == "zero_width" else np.isfinite(res["ei"]).all()
    return res


def main():
    torch.set_num_threads(ro.FIXTURE_THREADS)
    OUT.mkdir(exist_ok=True)
    for B in bc.BARS:
        res = {}
        for case in bc.cases(B):
            for k, v in reference_scores(case).items():
                res[f"{case['name']}_{k}"] = v
        path = OUT / f"score_B{B}.npz"
        np.savez_compressed(path, **res)
        print(f"bar score B={B}: {len(bc.cases(B))} cases -> {path.name} ({path.stat().st_size / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
