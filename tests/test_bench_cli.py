"""bench.py's command line (CPU): a plain run is the headline alone, ``--full`` opts into every other leg, and
``--dump-outputs DIR`` writes the last timed step's class probabilities as float32 ``DIR/proba.npy``."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.gpus, args.steps, args.warmup) == (1, 7, 2)
    assert args.full is False and args.dump_outputs is None


def test_full_and_dump_outputs_options(monkeypatch, tmp_path):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path), "--no-config-d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == str(tmp_path)
    assert args.config_d is False and args.config_b is True  # the --no-* options prune the --full legs


@pytest.mark.gpu
def test_plain_run_reports_the_headline_alone_and_dumps_its_output(tmp_path):
    """One plain run in a fresh process: ``--steps`` sets the timed steps, ``value`` is rows over those steps'
    time, every --full leg is null, and the dumped probabilities are the step's [Q, classes] output."""
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "rows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f16" and (line["steps"], line["warmup"], line["n_gpus"]) == (2, 1, 1)
    assert line["ms_per_step"] > 0
    rows_per_step = bench.MEMBERS_PER_GPU * bench.S_ROWS
    assert line["value"] == pytest.approx(rows_per_step / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for leg in ("roofline", "cpu_baseline", "cpu_baseline_einsum", "api_end_to_end", "other_16bit_mode",
                "api_end_to_end_default_preprocessing", "f32_parity_mode", "config_B", "config_D", "config_E",
                "kv_cache_predict", "modality_encoders"):
        assert line[leg] is None, leg
    proba = np.load(tmp_path / "out" / "proba.npy")
    assert proba.dtype == np.float32 and proba.shape == (bench.S_ROWS - bench.N_TRAIN, bench.N_CLASSES)
    assert np.isfinite(proba).all() and (proba >= 0).all()
    np.testing.assert_allclose(proba.sum(1), 1.0, atol=1e-5)


def test_dump_outputs_writes_float32_proba(tmp_path):
    q = bench.S_ROWS - bench.N_TRAIN
    probs = torch.softmax(torch.randn(q, bench.N_CLASSES, generator=torch.Generator().manual_seed(0),
                                      dtype=torch.float64), -1)
    out = tmp_path / "nested" / "dir"
    bench.dump_outputs(out, probs)
    assert sorted(p.name for p in out.iterdir()) == ["proba.npy"]
    got = np.load(out / "proba.npy")
    assert got.dtype == np.float32 and got.shape == (q, bench.N_CLASSES)
    assert np.array_equal(got, probs.to(torch.float32).numpy())
