"""Timing of the members' preprocessing on the device at config C's shape (1838 train rows, 460 test rows, 21
columns of which 18 categorical, 4 members), on one fitted default classifier and one default regressor, each with and
without the fingerprint feature (with it the SVD members keep the host transform), under ``fit_preprocessors`` and
``fit_with_cache``:

* ``predict_proba_device`` / ``predict_device`` wall time with ``X`` as a numpy array and as a CUDA tensor;
* per member, the host ``preprocessor.transform`` (wall) beside the ``member_transform`` launch (HIP events).

Best of 3 windows after a warm-up.  The numpy route is the code path of the parent commit.
    python tools/member_transform_time.py [out.txt]
"""
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "golden")]

import regression_oracle as ro  # noqa: E402
from api_cases import case_data  # noqa: E402
from test_api_host import make_classifier, write_ckpt  # noqa: E402
from test_regression_host import write_ckpt as write_reg_ckpt  # noqa: E402

N, Q, F, N_CAT = 1838, 460, 21, 18


def wall(fn, reps=5, windows=3):
    fn()
    best = float("inf")
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps)
    return best * 1e3


def events(fn, reps=20, windows=3):
    fn()
    best = float("inf")
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / reps)
    return best


def members(say, est, encode, X):
    ex = est.executor_
    eng = est.model_.engine(torch.device("cuda"))
    Xe, Xd = encode(X), torch.from_numpy(X).cuda()
    for i, (pipe, prog, why) in enumerate(zip(ex.preprocessors, ex.device_programs, ex.program_reasons)):
        name = ex.ensemble_configs[i].preprocess_config.name
        t0 = time.perf_counter()
        for _ in range(5):
            pipe.transform(Xe)
        host = (time.perf_counter() - t0) / 5 * 1e3
        if prog is None:
            say(f"    member {i} ({name}): host transform {host:.2f} ms; no device program ({why.split(' (')[0]})")
        else:
            say(f"    member {i} ({name}): host transform {host:.2f} ms; member_transform launch "
                f"{events(lambda: eng.member_transform(prog, Xd)) * 1e3:.1f} us")


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = Path(tempfile.mkdtemp())
    for fingerprint in (True, False):
        for fit_mode in ("fit_preprocessors", "fit_with_cache"):
            case = dict(name="time_c", model=dict(nlayers=12, mgm_heads=8, cap_heads=4), wseed=31,
                        clf=dict(mixer_type="MGM+CAP", mgm_heads=8, cap_heads=4, features_per_group=2, n_estimators=4,
                                 categorical_features_indices=list(range(N_CAT)), ignore_pretraining_limits=True,
                                 random_state=0),
                        interface=dict(FINGERPRINT_FEATURE=fingerprint),
                        data=dict(kind="pad", S=N + Q, N=N, F=F, n_cat=N_CAT, n_classes=6, n_mod=1, seed=2))
            d = case_data(case)
            clf = make_classifier(case, write_ckpt(case, tmp), fit_mode=fit_mode)
            clf.fit(d["X_train"], d["image_train"], d["y_train"])
            X, im = d["X_test"], d["image_test"]
            Xd = torch.from_numpy(X).cuda()
            say(f"classifier, default preprocessing, fingerprint {fingerprint}, {fit_mode}: predict_proba_device "
                f"numpy X {wall(lambda: clf.predict_proba_device(X, im)):.2f} ms, CUDA X "
                f"{wall(lambda: clf.predict_proba_device(Xd, im)):.2f} ms")
            if fit_mode == "fit_preprocessors":
                members(say, clf, clf._encode_predict_X, X)

            from multimodalpfn_amd import MMPFNRegressor

            rcase = dict(name="time_r", num_buckets=5000, N=N, Q=Q, F=F, seed=143, wseed=43)
            rd = ro.api_case_data(rcase)
            path, _, _ = write_reg_ckpt(rcase, tmp)
            kw = ro.api_regressor_kwargs(rcase, dict(average_before_softmax=False))
            kw.pop("inference_precision")
            reg = MMPFNRegressor(model_path=str(path), fit_mode=fit_mode,
                                 inference_config={"FINGERPRINT_FEATURE": fingerprint}, **kw)
            reg.fit(rd["X_train"], None, rd["y_train"])
            Xr, Xrd = rd["X_test"], torch.from_numpy(rd["X_test"]).cuda()
            say(f"regressor, default preprocessing, fingerprint {fingerprint}, {fit_mode}: predict_device numpy X "
                f"{wall(lambda: reg.predict_device(Xr, None)):.2f} ms, CUDA X "
                f"{wall(lambda: reg.predict_device(Xrd, None)):.2f} ms")
            if fit_mode == "fit_preprocessors":
                members(say, reg, reg._encode_host, Xr)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
