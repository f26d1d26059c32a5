"""Headline benchmark: in-context rows/sec on PAD-UFES-20-shaped inputs (BASELINE.json).

Workload (config C): N = 1838 support + Q = 460 query rows, F = 21
features (18 categorical + 3 numeric), one 768-d image embedding per row, MGM (64
heads) + CAP (24 queries) mixer, 12-layer E=192 PerFeatureTransformer, 4 ensemble
members per GPU (feature-shuffle + class-permutation members as EnsembleConfig
builds them), synthetic data and random-init weights of that architecture.

One step = one ``predict_proba`` of the hot path on device-resident inputs: mixer once
(the image is identical for every member), 4 member forwards per GPU, one RCCL
all-gather of the per-member logits, ensemble softmax-mean.  ``value`` = sum over
members of (N + Q) / wall time, aggregated over all ranks (weak scaling: 4 members
per GPU); nothing else runs in the timed region.  ``python bench.py --gpus N`` starts N rank
processes itself (``launch_ranks``: one per GPU, rendezvous on 127.0.0.1); ``torchrun --nproc-per-node N
bench.py --gpus N`` works the same way (every rank checks WORLD_SIZE == --gpus).

A plain run (``bench.py --gpus N --steps K --warmup W``) sets up, warms up, times the K steps and prints the
result line; ``--dump-outputs DIR`` also writes what the last timed step returned (``DIR/proba.npy``, float32).

With ``--full`` also reported (each in its own pass, outside the headline's timed region; null in a plain run):
``roofline`` of the dominant kernel (sample-axis attention, bf16 MFMA; algorithmic
flops 4*T*Nq*Nk*E per launch; every launch of a separate pass of the same steps
bracketed by HIP events on its lane stream, mmpfn_kernel_timing), ``f32_parity_mode``
(the same step in the fp32 parity mode), ``config_D`` (image + text, 32 members),
``api_end_to_end`` (MMPFNClassifier.predict_proba from host numpy, PCIe-inclusive),
``kv_cache_predict`` (fit_with_cache serving), ``modality_encoders`` (the DINOv2 / ELECTRA
towers that produce the image tokens) and ``cpu_baseline`` /
``cpu_baseline_einsum`` (the oracle's CPU restatement of the same forward in the
reference's two attention branches, on the host cores, one member).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

METRIC = "in-context rows/sec (support+query), PAD-UFES-20 shape, 1/2/4/8 MI355X"
BF16_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
# what each mode's MFMAs actually read (the bench line's config.operands), by dtype name
OPERANDS = {
    "f16": "fp16 state; fp16 MFMA operands in the feature attention, item QKV projection, MLP, out-projections and "
           "MGM head bank; bf16 operands in the item attention (Q, K of the Q.K^T scores; P, V^T of P.V: "
           "rowgemm_qkv2_kernel<true,true> stores bf16 Q / K / V^T for attn_pipe_kernel<0,false,true>) and in the CAP "
           "pooler; fp32 accumulation, softmax statistics and LayerNorm",
    "bf16": "fp32 state; bf16 MFMA operands everywhere; fp32 accumulation, softmax statistics and LayerNorm",
    "f32": "fp32 state; split-bf16 (hi + lo, three products) MFMA operands; fp32 accumulation",
}
HBM_PEAK_GBS = 8000.0

S_ROWS, N_TRAIN, N_FEAT, N_CAT, N_CLASSES = 2298, 1838, 21, 18, 6
MGM, CAP, MEMBERS_PER_GPU = 64, 24, 4


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--precision", choices=["f16", "bf16", "f32"], default="f16",
                   help="f16: MMPFN_PREC_F16, the reference's fp16 autocast (fp16 state + operands); bf16: bf16 "
                        "operands on an fp32 state; f32: the parity mode")
    p.add_argument("--members", type=int, default=MEMBERS_PER_GPU, help="members per GPU")
    p.add_argument("--full", action="store_true",
                   help="after the headline, also run every other leg (roofline, other precisions, API, KV cache, "
                        "configs B / D / E, modality towers, CPU baselines); the --no-* options prune them")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step returned (the class probabilities) to DIR/proba.npy")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--attn-reps", type=int, default=20)
    p.add_argument("--lanes", type=int, default=None, help="concurrent member lanes per GPU (default: engine's)")
    p.add_argument("--batch", type=int, default=None, help="members per batched forward (default: engine's)")
    p.add_argument("--mixer-stream", action="store_true",
                   help="headline step: the mixer on its own stream, overlapping the previous step's forwards")
    p.add_argument("--api-steps", type=int, default=10, help="timed predict_proba calls of the API leg (0: skip)")
    p.add_argument("--no-kv-cache", dest="kv_cache", action="store_false", help="skip the fit_with_cache leg")
    p.add_argument("--no-config-d", dest="config_d", action="store_false", help="skip the config-D leg")
    p.add_argument("--no-config-b", dest="config_b", action="store_false",
                   help="skip the config-B leg (4096 x 100 tabular, fp16 and bf16)")
    p.add_argument("--no-config-e", dest="config_e", action="store_false",
                   help="skip the config-E leg (fp16 vs the fp8 P.V path)")
    p.add_argument("--no-modality", dest="modality", action="store_false",
                   help="skip the modality-encoder leg (DINOv2 ViT-B/14, ELECTRA-base)")
    p.add_argument("--no-f32", dest="f32_leg", action="store_false", help="skip the fp32 parity-mode leg")
    p.add_argument("--no-cpu-einsum", dest="cpu_einsum", action="store_false",
                   help="skip the einsum-branch CPU baseline (the SDPA branch always runs)")
    return p.parse_args()


def build_workload(device, world, members_per_gpu, n_mod=1, seed=2):
    """Config C (seed 2, image [S,1,768]) or D (seed 3, image + text [S,2,768]), SURVEY.md 8d."""
    from synth import synth_image, synth_labels, synth_state_dict, synth_table

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec
    from multimodalpfn_amd.model.transformer import PerFeatureTransformer

    cfg = ModelConfig(mgm_heads=MGM, cap_heads=CAP)
    sd = synth_state_dict(state_dict_spec(cfg), seed)
    model = PerFeatureTransformer(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    norm = next(e for e in model.encoder if "InputNormalizationEncoderStep" in str(e.__class__))
    norm.remove_outliers, norm.remove_outliers_sigma = True, 12.0  # classifier.fit (classifier.py:396-406)
    model.to(device)
    x = synth_table(S_ROWS, N_FEAT, seed, n_cat=N_CAT)
    y = synth_labels(S_ROWS, N_CLASSES, seed)
    image = synth_image(S_ROWS, n_mod, seed)
    M = members_per_gpu * world
    rng = np.random.default_rng(seed - 2)
    members = []
    for m in range(M):
        fperm = rng.permutation(N_FEAT)  # ShuffleFeaturesStep
        cperm = rng.permutation(N_CLASSES)  # class_permutation
        xm = torch.from_numpy(np.ascontiguousarray(x[:, fperm])).to(device)
        ym = cperm[y[:N_TRAIN].astype(np.int64)].astype(np.float32)
        members.append((xm, ym, np.argsort(cperm)))
    return cfg, sd, model, x, y, image, members


def attn_traffic(T):
    """HBM bytes per attention launch over T token columns, from the committed PMC pass
    (tools/attn_pmc.sh: rocprofv3 FETCH_SIZE and WRITE_SIZE runs at that launch shape)."""
    H, d, S, N = 6, 32, S_ROWS, N_TRAIN
    # the shipped kernel's own pass only, newest first: the fp16 mode's launch (rounds 6, 5, 4), then the bf16 one
    # (round 3; older rounds measured attn_item2)
    cands = sorted((ROOT / "profiles" / "r06").glob("attn_pipe_pmc_T*_f16.json")) + \
        sorted((ROOT / "profiles" / "r05").glob("attn_pipe_pmc_T*_f16.json")) + \
        sorted((ROOT / "profiles" / "r04").glob("attn_pipe_pmc_T*_f16.json")) + \
        sorted((ROOT / "profiles" / "r03").glob("attn_pipe_pmc_T*[0-9].json"))
    for pmc in cands:
        rec = json.loads(pmc.read_text())
        if rec.get("shape") == {"T": T, "H": H, "d": d, "S": S, "N": N}:
            return rec["hbm_bytes_per_launch"], str(pmc.relative_to(ROOT))
    return None, None


def live_roofline(lib, ctx, T_launch):
    """Roofline of the dominant kernel from the launches INSIDE the timed region: HIP events
    recorded by the engine on each lane's stream around every item-attention launch."""
    import ctypes

    ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    assert lib.mmpfn_kernel_timing_read(ctx, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)) == 0
    if n.value == 0:
        return None
    H, d, S, N = 6, 32, S_ROWS, N_TRAIN
    per_ms, per_fl = ms.value / n.value, fl.value / n.value
    uniform = abs(per_fl - 4.0 * T_launch * S * N * H * d) < 1.0
    achieved = per_fl / (per_ms * 1e-3) / 1e12
    traffic, src = attn_traffic(T_launch) if uniform else (None, None)
    return {
        "bound": "mfma",
        "achieved": round(achieved, 1),
        "peak": BF16_PEAK_TFLOPS,
        "unit": "TFLOP/s",
        "frac": round(achieved / BF16_PEAK_TFLOPS, 4),
        "traffic": traffic,
        "traffic_unit": f"HBM bytes per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE, {src})" if src else None,
        "algorithmic_bytes": 2 * T_launch * H * d * (S + 2 * N) + 2 * T_launch * S * H * d,
        "kernel": "attn_pipe_kernel (sample-axis attention: train + test-MQA rows of one layer, all members "
                  "of a batched forward, per launch)",
        "launches_timed": n.value,
        "token_columns_per_launch": T_launch,
        "per_launch_ms": round(per_ms, 4),
        "per_launch_flop": per_fl,
        "timing": "HIP events on the launching lane stream around every launch in the timed region "
                  "(mmpfn_kernel_timing); lanes overlap, so a launch shares the GPU with the other lane's kernels",
    }


def time_item_attention(eng, T, reps, S=S_ROWS, N=N_TRAIN, precision=None):
    """Average launch duration of the sample-axis attention kernel at the workload's shape.

    One launch = the whole attention-between-items of one layer (train rows on their own
    heads + test rows of all heads on head 0's K/V), HIP events on the engine stream.  ``precision``:
    an engine code of mmpfn_item_attention_layer_ex (bf16 / f16 Q and K, optionally the fp8 P.V); the
    fp8 codes include the V^T conversion launch in the time."""
    from multimodalpfn_amd import _lib

    H, d = 6, 32
    Q = S - N
    Npad = (N + 63) // 64 * 64
    dev = eng.device
    precision = _lib.PREC_BF16 if precision is None else precision
    f16 = precision in (_lib.PREC_F16, _lib.PREC_F16_F8, _lib.PREC_F16_F8E5)
    if f16:  # the fp16 mode's forward form (bf16 q / k, fp16 out), as the engine launches it
        precision |= _lib.ATTN_QK_BF16
    g = torch.Generator(device="cpu").manual_seed(0)
    q = torch.randn(T, H, S, d, generator=g).to(dev, torch.bfloat16)
    k = torch.randn(T, H, Npad, d, generator=g).to(dev, torch.bfloat16)
    vt = torch.randn(T, H, d, Npad, generator=g).to(dev, torch.bfloat16)
    o = torch.empty(T, S, H * d, device=dev, dtype=torch.float16 if f16 else torch.bfloat16)
    lib, ctx = eng.lib, eng.ctx
    eng._bind_stream()
    stream = torch.cuda.current_stream(dev)

    def launch():
        rc = lib.mmpfn_item_attention_layer_ex(ctx, q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), S, T, H,
                                               Npad, N, precision)
        assert rc == 0, lib.mmpfn_last_error(ctx)

    for _ in range(3):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        launch()
    e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    flops = 4.0 * T * (N + Q) * N * H * d  # train 4*T*N*N*E + test (MQA) 4*T*Q*N*E
    achieved = flops / (ms * 1e-3) / 1e12
    traffic, src = attn_traffic(T) if (S, N) == (S_ROWS, N_TRAIN) else (None, None)
    return {
        "bound": "mfma",
        "achieved": round(achieved, 1),
        "peak": BF16_PEAK_TFLOPS,
        "unit": "TFLOP/s",
        "frac": round(achieved / BF16_PEAK_TFLOPS, 4),
        "traffic": traffic,
        "traffic_unit": f"HBM bytes per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE, {src})" if src else None,
        "algorithmic_bytes": 2 * T * H * d * (S + 2 * N) + 2 * T * S * H * d,
        "kernel": "attn_pipe_kernel (sample-axis attention, train + test-MQA rows of one layer per launch)",
        "per_launch_ms": round(ms, 4),
        "per_launch_flop": flops,
    }


def forward_flops(T, S=S_ROWS, N=N_TRAIN, E=192, FF=768, L=12) -> float:
    """Algorithmic flops of one member forward's layer stack:
    feature attention (QKV, T x T attention, out-projection), item attention (Q of all rows,
    K/V of the train rows, train + test-MQA attention, out-projection) and the MLP."""
    Q = S - N
    feat = 2 * S * T * E * 3 * E + 4 * S * T * T * E + 2 * S * T * E * E
    item = 2 * S * T * E * E + 2 * N * T * E * 2 * E + 4 * T * N * N * E + 4 * T * Q * N * E + 2 * S * T * E * E
    mlp = 4 * S * T * E * FF
    return float(L * (feat + item + mlp))


def mixer_flops(S=S_ROWS, D=768, E=192, mgm=MGM, cap=CAP) -> float:
    """MGM (per head Linear(768,768) + Linear(384,192)) and CAP (K|V projection of the
    mgm tokens, attention, out-projection, FFN) of one predict (A7-A8)."""
    mg = 2 * S * mgm * (D * D + (D // 2) * E)
    cp = 2 * S * mgm * E * 2 * E + 4 * S * cap * mgm * E + 2 * S * cap * (E * E + E * 2 * E + 2 * E * E)
    return float(mg + cp)


def kv_cache_leg(eng, members, img, prec, steps):
    """``fit_mode="fit_with_cache"`` serving rate: each member's train rows forwarded once
    (cache build, timed separately), then every predict forwards only the Q test rows of each
    member against its cached head-0 K/V (mmpfn_cache_predict).  Not the headline metric."""
    N, Q = N_TRAIN, S_ROWS - N_TRAIN
    tok = eng.mixer_tokens(img, prec)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    caches = [eng.cache_build(xm[:N], tok[:N], ym, prec) for xm, ym, _ in members]
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0

    def predict():
        tq = eng.mixer_tokens(img[N:], prec)
        return eng.cache_predict_many(caches, [xm[N:] for xm, _, _ in members], tq)

    predict()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        predict()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {
        "query_rows_per_s": round(len(members) * Q / dt, 1),
        "ms_per_predict": round(dt * 1e3, 3),
        "ms_cache_build_all_members": round(t_build * 1e3, 3),
        "cache_bytes_per_member": caches[0].nbytes,
        "note": "fit_with_cache: Q test rows per member against the device-resident train-KV cache",
    }
    for c in caches:
        c.free()
    return out


def cpu_baseline(sd, x, y, image, use_sdpa=True):
    """Oracle (CPU restatement of the reference forward) on one member, in the attention branch
    the reference takes on a GPU box (torch SDPA, multi_head_attention.py:693-717) or its
    explicit einsum-softmax fallback (:718-729, the branch a CPU-only host takes)."""
    from multimodalpfn_amd.model.spec import ModelConfig
    from oracle.forward import OracleSpec, oracle_forward

    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or (os.cpu_count() or 1)
    torch.set_num_threads(threads)
    cfg = ModelConfig(mgm_heads=MGM, cap_heads=CAP)
    spec = OracleSpec(mgm_heads=cfg.mgm_heads, cap_heads=cfg.cap_heads)
    w = {k: torch.from_numpy(v) for k, v in sd.items()}
    args = (spec, w, torch.from_numpy(x), torch.from_numpy(image), torch.from_numpy(y[:N_TRAIN]))
    t0 = time.perf_counter()
    oracle_forward(*args, use_sdpa=use_sdpa)
    dt = time.perf_counter() - t0
    branch = "torch SDPA branch" if use_sdpa else "einsum-softmax branch"
    return {
        "value": round(S_ROWS / dt, 2),
        "unit": "rows/s",
        "cores": threads,
        "kind": "port",
        "sample": f"1 member forward of config C (S={S_ROWS}, 12 layers, MGM64+CAP24, fp32, {branch}) on "
                  f"{threads} host threads: {dt:.1f} s",
    }


def api_end_to_end(cfg, sd, x, y, image, n_estimators, prec_f32, steps, world, preprocessing="none"):
    """``MMPFNClassifier.predict_proba`` wall time from host numpy inputs (PCIe-inclusive): SURVEY 8d's
    ``wall(predict_proba)`` with the model resident.

    ``preprocessing="none"``: run.py's interface config (no preprocessing, no fingerprint), the 18
    categorical columns marked.  ``"default"``: the reference's default ``ModelInterfaceConfig`` (its
    ``PREPROCESS_TRANSFORMS`` quantile / SVD / ordinal members and the fingerprint feature,
    preprocessing.py:228-335, classifier.py:466-481), so the members have ragged widths; the leg then
    also reports the host transform time and the ragged members' device-resident forward rate through
    ``forward_many`` (inference.py:294-349 runs such members one after another).
    """
    import tempfile

    import torch.distributed as dist

    from multimodalpfn_amd import MMPFNClassifier
    from multimodalpfn_amd.constants import ModelInterfaceConfig
    from multimodalpfn_amd.preprocessing import PreprocessorConfig
    from api_cases import ckpt_config

    ic = (ModelInterfaceConfig(FINGERPRINT_FEATURE=False, PREPROCESS_TRANSFORMS=[PreprocessorConfig(name="none")])
          if preprocessing == "none" else ModelInterfaceConfig())
    with tempfile.TemporaryDirectory() as tmp:
        ck = Path(tmp) / "mmpfn_configC.ckpt"
        torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "config": ckpt_config(cfg)}, ck)
        clf = MMPFNClassifier(
            model_path=str(ck), mixer_type="MGM+CAP", mgm_heads=MGM, cap_heads=CAP, features_per_group=2,
            n_estimators=n_estimators, categorical_features_indices=list(range(N_CAT)),
            ignore_pretraining_limits=True, inference_precision=torch.float32 if prec_f32 else "auto",
            inference_config=ic,
        )
        X = x.astype(np.float64)
        labels = y.astype(np.int64)
        t0 = time.perf_counter()
        clf.fit(X[:N_TRAIN], image[:N_TRAIN], labels[:N_TRAIN])
        t_fit = time.perf_counter() - t0
    Xq, imq = X[N_TRAIN:], image[N_TRAIN:]
    for _ in range(3):  # warm-up (engine build, weight upload, the allocator's pinned / device blocks)
        clf.predict_proba(Xq, imq)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        proba = clf.predict_proba(Xq, imq)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    assert np.isfinite(proba).all()
    out = {
        "value": round(n_estimators * S_ROWS * steps / dt, 1),
        "unit": "rows/s",
        "ms_per_predict": round(dt / steps * 1e3, 3),
        "members": n_estimators,
        "preprocessing": preprocessing,
        "ms_fit": round(t_fit * 1e3, 1),
        "note": "MMPFNClassifier.predict_proba on host numpy inputs: validation + per-member host transform, "
                "H2D copies, mixer, member forwards, aggregation, D2H (PCIe-inclusive; not the headline value)",
    }
    ex = clf.executor_
    if preprocessing != "none" and hasattr(ex, "preprocessors"):
        Xe = clf._encode_predict_X(Xq)
        t0 = time.perf_counter()
        for _ in range(steps):
            Xts = [p.transform(Xe).X for p in ex.preprocessors]
        t_tr = (time.perf_counter() - t0) / steps
        widths = [int(np.asarray(xt).shape[1]) for xt in ex.X_trains]
        out["member_widths"] = widths
        out["ms_host_transform_all_members"] = round(t_tr * 1e3, 3)
        # the ragged members on device-resident inputs, through the engine's lane / batch scheduler
        model = clf.model_
        eng = model.engine(clf.device_)
        prec = _lib_prec(prec_f32)
        img = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(eng.device)
        # this rank's members only, dealt exactly as the predict deals them (inference._run_members ->
        # parallel.member_shard: LPT over parallel.member_cost, keyed by geometry, in units of the engine's batch),
        # so the subtraction below compares the same work
        from multimodalpfn_amd.inference import _n_mixer_tokens
        from multimodalpfn_amd.parallel import lpt_assign, member_cost

        fpg = model.features_per_group
        C = _n_mixer_tokens(model, imq)
        keys = [(int(np.asarray(xt).shape[1]), len(yt)) for xt, yt in zip(ex.X_trains, ex.y_trains)]
        costs = [member_cost((f + fpg - 1) // fpg + C + 1, len(yt) + len(Xq), len(yt), model.cfg.emsize, model.cfg.nhid)
                 for (f, _), yt in zip(keys, ex.y_trains)]
        mine = (lpt_assign(costs, world, keys, eng.batch)[dist.get_rank()] if world > 1
                else list(range(len(ex.X_trains))))
        items = []
        for i in mine:
            xt, xq, yt = ex.X_trains[i], Xts[i], ex.y_trains[i]
            xf = torch.from_numpy(np.ascontiguousarray(np.concatenate([xt, xq], 0), dtype=np.float32)).to(eng.device)
            items.append((xf, np.asarray(yt, np.float32)))

        def fwd():
            tok = eng.mixer_tokens(img, prec)
            return eng.forward_many([(xf, tok, yt) for xf, yt in items], prec)

        fwd()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fwd()
        torch.cuda.synchronize()
        t_dev = (time.perf_counter() - t0) / steps
        out["ragged_members_device"] = {
            "value": round(len(items) * S_ROWS / t_dev, 1), "unit": "rows/s", "ms_per_step": round(t_dev * 1e3, 3),
            "members_this_rank": len(items),
            "geometries": len({w for w in widths}),
            "note": "mixer + the default-preprocessing members (ragged widths) through forward_many on "
                    "device-resident inputs; equal-width members batch, ragged ones overlap on lanes",
        }
        # the predict's wall time beyond the same members' device-resident forward: the host work that is
        # NOT hidden behind the GPU (validation, the first unit's transform and copies, the tail's gather,
        # aggregation and D2H).  The member transforms overlap the GPU, so they are not subtracted.
        out["ms_predict_beyond_device_forward"] = round(dt / steps * 1e3 - t_dev * 1e3, 3)
    return out


def _lib_prec(f32: bool) -> int:
    from multimodalpfn_amd import _lib

    return _lib.PREC_F32 if f32 else _lib.autocast_precision()


def timed_steps(step, steps, warmup, world, device, last=None):
    """W untimed steps, then K steps bracketed by barrier + synchronize on both sides; the max
    wall time over ranks (bench contract).  ``last``: a list that receives what the last timed step returned."""
    import torch.distributed as dist

    for _ in range(warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if last is not None and steps > 0:
        last.append(out)
    if world > 1:
        tt = torch.tensor([dt], device=device if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    return dt


def make_step(eng, members, mine, assignment, rank, img, prec, lanes, batch, mixer_stream=False):
    """One predict_proba of the hot path on device-resident inputs (classifier.py:517-576 minus the
    host-side input validation / per-member transform and the final copy to host): the mixer once,
    this rank's members through forward_many, one RCCL all-gather of the logits, the ensemble
    softmax-mean on the device.  mixer_stream: the mixer runs on its own stream, ordered only after the
    previous step's mixer (its input image is resident and never written), so the next step's modality
    projection overlaps this step's member forwards; the step's members wait for its tokens."""
    from multimodalpfn_amd.parallel import allgather_logits

    perms = np.stack([m[2] for m in members])
    mix = torch.cuda.Stream(eng.device) if mixer_stream else None

    def step():
        if mix is not None:
            with torch.cuda.stream(mix):
                tokens = eng.mixer_tokens(img, prec)
                ev = torch.cuda.Event()
                ev.record(mix)
            cur = torch.cuda.current_stream(eng.device)
            cur.wait_event(ev)
            tokens.record_stream(cur)
        else:
            tokens = eng.mixer_tokens(img, prec)
        outs = eng.forward_many([(members[m][0], tokens, members[m][1]) for m in mine], prec, lanes, batch)
        allm = allgather_logits(torch.stack(outs), assignment, rank)
        return eng.aggregate(allm, perms, N_CLASSES, 0.9, False)

    return step


def config_d_leg(device, world, rank, args, prec):
    """BASELINE config D: image + text [S,2,768] (petfinder.py:194 shape), MGM64 + CAP24 (CAP over
    2 x 64 MGM tokens), 32 members (run.py's no-preprocessing members: feature shuffle + class
    permutation) sharded over the ranks, one all-gather.  rows/s = 32 * (N + Q) / step time."""
    from multimodalpfn_amd.parallel import lpt_assign, member_cost

    members_total = 32
    per = -(-members_total // world)
    cfg, sd, model, x, y, image, members = build_workload(device, world, per, n_mod=2, seed=3)
    members = members[:members_total]
    eng = model.engine(device)
    img = torch.from_numpy(image).to(device)
    T = (N_FEAT + 1) // 2 + CAP + 1
    assignment = lpt_assign([member_cost(T, S_ROWS, N_TRAIN)] * members_total, world, [T] * members_total,
                            args.batch or eng.batch)
    step = make_step(eng, members, assignment[rank], assignment, rank, img, prec, args.lanes, args.batch)
    probs = step()
    eng.status()
    assert torch.isfinite(probs).all()
    k = max(3, args.steps // 4)
    dt = timed_steps(step, k, max(1, args.warmup // 4), world, device)
    eng.close()
    return {
        "value": round(members_total * S_ROWS * k / dt, 1),
        "unit": "rows/s",
        "ms_per_step": round(dt / k * 1e3, 3),
        "steps": k,
        "members_total": members_total,
        "members_per_gpu": len(assignment[rank]),
        "workload": "config D: image + text [S,2,768], MGM 64 + CAP 24 (CAP over 128 MGM tokens), N=1838 + Q=460, "
                    "F=21, 12 layers, 32 members (feature shuffle + class permutation) sharded over the GPUs, "
                    "one all-gather of the logits",
    }


def config_e_leg(device, args):
    """BASELINE config E: 10 000 support + 2 000 query rows, F = 20, tabular-only, 12 layers (SURVEY 8d seed 4),
    4 members (feature shuffle + class permutation) through forward_many: the fp16 mode, and the same with the
    sample-axis attention's P.V on fp8 MFMA (MMPFN_PREC_F16_F8, config E's "fp8 MFMA path").  rows/s =
    members * (N + Q) / step time; every attention launch also timed by HIP events (mmpfn_kernel_timing)."""
    from multimodalpfn_amd import _lib

    return tabular_config_leg(
        device, "config E: N=10000 support + Q=2000 query rows, F=20 tabular, 12 layers, 4 members",
        12000, 10000, 20, 4, 4,
        (("f16", _lib.PREC_F16), ("f16 + fp8 P.V (e4m3)", _lib.PREC_F16_F8),
         ("f16 + fp8 P.V (e5m2)", _lib.PREC_F16_F8E5), ("bf16", _lib.PREC_BF16)))


def config_b_leg(device, args):
    """BASELINE config B: 4096 support + 1024 query rows x 100 features, tabular-only, 12 layers (SURVEY 8d seed 1;
    T = 51 tokens per row, item attention ~72 % of the flops), 4 members through forward_many, fp16 and bf16."""
    from multimodalpfn_amd import _lib

    return tabular_config_leg(
        device, "config B: N=4096 support + Q=1024 query rows, F=100 tabular, 12 layers, 4 members",
        5120, 4096, 100, 2, 1, (("f16", _lib.PREC_F16), ("bf16", _lib.PREC_BF16)))


def tabular_config_leg(device, workload, S, N, F, ncls, seed, modes, M=4):
    """A tabular-only BASELINE config through forward_many, one record per precision mode (the first is the
    reference point of the others' logits deviation)."""
    import ctypes

    from synth import synth_labels, synth_state_dict, synth_table

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec
    from multimodalpfn_amd.model.transformer import PerFeatureTransformer

    cfg = ModelConfig(mgm_heads=8, cap_heads=4)
    sd = synth_state_dict(state_dict_spec(cfg), seed)
    model = PerFeatureTransformer(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    norm = next(e for e in model.encoder if "InputNormalizationEncoderStep" in str(e.__class__))
    norm.remove_outliers, norm.remove_outliers_sigma = True, 12.0
    model.to(device)
    eng = model.engine(device)
    x = synth_table(S, F, seed, nan_frac=0.01)
    y = synth_labels(S, ncls, seed)
    rng = np.random.default_rng(7)
    items = []
    for _ in range(M):
        xm = torch.from_numpy(np.ascontiguousarray(x[:, rng.permutation(F)])).to(device)
        items.append((xm, None, rng.permutation(ncls)[y[:N].astype(np.int64)].astype(np.float32)))
    out = {"workload": workload}
    ref = None
    ref_name = modes[0][0]
    for name, code in modes:
        def step():
            return eng.forward_many(items, code)

        lg = torch.stack(step())
        eng.status()
        k = 3
        dt = timed_steps(step, k, 1, 1, device)
        eng.lib.mmpfn_kernel_timing(eng.ctx, 1)
        timed_steps(step, 1, 0, 1, device)
        eng.lib.mmpfn_kernel_timing(eng.ctx, 0)
        ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        eng.lib.mmpfn_kernel_timing_read(eng.ctx, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
        rec = {"value": round(M * S * k / dt, 1), "unit": "rows/s", "ms_per_step": round(dt / k * 1e3, 2),
               "attention_ms_per_launch": round(ms.value / max(1, n.value), 4),
               "attention_frac": round(fl.value / (ms.value * 1e-3) / 1e12 / BF16_PEAK_TFLOPS, 4) if n.value else None}
        if ref is None:
            ref = lg
        else:
            d = (lg - ref).abs().max().item() / max(1.0, ref.abs().max().item())
            rec[f"logits_rel_dev_vs_{ref_name}"] = float(f"{d:.3e}")
            rec[f"argmax_agree_vs_{ref_name}"] = round(float((lg.argmax(-1) == ref.argmax(-1)).float().mean()), 4)
        out[name] = rec
    eng.close()
    return out


def vit_flops(B, H, W, D=768, depth=12, P=14, cls_only=True) -> float:
    """Executed flops of DINOv2 ViT-B/14 forward_features (the last block on the CLS rows only)."""
    np_ = (H // P) * (W // P)
    L = 1 + np_
    f = 2.0 * B * np_ * (3 * P * P) * D  # patch embedding
    full = 2.0 * L * D * 3 * D + 4.0 * L * L * D + 2.0 * L * D * D + 2.0 * 2 * L * D * 4 * D
    tail = 2.0 * L * D * 3 * D + 4.0 * L * D + 2.0 * D * D + 2.0 * 2 * D * 4 * D
    return f + B * ((depth - 1) * full + (tail if cls_only else full))


def modality_leg(device, args):
    """the image tower the reference runs once per dataset (pad_ufes_20.py:66-107):
    DINOv2 ViT-B/14 x_norm_clstoken of 336 x 336 images (the reference's img_size 14 * 24), and the
    ELECTRA-base text tower (petfinder.py:150-181), random-init weights of those architectures."""
    from modality_cases import text_config, text_state, vit_state

    from multimodalpfn_amd.modality import ElectraTextEncoder, vit_base

    out = {}
    c = dict(dim=768, depth=12, heads=12, patch=14, img_size=518, init_values=1.0, offset=0.1, seed=31)
    m = vit_base(patch_size=14, img_size=518, init_values=1.0, num_register_tokens=0, block_chunks=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vit_state(c).items()})
    B, H = 128, 336
    x = torch.rand((B, 3, H, H), generator=torch.Generator().manual_seed(5)).to(device)
    for prec in ("bf16", "f32"):
        m.precision = prec
        m.cls_embeddings(x)
        torch.cuda.synchronize(device)
        k = 5 if prec == "bf16" else 2
        t0 = time.perf_counter()
        for _ in range(k):
            m.cls_embeddings(x)
        torch.cuda.synchronize(device)
        dt = (time.perf_counter() - t0) / k
        fl = vit_flops(B, H, H)
        out["vit_b14_" + prec] = {"value": round(B / dt, 1), "unit": "images/s", "ms_per_batch": round(dt * 1e3, 2),
                                  "batch": B, "image": f"{H}x{H}", "tflops": round(fl / dt / 1e12, 1),
                                  "frac_of_bf16_peak": round(fl / dt / 1e12 / BF16_PEAK_TFLOPS, 4)}
    m._drop_contexts()
    tc = dict(vocab=30522, emb=768, dim=768, depth=12, heads=12, ffn=3072, max_pos=512, types=2, seed=32)
    t = ElectraTextEncoder(text_config(tc), precision="bf16")
    t.load_state_dict({k: torch.from_numpy(v) for k, v in text_state(tc).items()})
    Bt, Lt = 256, 128
    ids = torch.randint(1, 30522, (Bt, Lt), generator=torch.Generator().manual_seed(6)).to(device)
    mask = torch.ones_like(ids)
    t.cls_embeddings(ids, mask)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(5):
        t.cls_embeddings(ids, mask)
    torch.cuda.synchronize(device)
    dt = (time.perf_counter() - t0) / 5
    out["electra_base_bf16"] = {"value": round(Bt / dt, 1), "unit": "texts/s", "ms_per_batch": round(dt * 1e3, 2),
                                "batch": Bt, "tokens": Lt}
    t._drop_contexts()
    out["note"] = ("random-init weights of the reference's towers (the pretrained checkpoints are not available "
                   "offline); executed flops with the last block on the CLS rows only")
    return out


def free_port() -> int:
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_envs(n: int, port: int, base: dict | None = None) -> list[dict]:
    """The environment of each of the n rank processes ``launch_ranks`` starts on this node: torchrun's
    variables (one process per GPU, LOCAL_RANK = RANK), the rendezvous on 127.0.0.1, dmabuf IPC for RCCL."""
    base = dict(os.environ if base is None else base)
    envs = []
    for r in range(n):
        e = dict(base)
        e.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0",
                 MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        envs.append(e)
    return envs


def launch_ranks(n: int, cmd: list[str], stdout=None, poll_s: float = 0.2) -> int:
    """``bench.py --gpus N`` without torchrun: start N fresh rank processes running ``cmd`` (this script again,
    with WORLD_SIZE set) and wait for them.  The parent never initialises HIP -- it only forks children, so
    nothing is exec'd from a process that touched the GPU.  The first rank that fails ends the others; the
    return value is 0 or that rank's exit status (128 + signal for a killed rank).  Rank 0 prints the JSON line
    on the inherited stdout (the other ranks' stdout goes to stderr, so stdout carries one rank's output)."""
    import subprocess

    procs = [subprocess.Popen(cmd, env=e, stdout=stdout if r == 0 else sys.stderr)
             for r, e in enumerate(rank_envs(n, free_port()))]
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for i in sorted(pending):
                r = procs[i].poll()
                if r is None:
                    continue
                pending.discard(i)
                if r != 0 and rc == 0:
                    rc = r if r > 0 else 128 - r
                    print(f"bench launcher: rank {i} exited with {r}; stopping the other ranks", file=sys.stderr)
                    for p in procs:
                        if p.poll() is None:
                            p.terminate()
            if pending:
                time.sleep(poll_s)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    return rc


def dump_outputs(out_dir, probs):
    """``--dump-outputs DIR``: what the caller of the last timed step received, the ensemble's class
    probabilities of the Q query rows ([Q, N_CLASSES]), as ``DIR/proba.npy`` in float32.  The workload is
    seeded (build_workload), so two builds run with the same arguments can be compared array for array."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    np.save(out_dir / "proba.npy", probs.detach().to("cpu", torch.float32).numpy())


def engine_legs(args, eng, step, cfg, sd, x, y, image, members, mine, assignment, rank, world, device, img, prec, T):
    """``--full``: the legs that run on the headline's engine, each in a pass of its own after the headline's
    timed region: the live roofline of the dominant kernel, the other 16-bit mode, the fp32 parity mode, the
    classifier API from host numpy, fit_with_cache serving and the isolated attention launches."""
    from multimodalpfn_amd import _lib

    M = len(members)
    # ---- live roofline of the dominant kernel: a SEPARATE pass of the same steps with every
    #      attention launch bracketed by HIP events on its lane stream (kept out of the headline)
    #      Two such passes: the headline's own lane setting (launches share the CUs with the other
    #      lane's kernels, so their event durations are not the kernel's), and one lane (the same
    #      batched launch shape, kernels one after another): the kernel's own duration, the primary
    #      figure, which `rocprofv3 --kernel-trace -- bench.py --lanes 1` reproduces.
    batch = eng.batch if args.batch is None else args.batch
    lanes = eng.lanes if args.lanes is None else args.lanes
    T_launch = T * min(batch, len(mine))

    def live_pass(stp, t_launch=T_launch):
        eng.lib.mmpfn_kernel_timing(eng.ctx, 1)
        dt_l = timed_steps(stp, args.steps, 1, world, device)
        eng.lib.mmpfn_kernel_timing(eng.ctx, 0)
        r = live_roofline(eng.lib, eng.ctx, t_launch) if rank == 0 else None
        if r is not None:
            r["timing"] += f"; a separate pass of {args.steps} steps ({dt_l / args.steps * 1e3:.3f} ms per step)"
        return r

    live_ovl = live_pass(step)
    live = live_ovl
    if lanes > 1:
        step_l1 = make_step(eng, members, mine, assignment, rank, img, prec, 1, args.batch)
        live = live_pass(step_l1)
        if live is not None:
            live["timing"] = live["timing"].replace(
                "lanes overlap, so a launch shares the GPU with the other lane's kernels",
                "one lane: launches run one after another, as in `bench.py --lanes 1`")
            live["in_step_overlapped"] = {k: live_ovl[k] for k in ("achieved", "frac", "per_launch_ms", "timing")}
        if batch == 1 and len(mine) >= 2:
            # the same kernel at the two-member launch shape rounds 1-4 reported (T = 72: twice the blocks per
            # launch, so a smaller share of the grid's last round); the step itself runs one member per launch
            # because the two lanes then overlap each other's grid tails
            live_b2 = live_pass(make_step(eng, members, mine, assignment, rank, img, prec, 1, 2), 2 * T)
            if live is not None and live_b2 is not None:
                live["two_member_launch_one_lane"] = {k: live_b2[k] for k in ("achieved", "frac", "per_launch_ms",
                                                                             "traffic")}

    # ---- the other 16-bit mode (bf16 operands on an fp32 state, or the fp16 mode), same step
    other16 = None
    if prec in (_lib.PREC_F16, _lib.PREC_BF16):
        p2 = _lib.PREC_BF16 if prec == _lib.PREC_F16 else _lib.PREC_F16
        step2 = make_step(eng, members, mine, assignment, rank, img, p2, args.lanes, args.batch)
        k2 = max(3, args.steps // 3)
        dt2 = timed_steps(step2, k2, 2, world, device)
        other16 = {"value": round(M * S_ROWS * k2 / dt2, 1), "unit": "rows/s", "ms_per_step": round(dt2 / k2 * 1e3, 3),
                   "steps": k2, "dtype": "bf16" if p2 == _lib.PREC_BF16 else "f16",
                   "note": ("MMPFN_PREC_BF16: bf16 MFMA operands on an fp32 state" if p2 == _lib.PREC_BF16 else
                            "MMPFN_PREC_F16: fp16 state between kernels and fp16 MFMA operands (the reference's "
                            "fp16 autocast)") + ", the same step"}

    # ---- the fp32 parity mode (what the 1e-4 logits contract costs)
    f32 = None
    if args.f32_leg and prec != _lib.PREC_F32:
        step32 = make_step(eng, members, mine, assignment, rank, img, _lib.PREC_F32, args.lanes, args.batch)
        k32 = max(3, args.steps // 6)
        dt32 = timed_steps(step32, k32, 1, world, device)
        f32 = {"value": round(M * S_ROWS * k32 / dt32, 1), "unit": "rows/s", "ms_per_step": round(dt32 / k32 * 1e3, 3),
               "steps": k32, "dtype": "f32",
               "note": "the same step in the fp32 parity mode (MMPFN_PREC_F32: fp32 tensors, every contraction on "
                       "bf16 MFMA with split hi + lo operands, three products; logits within 1e-4 of the oracle)"}
        stepm = make_step(eng, members, mine, assignment, rank, img, _lib.PREC_F32_MFMA, args.lanes, args.batch)
        dtm = timed_steps(stepm, 3, 1, world, device)
        f32["fp32_input_mfma_mode"] = {
            "value": round(M * S_ROWS * 3 / dtm, 1), "unit": "rows/s", "ms_per_step": round(dtm / 3 * 1e3, 3),
            "note": "MMPFN_PREC_F32_MFMA: the same step on fp32-input MFMA (exact fp32 fma chains)"}

    api = api_def = None
    if args.api_steps > 0:
        try:
            api = api_end_to_end(cfg, sd, x, y, image, M, prec == _lib.PREC_F32, args.api_steps, world)
        except Exception as e:  # noqa: BLE001 - reported, the headline number stands on its own
            api = {"error": f"{type(e).__name__}: {e}"}
        try:
            api_def = api_end_to_end(cfg, sd, x, y, image, M, prec == _lib.PREC_F32, args.api_steps, world,
                                     preprocessing="default")
        except Exception as e:  # noqa: BLE001
            api_def = {"error": f"{type(e).__name__}: {e}"}
    kv = kv_cache_leg(eng, [members[m] for m in mine], img, prec, args.steps) if args.kv_cache and mine else None
    roof = None
    if rank == 0:
        iso = time_item_attention(eng, T, args.attn_reps)
        roof = live if live is not None else iso
        roof["isolated_single_member_launch"] = {k: iso[k] for k in ("achieved", "frac", "per_launch_ms", "traffic")}
        if live is not None and live["token_columns_per_launch"] != T:  # the step's launch shape, alone
            isb = time_item_attention(eng, live["token_columns_per_launch"], args.attn_reps)
            roof["isolated_same_shape_launch"] = {k: isb[k] for k in ("achieved", "frac", "per_launch_ms", "traffic")}
        # the same kernel at BASELINE.json's other single-GPU shapes (one layer's launch, alone):
        # B = 4096 support x 100 features (G = 50, T = 51), E = 10k support rows (G = 10, T = 11)
        # (the headline mode's Q / K precision; config E also with the fp8 P.V of MMPFN_PREC_*_F8 / _F8E5, whose
        # times include the V^T -> e4m3 conversion launch)
        roof["other_configs_isolated_launch"] = {}
        p16 = prec if prec in (_lib.PREC_F16, _lib.PREC_BF16) else _lib.PREC_BF16
        f8s = ((_lib.PREC_F16_F8, _lib.PREC_F16_F8E5) if p16 == _lib.PREC_F16 else
               (_lib.PREC_BF16_F8, _lib.PREC_BF16_F8E5))
        shapes = {"B: S=5120 N=4096 T=51": (51, 5120, 4096, (p16,)),
                  "E: S=12000 N=10000 T=11": (11, 12000, 10000, (p16,) + f8s)}
        names = {_lib.PREC_F16: "", _lib.PREC_BF16: "", _lib.PREC_F16_F8: " fp8 P.V (P e4m3)",
                 _lib.PREC_BF16_F8: " fp8 P.V (P e4m3)", _lib.PREC_F16_F8E5: " fp8 P.V (P e5m2)",
                 _lib.PREC_BF16_F8E5: " fp8 P.V (P e5m2)"}
        for name, (Tc, Sc, Nc, codes) in shapes.items():
            for code in codes:
                r = time_item_attention(eng, Tc, max(3, args.attn_reps // 4), Sc, Nc, code)
                roof["other_configs_isolated_launch"][name + names[code]] = {
                    k: r[k] for k in ("achieved", "frac", "per_launch_ms")}
                if code in (_lib.PREC_F16_F8, _lib.PREC_BF16_F8):
                    roof["other_configs_isolated_launch"][name + names[code]]["note"] = (
                        "random q / k: ~10 % of the waves fail the e4m3 range checks (first-tile scale, DESIGN 5.8) and "
                        "repeat their queries on the exact non-pipelined path (~4x a pipelined pass); e5m2 never does; "
                        "the model's own scores: config_E's 'f16 + fp8 P.V (e4m3)' step")
    return {"roofline": roof, "api_end_to_end": api, "api_end_to_end_default_preprocessing": api_def,
            "other_16bit_mode": other16, "f32_parity_mode": f32, "kv_cache_predict": kv}


def other_legs(args, sd, x, y, image, rank, world, device, prec):
    """``--full``: the legs that build engines or models of their own (configs D, B and E, the modality
    towers) and the CPU baselines; they run after the headline's engine is closed."""
    cfg_d = config_d_leg(device, world, rank, args, prec) if args.config_d else None
    cfg_b = None
    if args.config_b and rank == 0:
        try:
            cfg_b = config_b_leg(device, args)
        except Exception as e:  # noqa: BLE001 - reported, the headline number stands on its own
            cfg_b = {"error": f"{type(e).__name__}: {e}"}
    cfg_e = None
    if args.config_e and rank == 0:
        try:
            cfg_e = config_e_leg(device, args)
        except Exception as e:  # noqa: BLE001 - reported, the headline number stands on its own
            cfg_e = {"error": f"{type(e).__name__}: {e}"}
    mod = None
    if args.modality and rank == 0:
        try:
            mod = modality_leg(device, args)
        except Exception as e:  # noqa: BLE001 - reported, the headline number stands on its own
            mod = {"error": f"{type(e).__name__}: {e}"}
    cpu = cpu_e = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(sd, x, y, image, use_sdpa=True)
        if args.cpu_einsum:
            cpu_e = cpu_baseline(sd, x, y, image, use_sdpa=False)
    return {"cpu_baseline": cpu, "cpu_baseline_einsum": cpu_e, "config_B": cfg_b, "config_D": cfg_d,
            "config_E": cfg_e, "modality_encoders": mod}


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher of N rank processes (torchrun's job)
        sys.exit(launch_ranks(args.gpus, [sys.executable, "-u", str(Path(__file__).resolve()), *sys.argv[1:]]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: the world must be one rank per GPU")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # rehearsal knobs for a multi-rank run on a box with fewer GPUs than ranks (not for measurement):
    # MMPFN_BENCH_SHARE_GPUS=1 maps ranks onto the visible GPUs round-robin, MMPFN_BENCH_BACKEND=gloo
    # replaces RCCL (which refuses two ranks on one GPU)
    if os.environ.get("MMPFN_BENCH_SHARE_GPUS") == "1":
        local_rank %= torch.cuda.device_count()
    backend = os.environ.get("MMPFN_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group(backend, device_id=device if backend == "nccl" else None)

    from multimodalpfn_amd import _lib
    from multimodalpfn_amd.parallel import lpt_assign, member_cost

    prec = {"f16": _lib.PREC_F16, "bf16": _lib.PREC_BF16, "f32": _lib.PREC_F32}[args.precision]
    # the classifier legs (api_end_to_end) run inference_precision="auto" = the reference's fp16 autocast
    os.environ["MMPFN_AUTOCAST"] = "f16" if prec == _lib.PREC_F16 else "bf16"
    cfg, sd, model, x, y, image, members = build_workload(device, world, args.members)
    eng = model.engine(device)
    img = torch.from_numpy(image).to(device)
    M = len(members)
    T = (N_FEAT + 1) // 2 + CAP + 1
    assignment = lpt_assign([member_cost(T, S_ROWS, N_TRAIN)] * M, world, [T] * M, args.batch or eng.batch)
    mine = assignment[rank]
    step = make_step(eng, members, mine, assignment, rank, img, prec, args.lanes, args.batch, args.mixer_stream)

    probs = step()
    eng.status()  # NaN check once (reference raises ValueError)
    assert torch.isfinite(probs).all()
    # ---- headline: nothing but the steps in the timed region
    last = []
    dt = timed_steps(step, args.steps, args.warmup, world, device, last)
    rows = M * S_ROWS * args.steps
    value = rows / dt
    step_flop = len(mine) * forward_flops(T) + mixer_flops()  # per rank
    wf = step_flop * args.steps / dt / 1e12  # TFLOP/s of one rank (its wall time is the job's max)
    batch = eng.batch if args.batch is None else args.batch
    if args.dump_outputs and rank == 0 and last:
        dump_outputs(args.dump_outputs, last[0])

    # ---- everything else the benchmark measures: --full only (a plain run reports these as null)
    legs = dict.fromkeys(("roofline", "cpu_baseline", "cpu_baseline_einsum", "api_end_to_end",
                          "api_end_to_end_default_preprocessing", "other_16bit_mode", "f32_parity_mode", "config_B",
                          "config_D", "config_E", "kv_cache_predict", "modality_encoders"))
    if args.full:
        legs.update(engine_legs(args, eng, step, cfg, sd, x, y, image, members, mine, assignment, rank, world, device,
                                img, prec, T))
    eng.close()
    if args.full:
        legs.update(other_legs(args, sd, x, y, image, rank, world, device, prec))
    if rank == 0:
        line = {
            "metric": METRIC,
            "value": round(value, 1),
            "unit": "rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {_lib.PREC_F16: "f16", _lib.PREC_BF16: "bf16"}.get(prec, "f32"),
            "data": "synthetic (PAD-UFES-20 shape; random-init weights of the MMPFN architecture)",
            "config": {
                "workload": "config C: PAD-UFES-20 image+tabular, N=1838 support + Q=460 query rows, F=21 "
                            "(18 cat + 3 num), image [S,1,768], MGM 64 heads + CAP 24, 12 layers E=192",
                "step": "predict_proba on device-resident inputs (SURVEY 8d's wall(predict_proba) without the "
                        "host-side validation / per-member transform and the PCIe copies: those are in "
                        "api_end_to_end): mixer once, every member's 12-layer forward, all-gather, softmax-mean",
                "value_definition": "value = rows / wall time of K steps with the model and inputs resident in "
                                    "HBM (the bench contract: inputs already resident when the timed region "
                                    "starts); SURVEY 8d's wall(predict_proba) from host numpy, which adds the "
                                    "host validation / transform and the PCIe copies, is api_end_to_end (run.py's "
                                    "preprocessing) and api_end_to_end_default_preprocessing (the reference's "
                                    "default ragged members)",
                "members_per_gpu": args.members,
                "lanes": eng.lanes if args.lanes is None else args.lanes,
                "members_per_batched_forward": batch,
                "members_total": M,
                "rows_per_member": S_ROWS,
                "tokens_per_row": T,
                "parallelism": f"ensemble members sharded over {world} GPU(s) + RCCL all-gather of logits",
                "operands": OPERANDS[{_lib.PREC_F16: "f16", _lib.PREC_BF16: "bf16"}.get(prec, "f32")],
            },
            "roofline": legs["roofline"],
            "whole_forward": {
                "tflop_per_step_per_gpu": round(step_flop / 1e12, 3),
                "achieved": round(wf, 1),
                "unit": "TFLOP/s per GPU",
                "frac": round(wf / BF16_PEAK_TFLOPS, 4),
                "note": "algorithmic flops of the mixer + every member's 12-layer stack (SURVEY.md 8d) / step time",
            },
            **{k: v for k, v in legs.items() if k != "roofline"},
        }
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
