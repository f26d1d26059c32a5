"""Timing of the regression path's two new pieces at the reference's sizes (8 members, Q = 460 test rows, 5000 bars):

* the bar-distribution head (``mmpfn_bar_head``), with and without the ``[Q, B]`` logits output, and with every row
  scored at 1 and at 64 targets in the same kernel (``mmpfn_bar_head_score``);
* the same head as the restatement's torch operations on the device (the only "before" there is);
* the wide decoder per member (``mmpfn_decode`` on a value-target model) in the fp32, bf16 and fp16 modes.

Device events around ``reps`` back-to-back calls after a warm-up, three windows each; the spread is printed.
    python tools/regression_time.py [out.txt]
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "golden")]

import regression_oracle as ro  # noqa: E402

from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution, border_tables  # noqa: E402
from multimodalpfn_amd.engine import HipEngine  # noqa: E402
from multimodalpfn_amd.model.spec import ModelConfig  # noqa: E402

M, Q, B, N_TRAIN = 8, 460, 5000, 1838
LEVELS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]


def timed(fn, reps, windows=3):
    for _ in range(max(3, reps // 4)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def torch_head(logits, frm, to, masks, crit, inv_t, levels):
    """The restatement's operations (regression_oracle.head, float32) on device tensors."""
    bars = []
    for m in range(logits.shape[0]):
        out = logits[m] * inv_t
        if masks is not None:
            out = out.masked_fill(masks[m], float("-inf"))
        bars.append(ro.member_bars(out, frm[m], to))
    lg = torch.stack(bars).mean(0).log()
    probs = torch.softmax(lg, -1)
    res = [probs @ crit["bucket_means"], crit["mode_means"][(probs / crit["widths"]).argmax(-1)]]
    cum = torch.cumsum(probs, -1)
    cum0 = torch.cat([torch.zeros_like(cum[:, :1]), cum], -1)
    for lv in levels:
        idx = torch.searchsorted(cum, torch.full_like(cum[:, :1], lv)).squeeze(-1).clamp(0, B - 1)
        rest = lv - cum0.gather(-1, idx[:, None]).squeeze(-1)
        left, right = crit["borders"][idx], crit["borders"][idx + 1]
        res.append(left + (right - left) * rest / probs.gather(-1, idx[:, None]).squeeze(-1))
    return lg, res


def main():
    lines = []

    def say(s):
        print(s)
        lines.append(s)

    dev = torch.device("cuda")
    cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2, max_num_classes=0, num_buckets=B, remove_outliers_sigma=None)
    eng = HipEngine(cfg, ro.reg_state_dict(cfg, 61), dev)
    std = ro.normal_borders(B)
    kinds = ["identity", "warp", "affine", "cancel"]
    sets = [ro.member_border_set(kinds[m % 4], std) for m in range(M)]
    tabs = [border_tables(frm, std) for frm, _ in sets]
    idx, share = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    cancel = np.stack([np.zeros(B, bool) if mk is None else mk for _, mk in sets])
    crit = ro.criterion_tables(torch.from_numpy(std) * 2.5 + 1.0)
    g = torch.Generator().manual_seed(0)
    logits = (2.0 * torch.randn(M, Q, B, generator=g)).to(dev)
    say(f"bar head, M = {M} members, Q = {Q} rows, B = {B} bars, {len(LEVELS)} quantile levels; member logits "
        f"{logits.numel() * 4 / 1e6:.1f} MB")
    for want in (False, True):
        t = timed(lambda: eng.bar_head(logits, idx, share, crit, cancel=cancel, softmax_temperature=0.9,
                                       quantiles=LEVELS, want_logits=want), 50)
        say(f"  HipEngine.bar_head (table uploads and launch), logits output {'on ' if want else 'off'}: "
            f"{min(t) * 1e3:.1f} us per call (windows {', '.join(f'{v * 1e3:.1f}' for v in t)})")
    # the kernel alone: every table resident, the C entry point called directly
    ldt, ldc = (B + 4) & ~3, (B + 3) & ~3  # padded rows, as HipEngine.bar_head uploads them
    pad = lambda a, ld, fill: np.concatenate([a, np.full((M, ld - a.shape[1]), fill, a.dtype)], 1)  # noqa: E731
    d_idx, d_share = torch.from_numpy(pad(idx, ldt, -2)).to(dev), torch.from_numpy(pad(share, ldt, 0)).to(dev)
    d_cancel = torch.from_numpy(pad(cancel.astype(np.uint8), ldc, 0)).to(dev)
    d_crit = {k: v.float().contiguous().to(dev) for k, v in crit.items()}
    d_lv = torch.tensor(LEVELS, dtype=torch.float32, device=dev)
    o_mean, o_mode = torch.empty(Q, device=dev), torch.empty(Q, device=dev)
    o_q, o_lg = torch.empty(len(LEVELS), Q, device=dev), torch.empty(Q, B, device=dev)
    eng._bind_stream()
    for want in (False, True):
        def call():
            rc = eng.lib.mmpfn_bar_head(eng.ctx, logits.data_ptr(), M, Q, B, d_cancel.data_ptr(), ldc, d_idx.data_ptr(),
                                        d_share.data_ptr(), ldt, 1 / 0.9, 0, d_crit["borders"].data_ptr(),
                                        d_crit["bucket_means"].data_ptr(), d_crit["mode_means"].data_ptr(),
                                        d_crit["widths"].data_ptr(), d_lv.data_ptr(), len(LEVELS),
                                        o_lg.data_ptr() if want else None, o_mean.data_ptr(), o_mode.data_ptr(),
                                        o_q.data_ptr())
            assert rc == 0
        t = timed(call, 200)
        say(f"  bar_head_kernel alone (tables resident), logits output {'on ' if want else 'off'}: "
            f"{min(t) * 1e3:.1f} us (windows {', '.join(f'{v * 1e3:.1f}' for v in t)}); "
            f"{logits.numel() * 4 / (min(t) * 1e-3) / 1e12:.2f} TB/s of member logits")
    # the head with every row scored in the same kernel (mmpfn_bar_head_score), J targets per row, no logits output
    d_score = {k: v.to(dev) for k, v in FullSupportBarDistribution(crit["borders"]).score_tables().items()}
    lo, hi = float(crit["borders"][0]), float(crit["borders"][-1])
    for J in (1, 64):
        ys = (lo + (hi - lo) * torch.rand(Q, J, generator=g)).to(dev)
        outs = [torch.empty(Q, J, device=dev) for _ in range(4)] + [torch.empty(Q, device=dev)]

        def call_scored():
            rc = eng.lib.mmpfn_bar_head_score(eng.ctx, logits.data_ptr(), M, Q, B, d_cancel.data_ptr(), ldc,
                                              d_idx.data_ptr(), d_share.data_ptr(), ldt, 1 / 0.9, 0,
                                              d_crit["borders"].data_ptr(), d_crit["bucket_means"].data_ptr(),
                                              d_crit["mode_means"].data_ptr(), d_crit["widths"].data_ptr(),
                                              d_lv.data_ptr(), len(LEVELS), None, o_mean.data_ptr(), o_mode.data_ptr(),
                                              o_q.data_ptr(), d_score["log_widths"].data_ptr(),
                                              d_score["mean_squares"].data_ptr(), d_score["ei_mids"].data_ptr(),
                                              d_score["ends"].data_ptr(), ys.data_ptr(), J, *(o.data_ptr() for o in outs))
            assert rc == 0
        t = timed(call_scored, 200)
        say(f"  bar_head_kernel with the scores (tables resident), J = {J:2d} targets per row: "
            f"{min(t) * 1e3:.1f} us (windows {', '.join(f'{v * 1e3:.1f}' for v in t)})")
    frm_d = [torch.from_numpy(f).to(dev) for f, _ in sets]
    to_d = torch.from_numpy(std).to(dev)
    masks_d = torch.from_numpy(cancel).to(dev)
    crit_d = {k: v.to(dev) for k, v in crit.items()}
    with torch.inference_mode():
        t = timed(lambda: torch_head(logits, frm_d, to_d, masks_d, crit_d, 1 / 0.9, LEVELS), 10)
    say(f"  the restatement's torch operations on the device (fp32): {min(t) * 1e3:.1f} us per call (windows "
        f"{', '.join(f'{v * 1e3:.1f}' for v in t)})")
    got = eng.bar_head(logits, idx, share, crit, cancel=cancel, softmax_temperature=0.9, quantiles=LEVELS)
    with torch.inference_mode():
        _, ref = torch_head(logits, frm_d, to_d, masks_d, crit_d, 1 / 0.9, LEVELS)
    say(f"  kernel vs torch on the device: mean |d| {float((got['mean'] - ref[0]).abs().max()):.2e}, median |d| "
        f"{float((got['quantiles'][4] - ref[2 + 4]).abs().max()):.2e}")

    from synth import synth_table

    x = torch.from_numpy(synth_table(N_TRAIN + Q, 20, 61)).to(dev)
    y = np.random.default_rng(61).standard_normal(N_TRAIN).astype(np.float32)
    say(f"wide decoder, one member, Q = {Q} rows, nhid {cfg.nhid}, n_out = {B}")
    for prec, name in ((0, "fp32 (fp32-input MFMA)"), (1, "bf16"), (5, "fp16")):
        eng.embed_state(x, None, y, prec)
        eng.run_layers(0, 1)
        t = timed(lambda: eng.decode(Q), 50)
        flops = 2.0 * Q * cfg.nhid * (cfg.emsize + B)
        say(f"  {name}: {min(t) * 1e3:.1f} us per member (windows {', '.join(f'{v * 1e3:.1f}' for v in t)}); "
            f"{flops / (min(t) * 1e-3) / 1e12:.1f} TFLOP/s of {flops / 1e9:.2f} GFLOP")
    eng.status()
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
