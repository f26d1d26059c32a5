"""Diagnostics: the outputs of one engine library (MMPFN_LIB) over every precision mode and dispatch path, saved to
an .npz, so that two builds meant to be bitwise equal can be compared:  MMPFN_LIB=... python tools/lib_outputs.py out.npz
then  python tools/lib_outputs.py --compare a.npz b.npz
Legs: the fp16, bf16, fp32 (split-bf16) and fp32-MFMA logits of every golden case; the two fp16 + fp8 P.V modes on
pad_ufes_12l, and its four base modes with the last layer run in full; forward_many with 2 lanes and batch 2 on one
golden; a table wider than 64 tokens per row (the bf16 fallback path) in the bf16, fp32 and fp32-MFMA modes: the
forward, the cached predict, and the layer-0 attention taps, and that model's MGM bank and mixer tokens in the fp16 and
bf16 modes (the big-tile mixer GEMMs); the four C-ABI item-attention taps on a seeded case; and the modality towers'
GEMM (mmpfn_enc_linear) with each epilogue."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "golden")]


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = [k for k in a.files if k not in b.files or not np.array_equal(a[k], b[k])]
    bad += [k for k in b.files if k not in a.files]
    for k in a.files:
        if k not in bad:
            print(f"{k}: EQUAL")
        elif k in b.files and a[k].shape == b[k].shape:
            print(f"{k}: DIFF max {np.abs(a[k] - b[k]).max():.3e}")
        else:
            print(f"{k}: DIFF (missing or another shape)")
    for k in b.files:
        if k not in a.files:
            print(f"{k}: DIFF (only in {pb})")
    return 1 if bad else 0


def lanes_leg(z, model, _lib):
    """Four label-permuted members of one golden through forward_many, 2 lanes x batch 2."""
    import torch

    eng = model.engine()
    x = torch.from_numpy(z["x"]) if "x" in z else None
    tok = eng.mixer_tokens(torch.from_numpy(z["image"]).cuda(), _lib.PREC_BF16) if "image" in z else None
    y = z["y_train"]
    cls = np.unique(y)
    rng = np.random.default_rng(1)
    items = []
    for _ in range(4):
        perm = dict(zip(cls, rng.permutation(cls)))
        items.append((x, tok, np.array([perm[v] for v in y], dtype=np.float32)))
    with torch.inference_mode():
        outs = eng.forward_many(items, _lib.PREC_BF16, lanes=2, batch=2)
        eng.status()
    return np.stack([o.cpu().numpy() for o in outs])


def wide_legs(_lib):
    """71 tokens per row (140 features): 2 layers, S = 260, N = 200."""
    import torch
    from synth import synth_labels, synth_state_dict, synth_table
    from test_parity_gpu import make_model

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    cfg = ModelConfig(nlayers=2, mgm_heads=8, cap_heads=4)
    model = make_model(cfg, synth_state_dict(state_dict_spec(cfg), 21))
    eng = model.engine()
    S, N, F = 260, 200, 140
    x = torch.from_numpy(synth_table(S, F, 21, n_cat=2)).cuda()
    y = synth_labels(S, 3, 21)[:N]
    res = {}
    with torch.inference_mode():
        X = eng.embed_state(x, None, y, _lib.PREC_F32)
        for name, p in (("bf16", _lib.PREC_BF16), ("f32", _lib.PREC_F32), ("f32mfma", _lib.PREC_F32_MFMA)):
            res[f"wide_{name}"] = eng.forward(x, None, y, p)
            cache = eng.cache_build(x[:N], None, y, p)
            res[f"wide_cached_{name}"] = eng.cache_predict(cache, x[N:], None)
            cache.free()
            res[f"wide_feat_tap_{name}"] = eng.feature_attention(0, X, p)
            res[f"wide_item_tap_{name}"] = eng.item_attention_block(0, X, N, p)
        # the big-tile mixer GEMMs (gemm_glu_big_kernel, gemm_remap_big_kernel), S = 330: two M tiles of 256, one
        # full and one partial tile of 320; mixer_tokens of this MGM + CAP model takes the 16-bit token output
        im = torch.randn(330, 2, cfg.nhid, generator=torch.Generator().manual_seed(23)).cuda()
        for name, p in (("f16", _lib.PREC_F16), ("bf16", _lib.PREC_BF16)):
            res[f"mgm_{name}"] = eng.mgm(im, p)
            res[f"mixer_tokens_{name}"] = eng.mixer_tokens(im, p)
        eng.status()
    return {k: v.cpu().numpy() for k, v in res.items()}


def enc_linear_legs(_lib):
    """mmpfn_enc_linear (gemm_tile_kernel), M = 300 (two M tiles, the second partial), N = 512: K = 256 (eight
    slices: the four-stage ring wraps) and K = 64 (two slices, fewer than the stages), each epilogue."""
    import modality_kernel_cases as mk
    import torch

    lib = _lib.load_library()
    enc = lib.mmpfn_enc_create(0, None)
    assert enc
    M, N = 300, 512
    res = {}
    for K in (256, 64):
        ops = mk.operands(M, N, K, "normal", seed=K)
        A, W, bias, gamma = (ops[k].cuda() for k in ("A", "W", "bias", "gamma"))
        for name, epi, act in (("bf16", mk.EPI_BF16, 0), ("bf16_gelu", mk.EPI_BF16, 1), ("f32", mk.EPI_F32, 0),
                               ("resid", mk.EPI_RESID, 0)):
            C = ops["c0"].cuda() if epi == mk.EPI_RESID else torch.zeros(
                M, N, device="cuda", dtype=torch.bfloat16 if epi == mk.EPI_BF16 else torch.float32)
            rc = lib.mmpfn_enc_linear(enc, A.data_ptr(), W.data_ptr(), bias.data_ptr(),
                                      gamma.data_ptr() if epi == mk.EPI_RESID else None, C.data_ptr(), M, N, K, epi, act)
            assert rc == 0, (K, name, rc)
            torch.cuda.synchronize()
            res[f"enc_linear_K{K}_{name}"] = C.float().cpu().numpy()
    lib.mmpfn_enc_destroy(enc)
    return res


def attention_tap_legs(_lib):
    """The four C-ABI item-attention taps, S = 100, N = 70 (Npad = 128), T = 2, H = 6: mmpfn_item_attention in its
    three codes (train rows on their own heads, kvh = -1, then test rows against head 0), the bf16 layer tap, the
    layer_ex tap (fp8 P.V, fp16, and the fp16 forward's form) and the cached tap."""
    import torch
    from test_parity_gpu import _launch_cached, _launch_layer, _qkv_case

    S, N, T, H, d = 100, 70, 2, 6, 32
    q, k, v, Npad = _qkv_case(S, N, T, H, d, seed=5)
    kp = torch.zeros(T, H, Npad, d)
    kp[:, :, :N] = k
    vt = torch.zeros(T, H, d, Npad)
    vt[:, :, :, :N] = v.transpose(-1, -2)
    lib = _lib.load_library()
    ctx = lib.mmpfn_create(0, None)
    res = {}
    for code in (_lib.PREC_F32, _lib.PREC_BF16, _lib.PREC_F32_MFMA):
        dt = torch.bfloat16 if code == _lib.PREC_BF16 else torch.float32
        qd, kd, vd = q.to("cuda", dt), kp.to("cuda", dt), vt.to("cuda", dt)
        out = torch.zeros(T, S, H * d, device="cuda", dtype=dt)
        for s0, nq, kvh in ((0, N, -1), (N, S - N, 0)):
            rc = lib.mmpfn_item_attention(ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), S, T, H,
                                          Npad, s0, nq, N, kvh, code)
            assert rc == 0, (code, kvh, rc)
        torch.cuda.synchronize()
        res[f"tap_item_attention_{code}"] = out.float().cpu()
    lib.mmpfn_destroy(ctx)
    res["tap_layer"] = _launch_layer(q, k, v, Npad, N, 1)
    for code in (_lib.PREC_BF16_F8, _lib.PREC_F16, _lib.PREC_F16 | _lib.ATTN_QK_BF16):
        res[f"tap_layer_ex_{code}"] = _launch_layer(q, k, v, Npad, N, code)
    res["tap_cached"] = _launch_cached(q, k[:, 0], v[:, 0], Npad, N)
    return {k: v.numpy() for k, v in res.items()}


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    from helpers import CASES, load_case
    from test_parity_gpu import make_model, run_case

    from multimodalpfn_amd import _lib

    modes = (("f16", _lib.PREC_F16), ("bf16", _lib.PREC_BF16), ("f32", _lib.PREC_F32), ("f32mfma", _lib.PREC_F32_MFMA))
    res = {}
    for case in CASES:
        z, meta, cfg, sd = load_case(case)
        model = make_model(cfg, sd)
        for name, p in modes:
            res[f"{case}_{name}"] = run_case(z, model, precision=p)
        if case == "pad_ufes_12l":
            for name, p in (("f16_f8", _lib.PREC_F16_F8), ("f16_f8e5", _lib.PREC_F16_F8E5)):
                res[f"{case}_{name}"] = run_case(z, model, precision=p)
            res[f"{case}_lanes2_batch2_bf16"] = lanes_leg(z, model, _lib)
            model.engine().full_last_layer = True  # (the default, pruned form: the legs above)
            for name, p in modes:
                res[f"{case}_full_last_{name}"] = run_case(z, model, precision=p)
            model.engine().full_last_layer = False
    res.update(wide_legs(_lib))
    res.update(attention_tap_legs(_lib))
    res.update(enc_linear_legs(_lib))
    np.savez(sys.argv[1], **res)
    print("saved", len(res), "outputs to", sys.argv[1])


if __name__ == "__main__":
    main()
