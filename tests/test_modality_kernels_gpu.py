"""The modality towers' kernels alone (csrc/modality.hip behind include/mmpfn_modality.h), over the geometry
``mmpfn_enc_set_model`` accepts -- tests/test_modality_gpu.py pins the towers at the reference's one geometry.

* ``mmpfn_enc_linear`` (gemm_tile_kernel) against float64 of the same bf16 operands: integer data must come back
  exactly (fp32 sums of small integers are exact in any order), normal data within the per-element bounds derived
  in tests/modality_kernel_cases.py.  Every call's C has 256 guard rows past M that must keep their bit pattern.
* ``mmpfn_enc_attention`` (attn64_kernel / attn64_f32_kernel) against ``_attn_ref`` of test_modality_gpu.py, with its
  bounds (1e-2 bf16, 1e-4 fp32), around the 64-key tile and the 256-query chunk.
* Whole towers of depth 1 or 2 at the other accepted widths, patch sizes and positional grids against
  oracle/modality.py evaluated in float64 on the CPU.

Tower tolerances (rel = max |d| / max(1, max |ref|), as in test_modality_gpu.py): fp32 mode 1e-4; bf16 mode the band
written per case in ``BF16_TOL`` below, about twice the deviation measured on MI355X.  tests/
test_modality_kernels_sensitivity.py shows on the CPU what the GEMM and attention bounds catch.
"""

import numpy as np
import pytest
import torch

import modality_kernel_cases as mk
from helpers import report
from modality_cases import _lin, _ln, _rng, text_config, text_inputs, text_state
from multimodalpfn_amd import _lib
from multimodalpfn_amd.modality import DinoVisionTransformer, ElectraTextEncoder
from oracle.modality import electra_forward, vit_forward_features
from test_modality_gpu import _attn_ref, rel

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4
GUARD = 256                 # rows of C past M that no call may touch
PAT16, PAT32 = 0x7A5B, 0x7FA55AA5  # their bit patterns (bf16 / fp32 C)


@pytest.fixture(scope="module")
def tap():
    lib = _lib.load_library()
    enc = lib.mmpfn_enc_create(0, None)
    assert enc
    yield lib, enc
    lib.mmpfn_enc_destroy(enc)
    if any(_ATTN_WORST.values()):
        report(f"attention tap grid (L 1 .. 513): worst rel bf16 {_ATTN_WORST['bf16']:.3e}, f32 {_ATTN_WORST['f32']:.3e}")


# ------------------------------------------------------------------------------------------------ GEMM tap
def _linear(tap, ops, epi, act, gamma):
    """One mmpfn_enc_linear call on ``ops`` -> C[:M] on the host; asserts the guard rows kept their bits."""
    lib, enc = tap
    M, N, K = ops["M"], ops["N"], ops["K"]
    A, W, bias = ops["A"].cuda(), ops["W"].cuda(), ops["bias"].cuda()
    gd = gamma.cuda() if gamma is not None else None
    bf = epi == mk.EPI_BF16
    C = torch.empty(M + GUARD, N, device="cuda", dtype=torch.bfloat16 if bf else torch.float32)
    bits = C.view(torch.int16 if bf else torch.int32)
    bits.fill_(PAT16 if bf else PAT32)
    if epi == mk.EPI_RESID:
        C[:M] = ops["c0"].cuda()
    rc = lib.mmpfn_enc_linear(enc, A.data_ptr(), W.data_ptr(), bias.data_ptr(), gd.data_ptr() if gd is not None else None,
                              C.data_ptr(), M, N, K, epi, act)
    assert rc == 0, lib.mmpfn_enc_last_error(enc)
    torch.cuda.synchronize()
    assert bool((bits[M:] == (PAT16 if bf else PAT32)).all()), "rows past M were written"
    return C[:M].cpu()


def _assert_exact(tap, ops):
    """Integer operands: the three epilogues equal the float64 result (the bf16 store: its round-to-nearest-even)."""
    pre = mk.preactivation(ops["A"], ops["W"], ops["bias"])
    got = _linear(tap, ops, mk.EPI_F32, 0, None)
    assert torch.equal(got.double(), pre), "fp32 store"
    got = _linear(tap, ops, mk.EPI_BF16, 0, None)
    assert torch.equal(got, pre.float().bfloat16()), "bf16 store"
    for gamma in (ops["gamma"], None):
        got = _linear(tap, ops, mk.EPI_RESID, 0, gamma)
        assert torch.equal(got.double(), mk.expected(pre, mk.EPI_RESID, 0, gamma, ops["c0"])), "residual"


def _assert_bounded(tap, ops, forms, label):
    """Normal operands: every (epilogue, act, with gamma) of ``forms`` within its per-element bound."""
    pre = mk.preactivation(ops["A"], ops["W"], ops["bias"])
    ab = mk.accb(ops)
    worst = {}
    for epi, act, with_gamma in forms:
        gamma = ops["gamma"] if with_gamma else None
        ref = mk.expected(pre, epi, act, gamma, ops["c0"])
        got = _linear(tap, ops, epi, act, gamma).double()
        assert bool(torch.isfinite(got).all())
        worst[(epi, act, with_gamma)] = float(((got - ref).abs() / mk.bound(pre, ref, ab, epi, act, gamma)).max())
    names = {mk.EPI_BF16: "bf16", mk.EPI_RESID: "resid", mk.EPI_F32: "f32"}
    report(f"enc_linear {label}: worst |d| / bound " + ", ".join(
        f"{names[e]}{'+gelu' if a else ''}{'+gamma' if g else ''} {v:.3f}" for (e, a, g), v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


ALL_FORMS = [(mk.EPI_BF16, 0, False), (mk.EPI_BF16, 1, False), (mk.EPI_F32, 0, False), (mk.EPI_RESID, 0, True),
             (mk.EPI_RESID, 0, False)]


@pytest.mark.parametrize("N", [256, 768, 2304, 3072, 4352])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1025, 1300, 2305])
def test_linear_tile_map_is_exact_on_integers(tap, M, N):
    """The block-to-tile map (XCD-contiguous, 4 x 8 super-tiles with partial ones at both edges): M tiles 1, 1, 1,
    2, 5, 6, 10 x N tiles 1, 3, 9, 12, 17 at K = 64.  A misplaced, missing or doubly written tile cannot hide:
    the data is integer-valued, so every output is exact and compared with torch.equal."""
    _assert_exact(tap, mk.operands(M, N, 64, "int", seed=M * 10007 + N))


K_RING = [32, 64, 96, 128, 160, 256, 640, 768, 3072, 4096]


@pytest.mark.parametrize("K", K_RING)
def test_linear_k_ring_is_exact_on_integers(tap, K):
    """K / 32 = 1 .. 4 slices are the four branches of the prologue's vmcnt ladder (fewer slices than ring
    stages), 5 the first stage reuse; then the towers' own K.  A dropped or doubly counted slice changes integers."""
    _assert_exact(tap, mk.operands(257, 512, K, "int", seed=K))


@pytest.mark.parametrize("K", K_RING)
def test_linear_k_ring_within_summation_bounds(tap, K):
    _assert_bounded(tap, mk.operands(257, 512, K, "normal", seed=5000 + K), ALL_FORMS, f"K ring M 257 N 512 K {K}")


@pytest.mark.parametrize("name", sorted({s[0].replace("_gamma", "") for s in mk.TOWER_SHAPES}))
def test_linear_tower_shapes_within_summation_bounds(tap, name):
    """The towers' own GEMMs at 1300 rows (6 M tiles, the last of 20 rows), normal data.  The GELU case's reference
    is the tanh form in float64 on the float64 pre-activation -- the arithmetic the epilogue is specified to do;
    its bound adds to the bf16 rounding 2^-8 |ref| the pre-activation's summation bound through the largest slope
    1.13 and the allowance for evaluating the exponent in fp32, which modality_kernel_cases.gelu_allowance derives
    from |u| * 2^-23 (it is relative to the result and below 2e-5 of it)."""
    shapes = [s for s in mk.TOWER_SHAPES if s[0].replace("_gamma", "") == name]
    _, M, N, K, _, _, _ = shapes[0]
    ops = mk.tower_operands(name)
    _assert_bounded(tap, ops, [(epi, act, g) for _, _, _, _, epi, act, g in shapes], f"tower shape {name} {M} x {N} x {K}")


def test_linear_refuses_what_the_launcher_cannot_run(tap):
    lib, enc = tap
    A = torch.zeros(8, 64, device="cuda", dtype=torch.bfloat16)
    W = torch.zeros(512, 64, device="cuda", dtype=torch.bfloat16)
    C = torch.full((16, 256), 7.0, device="cuda", dtype=torch.float32)  # 8 rows of N = 256 and 8 guard rows
    ok = (8, 256, 64, mk.EPI_F32, 0)
    bad = {
        "N % 256": (8, 300, 64, mk.EPI_F32, 0),
        "K % 32": (8, 256, 48, mk.EPI_F32, 0),
        "K = 0": (8, 256, 0, mk.EPI_F32, 0),
        "K < 0": (8, 256, -32, mk.EPI_F32, 0),
        "act with the fp32 store": (8, 256, 64, mk.EPI_F32, 1),
        "act with the residual": (8, 256, 64, mk.EPI_RESID, 1),
        "act 2": (8, 256, 64, mk.EPI_BF16, 2),
        "unknown epilogue": (8, 256, 64, 3, 0),
        "M = 0": (0, 256, 64, mk.EPI_F32, 0),
    }
    for what, (M, N, K, epi, act) in bad.items():
        rc = lib.mmpfn_enc_linear(enc, A.data_ptr(), W.data_ptr(), None, None, C.data_ptr(), M, N, K, epi, act)
        assert rc == _lib.MMPFN_ERR_INVALID, what
        assert lib.mmpfn_enc_last_error(enc), what
    assert lib.mmpfn_enc_linear(enc, None, W.data_ptr(), None, None, C.data_ptr(), *ok) == _lib.MMPFN_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((C == 7.0).all())  # a refused call launches nothing
    # the context stays usable; bias NULL = 0
    assert lib.mmpfn_enc_linear(enc, A.data_ptr(), W.data_ptr(), None, None, C.data_ptr(), *ok) == 0
    torch.cuda.synchronize()
    assert bool((C[:8] == 0.0).all()) and bool((C[8:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ attention tap
ATTN_L = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513]
ATTN_BH = [(1, 1), (3, 4), (5, 3), (2, 12)]


def _attention(tap, qkv, kb, prec):
    """mmpfn_enc_attention on qkv [B][L][3][H][64] (fp32 host values) -> (output, fp64 reference, rel error)."""
    lib, enc = tap
    B, L, _, H, _ = qkv.shape
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    qd = qkv.to(dt).cuda()
    kbd = kb.cuda() if kb is not None else None
    out = torch.empty(B, L, H * 64, device="cuda", dtype=dt)
    rc = lib.mmpfn_enc_attention(enc, qd.data_ptr(), kbd.data_ptr() if kbd is not None else None, out.data_ptr(),
                                 B, L, H, 1 if prec == "bf16" else 0)
    assert rc == 0, lib.mmpfn_enc_last_error(enc)
    torch.cuda.synchronize()
    got = out.float().cpu()
    ref = _attn_ref(qd.float().cpu(), kb, bf16_q=prec == "bf16")
    assert bool(torch.isfinite(got).all())
    return got, ref, rel(got.numpy(), ref.numpy())


_ATTN_WORST = {"bf16": 0.0, "f32": 0.0}


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("B,H", ATTN_BH)
@pytest.mark.parametrize("L", ATTN_L)
def test_attention_tap_over_tile_and_chunk_edges(tap, L, B, H, prec):
    """L below, at and past the 64-key tile (the bf16 kernel's; 32 in the fp32 kernel) and the 256-query chunk (128
    in the fp32 kernel); B * H * chunks = 1 .. 72 covers the XCD task map with and without a remainder of 8."""
    g = torch.Generator().manual_seed(1000 * L + 10 * B + H)
    qkv = torch.randn(B, L, 3, H, 64, generator=g)
    _, _, err = _attention(tap, qkv, None, prec)
    _ATTN_WORST[prec] = max(_ATTN_WORST[prec], err)
    print(f"attention tap L {L} B {B} H {H} {prec}: {err:.3e}")
    assert err <= (1e-2 if prec == "bf16" else F32_TOL), err


def _bias_case(case):
    """(qkv, key bias) of the named case, B, H = 3, 4."""
    inf = float("inf")
    L = {"finite_65": 65, "finite_257": 257, "finite_masked_65": 65, "finite_masked_257": 257,
         "large_first_tile_masked": 130, "large_finite": 130, "last_partial_tile_masked": 70}[case]
    g = torch.Generator().manual_seed(len(case) * 100 + L)
    qkv = torch.randn(3, L, 3, 4, 64, generator=g)
    kb = 2.0 * torch.randn(3, L, generator=g)  # N(0, 2^2): the s + b log2(e) branch
    if case.startswith("finite_masked"):
        kb[torch.rand(3, L, generator=g) < 1 / 3] = -inf
        kb[:, 0] = 0.5
    elif case == "large_first_tile_masked":  # re-run pass entered with its first tile fully masked
        qkv[:, :, 0] *= 40.0
        kb = torch.zeros(3, L)
        kb[:, :64] = -inf
    elif case == "large_finite":
        qkv[:, :, 0] *= 40.0
    elif case == "last_partial_tile_masked":
        kb = torch.zeros(3, L)
        kb[:, 64:] = -inf
    return qkv, kb


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("case", ["finite_65", "finite_257", "finite_masked_65", "finite_masked_257",
                                  "large_first_tile_masked", "large_finite", "last_partial_tile_masked"])
def test_attention_tap_key_bias(tap, case, prec):
    """A finite non-zero key bias (natural-log units; the bf16 kernel's scores are in log2 units), alone and with a
    third of the keys excluded; q x 40 (row sums past 2^100: the bf16 kernel re-runs with a running max) with the
    whole first key tile excluded, so the re-run starts without a reference, and with the finite bias; the last,
    partial tile excluded entirely."""
    qkv, kb = _bias_case(case)
    _, _, err = _attention(tap, qkv, kb, prec)
    report(f"attention tap {case} {prec}: {err:.3e}")
    assert err <= (1e-2 if prec == "bf16" else F32_TOL), err


# ------------------------------------------------------------------------------------------------ towers
# bf16 bands: about twice the deviation measured on MI355X from the float64 oracle (worst of the full pass and the
# CLS-only path; the measured value is the comment beside each band)
BF16_TOL = {
    "vit_d256_kpad640": 1e-2,       # measured 4.86e-3 (patch tokens; cls and the CLS-only path 3.20e-3)
    "vit_d512_p8_c1": 9.5e-3,       # 4.59e-3 (cls 2.43e-3)
    "vit_d1024_identity": 6e-3,     # 2.99e-3 (cls 1.75e-3)
    "vit_d1024_up_offset": 6e-3,    # 2.98e-3 (cls 1.99e-3)
    "vit_d1024_up_exact": 6.5e-3,   # 3.12e-3 (cls 2.02e-3)
    "text_d256_e32": 1.1e-2,        # 5.54e-3 (padded batch, one text per call and the CLS-only path alike)
    "text_d256_e96": 9e-3,          # 4.46e-3
    "text_d256_e128": 1e-2,         # 5.04e-3
    "text_d512_e512": 8.5e-3,       # 4.10e-3
    "text_d256_e1024": 9e-3,        # 4.38e-3 (CLS-only path 3.88e-3)
}
# measured in the fp32 mode (bound F32_TOL): vit_d768_f32 1.36e-6, text_d768_e96_f32 1.29e-6

VIT = {
    # Kpad 640 > dim; 130 images x 10 tokens = 1300 rows = 6 M tiles; mlp_hidden 3 x dim
    "vit_d256_kpad640": dict(dim=256, heads=4, hidden=768, patch=14, chans=3, grid=37, depth=2, init_values=1.0,
                             offset=0.1, B=130, H=42, W=42, seed=31),
    # Kpad 64 = C * P * P: no zero padding
    "vit_d512_p8_c1": dict(dim=512, heads=8, hidden=2048, patch=8, chans=1, grid=7, depth=2, init_values=1.0,
                           offset=0.1, B=2, H=24, W=40, seed=32),
    # the patch grid equals pos_grid: the positional table as it is; LayerNorm V4 = 4
    "vit_d1024_identity": dict(dim=1024, heads=16, hidden=4096, patch=16, chans=3, grid=3, depth=1, init_values=1.0,
                               offset=0.1, B=2, H=48, W=48, seed=33),
    # bicubic up-sampling 3 -> 5 x 4 (clamped border taps), by scale factors and to the exact size
    "vit_d1024_up_offset": dict(dim=1024, heads=16, hidden=4096, patch=16, chans=3, grid=3, depth=1, init_values=None,
                                offset=0.1, B=2, H=80, W=64, seed=34),
    "vit_d1024_up_exact": dict(dim=1024, heads=16, hidden=4096, patch=16, chans=3, grid=3, depth=1, init_values=None,
                               offset=0.0, B=2, H=80, W=64, seed=34),
    # fp32 mode over many M tiles
    "vit_d768_f32": dict(dim=768, heads=12, hidden=3072, patch=14, chans=3, grid=37, depth=1, init_values=1.0,
                         offset=0.1, B=130, H=42, W=42, seed=35),
}


def _vit_state(c):
    """Seeded weights with the reference's state-dict names, as modality_cases.vit_state draws them, for any channel
    count and mlp_hidden."""
    r = _rng(c["seed"])
    D, P, G, C, F = c["dim"], c["patch"], c["grid"], c["chans"], c["hidden"]
    sd = {}
    sd["cls_token"] = r.standard_normal((1, 1, D), dtype=np.float32)
    sd["pos_embed"] = r.standard_normal((1, 1 + G * G, D), dtype=np.float32) * np.float32(0.5)
    sd["mask_token"] = np.zeros((1, D), np.float32)
    sd["patch_embed.proj.weight"] = r.standard_normal((D, C, P, P), dtype=np.float32) / np.float32(np.sqrt(C * P * P))
    sd["patch_embed.proj.bias"] = r.standard_normal(D, dtype=np.float32) * np.float32(0.05)
    for i in range(c["depth"]):
        p = f"blocks.{i}."
        _ln(r, p + "norm1", D, sd)
        _lin(r, p + "attn.qkv", 3 * D, D, sd)
        _lin(r, p + "attn.proj", D, D, sd)
        _ln(r, p + "norm2", D, sd)
        _lin(r, p + "mlp.fc1", F, D, sd)
        _lin(r, p + "mlp.fc2", D, F, sd)
        if c["init_values"]:
            sd[p + "ls1.gamma"] = r.uniform(0.2, 1.0, D).astype(np.float32)
            sd[p + "ls2.gamma"] = r.uniform(0.2, 1.0, D).astype(np.float32)
    _ln(r, "norm", D, sd)
    return sd


def _run_vit(name, prec):
    """(rel of cls, rel of the patch tokens, rel of the CLS-only path) against the float64 oracle."""
    c = VIT[name]
    sd = {k: torch.from_numpy(v) for k, v in _vit_state(c).items()}
    x = torch.from_numpy(_rng(c["seed"] + 1000).uniform(0.0, 1.0, (c["B"], c["chans"], c["H"], c["W"])).astype(np.float32))
    with torch.no_grad():
        ref = vit_forward_features({k: v.double() for k, v in sd.items()}, x.double(), patch=c["patch"],
                                   heads=c["heads"], depth=c["depth"], offset=c["offset"],
                                   layerscale=bool(c["init_values"]))
    assert ref["x_norm_clstoken"].dtype == torch.float64
    m = DinoVisionTransformer(img_size=c["grid"] * c["patch"], patch_size=c["patch"], in_chans=c["chans"],
                              embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"],
                              mlp_ratio=c["hidden"] / c["dim"], init_values=c["init_values"], block_chunks=0,
                              interpolate_offset=c["offset"], precision=prec)
    m.load_state_dict(sd)
    try:
        out = m.forward_features(x.cuda())
        fast = m.cls_embeddings(x.cuda()).cpu().numpy()
        cls, tok = out["x_norm_clstoken"].cpu().numpy(), out["x_norm_patchtokens"].cpu().numpy()
    finally:
        m._drop_contexts()
    assert np.isfinite(cls).all() and np.isfinite(tok).all() and np.isfinite(fast).all()
    rcls = ref["x_norm_clstoken"].numpy()
    return rel(cls, rcls), rel(tok, ref["x_norm_patchtokens"].numpy()), rel(fast, rcls)


@pytest.mark.parametrize("name", [n for n in VIT if n in BF16_TOL])
def test_vit_geometries_bf16(name):
    e = _run_vit(name, "bf16")
    report(f"{name} bf16: cls {e[0]:.3e}, patch tokens {e[1]:.3e}, CLS-only path {e[2]:.3e}")
    assert max(e) <= BF16_TOL[name]


def test_vit_many_m_tiles_f32():
    e = _run_vit("vit_d768_f32", "f32")
    report(f"vit_d768_f32 f32: cls {e[0]:.3e}, patch tokens {e[1]:.3e}, CLS-only path {e[2]:.3e}")
    assert max(e) <= F32_TOL


_LENGTHS = [260, 17, 512, 1, 300]  # padded: 5 x 512 = 2560 rows; alone: 1 .. 512 rows


def _text(dim, heads, ffn, emb, depth, seed):
    return dict(vocab=1000, emb=emb, dim=dim, depth=depth, heads=heads, ffn=ffn, max_pos=512, types=2,
                lengths=_LENGTHS, seed=seed)


TEXT = {
    # embeddings_project with K = 32, 96, 128: 1, 3, 4 slices of the GEMM's four-stage ring (text_embed V4 1)
    "text_d256_e32": _text(256, 4, 768, 32, 2, 41),
    "text_d256_e96": _text(256, 4, 768, 96, 2, 42),
    "text_d256_e128": _text(256, 4, 768, 128, 2, 43),
    "text_d512_e512": _text(512, 8, 2048, 512, 2, 44),    # text_embed V4 2, no projection
    "text_d256_e1024": _text(256, 4, 768, 1024, 2, 45),   # text_embed V4 4, E > D
    "text_d768_e96_f32": _text(768, 12, 3072, 96, 1, 46),
}


def _text_model(c, prec):
    m = ElectraTextEncoder(text_config(c), precision=prec)
    sd = {k: torch.from_numpy(v) for k, v in text_state(c).items()}
    m.load_state_dict(sd)
    return m, sd


def _text_errors(m, c, sd):
    """Worst rel over the five texts of (the padded batch under the mask, one text per call, the CLS-only path)
    against the float64 oracle of each text alone; token_type_ids None."""
    ids = [torch.from_numpy(t) for t in text_inputs(c)[0]]
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        refs = [electra_forward(sd64, t[None], None, None, heads=c["heads"], depth=c["depth"])[0].numpy() for t in ids]
    assert refs[0].dtype == np.float64
    L = max(len(t) for t in ids)
    bid = torch.zeros((len(ids), L), dtype=torch.long)
    bm = torch.zeros_like(bid)
    for j, t in enumerate(ids):
        bid[j, :len(t)], bm[j, :len(t)] = t, 1
    hb = m(bid.cuda(), bm.cuda()).last_hidden_state.cpu().numpy()
    cls = m.cls_embeddings(bid.cuda(), bm.cuda()).cpu().numpy()
    alone = [m(t[None].cuda()).last_hidden_state[0].cpu().numpy() for t in ids]
    assert np.isfinite(cls).all() and all(np.isfinite(a).all() for a in alone)
    e_batch = max(rel(hb[j, :len(t)], refs[j]) for j, t in enumerate(ids))
    e_alone = max(rel(a, r) for a, r in zip(alone, refs))
    e_cls = max(rel(cls[j], refs[j][0]) for j in range(len(ids)))
    return e_batch, e_alone, e_cls


@pytest.mark.parametrize("name", [n for n in TEXT if n in BF16_TOL])
def test_text_geometries_bf16(name):
    c = TEXT[name]
    m, sd = _text_model(c, "bf16")
    try:
        e = _text_errors(m, c, sd)
    finally:
        m._drop_contexts()
    report(f"{name} bf16: padded batch {e[0]:.3e}, one text per call {e[1]:.3e}, CLS-only path {e[2]:.3e}")
    assert max(e) <= BF16_TOL[name]


def test_text_projection_f32():
    c = TEXT["text_d768_e96_f32"]
    m, sd = _text_model(c, "f32")
    try:
        e = _text_errors(m, c, sd)
    finally:
        m._drop_contexts()
    report(f"text_d768_e96_f32 f32: padded batch {e[0]:.3e}, one text per call {e[1]:.3e}, CLS-only path {e[2]:.3e}")
    assert max(e) <= F32_TOL


def test_f32_mode_refuses_dim_256_and_leaves_the_context_usable():
    """The fp32 mode needs linear widths that are multiples of 192 (include/mmpfn_modality.h): a dim-256 model is
    refused there with that message, and the same context then runs the bf16 mode as if nothing had happened."""
    c = TEXT["text_d256_e32"]
    m, sd = _text_model(c, "f32")
    try:
        ids = torch.from_numpy(text_inputs(c)[0][1])[None]
        with pytest.raises(ValueError, match="multiples of 192"):
            m(ids.cuda())
        ctx = next(iter(m._contexts.values()))
        m.precision = "bf16"
        e = _text_errors(m, c, sd)
        assert next(iter(m._contexts.values())) is ctx  # the context that refused
    finally:
        m._drop_contexts()
    assert max(e) <= BF16_TOL["text_d256_e32"]
