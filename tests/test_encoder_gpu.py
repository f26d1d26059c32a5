"""GPU: the two ends of the forward -- input encoders, decoder and ensemble aggregation (csrc/encoder.hip).

* ``enc_stats_kernel`` / ``assemble_kernel`` against the reference's embedded input on the edge fixtures of
  ``tests/golden/encoder`` (pinned on the CPU by ``test_encoder_edges.py``), in the fp32 and the fp16 state, the
  reference's NaN ``ValueError``, every row-count path of the statistics kernel, and the cached (N = 0) assembly;
* ``dec_hidden_kernel`` + ``dec_sum_kernel`` and ``dec_mfma_kernel`` alone, from a read-back state, against the
  decoder in fp64 (the 16-bit form against its own arithmetic in fp64), at query counts around the 16- and
  32-row tiles and n_out = 1, 3, 10;
* ``aggregate_kernel`` against a float64 restatement of the reference's post-processing.

All models have one layer; measured errors go to the run's tail through ``helpers.report``.
"""

import math

import numpy as np
import pytest
import torch

from helpers import oracle_spec, rel_err, report, torch_sd
from oracle.forward import embed_inputs
from test_encoder_edges import ENC, ENC_CASES, load_encoder_case

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4  # logits of the fp32 parity mode (test_parity_gpu.F32_TOL)
EMBED_TOL = 1e-5  # the embedded input in fp32 (test_embedding_and_layer_taps_fp32)
_ENGINES: dict = {}


def _engine(cfg, sd, key):
    """One engine per (config, weights) of this file: the cases of one config run on the same context."""
    from multimodalpfn_amd.engine import HipEngine

    if key not in _ENGINES:
        _ENGINES[key] = HipEngine(cfg, sd, torch.device("cuda"))
    return _ENGINES[key]


def _fixture(case):
    z, meta, cfg, sd = load_encoder_case(case)
    eng = _engine(cfg, sd, ("enc", tuple(sorted(meta["cfg"].items())), meta["wseed"]))
    return z, meta, cfg, sd, eng, torch.from_numpy(z["x"]).cuda(), z["y_train"]


CLEAN = [c for c in ENC_CASES if "logits" in np.load(ENC / f"{c}.npz").files]  # the reference did not raise
RAISING = [c for c in ENC_CASES if c not in CLEAN]

# ------------------------------------------------------------------------------------------------ encoders


@pytest.mark.parametrize("case", CLEAN)
def test_embedding_matches_reference_on_edge_fixtures(case):
    """``embed_state`` against the reference's ``embedded_input``: fp32 state to 1e-5 (rel_err); fp16 state
    (precision 5) per element to half an fp16 ulp of the reference value plus the fp32 bound,
    ``|got - ref| <= 2^-11 |ref| + 1e-5 max(1, max|ref|)``, and finite (``train_const`` / ``one_valid`` reach
    |x| ~ 135); then the fp32 forward's logits against the reference's at 1e-4."""
    z, meta, cfg, sd, eng, x, y = _fixture(case)
    ref = z["embedded_input"].astype(np.float64)
    with torch.inference_mode():
        X0 = eng.embed_state(x, None, y, 0).cpu().numpy()
        X5 = eng.embed_state(x, None, y, 5).cpu().numpy()
        eng.status()
        out = eng.forward(x, None, y, 0).cpu().numpy()
    e0 = rel_err(X0, ref)
    d5 = np.abs(X5.astype(np.float64) - ref)
    lim5 = 2.0 ** -11 * np.abs(ref) + EMBED_TOL * max(1.0, np.abs(ref).max())
    el = rel_err(out, z["logits"])
    report(f"embedding {case}: fp32 rel err {e0:.2e}; fp16 state worst |d| / bound {float((d5 / lim5).max()):.3f} "
           f"(max|ref| {np.abs(ref).max():.1f}); fp32 logits rel err {el:.2e}")
    assert X0.shape == ref.shape and X5.shape == ref.shape
    assert e0 <= EMBED_TOL
    assert np.isfinite(X5).all()
    assert (d5 <= lim5).all(), float((d5 / lim5).max())
    assert el <= F32_TOL
    assert (out.argmax(1) == z["logits"].argmax(1)).all()


@pytest.mark.parametrize("case", RAISING)
def test_reference_nan_error_is_raised_once(case):
    """Where the reference raises "no NaNs in the encoded x and y" (one train row under the outlier step: NaN
    bounds; +inf in a train column: NaN mean), ``forward(check_nan=True)`` raises ``ValueError``; the flag is
    reported once and cleared, so the next, clean forward on the same engine succeeds and matches its fixture."""
    z, meta, cfg, sd, eng, x, y = _fixture(case)
    with torch.inference_mode():
        with pytest.raises(ValueError, match="no NaNs in the encoded x and y"):
            eng.forward(x, None, y, 0, check_nan=True)
        zc, metac, _, _, engc, xc, yc = _fixture("train_const")
        assert engc is eng  # same config and weights
        out = eng.forward(xc, None, yc, 0, check_nan=True).cpu().numpy()
    assert rel_err(out, zc["logits"]) <= F32_TOL


STATS_S = [255, 256, 257, 4096, 4097, 8192, 8193, 16384, 16385]


@pytest.mark.parametrize("S", STATS_S)
def test_stats_kernel_row_count_paths(S):
    """Every path of ``enc_stats_kernel`` by row count, F = 4 (G = 2, T = 3), fp32, N = floor(0.8 S): the
    256-thread stride (255 / 256 / 257), the register form against the generic form (4096 / 4097), the 64 KB LDS
    boundary and the 128 KB opt-in (8192 / 8193), staged columns against global reads (16384 / 16385).  The table has
    2 % NaN, a 1e4 outlier in a train row (N >= 204: the first pass of the two-pass bounds removes it) and NaN in
    the LAST row (the tail thread of the last stride).  Reference: the fp64 oracle on the same device, 1e-5.
    The engine's workspace at S = 16385 is about 1.6 GB (2 S x 64 padded tokens x E floats of attention scratch)."""
    from synth import synth_labels, synth_state_dict, synth_table

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2)
    sd = synth_state_dict(state_dict_spec(cfg), 23)
    eng = _engine(cfg, sd, "stats")
    N = (8 * S) // 10
    xn = synth_table(S, 4, 400 + S, nan_frac=0.02, add_outlier=True)
    xn[S - 1, 0] = np.nan
    assert (xn[:N] == 1e4).any()
    x = torch.from_numpy(xn).cuda()
    yn = synth_labels(S, 3, 400 + S)[:N]
    w = {k: v.cuda() for k, v in torch_sd(sd).items()}
    with torch.inference_mode():
        ref = embed_inputs(oracle_spec(cfg), w, x, None, torch.from_numpy(yn).cuda(), dtype=torch.float64)
        got = eng.embed_state(x, None, yn, 0)
        eng.status()
        err = float((got.double() - ref).abs().max() / max(1.0, float(ref.abs().max())))
    report(f"enc_stats S={S} N={N}: embedding rel err vs fp64 oracle {err:.2e}")
    assert got.shape == ref.shape
    assert err <= EMBED_TOL


@pytest.mark.parametrize("prec", [0, 1, 5])
@pytest.mark.parametrize("case", ["nan_mix", "train_const", "outliers"])
def test_cached_assembly_equals_forward(case, prec):
    """``cache_build`` + ``cache_predict`` (``assemble_kernel`` with N = 0 on the cached slots, label mean and
    uniques) give the test rows of ``forward`` bitwise, as in ``test_train_kv_cache_equals_full_forward``.

    ``train_const`` is the one case where the two differ by definition, in the reference too: its column is constant
    on the train rows only, the cache is fitted on the train rows alone (the reference's cached fit sees only them:
    ``RemoveEmptyFeatures._fit``), so the cached path drops the column that a full forward -- constancy over ALL
    rows -- keeps.  There the cached logits must equal, bitwise, the forward of the table the cached fit stands for
    (that column held at its train value on every row), and differ from the plain forward."""
    z, meta, cfg, sd, eng, x, y = _fixture(case)
    N = meta["N"]
    with torch.inference_mode():
        plain = eng.forward(x, None, y, prec)
        cache = eng.cache_build(x[:N], None, y, prec)
        got = eng.cache_predict(cache, x[N:], None)
        part = eng.cache_predict(cache, x[N:N + 3], None)
        if case == "train_const":
            xc = x.clone()
            assert bool((xc[:N, 1] == xc[0, 1]).all()) and not bool((xc[N:, 1] == xc[0, 1]).all())
            xc[:, 1] = xc[0, 1]
            want = eng.forward(xc, None, y, prec)
            assert not torch.equal(got, plain)
        else:
            want = plain
        eng.status()
        cache.free()
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(part, want[:3])


# ------------------------------------------------------------------------------------------------ decoder

DEC_Q = [1, 15, 16, 17, 31, 32, 33, 100]
DEC_N = 8
DEC_WSEED = 31
DEC_SWAP = {2: 689, 3: 689, 10: 460}  # hidden units (j, j + 1) swapped in the mutation check, per max_num_classes
DEC32_TOL = 2e-5  # plain fp32 fma chains (TOL[2] of test_taps_gpu.py)
# 16-bit decoder against its own arithmetic in fp64: the maximum of rel_err measured on an MI355X over all
# (Q, n_out) of test_decoder_16bit_against_quantising_reference -- bf16 (precision 1) 1.308e-4 at Q = 100, n_out = 10;
# fp16 (precision 5) 5.524e-5 at n_out = 3 -- and the bound, 4 x that
DEC16_MEASURED = {1: 1.31e-4, 5: 5.53e-5}
DEC16_TOL = {p: 4 * m for p, m in DEC16_MEASURED.items()}


def _gelu64(h):
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def _decoder_ref(h, sd, op=None, swap=None):
    """The decoder ``GELU(h W1^T + b1) W2^T + b2`` in fp64.  ``op`` (torch.float16 / torch.bfloat16): the MFMA
    kernel's own arithmetic -- h, W1, W2 rounded to the operand type, the hidden sum exact, exact-erf GELU, G
    rounded to the operand type, the second product exact.  ``swap``: hidden units (swap, swap + 1) of W2
    exchanged (the minimal permutation fault)."""
    q = (lambda t: t.to(op).double()) if op is not None else (lambda t: t.double())
    w = {k: torch.from_numpy(sd["decoder_dict.standard." + k]) for k in ("0.weight", "0.bias", "2.weight", "2.bias")}
    W1, b1, W2, b2 = q(w["0.weight"]), w["0.bias"].double(), q(w["2.weight"]), w["2.bias"].double()
    if swap is not None:
        W2 = W2.clone()
        W2[:, [swap, swap + 1]] = W2[:, [swap + 1, swap]]
    G = _gelu64(q(h) @ W1.T + b1)
    if op is not None:
        G = G.float().to(op).double()
    return G @ W2.T + b2


def _decoder_state(mc, Q, prec):
    """Engine, weights and the state rows the decoder reads: a small table embedded and run through the model's one
    layer (straight after the embedding every test row's target token is the same vector -- NaN label, train mean --
    and a decoder that mixed rows up could not be told from a correct one), read back with ``copy_state``; nothing
    runs between the read-back and ``decode``.  In precision 5 the read-back is exactly the fp16 state."""
    from synth import synth_labels, synth_state_dict, synth_table

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2, max_num_classes=mc)
    sd = synth_state_dict(state_dict_spec(cfg), DEC_WSEED)
    eng = _engine(cfg, sd, ("dec", mc))
    S = DEC_N + Q
    x = torch.from_numpy(synth_table(S, 2, 300 + Q)).cuda()
    y = synth_labels(S, 2, 300 + Q)[:DEC_N]
    eng.embed_state(x, None, y, prec)
    X = eng.run_layers(0, 1)
    eng.status()
    h = X[DEC_N:, -1].cpu()
    assert h.shape == (Q, cfg.emsize) and torch.isfinite(h).all()
    assert len(torch.unique(h, dim=0)) == Q  # distinct rows: a row mix-up shows
    return cfg, sd, eng, h


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("mc", [2, 3, 10])
def test_decoder_fp32_in_isolation(mc, prec):
    """``dec_hidden_kernel`` + ``dec_sum_kernel`` from a read-back state against the decoder in fp64, Q around the
    32-row tile (and the 16-row one), n_out = 1 / 3 / 10: rel_err <= 2e-5."""
    worst = 0.0
    with torch.inference_mode():
        for Q in DEC_Q:
            cfg, sd, eng, h = _decoder_state(mc, Q, prec)
            got = eng.decode(Q).cpu()
            ref = _decoder_ref(h, sd)
            assert got.shape == (Q, cfg.n_out) == ref.shape
            err = rel_err(got.numpy(), ref.numpy())
            worst = max(worst, err)
            assert err <= DEC32_TOL, (Q, err)
    report(f"decoder fp32 prec {prec} n_out {cfg.n_out}: worst rel err vs fp64 {worst:.2e}")


@pytest.mark.parametrize("prec", [1, 5])
@pytest.mark.parametrize("mc", [2, 3, 10])
def test_decoder_16bit_against_quantising_reference(mc, prec):
    """``dec_mfma_kernel`` (precision 1: bf16 operands, the fp32 state rounded by the kernel; precision 5: the fp16
    state and fp16 operands) against the same arithmetic in fp64 (``_decoder_ref`` with ``op``), Q around the
    16-row MFMA tile (the last tile reads clamped rows), n_out = 1 / 3 / 10 (the ``o < n_out`` guard).

    What is left between the two is the fp32 accumulation of the MFMAs, the fp32 GELU and the G values whose
    rounding to the operand type the two sides decide differently.  Measured on an MI355X, the maximum of rel_err
    over all Q per n_out = 1 / 3 / 10: bf16 3.87e-5 / 6.19e-5 / 1.31e-4, fp16 4.70e-5 / 5.52e-5 / 5.47e-5
    (DEC16_MEASURED holds the maximum per precision); the bound is 4 x that, 5.24e-4 (bf16) and 2.21e-4 (fp16).  The
    bound can see a permutation fault of ``pack_mlp2_perm``: exchanging one adjacent pair of W2's hidden units in the
    reference moves it by at least 10 x the bound in every (Q, n_out) case (asserted; the least move is 0.219)."""
    op = torch.bfloat16 if prec == 1 else torch.float16
    worst, least_move = 0.0, math.inf
    with torch.inference_mode():
        for Q in DEC_Q:
            cfg, sd, eng, h = _decoder_state(mc, Q, prec)
            if prec == 5:
                assert torch.equal(h, h.half().float())  # the read-back is the fp16 state itself
            got = eng.decode(Q).cpu()
            ref = _decoder_ref(h, sd, op)
            mut = _decoder_ref(h, sd, op, swap=DEC_SWAP[mc])
            assert got.shape == (Q, cfg.n_out) == ref.shape
            err, move = rel_err(got.numpy(), ref.numpy()), rel_err(mut.numpy(), ref.numpy())
            print(f"decoder prec {prec} n_out {cfg.n_out} Q {Q}: rel err {err:.3e}, pair swap moves the ref {move:.3e}")
            worst, least_move = max(worst, err), min(least_move, move)
            assert err <= DEC16_TOL[prec], (Q, err)
            assert move >= 10 * DEC16_TOL[prec], (Q, move)
    report(f"decoder 16-bit prec {prec} n_out {cfg.n_out}: worst rel err vs quantising fp64 {worst:.3e}; "
           f"least pair-swap move {least_move:.3e} (bound {DEC16_TOL[prec]:.2e})")


# ------------------------------------------------------------------------------------------------ aggregation

# absolute, per probability: fewer than 64 roundings of quantities <= 1; the expf argument error adds <= 0.37 eps
AGG_TOL = 64 * 2.0 ** -24
AGG_N_OUT = 10


def _aggregate_ref(logits, perms, n_cls, temp, avg_before, cw):
    """classifier.py:541-566 in float64."""
    outs = []
    for m in range(logits.shape[0]):
        o = logits[m].double()
        if temp != 1:
            o = o[:, :n_cls] / temp  # cut out the classes that do not exist
        if perms is not None:
            o = o[..., torch.as_tensor(perms[m], dtype=torch.long)]  # undo the member's class permutation
        outs.append(o)
    if avg_before:
        out = torch.softmax(torch.stack(outs).mean(0), dim=1)
    else:
        out = torch.stack([torch.softmax(o, dim=1) for o in outs]).mean(0)
    if cw is not None:
        out = out * torch.as_tensor(cw).double()
        out = out / out.sum(-1, keepdim=True)
    return out


def _aggregate_perms(M, n_cls, g):
    """One class permutation per member, none its own inverse where such exist (n_cls >= 3), so undoing it in the
    wrong direction gives other probabilities; distinct per member where enough exist (n_cls = 10)."""
    if n_cls == 2:
        pool = [[1, 0], [0, 1]]
    elif n_cls == 3:
        pool = [[1, 2, 0], [2, 0, 1]]  # the two 3-cycles: every other permutation of 3 is an involution
    else:
        pool = []
        while len(pool) < M:
            p = torch.randperm(n_cls, generator=g).tolist()
            if p not in pool and [p[c] for c in p] != list(range(n_cls)):
                pool.append(p)
    return [pool[m % len(pool)] for m in range(M)]


def _aggregate_logits(M, Q, n_cls, perms, g):
    """N(0, 3) logits; the first rows (as many as fit) carry entries of +-80 with equal maxima.  Those rows hold
    the same class values in every member (placed through the member's permutation) and only +-80 beyond them,
    so their sums and differences are exact and the bound's premise -- quantities <= 1 -- holds for them too."""
    lg = 3.0 * torch.randn(M, Q, AGG_N_OUT, generator=g)
    special = [
        [80.0, 80.0] + [-80.0] * (n_cls - 2),             # two equal maxima, the rest far below
        [80.0, -80.0] * (n_cls // 2) + [80.0] * (n_cls % 2),  # alternating
        [-80.0] * n_cls,                                   # all equal, all negative
    ]
    for q, row in enumerate(special[: max(0, Q - 1)]):
        for m in range(M):
            lg[m, q, :] = -80.0
            for c in range(n_cls):
                lg[m, q, perms[m][c] if perms is not None else c] = row[c]
    return lg


@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("Q", [1, 127, 128, 129, 300])
def test_aggregate_matches_float64_restatement(M, Q):
    """``eng.aggregate`` over n_cls in {2, 3, 10} of n_out = 10, class permutations (none / one distinct,
    non-symmetric permutation per member, so a wrong direction cannot pass), temperature 1 / 0.9 / 0.25, both
    orders of mean and softmax, class weights: each probability within 64 x 2^-24 of the float64 restatement, rows
    summing to 1 within the same, shape [Q, n_cls] ([Q, n_out] unsliced).  Q around the 128-thread block."""
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2)
    eng = _engine(cfg, synth_state_dict(state_dict_spec(cfg), 23), "stats")
    g = torch.Generator().manual_seed(1000 * M + Q)
    worst, worst_sum, n, where = 0.0, 0.0, 0, None
    for n_cls in (2, 3, 10):
        for with_perms in (False, True):
            perms = _aggregate_perms(M, n_cls, g) if with_perms else None
            lg = _aggregate_logits(M, Q, n_cls, perms, g)
            for temp in (1.0, 0.9, 0.25):
                sliced = temp != 1 or perms is not None
                C = n_cls if sliced else AGG_N_OUT
                for avg_before in (False, True):
                    for with_cw in (False, True):
                        cw = (0.2 + torch.rand(n_cls, generator=g)).numpy() if with_cw else None
                        if with_cw and not sliced and n_cls != AGG_N_OUT:
                            with pytest.raises(RuntimeError):  # the reference's broadcast fails here too
                                eng.aggregate(lg.cuda(), perms, n_cls, temp, avg_before, cw)
                            continue
                        got = eng.aggregate(lg.cuda(), perms, n_cls, temp, avg_before, cw).cpu().double()
                        ref = _aggregate_ref(lg, perms, n_cls, temp, avg_before, cw)
                        assert got.shape == (Q, C) == ref.shape
                        assert torch.isfinite(got).all()
                        err = float((got - ref).abs().max())
                        esum = float((got.sum(1) - 1).abs().max())
                        if err > worst:
                            worst, where = err, (n_cls, with_perms, temp, avg_before, with_cw)
                        worst_sum, n = max(worst_sum, esum), n + 1
                        assert err <= AGG_TOL, (n_cls, with_perms, temp, avg_before, with_cw, err)
                        assert esum <= AGG_TOL, (n_cls, with_perms, temp, avg_before, with_cw, esum)
    report(f"aggregate M={M} Q={Q}: {n} settings, worst |d prob| {worst:.2e} at {where}, worst |row sum - 1| "
           f"{worst_sum:.2e} (bound {AGG_TOL:.2e})")
