"""Host-side handle on one HIP engine context (one per GPU / rank).

Owns the packed device weights (uploaded once through the checkpoint ABI) and
drives the C-ABI entry points on the caller's current HIP stream.  All compute
of the forward runs in ``libmmpfn_hip.so``; this module only moves pointers,
shapes and the few host-side constants the reference also computes on the host:

* the subspace positional-embedding draw ``torch.randn`` from the model's CPU
  generator (``transformer.py:421-424,925-931``) -- bit-exact with the reference's CPU
  forward (see ``pos_rand`` for the GPU stream);
* the sorted unique train labels of the target encoder (``encoders.py:956-958``).
"""

from __future__ import annotations

import ctypes
import itertools
import os

import numpy as np
import torch

from multimodalpfn_amd import _lib
from multimodalpfn_amd.model.spec import CRITERION_PREFIX, ModelConfig, encoder_linear_name


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _count(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.numel()


def model_desc(cfg: ModelConfig) -> _lib.ModelDesc:
    d = _lib.ModelDesc()
    d.emsize = cfg.emsize
    d.nhead = cfg.nhead
    d.nlayers = cfg.nlayers
    d.nhid = cfg.nhid
    d.features_per_group = cfg.features_per_group
    d.encoder_features = cfg.encoder_features
    d.n_out = cfg.n_out
    d.mixer_type = _lib.MIXER_CODES[cfg.mixer_type]
    d.mgm_heads = cfg.mgm_heads
    d.cap_heads = cfg.cap_heads
    d.two_sets_of_queries = int(cfg.two_sets_of_queries)
    d.remove_duplicate_features = int(cfg.remove_duplicate_features)
    d.ln_eps = cfg.ln_eps
    d.outlier_sigma = float(cfg.remove_outliers_sigma) if cfg.remove_outliers_sigma else 0.0
    d.target_kind = _lib.TARGET_VALUE if cfg.is_regression else _lib.TARGET_CLASS
    return d


POS_RNG = os.environ.get("MMPFN_POS_RNG", "cpu")  # "cpu" (default) or "device"


def pos_rand(cfg: ModelConfig, n_tokens: int, device: torch.device | None = None) -> torch.Tensor:
    """``randn((n_tokens, E//4))`` from a fresh generator seeded like ``_init_rnd`` (transformer.py:421-424).

    The reference draws on the generator of the device its input lives on (:887-892): on a CPU
    forward that is the CPU Mersenne-Twister stream, which is what the goldens pin, and the engine
    reproduces it bit for bit.  On a GPU the reference draws from that GPU's Philox generator in the
    autocast dtype of its embedded input; that stream depends on the device's grid geometry and dtype,
    so it is not a fixed target.  ``MMPFN_POS_RNG=device`` draws from a generator on ``device`` (fp32)
    instead -- the reference's GPU behaviour in kind, parity unpinned.
    """
    gdev = device if (POS_RNG == "device" and device is not None) else torch.device("cpu")
    gen = torch.Generator(device=gdev)
    if cfg.model_seed:  # `if self.seed:` (transformer.py:423)
        gen.manual_seed(cfg.model_seed)
    return torch.randn((n_tokens, cfg.emsize // 4), generator=gen, dtype=torch.float32, device=gdev)


def target_uniques(y_train: np.ndarray) -> np.ndarray:
    """Sorted unique train targets after the y NaN fill (encoders.py:461-493,954-958)."""
    y = np.asarray(y_train, dtype=np.float32)
    nan = np.isnan(y)
    if nan.any():
        # the fill must be the value the device fills with (enc_stats_kernel's label block): the float64 sum
        # over the count, rounded to float32 once.  A float32 np.nanmean can land one ulp below it; the filled
        # rows then compare greater than their own entry here and every NaN-label row (every test row) codes
        # one class too high.  (A float64 sum of float32 labels is exact, so the same in any order, as long as
        # their count times their dynamic range stays below 2^29.)
        ok = y[~nan].astype(np.float64)
        with np.errstate(invalid="ignore"):
            fill = np.float32(ok.sum() / np.float64(ok.size))
        y = np.where(nan, fill, y)
    return np.unique(y).astype(np.float32)


# Lane streams are process-wide (one per device and lane index), shared by every engine: each HIP stream is bound to
# one of the device's few hardware queues (GPU_MAX_HW_QUEUES), and two lanes that land on the same queue run one after
# the other.  Which pool streams share a queue is not under the caller's control -- per-engine streams gave every second
# MMPFNClassifier of a process 15.0-15.9 instead of 13.6-13.8 ms per predict at config C -- so the first pair, made
# together at the first lanes' use, serves all engines (13.5-13.8 ms for all four classifiers of the same test;
# profiles/r06/api_lane_streams.txt; CU-masked streams 17-24 ms, a high-priority second lane 14.0-14.8 ms).
_LANE_STREAMS: dict = {}


def _lane_stream(device: torch.device, k: int) -> torch.cuda.Stream:
    key = (str(device), k)
    st = _LANE_STREAMS.get(key)
    if st is None:
        st = _LANE_STREAMS[key] = torch.cuda.Stream(device)
    return st


DEFAULT_LANES = int(os.environ.get("MMPFN_LANES", "2"))  # concurrent member lanes of forward_many
DEFAULT_BATCH = int(os.environ.get("MMPFN_BATCH", "1"))  # members per batched forward of forward_many (1: DESIGN 7)
# 1: the forwards run their last layer in full instead of pruned to the rows the decoder reads (the
# same logits bit for bit -- the pruned form's reference and A/B handle)
DEFAULT_FULL_LAST_LAYER = os.environ.get("MMPFN_FULL_LAST_LAYER") == "1"
_SERIAL = itertools.count(1)  # engine serial numbers: cache tags that a freed engine's id() could alias


class HipEngine:
    """One ``mmpfn_ctx`` bound to a CUDA(HIP) device."""

    def __init__(self, cfg: ModelConfig, state_dict: dict, device: torch.device):
        if not torch.cuda.is_available():
            raise RuntimeError("the MMPFN HIP engine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = _lib.load_library()
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"HipEngine needs a cuda device, got {self.device}")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.ctx = self.lib.mmpfn_create(idx, ctypes.c_void_p(self._stream()))
        if not self.ctx:
            raise _lib.EngineError(f"mmpfn_create failed on device {idx}")
        self.desc = model_desc(cfg)
        self._check(self.lib.mmpfn_set_model(self.ctx, ctypes.byref(self.desc)), "mmpfn_set_model")
        names = set()
        for name, t in state_dict.items():
            if name.startswith(CRITERION_PREFIX):  # the bar distribution's buffers stay on the host
                continue
            if isinstance(t, torch.Tensor):
                a = t.detach().to("cpu", torch.float32).contiguous().numpy()
            else:
                a = np.ascontiguousarray(t, dtype=np.float32)
            self._check(
                self.lib.mmpfn_load_weight(self.ctx, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size),
                f"mmpfn_load_weight({name})",
            )
            names.add(name)
        if encoder_linear_name(cfg) not in names:
            raise _lib.EngineError(f"state_dict lacks {encoder_linear_name(cfg)}")
        self._check(self.lib.mmpfn_finalize_weights(self.ctx), "mmpfn_finalize_weights")
        self._pos_cache: dict[int, torch.Tensor] = {}
        self._streams: list = []
        self.lanes = DEFAULT_LANES
        self.batch = DEFAULT_BATCH
        self.full_last_layer = DEFAULT_FULL_LAST_LAYER
        self.refs = 1  # model copies holding this engine (PerFeatureTransformer.__deepcopy__ shares it)
        self.serial = next(_SERIAL)

    # ------------------------------------------------------------------ plumbing
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc: int, what: str) -> None:
        _lib.check(self.lib, self.ctx, rc, what)

    def _bind_stream(self) -> None:
        self._check(self.lib.mmpfn_set_stream(self.ctx, ctypes.c_void_p(self._stream())), "mmpfn_set_stream")

    @property
    def full_last_layer(self) -> bool:
        """Whether ``forward`` / ``forward_batch`` / ``cache_build`` / ``cache_predict`` run the last layer in full
        (``mmpfn_set_full_last_layer``).  Off by default: they compute only the target token's test rows there."""
        return self._full_last_layer

    @full_last_layer.setter
    def full_last_layer(self, on: bool) -> None:
        self._check(self.lib.mmpfn_set_full_last_layer(self.ctx, int(bool(on))), "mmpfn_set_full_last_layer")
        self._full_last_layer = bool(on)

    def release(self) -> None:
        """Drop one holder's reference; the context is destroyed with the last one."""
        self.refs -= 1
        if self.refs <= 0:
            self.close()

    def close(self) -> None:
        if getattr(self, "ctx", None):
            self.lib.mmpfn_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def _dev(self, t, dtype=torch.float32) -> torch.Tensor:
        """To the engine device on the current stream.  Host data goes through pinned memory without a
        host wait: a pageable host-to-device copy blocks the host until the stream has drained up to it,
        so every launch after it would trail the GPU (the predict path's per-member labels, the
        all-gather's member order and the aggregation's class permutations left ~0.5 ms of idle GPU
        per step that way)."""
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if t.device.type == "cpu" and self.device.type == "cuda":
            return t.to(dtype).contiguous().pin_memory().to(self.device, non_blocking=True)
        return t.to(self.device, dtype).contiguous()

    def _pos(self, n: int) -> torch.Tensor:
        if n not in self._pos_cache:
            t = pos_rand(self.cfg, n, self.device).to(self.device)
            # drawn / copied on whichever stream (lane) asked first, read later from every lane: wait for
            # it here once, so no lane can read the cached table before it is complete
            torch.cuda.current_stream(self.device).synchronize()
            self._pos_cache[n] = t
        return self._pos_cache[n]

    # ------------------------------------------------------------------ compute
    def mixer_tokens(self, image, precision: int) -> torch.Tensor:
        """Modality projection heads: ``[S, n_mod, D]`` -> ``[S, C, E]`` tokens."""
        img = self._dev(image)
        if img.dim() == 2:
            img = img.unsqueeze(1)
        S, n_mod, D = img.shape
        if D != self.cfg.mixer_in_dim:
            raise ValueError(f"image embedding width {D} != {self.cfg.mixer_in_dim}")
        C = self.lib.mmpfn_mixer_tokens(self.ctx, n_mod)
        out = torch.empty((S, C, self.cfg.emsize), device=self.device, dtype=torch.float32)
        self._bind_stream()
        self._check(
            self.lib.mmpfn_mixer_forward(self.ctx, _ptr(img), S, n_mod, _ptr(out), precision), "mmpfn_mixer_forward"
        )
        return out

    def _prepare(self, x, tokens, y_train):
        y_np = y_train.detach().float().cpu().numpy() if isinstance(y_train, torch.Tensor) else np.asarray(y_train)
        y_np = y_np.reshape(-1).astype(np.float32)
        N = y_np.shape[0]
        xd = None if x is None else self._dev(x)
        if xd is not None and xd.dim() == 3:  # [S, 1, F] seam layout
            xd = xd.reshape(xd.shape[0], xd.shape[-1])
        td = None if tokens is None else self._dev(tokens)
        S = xd.shape[0] if xd is not None else td.shape[0]
        F = xd.shape[1] if xd is not None else 0
        C = td.shape[1] if td is not None else 0
        if td is not None and td.shape[0] != S:
            raise ValueError(f"tokens rows {td.shape[0]} != table rows {S}")
        fpg = self.cfg.features_per_group
        G = (F + fpg - 1) // fpg if xd is not None else 0
        # a value target has no class codes: nothing to compute or upload (the engine ignores uniq / U)
        uniq = None if self.cfg.is_regression else self._dev(torch.from_numpy(target_uniques(y_np)))
        yd = self._dev(torch.from_numpy(y_np))
        return xd, td, yd, uniq, S, F, C, N, G

    # ``embeddings=`` of the forward entry points -> (train rows' wanted, test rows' wanted)
    EMBEDDINGS = {"test": (False, True), "train": (True, False), "both": (True, True)}

    @classmethod
    def _check_embeddings(cls, embeddings) -> None:
        if embeddings is not None and embeddings not in cls.EMBEDDINGS:
            raise ValueError(f"embeddings must be None or one of {sorted(cls.EMBEDDINGS)}, got {embeddings!r}")

    def _embedding_outputs(self, embeddings: str, lead: tuple, N: int, Q: int):
        """The row-embedding outputs ``embeddings`` asks for, fp32 ``[*lead, N, E]`` / ``[*lead, Q, E]`` or None."""
        self._check_embeddings(embeddings)
        want_train, want_test = self.EMBEDDINGS[embeddings]
        E = self.cfg.emsize
        tr = torch.empty(lead + (N, E), device=self.device, dtype=torch.float32) if want_train else None
        te = torch.empty(lead + (Q, E), device=self.device, dtype=torch.float32) if want_test else None
        return tr, te

    def forward(self, x, tokens, y_train, precision: int, check_nan: bool = True, embeddings: str | None = None):
        """One ensemble member: logits ``[S - N, n_out]`` (fp32, on the engine device).

        ``embeddings``: ``"test"``, ``"train"`` or ``"both"`` returns ``(logits, train_emb, test_emb)`` instead
        (``mmpfn_forward_embed``): the target token's final state of the train rows ``[N, E]`` and of the test rows
        ``[S - N, E]``, fp32, the one not asked for None (the reference's ``train_embeddings`` / ``test_embeddings``,
        transformer.py:850-864).  The logits are those of the plain call bit for bit."""
        self._check_embeddings(embeddings)
        xd, td, yd, uniq, S, F, C, N, G = self._prepare(x, tokens, y_train)
        if N < 1 or N > S:
            raise ValueError(f"single_eval_pos must be in [1, {S}], got {N}")
        pr = self._pos(G + C)
        out = torch.empty((S - N, self.cfg.n_out), device=self.device, dtype=torch.float32)
        if embeddings is not None:
            tr, te = self._embedding_outputs(embeddings, (), N, S - N)
            self._bind_stream()
            if _count(out) or _count(tr) or _count(te):  # (an output of no rows has no address: it is not asked for)
                self._check(
                    self.lib.mmpfn_forward_embed(
                        self.ctx, _ptr(xd), S, F, _ptr(td), C, _ptr(yd), N, _ptr(uniq), _count(uniq), _ptr(pr),
                        _ptr(out) or None, _ptr(tr) or None, _ptr(te) or None, precision,
                    ),
                    "mmpfn_forward_embed",
                )
            if check_nan:
                self.status()
            return out, tr, te
        self._bind_stream()
        self._check(
            self.lib.mmpfn_forward(
                self.ctx, _ptr(xd), S, F, _ptr(td), C, _ptr(yd), N, _ptr(uniq), _count(uniq), _ptr(pr), _ptr(out),
                precision,
            ),
            "mmpfn_forward",
        )
        if check_nan:
            self.status()
        return out

    # ------------------------------------------------------------------ train-KV cache
    def cache_build(self, x, tokens, y_train, precision: int) -> "TrainCache":
        """``fit_mode="fit_with_cache"``: forward the train rows once and keep, per layer, head 0's
        K/V of the train rows plus the encoders' train statistics (``mmpfn_cache_build``;
        reference ``InferenceEngineCacheKV.prepare``, inference.py:403-445)."""
        xd, td, yd, uniq, S, F, C, N, G = self._prepare(x, tokens, y_train)
        if N != S:
            raise ValueError(f"cache_build takes the train rows only: {S} rows, {N} labels")
        pr = self._pos(G + C)
        h = ctypes.c_void_p()
        self._bind_stream()
        self._check(
            self.lib.mmpfn_cache_build(self.ctx, _ptr(xd), N, F, _ptr(td), C, _ptr(yd), _ptr(uniq), _count(uniq),
                                       _ptr(pr), precision, ctypes.byref(h)),
            "mmpfn_cache_build",
        )
        return TrainCache(self, h.value, N=N, F=F, C=C, precision=precision)

    def cache_predict(self, cache: "TrainCache", x, tokens, embeddings: str | None = None):
        """Test rows against a train-KV cache: logits ``[Q, n_out]`` (``mmpfn_cache_predict``;
        reference ``InferenceEngineCacheKV.iter_outputs``, inference.py:470-512).  ``embeddings="test"``:
        ``(logits, None, test_emb [Q, E])`` as ``forward`` returns them (``mmpfn_cache_predict_embed``); a cache
        holds no train rows' embeddings."""
        if cache.engine is not self or not cache.handle:
            raise ValueError("the cache belongs to another engine or was freed")
        if embeddings is not None and embeddings != "test":
            if embeddings in self.EMBEDDINGS:
                raise ValueError(f"a train-KV cache serves embeddings='test' only, got {embeddings!r}")
            raise ValueError(f"embeddings must be None or 'test', got {embeddings!r}")
        xd = None if x is None else self._dev(x)
        if xd is not None and xd.dim() == 3:
            xd = xd.reshape(xd.shape[0], xd.shape[-1])
        td = None if tokens is None else self._dev(tokens)
        Q = xd.shape[0] if xd is not None else td.shape[0]
        F = xd.shape[1] if xd is not None else 0
        C = td.shape[1] if td is not None else 0
        if (F, C) != (cache.F, cache.C):
            raise ValueError(f"test rows have F={F}, C={C}; the cache was built with F={cache.F}, C={cache.C}")
        out = torch.empty((Q, self.cfg.n_out), device=self.device, dtype=torch.float32)
        self._S = Q  # copy_state's row count: every row of a cache predict's state is a test row
        self._bind_stream()
        if embeddings is not None:
            _, te = self._embedding_outputs(embeddings, (), 0, Q)
            if _count(out) or _count(te):  # (an output of no rows has no address: it is not asked for)
                self._check(
                    self.lib.mmpfn_cache_predict_embed(self.ctx, ctypes.c_void_p(cache.handle), _ptr(xd), Q, F,
                                                       _ptr(td), C, _ptr(out) or None, _ptr(te) or None),
                    "mmpfn_cache_predict_embed",
                )
            return out, None, te
        self._check(
            self.lib.mmpfn_cache_predict(self.ctx, ctypes.c_void_p(cache.handle), _ptr(xd), Q, F, _ptr(td), C,
                                         _ptr(out)),
            "mmpfn_cache_predict",
        )
        return out

    def cache_predict_many(self, caches, xs, tokens, lanes: int | None = None, embeddings: str | None = None) -> list:
        """``cache_predict`` of several members, spread over concurrent lanes like ``forward_many``
        (2 lanes: 4.5 ms vs 6.7 ms for 4 members' 460 test rows; 4 lanes measured no better).  ``embeddings``: as
        ``cache_predict`` takes it, every member's result then its tuple."""
        n = len(caches)
        lanes = max(1, min(int(self.lanes if lanes is None else lanes), n, _lib.MMPFN_MAX_LANES))
        kw = {} if embeddings is None else {"embeddings": embeddings}
        if lanes == 1:
            return [self.cache_predict(c, x, tokens, **kw) for c, x in zip(caches, xs)]
        main = torch.cuda.current_stream(self.device)
        streams = self._lane_streams(lanes)
        for st in streams:
            st.wait_stream(main)
        outs = []
        try:
            for k, (c, x) in enumerate(zip(caches, xs)):
                with torch.cuda.stream(streams[k % lanes]):
                    self._check(self.lib.mmpfn_select_lane(self.ctx, k % lanes), "mmpfn_select_lane")
                    outs.append(self.cache_predict(c, x, tokens, **kw))
        finally:
            self._check(self.lib.mmpfn_select_lane(self.ctx, 0), "mmpfn_select_lane")
            for st in streams:
                main.wait_stream(st)
        for o in outs:
            for t in (o if isinstance(o, tuple) else (o,)):
                if t is not None:
                    t.record_stream(main)
        return outs

    def forward_batch(self, items, precision: int, embeddings: str | None = None) -> list:
        """Members of ONE geometry (same S, N, F and tokens) in one batched forward
        (``mmpfn_forward_batch``: every layer kernel runs once over all members).  ``embeddings``: as ``forward``
        takes it, every member's result then its ``(logits, train_emb, test_emb)``
        (``mmpfn_forward_batch_embed``)."""
        self._check_embeddings(embeddings)
        prep = [self._prepare(x, t, y) for x, t, y in items]
        M = len(prep)
        xd0, td, _, _, S, F, C, N, G = prep[0]
        for p in prep[1:]:
            if (p[4], p[5], p[6], p[7]) != (S, F, C, N):
                raise ValueError("forward_batch members must share S, F, C and N")
        if N < 1 or N > S:
            raise ValueError(f"single_eval_pos must be in [1, {S}], got {N}")
        pr = self._pos(G + C)
        out = torch.empty((M, S - N, self.cfg.n_out), device=self.device, dtype=torch.float32)
        arr = ctypes.c_void_p * M
        xs = arr(*[_ptr(p[0]) for p in prep]) if F > 0 else None
        ys = arr(*[_ptr(p[2]) for p in prep])
        us = arr(*[_ptr(p[3]) for p in prep])
        ns = (ctypes.c_int * M)(*[_count(p[3]) for p in prep])
        self._bind_stream()
        if embeddings is not None:
            tr, te = self._embedding_outputs(embeddings, (M,), N, S - N)
            if _count(out) or _count(tr) or _count(te):
                self._check(
                    self.lib.mmpfn_forward_batch_embed(self.ctx, M, xs, S, F, _ptr(td), C, ys, N, us, ns, _ptr(pr),
                                                       _ptr(out) or None, _ptr(tr) or None, _ptr(te) or None,
                                                       precision),
                    "mmpfn_forward_batch_embed",
                )
            none = [None] * M
            return list(zip(out.unbind(0), none if tr is None else tr.unbind(0), none if te is None else te.unbind(0)))
        self._check(
            self.lib.mmpfn_forward_batch(self.ctx, M, xs, S, F, _ptr(td), C, ys, N, us, ns, _ptr(pr), _ptr(out),
                                         precision),
            "mmpfn_forward_batch",
        )
        return list(out.unbind(0))

    def forward_many(self, items, precision: int, lanes: int | None = None,
                     batch: int | None = None, embeddings: str | None = None) -> list:
        """Independent ensemble members ``[(x, tokens, y_train), ...]`` -> logits list.

        Members are spread over ``lanes`` forward lanes (per-member workspaces of the same
        context), each on its own HIP stream, so one member's kernels fill the tails and
        latency gaps of another's; members of one geometry are stacked ``batch`` at a time
        into one batched forward.  ``items`` may be a generator: a unit is launched as soon as
        its members have arrived, so the caller's host work for later members (the per-member
        preprocessing of a predict) overlaps the GPU work of earlier ones.  The caller's stream
        waits for all of them.  The reference runs its members one after another
        (inference.py:294-349); the results do not depend on lanes or batching.  ``embeddings``: as ``forward``
        takes it, every member's result then its ``(logits, train_emb, test_emb)``.
        """
        self._check_embeddings(embeddings)
        kw = {} if embeddings is None else {"embeddings": embeddings}
        batch = max(1, int(self.batch if batch is None else batch))
        if isinstance(items, (list, tuple)):
            n_units = len({self._geometry(*it) for it in items})  # lower bound on the unit count
            n_units = max(n_units, -(-len(items) // batch))
        else:
            n_units = _lib.MMPFN_MAX_LANES
        lanes = max(1, min(int(self.lanes if lanes is None else lanes), n_units, _lib.MMPFN_MAX_LANES))
        outs: dict = {}
        store: dict[int, tuple] = {}

        def run(unit, stream=None):
            if len(unit) == 1:
                x, t, y = store[unit[0]]
                outs[unit[0]] = self.forward(x, t, y, precision, check_nan=False, **kw)
            else:
                for i, o in zip(unit, self.forward_batch([store[i] for i in unit], precision, **kw)):
                    outs[i] = o
            if stream is not None:
                # the unit's device inputs were made on the caller's stream (e.g. each member's
                # torch.cat of train and test rows): keep their blocks from being reused before the
                # lane's kernels have read them
                for i in unit:
                    for t in store[i]:
                        if isinstance(t, torch.Tensor) and t.is_cuda:
                            t.record_stream(stream)
            for i in unit:
                del store[i]

        main = torch.cuda.current_stream(self.device)
        streams = self._lane_streams(lanes) if lanes > 1 else [main]
        if lanes > 1:
            for st in streams:
                st.wait_stream(main)
        launched = 0

        def launch(unit):
            nonlocal launched
            if lanes == 1:
                run(unit)
            else:
                k = launched % lanes
                # the unit's inputs may have been produced on the caller's stream after the lanes forked
                # (a generator builds each member just before its unit launches): order the lane behind it
                streams[k].wait_stream(main)
                with torch.cuda.stream(streams[k]):
                    self._check(self.lib.mmpfn_select_lane(self.ctx, k), "mmpfn_select_lane")
                    run(unit, streams[k])
            launched += 1

        pending: dict = {}  # geometry -> member indices waiting for a full unit
        n = 0
        try:
            for i, it in enumerate(items):
                n = i + 1
                store[i] = it
                g = self._geometry(*it)
                pending.setdefault(g, []).append(i)
                if len(pending[g]) == batch:
                    launch(pending.pop(g))
            for unit in sorted(pending.values(), key=lambda u: u[0]):
                launch(unit)
        finally:
            if lanes > 1:
                self._check(self.lib.mmpfn_select_lane(self.ctx, 0), "mmpfn_select_lane")
                for st in streams:
                    main.wait_stream(st)
        result = [outs[i] for i in range(n)]
        if lanes > 1:
            for o in result:  # allocated on a lane stream, consumed on the caller's
                for t in (o if isinstance(o, tuple) else (o,)):
                    if t is not None:
                        t.record_stream(main)
        return result

    def _geometry(self, x, tokens, y_train) -> tuple:
        S = (x.shape[0] if x is not None else tokens.shape[0])
        F = 0 if x is None else x.shape[-1]
        C = 0 if tokens is None else tokens.shape[1]
        N = int(np.asarray(y_train.shape if isinstance(y_train, torch.Tensor) else np.shape(y_train)).prod())
        return (S, F, C, N, None if tokens is None else tokens.data_ptr())

    def _lane_streams(self, n: int) -> list:
        if len(self._streams) < n:
            self._streams += [_lane_stream(self.device, len(self._streams) + i) for i in range(n - len(self._streams))]
        return self._streams[:n]

    def aggregate(self, logits: torch.Tensor, perms, n_classes: int, temperature: float,
                  average_before_softmax: bool, class_weights=None) -> torch.Tensor:
        """Ensemble post-processing of classifier.py:541-566 on the device."""
        lg = logits.to(self.device, torch.float32).contiguous()
        M, Q, n_out = lg.shape
        pd = None
        if perms is not None:
            pd = self._dev(torch.as_tensor(np.asarray(perms, dtype=np.int32).reshape(M, n_classes)), torch.int32)
        C = n_classes if (temperature != 1 or perms is not None) else n_out
        cw = None
        if class_weights is not None:
            cw = self._dev(class_weights).reshape(-1)
            if cw.numel() != C:  # the reference's `output * class_prob_in_train` fails on this broadcast too
                raise RuntimeError(
                    f"The size of tensor a ({C}) must match the size of tensor b ({cw.numel()}) at non-singleton "
                    "dimension 1 (balance_probabilities with softmax_temperature == 1 and no class permutation)")
        out = torch.empty((Q, C), device=self.device, dtype=torch.float32)
        self._bind_stream()
        self._check(
            self.lib.mmpfn_aggregate(self.ctx, _ptr(lg), M, Q, n_out, _ptr(pd), n_classes, float(temperature),
                                     int(average_before_softmax), _ptr(cw), _ptr(out)),
            "mmpfn_aggregate",
        )
        return out

    SCORE_KINDS = ("nll", "cdf", "pi", "ei", "mean_of_square")  # mmpfn_bar_score's outputs; the last one is per row

    def _score_tables(self, tables: dict, B: int, keys) -> dict:
        tabs = {k: self._dev(tables[k]).reshape(-1) for k in keys}
        sizes = {"borders": B + 1, "ends": _lib.BAR_SCORE_ENDS}
        if any(t.numel() != sizes.get(k, B) for k, t in tabs.items()):
            raise ValueError(f"score tables do not fit {B} bars")
        return tabs

    def _score_buffers(self, ys, Q: int, B: int, want) -> tuple:
        """Device targets ``[Q, J]`` (``[Q]`` is one target per row) and one output tensor per wanted kind."""
        unknown = set(want) - set(self.SCORE_KINDS)
        if unknown:
            raise ValueError(f"unknown score kinds {sorted(unknown)}")
        if not 2 <= B <= _lib.BAR_MAX_BARS:
            raise ValueError(f"mmpfn_bar_score holds 2..{_lib.BAR_MAX_BARS} bars; got {B}")
        per_target = [k for k in want if k != "mean_of_square"]
        yd, J = None, 0
        if ys is not None:
            yd = self._dev(ys)
            yd = (yd[:, None] if yd.dim() == 1 else yd).contiguous()
            if yd.dim() != 2 or yd.shape[0] != Q:
                raise ValueError(f"targets [{Q}] or [{Q}, J] expected, got {tuple(yd.shape)}")
            J = yd.shape[1]
            if not 1 <= J <= _lib.BAR_MAX_TARGETS:
                raise ValueError(f"mmpfn_bar_score holds 1..{_lib.BAR_MAX_TARGETS} targets per row; got {J}")
        elif per_target:
            raise ValueError(f"{per_target} need targets")
        out = {k: torch.empty((Q,) if k == "mean_of_square" else (Q, J), device=self.device, dtype=torch.float32)
               for k in want}
        return yd, J, out

    def bar_score(self, logits: torch.Tensor, criterion_tables: dict, ys, *, softmax_temperature: float = 1.0,
                  want=SCORE_KINDS) -> dict:
        """Scores of the bar distributions ``softmax(logits / softmax_temperature)`` ``[Q, B]`` at the targets ``ys``
        ``[Q, J]`` (or ``[Q]``; ``None`` when only ``mean_of_square`` is wanted) on the device (``mmpfn_bar_score``).
        ``criterion_tables``: ``FullSupportBarDistribution.head_tables()`` and ``.score_tables()`` in one dict.
        Returns device tensors, the kinds in ``want``: ``nll`` / ``cdf`` / ``pi`` / ``ei`` ``[Q, J]`` (the target as
        ``best_f``), ``mean_of_square`` ``[Q]``."""
        lg = logits.to(self.device, torch.float32).contiguous()
        Q, B = lg.shape
        if not softmax_temperature > 0:
            raise ValueError(f"softmax_temperature must be > 0, got {softmax_temperature}")
        yd, J, out = self._score_buffers(ys, Q, B, want)
        t = self._score_tables(criterion_tables, B, ("borders", "widths", "log_widths", "mean_squares", "ei_mids", "ends"))
        self._bind_stream()
        self._check(
            self.lib.mmpfn_bar_score(self.ctx, _ptr(lg), Q, B, 1.0 / float(softmax_temperature), _ptr(t["borders"]),
                                     _ptr(t["widths"]), _ptr(t["log_widths"]), _ptr(t["mean_squares"]),
                                     _ptr(t["ei_mids"]), _ptr(t["ends"]), _ptr(yd), J,
                                     *(_ptr(out.get(k)) for k in self.SCORE_KINDS)),
            "mmpfn_bar_score",
        )
        return out

    SAMPLE_TAILS = {"linear": 0, "halfnormal": 1}  # mmpfn_bar_sample's tails

    def bar_sample(self, logits: torch.Tensor, criterion_tables: dict, n: int, *, seed: int = 0, first_draw: int = 0,
                   uniforms=None, temperature: float = 1.0, tails: str = "linear", return_uniforms: bool = False):
        """``n`` draws per row from the bar distributions ``softmax(logits / temperature)`` ``[Q, B]`` on the device
        (``mmpfn_bar_sample``): a device tensor ``[Q, n]``, with ``return_uniforms`` also the levels used ``[Q, n]``.
        ``criterion_tables`` as ``bar_score`` takes them (``borders``, and ``ends`` for the half-normal tails).
        Draw ``j`` of the call is draw ``first_draw + j`` of its row and depends on ``(seed, row, first_draw + j)``
        alone, so a row's draws may be split over calls; ``uniforms`` ``[Q, n]`` supplies the levels instead.
        ``tails``: ``"linear"`` (the reference's ``sample``) or ``"halfnormal"`` (the end buckets as the density
        ``bar_score``'s ``nll`` scores has them)."""
        lg = logits.to(self.device, torch.float32).contiguous()
        Q, B = lg.shape
        n = int(n)
        if not 2 <= B <= _lib.BAR_MAX_BARS:
            raise ValueError(f"mmpfn_bar_sample holds 2..{_lib.BAR_MAX_BARS} bars; got {B}")
        if not 0 <= n <= _lib.BAR_MAX_DRAWS:
            raise ValueError(f"mmpfn_bar_sample holds 0..{_lib.BAR_MAX_DRAWS} draws per row; got {n}")
        if not temperature > 0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        if tails not in self.SAMPLE_TAILS:
            raise ValueError(f"tails must be one of {sorted(self.SAMPLE_TAILS)}, got {tails!r}")
        if not (0 <= int(seed) < 2 ** 64 and 0 <= int(first_draw) < 2 ** 64):
            raise ValueError("seed and first_draw are unsigned 64-bit numbers")
        t = self._score_tables(criterion_tables, B, ("borders", "ends") if tails == "halfnormal" else ("borders",))
        ud = None
        if uniforms is not None:
            ud = self._dev(uniforms).contiguous()
            if tuple(ud.shape) != (Q, n):
                raise ValueError(f"uniforms [{Q}, {n}] expected, got {tuple(ud.shape)}")
        out = torch.empty((Q, n), device=self.device, dtype=torch.float32)
        u_out = torch.empty((Q, n), device=self.device, dtype=torch.float32) if return_uniforms else None
        if Q == 0 or n == 0:  # nothing to launch, and an empty tensor has no address to pass
            return (out, u_out) if return_uniforms else out
        self._bind_stream()
        self._check(
            self.lib.mmpfn_bar_sample(self.ctx, _ptr(lg), Q, B, 1.0 / float(temperature), _ptr(t["borders"]),
                                      _ptr(t.get("ends")), self.SAMPLE_TAILS[tails], _ptr(ud), int(seed),
                                      int(first_draw), n, _ptr(out), _ptr(u_out)),
            "mmpfn_bar_sample",
        )
        return (out, u_out) if return_uniforms else out

    def bar_head(self, logits: torch.Tensor, idx, share, criterion: dict, *, cancel=None,
                 softmax_temperature: float = 1.0, average_before_softmax: bool = False, quantiles=(),
                 want_logits: bool = False, targets=None, score_tables: dict | None = None) -> dict:
        """Regression post-processing of regressor.py:652-765 on the device (``mmpfn_bar_head``).

        ``logits`` ``[M, Q, B]``; ``idx`` / ``share`` ``[M, B + 1]`` from ``bar_distribution.border_tables``;
        ``cancel`` ``[M, B]`` bool or ``None``; ``criterion``: ``FullSupportBarDistribution.head_tables()`` of the
        renormalised criterion.  Returns device tensors ``mean`` / ``mode`` ``[Q]``, ``quantiles`` ``[K, Q]`` and
        ``logits`` ``[Q, B]`` (``None`` unless ``want_logits``).  With ``targets`` ``[Q, J]`` (or ``[Q]``) and
        ``score_tables`` (``FullSupportBarDistribution.score_tables()``) the same kernel scores every finished row
        (``mmpfn_bar_head_score``) and ``bar_score``'s keys come back as well."""
        lg = logits.to(self.device, torch.float32).contiguous()
        M, Q, B = lg.shape
        if B > _lib.BAR_MAX_BARS or M > _lib.BAR_MAX_MEMBERS or len(quantiles) > _lib.BAR_MAX_LEVELS or B < 1 or M < 1:
            raise ValueError(f"mmpfn_bar_head holds 1..{_lib.BAR_MAX_BARS} bars, 1..{_lib.BAR_MAX_MEMBERS} members and "
                             f"{_lib.BAR_MAX_LEVELS} levels; got {B}, {M}, {len(quantiles)}")
        if not softmax_temperature > 0:
            raise ValueError(f"softmax_temperature must be > 0, got {softmax_temperature}")
        # rows padded to a multiple of 4 entries: the kernel then reads them in 16-byte (tables) / 4-byte (mask) pieces
        ldt, ldc = (B + 4) & ~3, (B + 3) & ~3
        ix_h = np.full((M, ldt), -2, dtype=np.int32)
        ix_h[:, :B + 1] = np.asarray(idx, dtype=np.int32).reshape(M, B + 1)
        sh_h = np.zeros((M, ldt), dtype=np.float32)
        sh_h[:, :B + 1] = np.asarray(share, dtype=np.float32).reshape(M, B + 1)
        ix, sh, cm = self._dev(ix_h, torch.int32), self._dev(sh_h), None
        if cancel is not None:
            cm_h = np.zeros((M, ldc), dtype=np.uint8)
            cm_h[:, :B] = np.asarray(cancel, dtype=np.uint8).reshape(M, B)
            cm = self._dev(cm_h, torch.uint8)
        tabs = {k: self._dev(criterion[k]).reshape(-1) for k in ("borders", "bucket_means", "mode_means", "widths")}
        if tabs["borders"].numel() != B + 1 or any(tabs[k].numel() != B for k in ("bucket_means", "mode_means", "widths")):
            raise ValueError(f"criterion tables do not fit {B} bars")
        K = len(quantiles)
        lv = self._dev(np.asarray(quantiles, dtype=np.float32)) if K else None
        out = torch.empty((Q, B), device=self.device, dtype=torch.float32) if want_logits else None
        mean = torch.empty((Q,), device=self.device, dtype=torch.float32)
        mode = torch.empty((Q,), device=self.device, dtype=torch.float32)
        qs = torch.empty((K, Q), device=self.device, dtype=torch.float32)
        head_args = (self.ctx, _ptr(lg), M, Q, B, _ptr(cm), ldc, _ptr(ix), _ptr(sh), ldt,
                     1.0 / float(softmax_temperature), int(average_before_softmax), _ptr(tabs["borders"]),
                     _ptr(tabs["bucket_means"]), _ptr(tabs["mode_means"]), _ptr(tabs["widths"]), _ptr(lv),
                     K, _ptr(out), _ptr(mean), _ptr(mode), _ptr(qs) if K else None)
        res = {"mean": mean, "mode": mode, "quantiles": qs, "logits": out}
        if targets is None:
            self._bind_stream()
            self._check(self.lib.mmpfn_bar_head(*head_args), "mmpfn_bar_head")
            return res
        if score_tables is None:
            raise ValueError("targets need score_tables")
        yd, J, scores = self._score_buffers(targets, Q, B, self.SCORE_KINDS)
        st = self._score_tables(score_tables, B, ("log_widths", "mean_squares", "ei_mids", "ends"))
        self._bind_stream()
        self._check(
            self.lib.mmpfn_bar_head_score(*head_args, _ptr(st["log_widths"]), _ptr(st["mean_squares"]),
                                          _ptr(st["ei_mids"]), _ptr(st["ends"]), _ptr(yd), J,
                                          *(_ptr(scores[k]) for k in self.SCORE_KINDS)),
            "mmpfn_bar_head_score",
        )
        return {**res, **scores}

    def xform_upload(self, program) -> "XformProgram":
        """A ``device_transform.MemberProgram`` copied to the device (``mmpfn_xform_create``, which checks every
        index in it); the handle frees the copy when it goes away."""
        ops = np.ascontiguousarray(program.ops, dtype=np.int32)
        ints = np.ascontiguousarray(program.ints, dtype=np.int32)
        dbl = np.ascontiguousarray(program.doubles, dtype=np.float64)
        h = ctypes.c_void_p()
        self._check(
            self.lib.mmpfn_xform_create(self.ctx, ops.ctypes.data, ops.shape[0], ints.ctypes.data, ints.size,
                                        dbl.ctypes.data, dbl.size, int(program.n_in), ctypes.byref(h)),
            "mmpfn_xform_create",
        )
        return XformProgram(self, h.value, n_in=int(program.n_in), n_out=int(program.n_out))

    def member_transform(self, program, X: torch.Tensor, out: torch.Tensor | None = None, want64: bool = False):
        """A member's preprocessing of the test rows ``X`` ``[Q, n_in]`` (a float32 or float64 tensor on this device;
        rows may be strided) on the current stream, one launch (``mmpfn_member_transform``).  ``program``: an
        ``XformProgram`` of this engine, or a ``MemberProgram`` (uploaded on first use and kept with it).  ``out``:
        a float32 ``[Q, >= n_out]`` view to write into (say rows ``[N, N + Q)`` of the member's full table), else a
        new ``[Q, n_out]`` tensor.  Returns ``out``, with ``want64`` ``(out, out64)``, ``out64`` the float64 values
        before the final rounding (``want64`` may be the float64 ``[Q, >= n_out]`` view to put them in).  A ``+-inf``
        cell raises sklearn's ``ValueError`` at the next ``status()``."""
        if not isinstance(program, XformProgram):
            held = program._handles.get(self.serial)
            if held is None:
                held = program._handles[self.serial] = self.xform_upload(program)
            program = held
        if program.engine is not self or not program.handle:
            raise ValueError("the program belongs to another engine or was freed")
        if not isinstance(X, torch.Tensor) or X.device != self.device or X.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"X must be a float32 or float64 tensor on {self.device}")
        if X.dim() != 2 or X.shape[1] != program.n_in:
            raise ValueError(f"X has shape {tuple(X.shape)}, the program takes [Q, {program.n_in}]")
        if X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
            X = X.contiguous()
        Q = X.shape[0]
        if out is None:
            out = torch.empty((Q, program.n_out), device=self.device, dtype=torch.float32)
        if (out.dtype != torch.float32 or out.device != self.device or out.dim() != 2 or out.shape[0] != Q
                or out.shape[1] < program.n_out or out.stride(1) != 1 or (Q > 1 and out.stride(0) < program.n_out)):
            raise ValueError(f"out must be a float32 [{Q}, >= {program.n_out}] view with unit column stride")
        out64 = None
        if isinstance(want64, torch.Tensor):
            out64 = want64
            if (out64.dtype != torch.float64 or out64.device != self.device or out64.dim() != 2 or out64.shape[0] != Q
                    or out64.shape[1] < program.n_out or out64.stride(1) != 1
                    or (Q > 1 and out64.stride(0) < program.n_out)):
                raise ValueError(f"want64 must be a float64 [{Q}, >= {program.n_out}] view with unit column stride")
        elif want64:
            out64 = torch.empty((Q, program.n_out), device=self.device, dtype=torch.float64)
        if Q:
            self._bind_stream()
            self._check(
                self.lib.mmpfn_member_transform(self.ctx, ctypes.c_void_p(program.handle), _ptr(X),
                                                int(X.dtype == torch.float64), Q, program.n_in,
                                                X.stride(0) if Q > 1 else program.n_in, _ptr(out),
                                                out.stride(0) if Q > 1 else out.shape[1], _ptr(out64),
                                                program.n_out if out64 is None or Q == 1 else out64.stride(0)),
                "mmpfn_member_transform",
            )
        return out if out64 is None else (out, out64)

    def status(self) -> None:
        """Wait for every stream the context ran on and raise ``ValueError`` if any forward since the
        last call saw NaNs in its embedded input (transformer.py:727-731,790-796), or a member transform an
        infinity in a device ``X`` (the host path's ``validate_X_predict``)."""
        self._bind_stream()
        self._check(self.lib.mmpfn_status(self.ctx), "mmpfn_forward")

    # ------------------------------------------------------------------ parity taps
    def embed_state(self, x, tokens, y_train, precision: int) -> torch.Tensor:
        """Embedded transformer input in reference order ``[S, T, E]``."""
        xd, td, yd, uniq, S, F, C, N, G = self._prepare(x, tokens, y_train)
        pr = self._pos(G + C)
        self._S = S
        self._bind_stream()
        self._check(
            self.lib.mmpfn_embed(
                self.ctx, _ptr(xd), S, F, _ptr(td), C, _ptr(yd), N, _ptr(uniq), _count(uniq), _ptr(pr), precision
            ),
            "mmpfn_embed",
        )
        return self.copy_state()

    def run_layers(self, l0: int, l1: int) -> torch.Tensor:
        self._bind_stream()
        self._check(self.lib.mmpfn_run_layers(self.ctx, l0, l1), "mmpfn_run_layers")
        return self.copy_state()

    def copy_state(self) -> torch.Tensor:
        T = self.lib.mmpfn_state_tokens(self.ctx)
        out = torch.empty((self._S, T, self.cfg.emsize), device=self.device, dtype=torch.float32)
        self._check(self.lib.mmpfn_copy_state(self.ctx, _ptr(out), out.numel()), "mmpfn_copy_state")
        torch.cuda.current_stream(self.device).synchronize()
        return out

    # ------------------------------------------------------------------ per-sublayer taps
    def _state_tap(self, X: torch.Tensor, fn, argf) -> torch.Tensor:
        """Run a C-ABI sublayer tap on a reference-order state ``[S, T, E]`` (copied to the
        engine's token-major ``[T, S, E]``, updated in place, copied back).  The working copy is always a
        new tensor: with S == 1 or T == 1 the transposed view is already contiguous, and ``.contiguous()``
        would hand the caller's own storage to the kernel."""
        Xd = self._dev(X)
        Xt = torch.empty((Xd.shape[1], Xd.shape[0]) + tuple(Xd.shape[2:]), dtype=Xd.dtype, device=Xd.device)
        Xt.copy_(Xd.transpose(0, 1))
        T, S, _ = Xt.shape
        self._bind_stream()
        self._check(fn(self.ctx, *argf(Xt, S, T)), fn.__name__)
        return Xt.transpose(0, 1).contiguous()

    def feature_attention(self, layer: int, X: torch.Tensor, precision: int) -> torch.Tensor:
        """``LN(X + FeatAttn_layer(X))`` (layer.py:332-339) through ``mmpfn_feature_attention``."""
        return self._state_tap(X, self.lib.mmpfn_feature_attention,
                               lambda Xt, S, T: (layer, _ptr(Xt), S, T, precision))

    def feature_attention_ex(self, layer: int, X: torch.Tensor, precision: int, last: bool = False) -> torch.Tensor:
        """The same sublayer on the states of M members in one call, ``X`` ``[M, S, T, E]`` (each in reference
        order), through ``mmpfn_feature_attention_ex``: every form the forwards run it in.  ``last``: the pruned
        last layer's form, which on the row-resident kernel updates token T - 1 of every row alone."""
        Xd = self._dev(X)
        if Xd.dim() != 4:
            raise ValueError(f"X must be [M, S, T, E], got {tuple(Xd.shape)}")
        Xt = torch.empty((Xd.shape[0], Xd.shape[2], Xd.shape[1], Xd.shape[3]), dtype=Xd.dtype, device=Xd.device)
        Xt.copy_(Xd.transpose(1, 2))  # a new tensor always (see _state_tap)
        M, T, S, _ = Xt.shape
        self._bind_stream()
        self._check(self.lib.mmpfn_feature_attention_ex(self.ctx, layer, _ptr(Xt), S, T, M, int(last), precision),
                    "mmpfn_feature_attention_ex")
        return Xt.transpose(1, 2).contiguous()

    def item_attention_block(self, layer: int, X: torch.Tensor, n_train: int, precision: int) -> torch.Tensor:
        """``LN(X + ItemAttn_layer(X))`` (layer.py:341-379) through ``mmpfn_item_attention_block``."""
        return self._state_tap(X, self.lib.mmpfn_item_attention_block,
                               lambda Xt, S, T: (layer, _ptr(Xt), S, T, n_train, precision))

    def mlp_ln(self, layer: int, X: torch.Tensor, precision: int) -> torch.Tensor:
        """``LN(X + MLP_layer(X))`` (mlp.py:93-138) through ``mmpfn_mlp_ln`` (row-wise: any order)."""
        Xd = self._dev(X).contiguous().clone()
        self._bind_stream()
        self._check(self.lib.mmpfn_mlp_ln(self.ctx, layer, _ptr(Xd), Xd.numel() // self.cfg.emsize, precision),
                    "mmpfn_mlp_ln")
        return Xd

    def outproj_mlp_ln(self, layer: int, X: torch.Tensor, O: torch.Tensor, precision: int) -> torch.Tensor:
        """``LN(X' + MLP_layer(X'))`` with ``X' = LN(X + O Wout_layer^T)`` through ``mmpfn_outproj_mlp_ln``: the
        step behind the item attention on the forwards' own kernels (the 16-bit modes: one launch).  ``O`` ``[rows, E]``,
        the attention output, is converted to the mode's type (fp32 / bf16 / fp16); returns fp32 ``[rows, E]``."""
        odt = (torch.float32 if precision in (_lib.PREC_F32, _lib.PREC_F32_MFMA)
               else torch.float16 if precision in (_lib.PREC_F16, _lib.PREC_F16_F8, _lib.PREC_F16_F8E5)
               else torch.bfloat16)
        Xd = self._dev(X).contiguous().clone()
        Od = self._dev(O, odt)
        rows = Xd.numel() // self.cfg.emsize
        if Od.numel() != Xd.numel():
            raise ValueError(f"O has {Od.numel()} elements, X {Xd.numel()}")
        self._bind_stream()
        self._check(self.lib.mmpfn_outproj_mlp_ln(self.ctx, layer, _ptr(Xd), _ptr(Od), rows, precision),
                    "mmpfn_outproj_mlp_ln")
        return Xd

    def item_qkv(self, layer: int, X: torch.Tensor, n_train: int, precision: int, last: bool = False,
                 fill: torch.Tensor | None = None):
        """The item attention's projection alone through ``mmpfn_item_qkv``: ``X`` ``[M, S, T, E]`` (each member in
        reference order) -> ``(q [TM, H, S, 32], k [TM, H, Npad, 32], vt [TM, H, 32, Npad])`` in the mode's operand
        type (fp32 in the fp32 modes, bf16 in every 16-bit one), TM = M if ``last`` (column T - 1 only) else M * T,
        Npad = n_train rounded up to 64.  ``n_train == 0``: the train-KV cache's predict form, q of all S rows through
        the test rows' weights; k and vt come back empty.  ``fill``: a one-element tensor of the operand type that the
        outputs are pre-filled with (what the kernels do not store keeps it); without it they are zero-filled."""
        Xd = self._dev(X)
        if Xd.dim() != 4:
            raise ValueError(f"X must be [M, S, T, E], got {tuple(Xd.shape)}")
        Xt = Xd.transpose(1, 2).contiguous()
        M, T, S, _ = Xt.shape
        odt = torch.float32 if precision in (_lib.PREC_F32, _lib.PREC_F32_MFMA) else torch.bfloat16
        TM, H, npad = (M if last else M * T), self.cfg.nhead, (n_train + 63) // 64 * 64
        q, k, vt = (torch.zeros(shape, dtype=odt, device=Xt.device)
                    for shape in ((TM, H, S, 32), (TM, H, npad, 32), (TM, H, 32, npad)))
        if fill is not None:
            for t in (q, k, vt):
                t.copy_(fill.to(device=t.device).reshape(()).expand_as(t))
        self._bind_stream()
        self._check(self.lib.mmpfn_item_qkv(self.ctx, layer, _ptr(Xt), S, T, n_train, M, int(last), precision,
                                            _ptr(q), _ptr(k) if n_train else None, _ptr(vt) if n_train else None),
                    "mmpfn_item_qkv")
        return q, k, vt

    def mgm(self, image, precision: int) -> torch.Tensor:
        """MultiheadGatedMLP tokens ``[S, mgm * n_mod, E]`` (transformer.py:33-57)."""
        img = self._dev(image)
        if img.dim() == 2:
            img = img.unsqueeze(1)
        S, n_mod, _ = img.shape
        out = torch.empty((S, self.cfg.mgm_heads * n_mod, self.cfg.emsize), device=self.device)
        self._bind_stream()
        self._check(self.lib.mmpfn_mgm(self.ctx, _ptr(img), S, n_mod, _ptr(out), precision), "mmpfn_mgm")
        return out

    def cap(self, mgm_tokens, precision: int) -> torch.Tensor:
        """CrossAttentionPooler tokens ``[S, cap, E]`` (transformer.py:60-88)."""
        tok = self._dev(mgm_tokens)
        S, M, _ = tok.shape
        out = torch.empty((S, self.cfg.cap_heads, self.cfg.emsize), device=self.device)
        self._bind_stream()
        self._check(self.lib.mmpfn_cap(self.ctx, _ptr(tok), S, M, _ptr(out), precision), "mmpfn_cap")
        return out

    def decode(self, n_query: int) -> torch.Tensor:
        out = torch.empty((n_query, self.cfg.n_out), device=self.device, dtype=torch.float32)
        self._bind_stream()
        self._check(self.lib.mmpfn_decode(self.ctx, _ptr(out)), "mmpfn_decode")
        return out


class XformProgram:
    """Device copy of one member's preprocessing program (owned by its engine's context)."""

    def __init__(self, engine: HipEngine, handle: int, *, n_in: int, n_out: int):
        self.engine, self.handle, self.n_in, self.n_out = engine, handle, n_in, n_out

    def free(self) -> None:
        if self.handle and getattr(self.engine, "ctx", None):
            self.engine.lib.mmpfn_xform_free(self.engine.ctx, ctypes.c_void_p(self.handle))
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class TrainCache:
    """Device-resident train-KV cache of one ensemble member (owned by its engine's context)."""

    def __init__(self, engine: HipEngine, handle: int, *, N: int, F: int, C: int, precision: int):
        self.engine, self.handle = engine, handle
        self.N, self.F, self.C, self.precision = N, F, C, precision

    @property
    def nbytes(self) -> int:
        return int(self.engine.lib.mmpfn_cache_bytes(ctypes.c_void_p(self.handle))) if self.handle else 0

    def free(self) -> None:
        if self.handle and getattr(self.engine, "ctx", None):
            self.engine.lib.mmpfn_cache_free(self.engine.ctx, ctypes.c_void_p(self.handle))
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
