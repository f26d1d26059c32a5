"""Model initialisation, precision choice and engine construction (mirror of ``base.py``).

``initialize_mmpfn_model`` / ``determine_precision`` / ``create_inference_engine``
keep the reference signatures (``mmpfn/models/mmpfn/base.py:54-270``).
"""

from __future__ import annotations

from pathlib import Path
from typing import Any, Literal

import numpy as np
import torch
from sklearn.utils.validation import check_is_fitted

from multimodalpfn_amd.constants import AUTOCAST_DTYPE_BYTE_SIZE, DEFAULT_DTYPE_BYTE_SIZE
from multimodalpfn_amd.device_transform import device_table
from multimodalpfn_amd.inference import (
    InferenceEngineCacheKV,
    InferenceEngineCachePreprocessing,
    InferenceEngineOnDemand,
    check_embedding_source,
)
from multimodalpfn_amd.utils import infer_fp16_inference_mode, load_model_criterion_config


class EmbeddingsMixin:
    """``get_embeddings`` of both estimators (TabPFN's method of that name): every member's row embeddings, the
    target token's final state of each row, which the forward returns beside the logits.  The estimator supplies
    ``_encode_for_predict`` (its host encoding of a predict table)."""

    def get_embeddings_device(self, X, image_test: np.ndarray | None,
                              data_source: Literal["test", "train"] = "test") -> torch.Tensor:
        """``[n_members, rows, emsize]`` fp32 left on the GPU, members in the order of the ensemble configs.

        ``data_source="test"``: the embeddings of the rows of ``X`` / ``image_test`` (``X`` as ``predict`` takes it:
        an array, a DataFrame or a CUDA tensor on the estimator's device).  ``"train"``: those of the fitted train
        rows; ``X`` only rides along as the forward's test rows, which no train row reads, so the result does not
        depend on it.  ``fit_mode="fit_with_cache"`` serves ``"test"`` only: its cache keeps the train rows' keys
        and values, not their embeddings."""
        check_embedding_source(data_source, cached=getattr(self, "fit_mode", None) == "fit_with_cache", required=True)
        check_is_fitted(self)
        ex = self.executor_
        try:
            if image_test is not None:
                ex.launch_mixer_early(image_test, device=self.device_, autocast=self.use_autocast_)
            if isinstance(X, torch.Tensor) and X.is_cuda:
                X = device_table(self, X, self.device_, self._encode_for_predict)
            elif X is not None:
                X = self._encode_for_predict(X)
            outs = [out for out, _ in ex.iter_outputs(X, image_test=image_test, device=self.device_,
                                                      autocast=self.use_autocast_, embeddings=data_source)]
        finally:
            ex._early_tokens = None
        return torch.stack(outs)

    def get_embeddings(self, X, image_test: np.ndarray | None,
                       data_source: Literal["test", "train"] = "test") -> np.ndarray:
        """``get_embeddings_device`` as a float32 array ``[n_members, rows, emsize]``."""
        return self.get_embeddings_device(X, image_test, data_source).cpu().numpy()


def initialize_mmpfn_model(
    model_path: str | Path | Literal["auto"],
    which: Literal["classifier", "regressor"],
    fit_mode: Literal["low_memory", "fit_preprocessors", "fit_with_cache"],
    static_seed: int,
    mixer_type: str,
    mgm_heads: int,
    cap_heads: int,
    features_per_group: int,
):
    """Load the checkpoint -> (model, config, None) for the classifier, (model, config, bar distribution) for
    the regressor (``base.py:54-120``)."""
    if isinstance(model_path, str) and model_path == "auto":
        model_path = None  # type: ignore[assignment]
    if which not in ("classifier", "regressor"):
        raise ValueError(f"Invalid which: {which}")
    model, criterion, config = load_model_criterion_config(
        model_path=model_path,
        check_bar_distribution_criterion=which == "regressor",
        cache_trainset_representation=(fit_mode == "fit_with_cache"),
        which=which,
        version="v2",
        download=False,
        model_seed=static_seed,
        mixer_type=mixer_type,
        mgm_heads=mgm_heads,
        cap_heads=cap_heads,
        features_per_group=features_per_group,
    )
    return model, config, criterion if which == "regressor" else None


def determine_precision(inference_precision, device_: torch.device) -> tuple[bool, torch.dtype | None, int]:
    """(use_autocast, forced dtype, byte size), ``base.py:123-165``.

    On the engine, autocast selects the bf16-MFMA mode (fp32 accumulation, fp32
    residual stream / LayerNorm); a forced float32 / float64 selects the fp32 parity
    mode; a forced 16-bit dtype selects bf16.
    """
    if inference_precision in ("autocast", "auto"):
        use_autocast = infer_fp16_inference_mode(
            device=device_, enable=True if inference_precision == "autocast" else None
        )
        return use_autocast, None, AUTOCAST_DTYPE_BYTE_SIZE if use_autocast else DEFAULT_DTYPE_BYTE_SIZE
    if isinstance(inference_precision, torch.dtype):
        return False, inference_precision, inference_precision.itemsize
    raise ValueError(f"Unknown inference_precision={inference_precision}")


def create_inference_engine(
    *,
    X_train,
    y_train,
    image_train,
    model,
    ensemble_configs: Any,
    cat_ix: list[int],
    fit_mode: Literal["low_memory", "fit_preprocessors", "fit_with_cache"],
    device_: torch.device,
    rng,
    n_jobs: int,
    byte_size: int,
    forced_inference_dtype_: torch.dtype | None,
    memory_saving_mode,
    use_autocast_: bool,
):
    """Engine per ``fit_mode`` (``base.py:168-270``)."""
    common = dict(cat_ix=cat_ix, model=model, ensemble_configs=ensemble_configs, n_workers=n_jobs, rng=rng,
                  dtype_byte_size=byte_size, force_inference_dtype=forced_inference_dtype_,
                  save_peak_mem=memory_saving_mode)
    if fit_mode == "low_memory":
        return InferenceEngineOnDemand.prepare(X_train, y_train, image_train, **common)
    if fit_mode == "fit_preprocessors":
        return InferenceEngineCachePreprocessing.prepare(X_train, y_train, image_train, **common)
    if fit_mode == "fit_with_cache":
        return InferenceEngineCacheKV.prepare(X_train, y_train, image_train, device=device_,
                                              autocast=use_autocast_, **common)
    raise ValueError(f"Invalid fit_mode: {fit_mode}")
