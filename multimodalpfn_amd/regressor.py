"""``MMPFNRegressor``: the reference's scikit-learn regression interface over the HIP engine.

Same constructor (``mmpfn/models/mmpfn/regressor.py:151-376``), same ``fit(X, image, y)`` /
``predict(X, image_test, *, output_type, quantiles)`` and fitted attributes.  Host-side work is the
reference's algorithm on numpy / scikit-learn: validation, ordinal encoding, the members' feature
preprocessing and target transforms, and the transformed borders of every member (``utils.py:748-795``).
Every forward runs in ``libmmpfn_hip.so`` on an MI355X, and so does the whole post-processing of
``regressor.py:652-765`` -- temperature, cancel mask, each member's distribution moved onto the criterion's
borders, the ensemble mean, and the criterion's mean / median / mode / quantiles -- in one kernel over the
members' logits where they lie (``mmpfn_bar_head``); only what the ``output_type`` asks for is copied back.
``score_samples`` (log predictive density) and ``acquisition`` (``ei`` / ``pi`` / ``ucb``) score the rows in that same
kernel (``mmpfn_bar_head_score``); ``sample`` / ``sample_device`` draw from each row's distribution on the device
(``mmpfn_bar_sample``).
There is no CPU forward: without a ROCm GPU ``fit`` / ``predict`` raise the engine's ``RuntimeError``.
"""

from __future__ import annotations

from collections.abc import Sequence
from pathlib import Path
from typing import Any, Literal

import numpy as np
import torch
from sklearn.base import BaseEstimator, RegressorMixin, check_is_fitted

from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution, border_tables
from multimodalpfn_amd.base import (
    EmbeddingsMixin,
    create_inference_engine,
    determine_precision,
    initialize_mmpfn_model,
)
from multimodalpfn_amd.constants import ModelInterfaceConfig
from multimodalpfn_amd.device_transform import device_table, plan_front_encoder
from multimodalpfn_amd.model.preprocessing import ReshapeFeatureDistributionsStep
from multimodalpfn_amd.preprocessing import (
    EnsembleConfig,
    RegressorEnsembleConfig,
    default_regressor_preprocessor_configs,
)
from multimodalpfn_amd.utils import (
    _fix_dtypes,
    _get_ordinal_encoder,
    _transform_borders_one,
    infer_categorical_features,
    infer_device_and_type,
    infer_random_state,
    update_encoder_outlier_params,
    validate_X_predict,
    validate_Xy_fit,
)

DEFAULT_QUANTILES = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]  # regressor.py:631-632


class MMPFNRegressor(EmbeddingsMixin, RegressorMixin, BaseEstimator):
    """Multimodal PFN regressor (tabular + image/text embeddings), MI355X engine."""

    _OUTPUT_TYPES_BASIC = ("mean", "median", "mode")
    _OUTPUT_TYPES_QUANTILES = ("quantiles",)
    _OUTPUT_TYPES = _OUTPUT_TYPES_BASIC + _OUTPUT_TYPES_QUANTILES  # what "main" returns
    _OUTPUT_TYPES_COMPOSITE = ("full", "main")
    _USABLE_OUTPUT_TYPES = _OUTPUT_TYPES + _OUTPUT_TYPES_COMPOSITE

    def __init__(
        self,
        *,
        mixer_type: str,
        mgm_heads: int,
        cap_heads: int,
        features_per_group: int,
        n_estimators: int = 8,
        categorical_features_indices: Sequence[int] | None = None,
        softmax_temperature: float = 0.9,
        average_before_softmax: bool = False,
        model_path: str | Path | Literal["auto"] = "auto",
        device: str | torch.device | Literal["auto"] = "auto",
        ignore_pretraining_limits: bool = False,
        inference_precision: torch.dtype | Literal["autocast", "auto"] = "auto",
        fit_mode: Literal["low_memory", "fit_preprocessors", "fit_with_cache"] = "fit_preprocessors",
        memory_saving_mode: bool | Literal["auto"] | float | int = "auto",
        random_state: int | np.random.RandomState | np.random.Generator | None = 0,
        n_jobs: int = -1,
        inference_config: dict | ModelInterfaceConfig | None = None,
    ) -> None:
        super().__init__()
        self.n_estimators = n_estimators
        self.categorical_features_indices = categorical_features_indices
        self.softmax_temperature = softmax_temperature
        self.average_before_softmax = average_before_softmax
        self.model_path = model_path
        self.device = device
        self.ignore_pretraining_limits = ignore_pretraining_limits
        self.inference_precision = inference_precision
        self.fit_mode = fit_mode
        self.memory_saving_mode = memory_saving_mode
        self.random_state = random_state
        self.n_jobs = n_jobs
        self.inference_config = inference_config
        self.mixer_type = mixer_type
        self.mgm_heads = mgm_heads
        self.cap_heads = cap_heads
        self.features_per_group = features_per_group

    def _more_tags(self) -> dict[str, Any]:
        return {"allow_nan": True}

    def __sklearn_tags__(self):
        tags = super().__sklearn_tags__()
        tags.input_tags.allow_nan = True
        tags.estimator_type = "regressor"
        return tags

    # ------------------------------------------------------------------ fit
    def fit(self, X, image: np.ndarray | None, y):
        """``regressor.py:390-538``: load the model and its bar distribution, encode the inputs, build the members
        (feature preprocessing x target transform), standardise the target, fit the members."""
        static_seed, rng = infer_random_state(self.random_state)
        self.model_, self.config_, self.bardist_ = initialize_mmpfn_model(
            model_path=self.model_path,
            which="regressor",
            fit_mode=self.fit_mode,
            static_seed=static_seed,
            mixer_type=self.mixer_type,
            mgm_heads=self.mgm_heads,
            cap_heads=self.cap_heads,
            features_per_group=self.features_per_group,
        )
        self.device_ = infer_device_and_type(self.device)
        self.use_autocast_, self.forced_inference_dtype_, byte_size = determine_precision(
            self.inference_precision, self.device_
        )
        ic = self.interface_config_ = ModelInterfaceConfig.from_user_input(inference_config=self.inference_config)
        sigma = ic.OUTLIER_REMOVAL_STD
        if sigma == "auto":
            sigma = ic._REGRESSION_DEFAULT_OUTLIER_REMOVAL_STD
        update_encoder_outlier_params(model=self.model_, remove_outliers_std=sigma, seed=static_seed, inplace=True)

        if X is not None:
            X, y, names, n_in = validate_Xy_fit(
                X,
                y,
                estimator=self,
                ensure_y_numeric=False,
                max_num_samples=ic.MAX_NUMBER_OF_SAMPLES,
                max_num_features=ic.MAX_NUMBER_OF_FEATURES,
                ignore_pretraining_limits=self.ignore_pretraining_limits,
            )
            if names is not None:
                self.feature_names_in_ = names
            self.n_features_in_ = n_in
            X = _fix_dtypes(X, cat_indices=self.categorical_features_indices)
            enc = _get_ordinal_encoder()
            X = enc.fit_transform(X)
            self.preprocessor_ = enc
            self._ordinal_plan_ = plan_front_encoder(enc)  # the front encoder's device form (None: string categories)
            self.inferred_categorical_indices_ = infer_categorical_features(
                X=X,
                provided=self.categorical_features_indices,
                min_samples_for_inference=ic.MIN_NUMBER_SAMPLES_FOR_CATEGORICAL_INFERENCE,
                max_unique_for_category=ic.MAX_UNIQUE_FOR_CATEGORICAL_FEATURES,
                min_unique_for_numerical=ic.MIN_UNIQUE_FOR_NUMERICAL_FEATURES,
            )
            max_index = len(X)
        else:
            self.inferred_categorical_indices_ = []
            max_index = len(image)
        y = np.asarray(y)

        known = ReshapeFeatureDistributionsStep.get_all_preprocessors(num_examples=y.shape[0],
                                                                      random_state=static_seed)
        target_transforms = [None if name is None else known[name]
                             for name in ic.REGRESSION_Y_PREPROCESS_TRANSFORMS]
        configs = EnsembleConfig.generate_for_regression(
            n=self.n_estimators,
            subsample_size=ic.SUBSAMPLE_SAMPLES,
            add_fingerprint_feature=ic.FINGERPRINT_FEATURE,
            feature_shift_decoder=ic.FEATURE_SHIFT_METHOD,
            polynomial_features=ic.POLYNOMIAL_FEATURES,
            max_index=max_index,
            preprocessor_configs=(
                ic.PREPROCESS_TRANSFORMS if ic.PREPROCESS_TRANSFORMS is not None
                else default_regressor_preprocessor_configs()
            ),
            target_transforms=target_transforms,
            random_state=rng,
        )
        assert len(configs) == self.n_estimators

        # the model sees the standardised target; the criterion is moved back to the target's scale (:510-518)
        self.y_train_std_ = np.std(y).item() + 1e-20
        self.y_train_mean_ = np.mean(y).item()
        y = (y - self.y_train_mean_) / self.y_train_std_
        self.renormalized_criterion_ = FullSupportBarDistribution(
            self.bardist_.borders * self.y_train_std_ + self.y_train_mean_
        ).float()
        self._head_tables_ = None  # per-member border tables, built at the first predict (fixed after fit)

        self.executor_ = create_inference_engine(
            X_train=X,
            y_train=y,
            image_train=image,
            model=self.model_,
            ensemble_configs=configs,
            cat_ix=self.inferred_categorical_indices_,
            fit_mode=self.fit_mode,
            device_=self.device_,
            rng=rng,
            n_jobs=self.n_jobs,
            byte_size=byte_size,
            forced_inference_dtype_=self.forced_inference_dtype_,
            memory_saving_mode=self.memory_saving_mode,
            use_autocast_=self.use_autocast_,
        )
        if X is not None:
            self.executor_.attach_front(self._ordinal_plan_)
        return self

    # ------------------------------------------------------------------ predict
    def _member_tables(self, configs) -> tuple[np.ndarray, np.ndarray, np.ndarray | None]:
        """Per member: the criterion's borders through the inverse of its fitted target transform
        (regressor.py:668-683), then the head's per-border tables (``bar_distribution.border_tables``) and cancel
        mask.  They depend on the fit alone, so the engines that fit their members once keep them."""
        keep = self.fit_mode != "low_memory"  # low_memory re-fits the target transforms at every predict
        if keep and self._head_tables_ is not None:
            return self._head_tables_
        std_borders = self.bardist_.borders.cpu().numpy()
        idx, share, cancel = [], [], []
        for config in configs:
            assert isinstance(config, RegressorEnsembleConfig)
            mask = None
            if config.target_transform is None:
                borders_t = std_borders.copy()
            else:
                mask, descending, borders_t = _transform_borders_one(
                    std_borders,
                    target_transform=config.target_transform,
                    repair_nan_borders_after_transform=self.interface_config_.FIX_NAN_BORDERS_AFTER_TARGET_TRANSFORM,
                )
                if descending:  # regressor.py:680-681 calls ndarray.flip there, which does not exist
                    raise AttributeError("a target transform that reverses the borders is not served "
                                         "(the reference fails on it: 'numpy.ndarray' object has no attribute 'flip')")
            i, s = border_tables(borders_t, std_borders)
            idx.append(i)
            share.append(s)
            cancel.append(mask)
        masks = None
        if any(m is not None for m in cancel):
            masks = np.stack([np.zeros(len(std_borders) - 1, bool) if m is None else np.asarray(m, bool)
                              for m in cancel])
        tables = (np.stack(idx), np.stack(share), masks)
        if keep:
            self._head_tables_ = tables
        return tables

    def _encode_host(self, X) -> np.ndarray:
        """validate -> _fix_dtypes -> fitted ordinal encoder (``regressor.py:604-607``)."""
        X = validate_X_predict(X, self)
        X = _fix_dtypes(X, cat_indices=self.categorical_features_indices)
        return self.preprocessor_.transform(X)

    _encode_for_predict = _encode_host  # (EmbeddingsMixin)

    def predict_device(self, X, image_test: np.ndarray | None, *, quantiles: Sequence[float] = (),
                       want_logits: bool = False, targets=None) -> dict:
        """The head's outputs left on the GPU: ``mean`` / ``mode`` ``[Q]``, ``quantiles`` ``[K, Q]``, ``logits``
        ``[Q, B]`` or None, and the members' logits ``member_logits`` ``[M, Q, B]``.  With ``targets`` ``[Q]`` or
        ``[Q, J]`` on the target's original scale (the renormalised criterion's borders are on that scale) the same
        kernel scores every row's distribution there: ``nll`` (the negative log density, 0 at a NaN target), ``cdf``,
        ``pi`` and ``ei`` (the target as the incumbent) ``[Q, J]``, and ``mean_of_square`` / ``variance`` ``[Q]`` --
        the ``[Q, B]`` log-probabilities reach memory only with ``want_logits``."""
        check_is_fitted(self)
        if isinstance(X, torch.Tensor) and X.is_cuda:
            # a table on the GPU (``[Q, n_features_in_]``, here and in every method built on this one): encoded and
            # preprocessed there by the members that have a device program (device_transform.py)
            X = device_table(self, X, self.device_, self._encode_host)
        elif X is not None:
            X = self._encode_host(X)
        logits, configs = [], []
        for out, config in self.executor_.iter_outputs(X, image_test=image_test, device=self.device_,
                                                       autocast=self.use_autocast_):
            assert out.ndim == 2
            logits.append(out)
            configs.append(config)
        idx, share, cancel = self._member_tables(configs)
        stacked = torch.stack(logits)
        eng = self.model_.engine(stacked.device)
        crit = self.renormalized_criterion_
        out = eng.bar_head(stacked, idx, share, crit.head_tables(), cancel=cancel,
                           softmax_temperature=float(self.softmax_temperature),
                           average_before_softmax=bool(self.average_before_softmax), quantiles=list(quantiles),
                           want_logits=want_logits, targets=targets,
                           score_tables=None if targets is None else crit.score_tables())
        if targets is not None:
            out["variance"] = out["mean_of_square"] - out["mean"].square()
        out["member_logits"] = stacked
        return out

    def score_samples(self, X, image_test: np.ndarray | None, y) -> np.ndarray:
        """The log predictive density of ``y`` ``[Q]`` (original scale) under each row's distribution, ``[Q]``; 0
        where ``y`` is NaN.  Scored on the device: no ``[Q, B]`` logits are stored or copied."""
        y = np.asarray(y, dtype=np.float32).reshape(-1)
        nll = self.predict_device(X, image_test, targets=y)["nll"][:, 0]
        return (0.0 - nll).cpu().numpy()

    def acquisition(self, X, image_test: np.ndarray | None, best_f, *, kind: Literal["ei", "pi", "ucb"] = "ei",
                    rest_prob: float = (1 - 0.682) / 2) -> np.ndarray:
        """A Bayesian-optimisation acquisition value per row, ``[Q]`` (maximising): the expected improvement over /
        the probability of improving on the incumbent ``best_f`` (a number or one per row, original scale), or
        ``ucb``, the quantile that leaves ``rest_prob`` above it (``best_f`` unused, as in the reference)."""
        if kind not in ("ei", "pi", "ucb"):
            raise ValueError(f"Invalid acquisition kind: {kind}")
        if kind == "ucb":
            return self.predict_device(X, image_test, quantiles=[1.0 - rest_prob])["quantiles"][0].cpu().numpy()
        n_rows = len(X) if X is not None else len(image_test)
        best = np.array(np.broadcast_to(np.asarray(best_f, dtype=np.float32), (n_rows,)))
        return self.predict_device(X, image_test, targets=best)[kind][:, 0].cpu().numpy()

    def sample_device(self, X, image_test: np.ndarray | None, n_samples: int = 1, *, random_state=None,
                      uniforms=None, temperature: float = 1.0,
                      tails: Literal["linear", "halfnormal"] = "linear") -> torch.Tensor:
        """``n_samples`` draws from each row's predictive distribution on the target's original scale, a device
        tensor ``[Q, n_samples]`` (``HipEngine.bar_sample`` on the head's log-probabilities where they lie: nothing
        of the bars' size reaches the host).  ``random_state`` (``None``, an int or a ``np.random.Generator``) gives
        the one 64-bit seed of the device generator, so equal ints give equal draws; ``uniforms`` ``[Q, n_samples]``
        supplies the levels instead.  ``temperature`` is the ``t`` of the reference's ``sample(logits, t)``, on top
        of ``softmax_temperature``, which the head has applied.  ``tails``: ``"linear"`` as the reference's ``sample``,
        or ``"halfnormal"``, the end buckets as ``score_samples`` scores them."""
        seed = int(np.random.default_rng(random_state).integers(0, 2 ** 64, dtype=np.uint64))
        logits = self.predict_device(X, image_test, want_logits=True)["logits"]
        eng = self.model_.engine(logits.device)
        crit = self.renormalized_criterion_
        return eng.bar_sample(logits, {**crit.head_tables(), **crit.score_tables()}, n_samples, seed=seed,
                              uniforms=uniforms, temperature=temperature, tails=tails)

    def sample(self, X, image_test: np.ndarray | None, n_samples: int = 1, *, random_state=None, uniforms=None,
               temperature: float = 1.0, tails: Literal["linear", "halfnormal"] = "linear") -> np.ndarray:
        """``sample_device`` as float32 numpy ``[Q, n_samples]``."""
        return self.sample_device(X, image_test, n_samples, random_state=random_state, uniforms=uniforms,
                                  temperature=temperature, tails=tails).cpu().numpy()

    def predict(self, X, image_test: np.ndarray | None, *,
                output_type: Literal["mean", "median", "mode", "quantiles", "full", "main"] = "mean",
                quantiles: list[float] | None = None):
        """``regressor.py:577-729``: ``mean`` / ``median`` / ``mode`` -> ``[Q]``; ``quantiles`` -> one ``[Q]`` array
        per level; ``main`` -> a dict of those four; ``full`` -> ``main`` plus ``criterion`` (the renormalised bar
        distribution) and ``logits`` (the ensemble's log-probabilities ``[Q, B]``, a CPU tensor)."""
        check_is_fitted(self)
        if quantiles is None:
            quantiles = list(DEFAULT_QUANTILES)
        else:
            assert all((0 <= q <= 1) and (isinstance(q, float)) for q in quantiles), \
                "All quantiles must be between 0 and 1 and floats."
        if output_type not in self._USABLE_OUTPUT_TYPES:
            raise ValueError(f"Invalid output type: {output_type}")
        # the kernel's quantile levels: what the output type reads, the median as the level 0.5 (:244-245)
        composite = output_type in self._OUTPUT_TYPES_COMPOSITE
        levels = list(quantiles) if composite or output_type == "quantiles" else []
        if composite or output_type == "median":
            levels = levels + [0.5]
        out = self.predict_device(X, image_test, quantiles=levels, want_logits=output_type == "full")
        if output_type in ("mean", "mode"):
            return out[output_type].cpu().numpy()
        q = out["quantiles"].cpu().numpy()
        if output_type == "median":
            return q[-1]
        if output_type == "quantiles":
            return [q[k] for k in range(len(quantiles))]
        res = {"mean": out["mean"].cpu().numpy(), "median": q[-1], "mode": out["mode"].cpu().numpy(),
               "quantiles": [q[k] for k in range(len(quantiles))]}
        if output_type == "full":
            res = {"criterion": self.renormalized_criterion_, "logits": out["logits"].cpu(), **res}
        return res
