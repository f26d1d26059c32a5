"""CPU: the regression path's host side and restatement against the reference's recorded outputs
(``tests/golden/regression``, ``make_regression_golden.py``): the value-target model restatement (model fixtures),
the members a fit builds and the head on their recorded logits (API fixtures), the border transforms, the
checkpoint ABI of a regression model, and ``MMPFNRegressor``'s behaviour without a GPU."""

import json

import numpy as np
import pytest
import torch

import regression_oracle as ro
from helpers import oracle_spec, rel_err, torch_sd
from test_regression_head import REG

from multimodalpfn_amd import MMPFNRegressor, _lib
from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution, border_tables
from multimodalpfn_amd.model.spec import CRITERION_PREFIX, ModelConfig, state_dict_spec
from multimodalpfn_amd.utils import _transform_borders_one

MODEL_NAMES = [c["name"] for c in ro.MODEL_CASES]
API_NAMES = [c["name"] for c in ro.API_CASES]


def model_case(name):
    case = next(c for c in ro.MODEL_CASES if c["name"] == name)
    z = np.load(REG / f"model_{name}.npz")
    assert json.loads(str(z["meta"])) == case
    cfg = ModelConfig(**case["cfg"])
    return case, z, cfg, ro.reg_state_dict(cfg, case["wseed"]), ro.model_case_inputs(case)


def api_case(name):
    case = next(c for c in ro.API_CASES if c["name"] == name)
    z = dict(np.load(REG / f"api_{name}.npz"))
    assert json.loads(str(z["meta"])) == case
    for m in range(4):
        if f"m{m}_logits" not in z:
            z[f"m{m}_logits"] = np.load(REG / f"api_{name}_m{m}.npz")["logits"]
    return case, z


def write_ckpt(case, tmp):
    from api_cases import ckpt_config

    cfg = ModelConfig(num_buckets=case["num_buckets"], **ro.API_MODEL)
    sd = ro.reg_state_dict(cfg, case["wseed"])
    path = tmp / f"{case['name']}.ckpt"
    config = dict(ckpt_config(cfg), num_buckets=case["num_buckets"], task_type="regression")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "config": config}, path)
    return path, cfg, sd


# ------------------------------------------------------------------------------------------------ model level


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_value_target_restatement_matches_reference_model(name):
    """The label token bit for bit (same operations, same order); the logits within the oracle's golden
    tolerance (``test_oracle_golden``: 1e-5 of max(1, max|ref|))."""
    case, z, cfg, sd, d = model_case(name)
    taps = {}
    x = None if d["x"] is None else torch.from_numpy(d["x"])
    img = None if d["image"] is None else torch.from_numpy(d["image"])
    out = ro.forward_value(oracle_spec(cfg), torch_sd(sd), x, img, torch.from_numpy(d["y_train"]), taps=taps)
    assert out.shape == z["logits"].shape == (case["S"] - case["N"], cfg.num_buckets)
    assert torch.equal(taps["embedded_input"][:, -1], torch.from_numpy(z["y_token"]))
    assert rel_err(out.numpy(), z["logits"]) < 1e-5
    if case["nan_labels"]:
        assert np.isnan(d["y_train"]).sum() == case["nan_labels"]


# ------------------------------------------------------------------------------------------------ checkpoint ABI


def test_regression_spec_and_default_spec():
    """``max_num_classes == 0``: n_out = num_buckets, the y encoder's Linear at step 1, the criterion's buffers; the
    default config's spec has none of it (``test_boundary`` pins it against the module tree)."""
    cfg = ModelConfig(max_num_classes=0, num_buckets=37, nlayers=1, mgm_heads=2, cap_heads=2)
    spec = dict(state_dict_spec(cfg))
    assert cfg.is_regression and cfg.n_out == 37
    assert spec["criterion.borders"] == (38,) and spec["criterion.losses_per_bucket"] == (37,)
    assert spec["decoder_dict.standard.2.weight"] == (37, cfg.nhid) and spec["y_encoder.1.layer.weight"] == (192, 2)
    assert "y_encoder.2.layer.weight" not in spec
    from multimodalpfn_amd.model.transformer import PerFeatureTransformer

    got = sorted((k, tuple(v.shape)) for k, v in PerFeatureTransformer(cfg).state_dict().items())
    assert got == sorted((k, s) for k, s in spec.items() if not k.startswith(CRITERION_PREFIX))
    default = dict(state_dict_spec(ModelConfig()))
    assert not any(k.startswith(CRITERION_PREFIX) for k in default) and "y_encoder.2.layer.weight" in default
    assert ModelConfig().n_out == 10 and not ModelConfig().is_regression
    from multimodalpfn_amd.engine import model_desc

    assert model_desc(cfg).target_kind == _lib.TARGET_VALUE and model_desc(ModelConfig()).target_kind == _lib.TARGET_CLASS


def test_regression_checkpoint_loads(tmp_path):
    """``load_model_criterion_config`` / ``initialize_mmpfn_model(which="regressor")`` on a synthetic regression
    checkpoint: the model's config, and the bar distribution built from ``criterion.borders``."""
    from multimodalpfn_amd.base import initialize_mmpfn_model
    from multimodalpfn_amd.utils import load_model_criterion_config

    case = ro.API_CASES[0]
    path, cfg, sd = write_ckpt(case, tmp_path)
    kw = dict(mixer_type="MGM+CAP", mgm_heads=2, cap_heads=2, features_per_group=2)
    model, config, bardist = initialize_mmpfn_model(str(path), "regressor", "fit_preprocessors", 0, **kw)
    assert model.cfg.is_regression and model.cfg.n_out == case["num_buckets"] and config["max_num_classes"] == 0
    assert isinstance(bardist, FullSupportBarDistribution)
    assert torch.equal(bardist.borders, torch.from_numpy(sd["criterion.borders"]))
    assert torch.equal(model.state_dict()["y_encoder.1.layer.weight"], torch.from_numpy(sd["y_encoder.1.layer.weight"]))
    # a classifier checkpoint is refused where a bar distribution is expected (utils.py:360-368)
    from api_cases import ckpt_config
    from synth import synth_state_dict

    ccfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2)
    cpath = tmp_path / "clf.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in synth_state_dict(state_dict_spec(ccfg), 3).items()},
                "config": ckpt_config(ccfg)}, cpath)
    with pytest.raises(ValueError, match="FullSupportBarDistribution"):
        load_model_criterion_config(cpath, check_bar_distribution_criterion=True, cache_trainset_representation=False,
                                    which="regressor", download=False, model_seed=0, **kw)
    # borders that do not fit the config's num_buckets
    bad = dict(sd)
    bad["criterion.borders"] = bad["criterion.borders"][:-1]
    bpath = tmp_path / "bad.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in bad.items()},
                "config": dict(ckpt_config(cfg), num_buckets=case["num_buckets"])}, bpath)
    with pytest.raises(ValueError, match="criterion.borders"):
        initialize_mmpfn_model(str(bpath), "regressor", "fit_preprocessors", 0, **kw)


# ------------------------------------------------------------------------------------------------ border transforms


def test_border_transform_ports_match_reference_exactly():
    """``_transform_borders_one`` (with ``_cancel_nan_borders`` / ``_repair_borders`` and the two limits) on every
    target transform the regressor offers, one with poles at both ends (cancel mask) and a reversing one."""
    z = np.load(REG / "borders.npz")
    seen = set()
    for name, (t, std) in ro.border_transform_cases().items():
        mask, desc, out = _transform_borders_one(std.copy(), t, repair_nan_borders_after_transform=True)
        assert np.array_equal(out, z[f"{name}_borders"]), name
        assert bool(desc) == bool(z[f"{name}_descending"]), name
        ref_mask = z[f"{name}_cancel"]
        assert (mask is None) == (ref_mask.size == 0), name
        if mask is not None:
            assert np.array_equal(mask, ref_mask), name
            seen.add("cancel")
        if desc:
            seen.add("descending")
    assert seen == {"cancel", "descending"}


# ------------------------------------------------------------------------------------------------ API level


def _eq(a, b, what):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-12, atol=1e-12,
                               equal_nan=True, err_msg=what)


@pytest.mark.parametrize("name", API_NAMES)
def test_fit_members_match_reference(name, tmp_path):
    """``generate_for_regression`` and the fitted members: preprocessor, feature shift, target (after its
    transform), train / test tables, categorical indices, transformed borders and cancel mask of every member, to
    the API tests' host bound (1e-12); then the standardisation and the renormalised criterion."""
    case, z = api_case(name)
    d = ro.api_case_data(case)
    path, _, _ = write_ckpt(case, tmp_path)
    reg = MMPFNRegressor(model_path=str(path), device="cpu", **ro.api_regressor_kwargs(case, case["variants"][0]))
    reg.fit(d["X_train"], None, d["y_train"])
    assert reg.y_train_mean_ == float(z["y_train_mean"]) and reg.y_train_std_ == float(z["y_train_std"])
    assert np.array_equal(reg.bardist_.borders.numpy(), z["std_borders"])
    assert np.array_equal(reg.renormalized_criterion_.borders.numpy(), z["crit_borders"])
    ex = reg.executor_
    assert len(ex.ensemble_configs) == 4
    X_enc = reg.preprocessor_.transform(d["X_test"])
    idx, share, cancel = reg._member_tables(ex.ensemble_configs)
    kinds = []
    for m, c in enumerate(ex.ensemble_configs):
        assert str(c.preprocess_config) == str(z[f"m{m}_pp"]), m
        assert int(c.feature_shift_count) == int(z[f"m{m}_feature_shift"]), m
        _eq(ex.y_trains[m], z[f"m{m}_y_train"], f"m{m} y_train")
        _eq(ex.X_trains[m], z[f"m{m}_X_train"], f"m{m} X_train")
        _eq(ex.preprocessors[m].transform(X_enc).X, z[f"m{m}_X_test"], f"m{m} X_test")
        assert list(ex.cat_ixs[m]) == list(z[f"m{m}_cat_ix"]), m
        kinds.append(c.target_transform is None)
        # the head's tables are those of the reference's borders for this member
        ri, rs = border_tables(z[f"m{m}_borders"], z["std_borders"])
        assert np.array_equal(idx[m], ri) and np.array_equal(share[m], rs), m
        assert np.array_equal(np.zeros(len(ri) - 1, bool) if cancel is None else cancel[m], z[f"m{m}_cancel"]), m
    assert sorted(kinds) == [False, False, True, True]  # two members without, two with a target transform
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            reg.predict(d["X_test"], None)


@pytest.mark.parametrize("name", API_NAMES)
def test_head_restatement_on_recorded_member_logits(name):
    """The float32 restatement of the head on the reference members' recorded logits, borders and cancel masks:
    ``torch.equal`` to the reference regressor's ``full`` output, for every variant."""
    case, z = api_case(name)
    for variant in case["variants"]:
        tag = variant["tag"]
        masks = [z[f"m{m}_cancel"] if z[f"m{m}_cancel"].any() else None for m in range(4)]
        with ro.fixture_threads():
            got = ro.head([torch.from_numpy(z[f"m{m}_logits"]) for m in range(4)],
                          [z[f"m{m}_borders"].astype(np.float32) for m in range(4)], z["std_borders"], masks,
                          temperature=0.9, average_before_softmax=variant["average_before_softmax"],
                          crit_borders=z["crit_borders"], levels=ro.API_QUANTILES + [0.5], dtype=torch.float32)
        assert torch.equal(got["logits"], torch.from_numpy(z[f"{tag}_logits"])), tag
        assert torch.equal(got["mean"], torch.from_numpy(z[f"{tag}_mean"])), tag
        assert torch.equal(got["mode"], torch.from_numpy(z[f"{tag}_mode"])), tag
        assert torch.equal(got["quantiles"][:-1], torch.from_numpy(z[f"{tag}_quantiles"])), tag
        assert torch.equal(got["quantiles"][-1], torch.from_numpy(z[f"{tag}_median"])), tag


# ------------------------------------------------------------------------------------------------ the estimator


def _regressor(**kw):
    return MMPFNRegressor(mixer_type="MGM+CAP", mgm_heads=2, cap_heads=2, features_per_group=2, **kw)


def test_regressor_construction_and_validation(tmp_path):
    from sklearn.base import clone
    from sklearn.exceptions import NotFittedError

    reg = _regressor(n_estimators=3, softmax_temperature=0.7)
    assert reg.get_params()["n_estimators"] == 3 and clone(reg).softmax_temperature == 0.7
    assert _regressor().n_estimators == 8  # the reference's default
    assert reg.__sklearn_tags__().estimator_type == "regressor"
    with pytest.raises(NotFittedError):
        reg.predict(np.zeros((3, 2)), None)
    case = ro.API_CASES[0]
    d = ro.api_case_data(case)
    path, _, _ = write_ckpt(case, tmp_path)
    reg = _regressor(model_path=str(path), device="cpu", n_estimators=2, ignore_pretraining_limits=True)
    reg.fit(d["X_train"], None, d["y_train"])
    for attr in ("y_train_mean_", "y_train_std_", "bardist_", "renormalized_criterion_", "executor_", "model_"):
        assert hasattr(reg, attr), attr
    assert reg.y_train_std_ > 0 and isinstance(reg.renormalized_criterion_, FullSupportBarDistribution)
    with pytest.raises(ValueError, match="Invalid output type"):
        reg.predict(d["X_test"], None, output_type="ei")
    with pytest.raises(AssertionError, match="quantiles"):
        reg.predict(d["X_test"], None, output_type="quantiles", quantiles=[1.5])
    with pytest.raises(AssertionError, match="quantiles"):
        reg.predict(d["X_test"], None, output_type="quantiles", quantiles=[1])  # an int, as in the reference
    with pytest.raises(ValueError):
        reg.predict(d["X_test"][:, :2], None)  # feature count of the fit
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            reg.predict(d["X_test"], None)
        cached = _regressor(model_path=str(path), device="cpu", n_estimators=2, fit_mode="fit_with_cache")
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            cached.fit(d["X_train"], None, d["y_train"])
