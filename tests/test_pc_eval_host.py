"""Host-side checks of the principal-components evaluation (no GPU): the fp64 yardstick tests/pc_eval_fp64.py against the
fixture recorded from the reference's own functions (tests/golden/make_golden_pc_eval.py), the two entry points' signatures, the
header's new entry points and the two synthetic configs."""
import ast
import json
import os
import re

import numpy as np
import pytest
import yaml

import pc_eval_fp64 as Y
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return load_golden("pc_eval")


def _rel(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_fixture_holds_the_generation_time_check(fx):
    """The reference's mm errors were within 1e-3 of the fp64 direct-difference restatement when the fixture was made."""
    assert float(fx["full.errors_vs_fp64"]) <= 1e-3
    assert json.loads(str(fx["checks"]))["full_autoencoder"]["errors_vs_fp64"] == float(fx["full.errors_vs_fp64"])


def test_yardstick_reproduces_the_reconstruction_errors(fx):
    _, _, err = Y.shapes_eval(fx["full.recon"], fx["full.frames"], fx["full.norm_mean"], fx["full.norm_std"], float(fx["full.to_mm"]))
    assert err.shape == fx["full.errors"].shape == (37, 5)
    per_element = float((np.abs(err - fx["full.errors"]) / np.abs(fx["full.errors"])).max())
    print(f"errors: max relative difference {per_element:.2e}")
    assert per_element <= 1e-3
    assert _rel(err, fx["full.errors_csv"]) <= 1e-3


def test_yardstick_reproduces_the_aggregated_table(fx):
    """mean / std (n - 1) / median / min / max of the recorded errors against pandas' agg in the reference."""
    m = Y.moments(fx["full.errors"])
    agg = dict(zip([str(s) for s in fx["full.agg_index"]], fx["full.agg"]))
    assert list(agg) == ["mean", "std", "median", "min", "max"]
    assert _rel(m["mean"], agg["mean"]) <= 1e-5
    assert _rel(m["std"], agg["std"]) <= 1e-5
    for key in ("median", "min", "max"):
        assert _rel(m[key], agg[key]) <= 1e-3, key


def test_yardstick_reproduces_the_latent_covariance(fx):
    """np moments of the recorded latents against the reference's fp32 torch.cov, whole and per articulator."""
    m = Y.moments(fx["small.latents"])
    assert _rel(m["cov"], fx["small.cov"]) <= 1e-5
    lo = 0
    for name, k in zip(fx["small.comps_names"], fx["small.comps"]):   # indices in the order of the components dict
        block = m["cov"][lo:lo + k, lo:lo + k]
        assert _rel(block, fx[f"small.cov.{name}"]) <= 1e-5, name
        lo += int(k)
    assert lo == fx["small.latents"].shape[1]


def test_latent_space_table_is_the_latents_in_loader_order(fx):
    assert [str(c) for c in fx["full.latent_columns"]] == [str(i) for i in range(1, fx["full.latents"].shape[1] + 1)]
    assert _rel(fx["full.latent_space"], fx["full.latents"]) <= 1e-6


def test_yardstick_layout_reference_channel_and_masking():
    rng = np.random.RandomState(0)
    B, T, A, N = 2, 3, 2, 4
    shapes, targets = rng.rand(B, T, A, 2 * N).astype(np.float32), rng.rand(B, T, A, 2, N).astype(np.float32)
    mean, std = rng.rand(A, 2, N).astype(np.float32), (0.5 + rng.rand(A, 2, N)).astype(np.float32)
    ref = rng.rand(B, T, 1, 2, N).astype(np.float32)
    pred, tgt, err = Y.shapes_eval(shapes, targets, mean, std, 2.0, lengths=[3, 1], reference=ref, ref_idx=1)
    assert pred.shape == tgt.shape == (B, T, A + 1, 2, N) and err.shape == (B, T, A)
    assert np.array_equal(pred[0, :, 1], ref[0, :, 0]) and np.array_equal(tgt[0, :, 1], ref[0, :, 0])
    assert np.array_equal(pred[0, :, 2], shapes[0, :, 1].reshape(T, 2, N) * std[1] + mean[1])
    assert not pred[1, 1:].any() and not tgt[1, 1:].any() and not err[1, 1:].any() and err[1, 0].all()
    same = Y.shapes_eval(targets.reshape(B, T, A, 2 * N), targets, mean, std)[2]
    assert np.array_equal(same, np.zeros_like(same))


def _script_signature(path):
    tree = ast.parse(open(path).read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    names = [a.arg for a in main.args.args]
    defaults = [ast.literal_eval(d) for d in main.args.defaults]
    keys = {n: None for n in names}
    keys.update(dict(zip(names[len(names) - len(defaults):], defaults)))
    flags = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: ast.literal_eval(k.value) for k in node.keywords}
            flags.append([node.args[0].value, kw.get("dest"), kw.get("default")])
    return keys, flags


@pytest.mark.parametrize("which,script,extras", [
    ("autoencoder", "test_principal_components_autoencoder.py", {"synthetic", "seed"}),
    ("method", "test_phoneme_to_principal_components.py", {"synthetic", "seed", "encoder_type", "decoder_type"})])
def test_entry_point_flags_and_main_keys_match_the_reference(fx, which, script, extras):
    """Same --config flag and every main() keyword of the reference, in its order and with its default; the extra keys are
    the engine's synthetic data switch and, for the method, the trainer's encoder_type / decoder_type."""
    ref = json.loads(str(fx["signatures"]))[which]
    keys, flags = _script_signature(os.path.join(ROOT, script))
    assert flags == ref["flags"] == [["--config", "cfg_filepath", None]]
    ref_keys = dict((k, v) for k, v in ref["main"])
    assert list(keys)[:len(ref_keys)] == [k for k, _ in ref["main"]]
    assert {k: keys[k] for k in ref_keys} == ref_keys
    assert set(keys) - set(ref_keys) == extras
    if which == "method":
        assert keys["encoder_type"] == keys["decoder_type"] == "AE"


def test_header_declares_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("as_pc_shapes_eval", "as_pc_eval_accumulate"):
        assert re.search(rf"\bint\s+{name}\s*\(", code), f"{name} is not declared in the header"
    from artspeech_amd import _lib
    assert len(_lib.PROTOTYPES["as_pc_shapes_eval"][1]) == 16 and len(_lib.PROTOTYPES["as_pc_eval_accumulate"][1]) == 10
    from artspeech_amd import build
    assert build.SOURCES["pc_eval.hip"] == ["-ffp-contract=off"]


@pytest.mark.parametrize("config,script,train_config", [
    ("test_pc_autoencoder_synthetic.yaml", "test_principal_components_autoencoder.py", "train_pc_autoencoder_synthetic.yaml"),
    ("test_pc_based_synthetic.yaml", "test_phoneme_to_principal_components.py", "train_pc_based_synthetic.yaml")])
def test_configs_load_and_read_what_the_training_configs_write(config, script, train_config):
    with open(os.path.join(ROOT, "configs", config)) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "configs", train_config)) as f:
        train = yaml.safe_load(f)
    keys, _ = _script_signature(os.path.join(ROOT, script))
    assert set(cfg) <= set(keys)
    assert {k for k, v in keys.items() if v is None and k not in ("recognizer_filepath", "recognizer_params", "voicing_filepath",
                                                                  "TV_to_phoneme_map", "synthetic", "vocab_filepath")} <= set(cfg)
    assert cfg["datadir"] == "synthetic"
    if "model_params" in cfg:
        assert cfg["model_params"] == train["model_params"]
        assert os.path.dirname(cfg["encoders_filepath"]) == os.path.dirname(cfg["decoders_filepath"]) == train["results_dir"]
    else:
        assert cfg["indices_dict"] == train["indices_dict"] and cfg["modelkwargs"] == train["modelkwargs"]
        assert cfg["autoencoder_kwargs"] == train["autoencoder_kwargs"]
        assert cfg["state_dict_filepath"] == os.path.join(train["results_dir"], "best_model.pt")
        assert cfg["encoder_state_dict_filepath"] == train["encoder_state_dict_filepath"]
        assert cfg["decoder_state_dict_filepath"] == train["decoder_state_dict_filepath"]
