"""CPU tests of the point-to-closest-point loss's host side: the C-ABI surface, the build recipe, the trainer's `loss` key and
its config, and the float64 yardstick against the reference fixture."""
import inspect
import os
import re

import pytest
import torch
import yaml

import p2cp_fp64 as Y
from conftest import ROOT, load_golden

SYMBOLS = ["as_p2cp_bwd", "as_p2cp_masked_partials", "as_p2cp_masked_fwd_bwd"]


def test_new_symbols_are_declared_exported_and_bound():
    from artspeech_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    declared = set(re.findall(r"\b(as_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _lib.PROTOTYPES and hasattr(L, name), f"{name} is not bound / exported"
    assert len(_lib.PROTOTYPES["as_p2cp_bwd"][1]) == 21 and len(_lib.PROTOTYPES["as_p2cp_masked_fwd_bwd"][1]) == 13
    assert L.as_p2cp_masked_partials() >= 1
    assert build.SOURCES["p2cp_loss.hip"] == ["-ffp-contract=off"]           # the closest points of the un-contracted forward
    for comment in re.findall(r"/\*(?:(?!\*/).)*\*/\s*(?:int32_t as_p2cp_masked_partials\(void\);\s*)?int as_p2cp_(?:bwd|masked_fwd_bwd)\(",
                              header, flags=re.S):
        assert "metrics.py:27-46" in comment                                  # the prototypes cite their reference lines
    assert header.count("metrics.py:27-46") >= 3


def test_limits_are_refused_on_the_host():
    """Point counts beyond 256 are refused before any launch, so this needs no GPU."""
    from artspeech_amd import _lib
    L = _lib.lib()
    assert L.as_p2cp_bwd(None, 0, 0, 0, 257, None, 0, 0, 0, 4, 1, None, None, 0, 0, 0, None, 0, 0, 0, None) == -2
    assert b"as_p2cp_bwd" in L.as_last_error()
    assert L.as_p2cp_bwd(None, 0, 0, 0, 4, None, 0, 0, 0, 4, 1, None, None, 0, 0, 0, None, 0, 0, 0, None) == -1   # null pointers


def test_new_config_binds_to_main_and_an_unknown_loss_raises_without_a_gpu():
    import train_phoneme_to_articulation as trainer
    path = os.path.join(ROOT, "configs", "train_p2cp_synthetic.yaml")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    bound = inspect.signature(trainer.main).bind(**cfg)                       # every key is an argument of main()
    assert bound.arguments["loss"] == "p2cp" and bound.arguments["datadir"] == "synthetic"
    params = inspect.signature(trainer.main).parameters
    assert list(params)[-1] == "loss" and params["loss"].default == "euclidean"
    with pytest.raises(ValueError, match="'euclidean' or 'p2cp'.*chamfer"):   # before the device is touched
        trainer.main(**dict(cfg, loss="chamfer"))


def test_cpu_tensors_fail_loudly():
    from artspeech_amd.phoneme_to_articulation.metrics import MeanP2CPDistance, masked_p2cp_loss
    with pytest.raises(RuntimeError, match="no CPU path"):
        MeanP2CPDistance("mean")(torch.rand(2, 5, 2).requires_grad_(), torch.rand(2, 5, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        masked_p2cp_loss(torch.rand(1, 2, 1, 2, 5), torch.rand(1, 2, 1, 2, 5), [2])


def test_fp64_yardstick_agrees_with_the_reference_fixture():
    """At 20 x 25 points torch.cdist takes direct differences: the reference's own gradient is the float64 direct formula to
    rounding, the coincident pair contributes nothing and the exact tie goes to the lowest index."""
    z = load_golden("p2cp_grad")
    u, v, dout = (torch.from_numpy(z[k]) for k in ("u", "v", "dout"))
    assert u.shape == (12, 20, 2) and v.shape == (12, 25, 2) and u.dtype == torch.float32 and bool((dout == 0).any())
    val, du, dv = Y.value_and_grads(u, v, dout)
    keep = torch.ones(12, dtype=torch.bool)
    keep[int(z["tie"])] = bool(z["tie_lowest"])
    scale = float(du.abs().max())
    assert float((du - torch.from_numpy(z["du"]).double())[keep].abs().max()) < 1e-6 * scale
    assert float((dv - torch.from_numpy(z["dv"]).double())[keep].abs().max()) < 1e-6 * scale
    assert float((val - torch.from_numpy(z["value"]).double()).abs().max()) < 1e-6
    c, t = int(z["coincident"]), int(z["tie"])
    assert torch.equal(u[c, 4], v[c, 7]) and torch.isfinite(du[c]).all()
    dec = Y.decided(u, v)
    assert not dec[c] and not dec[t] and int(dec.sum()) == 10                 # the two convention tiles are the undecided ones
    # the tie: u_3's row term goes to v_5 (index 5 < 9), so v_9 keeps only its own column term of 1 / (2 M)
    assert dv[t, 9].tolist() == pytest.approx([-dout[t].item() / 50, 0.0], abs=1e-12)
    assert dv[t, 5].tolist() == pytest.approx([dout[t].item() * (1 / 50 + 1 / 40), 0.0], abs=1e-12)
