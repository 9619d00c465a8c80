"""GPU tests of the incremental PCA fit (artspeech_amd/csrc/pca.hip, principal_components/pca.py, train_articulatory_PCA.py)
against the float64 yardstick tests/pca_fp64.py and the fixture written by the reference's own trainer code.

Bound of every fitted quantity: max(4 x d_ref, 8 fp32 ulps of the quantity's scale), d_ref being the distance of the yardstick's
float32 run from its float64 run on the same inputs (two backward-stable fp32 orderings differ by small multiples of it, a method
that squares the condition number in fp32 by about 20 x; the floor is there because the results are stored in fp32).  mean_ and
var_ are float64 state: 1e-12 relative.  Every parity test first asserts that the yardstick's relative eigenvalue gap is >= 1e-4,
a condition on the inputs.  The observed worst ratios (error / bound) are written to profiles/pca_fit_parity.json.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from pca_fp64 import IncrementalPCAYardstick

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
ATTRS = ("components_", "singular_values_", "explained_variance_", "explained_variance_ratio_", "noise_variance_")
WORST = {}
THESIS = {"arytenoid-cartilage": 4, "epiglottis": 3, "lower-incisor": 3, "lower-lip": 4, "pharynx": 2, "soft-palate-midline": 3,
          "thyroid-cartilage": 2, "tongue": 8, "upper-lip": 4, "vocal-folds": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_worst_ratios():
    yield
    out = os.path.join(ROOT, "profiles")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "pca_fit_parity.json"), "w") as f:
            json.dump({k: float(f"{v:.3e}") for k, v in sorted(WORST.items())}, f, indent=1)
    except OSError:
        pass


def _frames(N, A, F, seed, rank=24):
    from artspeech_amd.phoneme_to_articulation.principal_components.dataset import low_rank_frames
    return low_rank_frames(N, A, F, rank, torch.Generator().manual_seed(seed)).float()


def _yardsticks(x, ks, b, order=None):
    """per articulator (float64 run, float32 run) of the chain over x (N, A, F) numpy float32"""
    runs = []
    for a, k in enumerate(ks):
        y64 = IncrementalPCAYardstick(k).fit(x[:, a], b, order)
        y32 = IncrementalPCAYardstick(k, dtype=np.float32).fit(x[:, a], b, order)
        runs.append((y64, y32))
    return runs


def _scale(name, want):
    return 1.0 if name == "components_" else max(float(np.abs(want).max()), 1e-300)   # components are unit vectors


def _check_attrs(got, y64, y32, label):
    """got: {attribute: numpy array} of one articulator; asserts every quantity's bound and records error / bound"""
    assert y64.eigenvalue_gap() >= 1e-4, f"{label}: ill-conditioned inputs (gap {y64.eigenvalue_gap():.2e})"
    for name in ATTRS:
        want, ref32 = np.asarray(getattr(y64, name), np.float64), np.asarray(getattr(y32, name), np.float64)
        have = np.asarray(got[name], np.float64)
        assert have.shape == want.shape, (label, name, have.shape, want.shape)
        d_ref = float(np.abs(ref32 - want).max()) if want.size else 0.0
        bound = max(4.0 * d_ref, 8.0 * EPS32 * _scale(name, want))
        err = float(np.abs(have - want).max()) if want.size else 0.0
        ratio = err / bound
        WORST[name] = max(WORST.get(name, 0.0), ratio)
        print(f"{label}: {name} err {err:.3e} d_ref {d_ref:.3e} bound {bound:.3e} ratio {ratio:.3f}")
        assert err <= bound, f"{label}: {name} off by {err:.3e}, bound {bound:.3e} (d_ref {d_ref:.3e})"
    for name in ("mean_", "var_"):
        want, have = np.asarray(getattr(y64, name)), np.asarray(got[name])
        assert have.dtype == np.float64
        rel = float((np.abs(have - want) / np.abs(want)).max())
        WORST[name] = max(WORST.get(name, 0.0), rel / 1e-12)
        print(f"{label}: {name} rel {rel:.3e}")
        assert rel <= 1e-12, f"{label}: {name} off by {rel:.3e} relative"
    comps = np.asarray(got["components_"])
    lead = comps[np.arange(comps.shape[0]), np.abs(comps).argmax(axis=1)]
    assert (lead > 0).all(), f"{label}: a component's largest-magnitude entry is negative"
    assert got["n_samples_seen_"] == y64.n_samples_seen_


def _attrs(pca, articulator):
    out = {n: getattr(pca, n)[articulator].cpu().numpy() for n in ATTRS + ("mean_", "var_")}
    for n in ATTRS:
        assert out[n].dtype == np.float32, n
    out["n_samples_seen_"] = pca.n_samples_seen_
    return out


def _fit_and_check(x, comps, b, dev, label, order=None):
    from artspeech_amd.phoneme_to_articulation.principal_components.pca import MultiArticulatorPCA
    pca = MultiArticulatorPCA(comps, b)
    pca.fit(x.to(dev), None if order is None else torch.as_tensor(order).to(dev))
    names = sorted(comps)
    runs = _yardsticks(x.numpy(), [comps[a] for a in names], b, order)
    for a, (y64, y32) in zip(names, runs):
        _check_attrs(_attrs(pca, a), y64, y32, f"{label} {a}")
    return pca, runs


SHAPES = [(4096, 100, 12, 256), (4000, 100, 8, 256), (1024, 100, 8, 8), (640, 20, 4, 32), (4096, 100, 2, 256), (2048, 100, 12, 100),
          (1000, 100, 12, 13)]


@pytest.mark.parametrize("N,F,k,b", SHAPES)
def test_fit_matches_the_fp64_yardstick(N, F, k, b, dev):
    comps = {"tongue": k, "lower-lip": max(1, k // 2), "pharynx": max(1, k - 1)}
    x = _frames(N, 3, F, seed=N + F + k + b)
    order = np.random.default_rng(N + b).permutation(N)
    _fit_and_check(x, comps, b, dev, f"N{N} F{F} k{k} b{b}", order)


def test_thesis_shape_matches_the_fp64_yardstick(dev):
    x = _frames(4096, 10, 100, seed=7)
    _fit_and_check(x, THESIS, 256, dev, "thesis")
    _fit_and_check(x[:1024], THESIS, 8, dev, "thesis b8")


def test_fixture_of_the_reference_is_reproduced(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.pca import MultiArticulatorPCA
    g = load_golden("pca_fit")
    for case in range(int(g["n_cases"])):
        pre = f"c{case}."
        N, A, F, b, seed, rank = (int(v) for v in g[pre + "shape"])
        names = [str(s) for s in g[pre + "articulators"]]            # the reference's dict order
        ks = [int(v) for v in g[pre + "k"]]
        comps = dict(zip(names, ks))
        x = _frames(N, A, F, seed, rank)
        order = g[pre + "order"]
        pca = MultiArticulatorPCA(comps, b).fit(x.to(dev), torch.from_numpy(order).to(dev))
        runs = dict(zip(sorted(comps), _yardsticks(x.numpy(), [comps[a] for a in sorted(comps)], b, order)))
        for a in names:
            y64, y32 = runs[a]
            assert y64.eigenvalue_gap() >= 1e-4
            got = _attrs(pca, a)
            for name in ATTRS:
                want = np.asarray(g[f"{pre}{a}.{name}"], np.float64)
                d_ref = float(np.abs(np.asarray(getattr(y32, name), np.float64) - np.asarray(getattr(y64, name), np.float64)).max())
                bound = max(4.0 * d_ref, 8.0 * EPS32 * _scale(name, want))
                err = float(np.abs(got[name] - want).max())
                WORST["fixture " + name] = max(WORST.get("fixture " + name, 0.0), err / bound)
                print(f"fixture {case} {a}: {name} err {err:.3e} bound {bound:.3e}")
                assert err <= bound, f"fixture {case} {a}: {name} off by {err:.3e}, bound {bound:.3e}"
            for name in ("mean_", "var_"):
                want = g[f"{pre}{a}.{name}"]
                assert (np.abs(got[name] - want) <= 1e-12 * np.abs(want)).all(), (case, a, name)
        enc, dec = pca.state_dicts()
        for sd, which in ((enc, "enc"), (dec, "dec")):
            keys = [str(s) for s in g[f"{pre}{which}.keys"]]
            assert list(sd) == keys                                  # names and iteration order
            for i, key in enumerate(keys):
                want = g[f"{pre}{which}.{i}"]
                assert tuple(sd[key].shape) == want.shape and sd[key].dtype == torch.float32 and want.dtype == np.float32, key
                a = key.split(".")[1]
                name = "explained_variance_" if key.endswith("eigenvalues") else "components_"
                y64, y32 = runs[a]
                d_ref = float(np.abs(np.asarray(getattr(y32, name), np.float64) - np.asarray(getattr(y64, name), np.float64)).max())
                bound = max(4.0 * d_ref, 8.0 * EPS32 * _scale(name, want))
                assert float(np.abs(sd[key].cpu().numpy().astype(np.float64) - want).max()) <= bound, key
        held = _frames(64, A, F, seed + 1, rank)
        rec = pca.inverse_transform(pca.transform(held.to(dev))).cpu().numpy()
        assert np.abs(rec - g[pre + "reconstruction"]).max() <= 1e-4 * float(np.abs(held.numpy()).max())


def test_fit_equals_the_partial_fit_loop_bit_for_bit(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.pca import IncrementalPCA, MultiArticulatorPCA
    N, b = 4000, 256                                                 # a short last batch of 160 rows
    comps = {"tongue": 8, "lower-lip": 4, "pharynx": 3}
    x = _frames(N, 3, 100, seed=11).to(dev)
    order = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(dev)
    whole = MultiArticulatorPCA(comps, b).fit(x, order)
    loop = MultiArticulatorPCA(comps, b)
    singles = {a: IncrementalPCA(k) for a, k in comps.items()}
    for i in range(0, N, b):
        batch = x[order[i:i + b]]
        loop.partial_fit(batch)
        for j, a in enumerate(sorted(comps)):
            singles[a].partial_fit(batch[:, j])
    assert loop.n_samples_seen_ == whole.n_samples_seen_ == N
    for name in ATTRS + ("mean_", "var_"):
        for a in comps:
            assert torch.equal(getattr(whole, name)[a], getattr(loop, name)[a]), (name, a)
            assert torch.equal(getattr(singles[a], name), getattr(loop, name)[a]), (name, a, "single")
    assert torch.equal(whole._state, loop._state)


def test_reconstruction_and_state_dicts(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models.autoencoder import MultiDecoder, MultiEncoder
    from artspeech_amd.phoneme_to_articulation.principal_components.pca import IncrementalPCA
    comps = {"tongue": 8, "lower-lip": 4, "pharynx": 3}
    names = sorted(comps)
    x = _frames(2048 + 64, 3, 100, seed=5)
    train, held = x[:2048], x[2048:]
    pca, runs = _fit_and_check(train, comps, 256, dev, "reconstruction")
    scale = float(held.abs().max())
    latent = pca.transform(held.to(dev))
    assert latent.shape == (64, pca.latent_size)
    rec = pca.inverse_transform(latent).cpu().numpy()
    for j, (a, (y64, _)) in enumerate(zip(names, runs)):
        z = y64.transform(held[:, j].numpy())
        assert np.abs(latent[:, pca.indices_dict[a]].cpu().numpy() - z).max() <= 1e-4 * scale
        assert np.abs(rec[:, j] - y64.inverse_transform(z)).max() <= 1e-4 * scale
    enc_sd, dec_sd = pca.state_dicts()
    enc = MultiEncoder(comps, 100, 50, encoder_cls="PCA")
    dec = MultiDecoder(comps, 100, 50, decoder_cls="PCA")
    enc.load_state_dict(enc_sd, strict=True)
    dec.load_state_dict(dec_sd, strict=True)
    enc.to(dev), dec.to(dev)
    with torch.no_grad():
        got = enc(held.to(dev)).cpu().numpy()
    for j, (a, (y64, _)) in enumerate(zip(names, runs)):             # the files hold no mean: projection without centring
        want = held[:, j].numpy().astype(np.float64) @ y64.components_.T
        assert np.abs(got[:, pca.indices_dict[a]] - want).max() <= 1e-4 * scale
    single = IncrementalPCA(8, batch_size=256).fit(train[:, names.index("tongue")].to(dev))
    assert torch.equal(single.components_, pca.components_["tongue"])
    z = single.transform(held[:, names.index("tongue")].to(dev))
    assert z.shape == (64, 8) and single.inverse_transform(z).shape == (64, 100)
    assert np.abs(z.cpu().numpy() - runs[names.index("tongue")][0].transform(held[:, names.index("tongue")].numpy())).max() <= 1e-4 * scale


def test_trainer_end_to_end_feeds_the_phoneme_to_components_trainer(dev, tmp_path):
    import csv

    import yaml

    import train_articulatory_PCA as T
    import train_phoneme_to_principal_components as P2
    with open(os.path.join(ROOT, "configs", "train_articulatory_pca_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["results_dir"] = str(tmp_path / "pca")
    info = T.main(**cfg)
    for name in ("best_encoders.pt", "best_decoders.pt", "reconstruction_errors.csv", "reconstruction_errors_agg.csv"):
        assert os.path.exists(os.path.join(cfg["results_dir"], name)), name
    with open(os.path.join(cfg["results_dir"], "reconstruction_errors.csv")) as f:
        rows = list(csv.reader(f))
    articulators = sorted(cfg["model_params"]["indices_dict"])
    assert rows[0] == ["subject", "sequence", "frame"] + articulators
    assert len(rows) - 1 == cfg["test_seq_dict"]["num_frames"] == info["num_test_frames"]
    assert all(np.isfinite(float(v)) and float(v) >= 0 for r in rows[1:] for v in r[3:])
    with open(os.path.join(ROOT, "configs", "train_pc_based_synthetic.yaml")) as f:
        cfg2 = yaml.safe_load(f)
    cfg2["num_epochs"] = 1
    cfg2["results_dir"] = str(tmp_path / "pc")
    cfg2["indices_dict"] = dict(cfg["model_params"]["indices_dict"])
    cfg2["autoencoder_kwargs"]["in_features"] = cfg["model_params"]["in_features"]
    cfg2["encoder_type"] = cfg2["decoder_type"] = "PCA"
    cfg2["encoder_state_dict_filepath"] = os.path.join(cfg["results_dir"], "best_encoders.pt")
    cfg2["decoder_state_dict_filepath"] = os.path.join(cfg["results_dir"], "best_decoders.pt")
    out = P2.main(**cfg2)
    losses = [h["train"]["loss"] for h in out["history"]]
    assert len(losses) == 1 and np.isfinite(losses[0])


def _draw(rng):
    A = int(rng.integers(1, 11))
    F = int(rng.integers(8, 257))
    ks = [int(rng.integers(1, min(12, F // 2) + 1)) for _ in range(A)]
    b = int(rng.integers(max(ks), 400))
    N = int(rng.integers(max(4 * b, 512), 4097))
    return A, F, ks, b, N, int(rng.integers(0, 2 ** 31 - 1))


@pytest.mark.parametrize("seed", range(int(os.environ.get("AS_FUZZ_SEEDS", "10"))))
def test_random_configurations_vs_the_fp64_yardstick(seed, dev):
    """A in 1..10, F in 8..256 (odd values included), k in 1..min(12, F // 2) per articulator, b in k..399 (smaller and larger than
    F), N in max(4 b, 512)..4096 (ragged tails).  A draw whose yardstick gap is below 1e-4 is redrawn, at most one in five."""
    rng = np.random.default_rng(1000 + seed)
    redraws = _REDRAWS
    while True:
        A, F, ks, b, N, s = _draw(rng)
        x = _frames(N, A, F, s)
        order = rng.permutation(N)
        comps = {f"a{i:02d}": k for i, k in enumerate(ks)}
        gaps = [IncrementalPCAYardstick(k).fit(x[:, i].numpy(), b, order).eigenvalue_gap() for i, k in enumerate(ks)]
        if min(gaps) >= 1e-4:
            break
        redraws.append(seed)
        assert len(redraws) <= max(1, int(os.environ.get("AS_FUZZ_SEEDS", "10")) // 5), f"too many ill-conditioned draws: {redraws}"
    _fit_and_check(x, comps, b, dev, f"draw {seed}: A{A} F{F} b{b} N{N}", order)


_REDRAWS = []
