"""Fixture of the principal-components evaluation, produced by the reference's own CPU code
(phoneme_to_articulation/principal_components/evaluation.py, test_principal_components_autoencoder.py and the signature of
test_phoneme_to_principal_components.py).  Run from the repository root with the reference checkout at make_golden.REF:

    python tests/golden/make_golden_pc_eval.py

Writes tests/golden/pc_eval.npz.  Uses make_golden.py's name-only shims plus empty ``seaborn`` / ``matplotlib.pyplot``; the
reference's plot functions (plot_cov_matrix, plot_nomograms, plot_latent_space_distribution) are stubbed to no-ops and its data
set class is replaced by an in-script one that yields the fixture's frames.  All weights are random (untrained), so the
reconstructions are not close to the targets.

Two cases, because the reference fixes 50 points per contour in evaluate_autoencoder (``reshape(bs, n_articulators, 2, 50)``) and
the tract variables need 50 points and the five articulators they are measured between:
  small  ARTS / N = 10 / HIDDEN = 10 / COMPS of make_golden_pc_training.py, 37 frames in batches of 8:
         run_multiart_autoencoder_test (info, the covariance per articulator and the whole matrix)
  full   the five tract-variable articulators, N = 50, HIDDEN = 10, 37 frames in batches of 8: evaluate_autoencoder (the four
         tables), and run_phoneme_to_principal_components_test on 4 sentences of lengths 9, 5, 5, 1 in batches of 2 with outputs_dir
         (info, the dumped contours and tract_variables.csv of the 9-frame sentence)
At generation time the reference's mm errors are asserted to lie within 1e-3 (relative, per element) of the fp64 direct-difference
restatement tests/pc_eval_fp64.py fed the reference's own reconstructions; the measured figure is stored in the file."""
import csv
import json
import os
import sys
import tempfile
import types

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import pc_eval_fp64 as Y  # noqa: E402
from make_golden import _load, _shim, save, sd_to_np  # noqa: E402
from make_golden_pc_training import ARTS, COMPS, HIDDEN, N, _signature, load_reference  # noqa: E402

TV_ARTS = ["lower-lip", "pharynx", "soft-palate-midline", "tongue", "upper-lip"]   # sorted; the upper incisor is injected
N_FULL = 50
COMPS_FULL = {"lower-lip": 3, "pharynx": 2, "soft-palate-midline": 2, "tongue": 4, "upper-lip": 2}
FRAMES, BATCH = 37, 8
SENT_LENGTHS = [9, 5, 5, 1]
SEED = 131


def load_harnesses(dataset):
    """evaluation.py and test_principal_components_autoencoder.py imported as they are, behind name-only shims."""
    plt = _shim("matplotlib.pyplot")
    _shim("matplotlib", pyplot=plt)
    _shim("seaborn")
    _shim("ujson", dump=json.dump, load=json.load)
    sys.modules["vt_tools"].COLORS = {}
    _shim("vt_shape_gen")
    _shim("vt_shape_gen.helpers", load_articulator_array=None)
    _shim("vt_tools.bs_regularization", regularize_Bsplines=None)
    _shim("phoneme_to_articulation.tail_clipper", TailClipper=None)
    _load("tract_variables", "tract_variables.py")
    ref_init = _load("ref_p2a_init_for_pc_eval", "phoneme_to_articulation/__init__.py")
    pkg = sys.modules["phoneme_to_articulation"]
    pkg.save_outputs, pkg.tract_variables = ref_init.save_outputs, ref_init.tract_variables
    pkg.REQUIRED_ARTICULATORS_FOR_TVS, pkg.RNNType = ref_init.REQUIRED_ARTICULATORS_FOR_TVS, ref_init.RNNType
    ref_eval = _load("phoneme_to_articulation.principal_components.evaluation",
                     "phoneme_to_articulation/principal_components/evaluation.py")
    ref_eval.plot_cov_matrix = lambda *a, **k: None
    sys.modules["phoneme_to_articulation.principal_components.dataset"] = dataset
    rnn = _load("phoneme_to_articulation.principal_components.models.rnn", "phoneme_to_articulation/principal_components/models/rnn.py")
    ref_test = _load("ref_test_pc_autoencoder", "test_principal_components_autoencoder.py")
    ref_test.plot_nomograms = lambda *a, **k: None
    ref_test.plot_latent_space_distribution = lambda *a, **k: None
    ref_test.sequences_from_dict = lambda datadir, seq_dict: []
    return ref_eval, ref_test, rnn


class FixtureFrames(torch.utils.data.Dataset):
    """Stand-in of PrincipalComponentsAutoencoderDataset2 with its constructor's keywords and item layout."""
    frames = weights = normalize = None

    def __init__(self, database_name=None, datadir=None, sequences=None, articulators=None, clip_tails=True):
        self.articulators = articulators

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return f"sub{1 + i // 20}_S{1 + i % 3}_{i:04d}", self.frames[i].clone(), self.weights[i], "a"


class _Loader:
    def __init__(self, batches, **dataset_attrs):
        self.batches, self.dataset = batches, types.SimpleNamespace(**dataset_attrs)

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _normalizers(transforms, arts, n, g):
    return {a: transforms.Normalize(torch.rand(2, n, generator=g) * 0.2, 0.5 + torch.rand(2, n, generator=g)) for a in arts}


def _norm_arrays(prefix, norm, arts):
    return {prefix + "norm_mean": np.stack([norm[a].mean.numpy() for a in arts]),
            prefix + "norm_std": np.stack([norm[a].std.numpy() for a in arts])}


def gen_small(settings, transforms, ae, losses, ref_eval, arrays, checks):
    torch.manual_seed(SEED)
    g = torch.Generator().manual_seed(SEED)
    model = ae.MultiArticulatorAutoencoder(in_features=2 * N, indices_dict=COMPS, hidden_features=HIDDEN)
    FixtureFrames.frames = torch.rand(FRAMES, len(ARTS), 2 * N, generator=g)
    FixtureFrames.weights = torch.rand(FRAMES, generator=g)
    FixtureFrames.normalize = _normalizers(transforms, ARTS, N, g)
    loader = torch.utils.data.DataLoader(FixtureFrames(articulators=ARTS), batch_size=BATCH, shuffle=False)
    crit = losses.RegularizedLatentsMSELoss2(alpha=0.1, indices_dict=model.indices_dict)
    cfg = settings.DATASET_CONFIG["artspeech2"]
    with tempfile.TemporaryDirectory() as d:
        info = ref_eval.run_multiart_autoencoder_test(0, model, loader, crit, cfg, plots_dir=d, indices_dict=model.indices_dict,
                                                      device=torch.device("cpu"))
        blocks = {a: np.load(os.path.join(d, f"covariance_matrix_{a}.npy")) for a in model.indices_dict}
        info2 = ref_eval.run_multiart_autoencoder_test(0, model, loader, crit, cfg, plots_dir=d, device=torch.device("cpu"))
        cov = np.load(os.path.join(d, "covariance_matrix.npy"))
    assert info == info2 and set(info) == {"loss"}
    with torch.no_grad():
        _, latents = model(FixtureFrames.frames)
    p = "small."
    arrays.update(sd_to_np(p + "w.", model.state_dict()))
    arrays.update(_norm_arrays(p, FixtureFrames.normalize, ARTS))
    arrays.update({p + "frames": FixtureFrames.frames.numpy(), p + "weights": FixtureFrames.weights.numpy(),
                   p + "latents": latents.numpy(), p + "loss": np.float64(info["loss"]), p + "cov": cov,
                   p + "articulators": np.array(ARTS), p + "comps_names": np.array(list(COMPS)),
                   p + "comps": np.array(list(COMPS.values()))})   # in the dict's order, which fixes the latent indices
    arrays.update({p + f"cov.{a}": b for a, b in blocks.items()})
    checks["small"] = dict(seed=SEED, loss=float(info["loss"]), cov_trace=float(np.trace(cov)))


def gen_full_autoencoder(settings, helpers, transforms, ae, ref_test, tmp, arrays, checks):
    torch.manual_seed(SEED + 1)
    g = torch.Generator().manual_seed(SEED + 1)
    indices = helpers.make_indices_dict(COMPS_FULL)
    params = {"in_features": 2 * N_FULL, "indices_dict": indices, "hidden_features": HIDDEN}
    model = ae.MultiArticulatorAutoencoder(**params)
    enc_path, dec_path = os.path.join(tmp, "enc.pt"), os.path.join(tmp, "dec.pt")
    torch.save(model.encoders.state_dict(), enc_path)
    torch.save(model.decoders.state_dict(), dec_path)
    FixtureFrames.frames = torch.rand(FRAMES, len(TV_ARTS), 2 * N_FULL, generator=g)
    FixtureFrames.weights = torch.rand(FRAMES, generator=g)
    FixtureFrames.normalize = _normalizers(transforms, TV_ARTS, N_FULL, g)
    frames_in = FixtureFrames.frames.clone()   # the reference denormalises the batch it is handed in place
    ref_test.PrincipalComponentsAutoencoderDataset2 = FixtureFrames
    cfg = settings.DATASET_CONFIG["artspeech2"]
    save_to = os.path.join(tmp, "eval")
    with torch.no_grad():
        ref_test.evaluate_autoencoder("artspeech2", tmp, cfg, BATCH, {}, params, enc_path, dec_path, save_to)
        recon, latents = model(frames_in)
    latent_csv = pd.read_csv(os.path.join(save_to, "latent_space.csv"))
    errors = np.load(os.path.join(save_to, "reconstruction_errors.npy"))
    errors_csv = pd.read_csv(os.path.join(save_to, "reconstruction_errors.csv"), dtype={"frame": str})
    agg_csv = pd.read_csv(os.path.join(save_to, "reconstruction_errors_agg.csv"))
    assert list(errors_csv.columns) == ["subject", "sequence", "frame"] + TV_ARTS and list(agg_csv.columns) == ["index"] + TV_ARTS
    assert list(agg_csv["index"]) == ["mean", "std", "median", "min", "max"]
    to_mm = cfg.PIXEL_SPACING * cfg.RES
    norm = _norm_arrays("", FixtureFrames.normalize, TV_ARTS)
    _, _, yard = Y.shapes_eval(recon.numpy(), frames_in.numpy(), norm["norm_mean"], norm["norm_std"], to_mm)
    rel = float((np.abs(errors - yard) / yard).max())
    assert rel <= 1e-3, f"the reference's mm errors are {rel:.2e} from the fp64 restatement: change SEED, not the bound"
    p = "full."
    arrays.update(sd_to_np(p + "enc.", model.encoders.state_dict()))
    arrays.update(sd_to_np(p + "dec.", model.decoders.state_dict()))
    arrays.update(_norm_arrays(p, FixtureFrames.normalize, TV_ARTS))
    arrays.update({p + "frames": frames_in.numpy(), p + "weights": FixtureFrames.weights.numpy(), p + "recon": recon.numpy(),
                   p + "latents": latents.numpy(), p + "articulators": np.array(TV_ARTS),
                   p + "comps_names": np.array(list(COMPS_FULL)), p + "comps": np.array(list(COMPS_FULL.values())), p + "to_mm": np.float64(to_mm),
                   p + "latent_columns": np.array(list(latent_csv.columns)), p + "latent_space": latent_csv.to_numpy(np.float64),
                   p + "errors": errors, p + "errors_csv_names": errors_csv[["subject", "sequence", "frame"]].to_numpy(str),
                   p + "errors_csv": errors_csv[TV_ARTS].to_numpy(np.float64), p + "agg_index": np.array(list(agg_csv["index"])),
                   p + "agg": agg_csv[TV_ARTS].to_numpy(np.float64), p + "errors_vs_fp64": np.float64(rel)})
    checks["full_autoencoder"] = dict(seed=SEED + 1, errors_vs_fp64=rel, mean_error_mm=float(errors.mean()))
    return model, enc_path, dec_path, indices


def gen_sentences(settings, transforms, losses, metrics, dataset, ref_eval, rnn, enc_path, dec_path, indices, tmp, arrays, checks):
    torch.manual_seed(SEED + 2)
    g = torch.Generator().manual_seed(SEED + 2)
    V, A = 12, len(TV_ARTS)
    norm = _normalizers(transforms, TV_ARTS, N_FULL, g)
    TVs = ["LA", "TTCD"]
    items = []
    for i, l in enumerate(SENT_LENGTHS):
        items.append((f"sent{i}", torch.randint(2, V, (l,), generator=g), torch.rand(l, A, 2, N_FULL, generator=g),
                      [f"ph{int(t)}" for t in torch.randint(0, 9, (l,), generator=g)],
                      (torch.rand(len(TVs), l, generator=g) > 0.5).int(), torch.rand(l, 1, 2, N_FULL, generator=g),
                      [f"{1000 * i + j:04d}" for j in range(l)], (torch.rand(l, generator=g) > 0.5).float()))
    batches = [dataset.pad_sequence_collate_fn(items[:2]), dataset.pad_sequence_collate_fn(items[2:])]
    loader = _Loader(batches, articulators=list(TV_ARTS), normalize=norm)
    model = rnn.PrincipalComponentsArtSpeech(V, COMPS_FULL, embed_dim=16, hidden_size=32)
    cfg = settings.DATASET_CONFIG["artspeech2"]
    kwargs = {"in_features": 2 * N_FULL, "hidden_features": HIDDEN}
    denorm = {a: n.inverse for a, n in norm.items()}
    crit = losses.AutoencoderLoss2(indices, TVs, 2 * N_FULL, HIDDEN, enc_path, dec_path, "cpu", denormalize_fn=denorm, beta1=0.7,
                                   beta2=1.3, beta3=0.4)
    metric = metrics.DecoderMeanP2CPDistance2(cfg, dec_path, indices, kwargs, denorm, "cpu")
    # the reference's metric denormalises the targets it is given in place, which would reach the dumps: it gets a copy
    fn_metrics = {"p2cp_mean": lambda outputs, targets, lengths: metric(outputs, targets.clone(), lengths)}
    out_dir = os.path.join(tmp, "sentences")
    info = ref_eval.run_phoneme_to_principal_components_test(3, model, loader, crit, fn_metrics=fn_metrics, outputs_dir=out_dir,
                                                             decode_transform=crit.decode, device=torch.device("cpu"))
    tv_arts = sorted(TV_ARTS + ["upper-incisor"])
    sdir = os.path.join(out_dir, "3", "sent0")
    with open(os.path.join(sdir, "tract_variables.csv")) as f:
        rows = list(csv.reader(f))
    tv_cols, tv_rows = rows[0], rows[1:]
    num = [c for c in tv_cols if c not in ("sentence", "frame", "phoneme")]
    with open(os.path.join(sdir, "phonemes.csv")) as f:
        ph_rows = list(csv.reader(f))
    frames0 = items[0][6]
    pred = np.stack([[np.load(os.path.join(sdir, "contours", f"{fr}_{a}.npy")) for a in tv_arts] for fr in frames0])
    true = np.stack([[np.load(os.path.join(sdir, "contours", f"{fr}_{a}_true.npy")) for a in tv_arts] for fr in frames0])
    p = "sent."
    arrays.update(sd_to_np(p + "w.", model.state_dict()))
    arrays.update(_norm_arrays(p, norm, TV_ARTS))
    for i, it in enumerate(items):
        arrays.update({p + f"in{i}.tokens": it[1].numpy(), p + f"in{i}.targets": it[2].numpy(), p + f"in{i}.phonemes": np.array(it[3]),
                       p + f"in{i}.mask": it[4].numpy(), p + f"in{i}.ref": it[5].numpy(), p + f"in{i}.frames": np.array(it[6]),
                       p + f"in{i}.voicing": it[7].numpy()})
    arrays.update({p + "cfg": np.array([V, 16, 32], dtype=np.int64), p + "TVs": np.array(TVs), p + "betas": np.array([0.7, 1.3, 0.4]),
                   p + "loss": np.float64(info["loss"]), p + "p2cp_mean": np.float64(info["p2cp_mean"]),
                   p + "tv_articulators": np.array(tv_arts), p + "contours_pred": pred, p + "contours_true": true,
                   p + "contour_files": np.array(sorted(os.listdir(os.path.join(sdir, "contours")))),
                   p + "sentence_dirs": np.array(sorted(os.listdir(os.path.join(out_dir, "3")))),
                   p + "phonemes_csv": np.array(ph_rows), p + "tv_columns": np.array(tv_cols), p + "tv_numeric_columns": np.array(num),
                   p + "tv_values": np.array([[float(r[tv_cols.index(c)]) for c in num] for r in tv_rows], dtype=np.float64),
                   p + "tv_frames": np.array([r[tv_cols.index("frame")] for r in tv_rows])})
    checks["sentences"] = dict(seed=SEED + 2, loss=float(info["loss"]), p2cp_mean=float(info["p2cp_mean"]))


def main():
    settings, _, transforms, ae, losses, metrics, dataset, _ = load_reference()
    helpers = sys.modules["helpers"]
    ref_eval, ref_test, rnn = load_harnesses(dataset)
    arrays, checks = {}, {}
    gen_small(settings, transforms, ae, losses, ref_eval, arrays, checks)
    with tempfile.TemporaryDirectory() as tmp:
        _, enc_path, dec_path, indices = gen_full_autoencoder(settings, helpers, transforms, ae, ref_test, tmp, arrays, checks)
        gen_sentences(settings, transforms, losses, metrics, dataset, ref_eval, rnn, enc_path, dec_path, indices, tmp, arrays, checks)
    sigs = {"autoencoder": _signature("test_principal_components_autoencoder.py"),
            "method": _signature("test_phoneme_to_principal_components.py")}
    arrays["signatures"] = np.array(json.dumps(sigs))
    arrays["checks"] = np.array(json.dumps(checks))
    save("pc_eval", **arrays)
    print(json.dumps(checks, indent=1))


if __name__ == "__main__":
    main()
