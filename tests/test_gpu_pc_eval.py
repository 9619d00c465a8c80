"""GPU checks of the principal-components evaluation: the two kernels of csrc/pc_eval.hip against torch (bit-exact
denormalisation), the fp64 yardstick tests/pc_eval_fp64.py and numpy's moments; the two test loops and evaluate_autoencoder
against the fixture recorded from the reference's own functions (tests/golden/make_golden_pc_eval.py); both entry points end to
end from the synthetic configs."""
import csv
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import pc_eval_fp64 as Y
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AS_ERR_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_golden("pc_eval")


def _rel(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}


def _normalize(g, prefix, arts):
    from artspeech_amd.phoneme_to_articulation.transforms import Normalize
    return {a: Normalize(torch.from_numpy(g[prefix + "norm_mean"][i]), torch.from_numpy(g[prefix + "norm_std"][i]))
            for i, a in enumerate(arts)}


# ------------------------------------------------------------------------------------------------ 1. as_pc_shapes_eval
def _case(rows_shape, A, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    shapes = (torch.rand(*rows_shape, A, 2 * N, generator=g) * 2 - 0.5).to(dev)
    targets = torch.rand(*rows_shape, A, 2, N, generator=g).to(dev)
    mean = (torch.rand(A, 2, N, generator=g) * 0.5).to(dev)
    std = (0.1 + 0.2 * torch.rand(A, 2, N, generator=g)).to(dev)
    reference = torch.rand(*rows_shape, 1, 2, N, generator=g).to(dev)
    return shapes, targets, mean, std, reference


def _check_shapes_eval(shapes, targets, mean, std, reference, ref_idx, to_mm, lengths, what):
    """bit-equal contours (torch's x * std + mean on the same tensors, reference channel in place, zeros on invalid rows) and
    errors within 2e-6 (max error over max reference) of the fp64 yardstick fed the device's own fp32 contours."""
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import pc_shapes_eval
    A, N = mean.shape[0], mean.shape[2]
    pred, tgt, err = pc_shapes_eval(shapes, targets, mean, std, to_mm=to_mm, lengths=lengths, reference=reference, ref_idx=ref_idx)
    want_pred = shapes.reshape(*shapes.shape[:-1], 2, N) * std + mean
    want_tgt = targets * std + mean
    if ref_idx >= 0:
        want_pred = torch.cat([want_pred[..., :ref_idx, :, :], reference, want_pred[..., ref_idx:, :, :]], dim=-3)
        want_tgt = torch.cat([want_tgt[..., :ref_idx, :, :], reference, want_tgt[..., ref_idx:, :, :]], dim=-3)
    valid = None
    if lengths is not None:
        valid = (torch.arange(shapes.shape[1])[None, :] < torch.as_tensor(lengths)[:, None]).to(shapes.device)
        want_pred = want_pred * valid[..., None, None, None]
        want_tgt = want_tgt * valid[..., None, None, None]
    assert pred.shape == want_pred.shape and err.shape == tuple(shapes.shape[:-1])
    assert torch.equal(pred, want_pred), f"{what}: predictions differ from x * std + mean"
    assert torch.equal(tgt, want_tgt), f"{what}: targets differ from x * std + mean"
    keep = [i for i in range(pred.shape[-3]) if i != ref_idx]
    want_err = Y.p2cp_mm(pred[..., keep, :, :].cpu().numpy(), tgt[..., keep, :, :].cpu().numpy(), to_mm)
    if valid is not None:
        want_err = want_err * valid.cpu().numpy()[..., None]
        assert not err[~valid].any(), f"{what}: errors of invalid rows are not zero"
    rel = _rel(err.cpu().numpy(), want_err)
    print(f"{what}: p2cp_mm max error / max reference = {rel:.2e}")
    assert rel <= 2e-6, (what, rel)


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("N", [7, 10, 50, 64])
def test_shapes_eval_every_row_count_and_reference_position(N, A, dev):
    """rows 1 (one tile per wave), 3 / 4 / 5 (around four tiles per workgroup), 257 (a short last workgroup), with the
    reference contour absent, first, inside and last."""
    for rows in (1, 3, 4, 5, 257):
        shapes, targets, mean, std, reference = _case((rows,), A, N, 1000 * N + 10 * A + rows, dev)
        for ref_idx in sorted({-1, 0, 1, A}):
            _check_shapes_eval(shapes, targets, mean, std, reference, ref_idx, 220.0, None, f"N={N} A={A} rows={rows} ref={ref_idx}")


@pytest.mark.parametrize("N,A", [(10, 3), (50, 1), (64, 3)])
def test_shapes_eval_masks_rows_by_length(N, A, dev):
    B, T = 5, 9
    shapes, targets, mean, std, reference = _case((B, T), A, N, 77 + N, dev)
    for lengths in ([9, 7, 4, 2, 1], [9, 9, 9, 9, 9], [1, 1, 1, 1, 1]):
        for ref_idx in (-1, 1):
            _check_shapes_eval(shapes, targets, mean, std, reference, ref_idx, 1.0, lengths, f"N={N} A={A} lengths={lengths} ref={ref_idx}")


def test_shapes_eval_leaves_its_inputs_alone_and_each_output_is_optional(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import pc_shapes_eval
    shapes, targets, mean, std, reference = _case((4, 6), 3, 10, 5, dev)
    keep = [t.clone() for t in (shapes, targets, mean, std, reference)]
    full = pc_shapes_eval(shapes, targets, mean, std, to_mm=3.0, lengths=[6, 3, 2, 1], reference=reference, ref_idx=2)
    for p in (False, True):
        for t in (False, True):
            for e in (False, True):
                got = pc_shapes_eval(shapes, targets, mean, std, to_mm=3.0, lengths=[6, 3, 2, 1], reference=reference, ref_idx=2,
                                     pred=p, tgt=t, p2cp=e)
                for want, have, asked in zip(full, got, (p, t, e)):
                    assert (have is not None) == asked
                    assert have is None or torch.equal(have, want)
    for before, after in zip(keep, (shapes, targets, mean, std, reference)):
        assert torch.equal(before, after)
    # targets may come flattened, (..., A, 2 N), as the autoencoder's inputs do
    flat = pc_shapes_eval(shapes, targets.reshape(4, 6, 3, 20), mean, std, to_mm=3.0, lengths=[6, 3, 2, 1], reference=reference, ref_idx=2)
    assert all(torch.equal(a, b) for a, b in zip(full, flat))


def test_shapes_eval_refuses_more_than_128_points(dev):
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import pc_shapes_eval
    shapes, targets, mean, std, _ = _case((2,), 1, 129, 3, dev)
    out = torch.full((2, 1), -1.0, device=dev)
    rc = _lib.lib().as_pc_shapes_eval(_lib.ptr(shapes), _lib.ptr(targets), _lib.ptr(mean), _lib.ptr(std), None, 0, None, -1, 2, 1, 129,
                                      C.c_float(1.0), None, None, _lib.ptr(out), _lib.stream_ptr())
    assert rc == AS_ERR_UNSUPPORTED and b"129" in _lib.lib().as_last_error()
    torch.cuda.synchronize()
    assert (out == -1).all(), "nothing may be launched"
    with pytest.raises(RuntimeError, match="at most 128"):
        pc_shapes_eval(shapes, targets, mean, std)
    shapes, targets, mean, std, _ = _case((3,), 2, 128, 4, dev)   # the limit itself
    _check_shapes_eval(shapes, targets, mean, std, None, -1, 1.0, None, "N=128")


def test_shapes_eval_matches_the_reference_fixture(fx, dev):
    """The reference's mm errors (cdist expansion, fp32) of its own reconstructions: 2e-3."""
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import pc_shapes_eval
    t = lambda k: torch.from_numpy(fx[k]).to(dev)   # noqa: E731
    _, _, err = pc_shapes_eval(t("full.recon"), t("full.frames"), t("full.norm_mean"), t("full.norm_std"), to_mm=float(fx["full.to_mm"]))
    rel = _rel(err.cpu().numpy(), fx["full.errors"])
    print(f"p2cp_mm against the reference fixture: {rel:.2e}")
    assert rel <= 2e-3


# ------------------------------------------------------------------------------------------------ 2. as_pc_eval_accumulate
ROWS, ERR_A = 1000, 3
FEEDINGS = {"one batch": [1000], "1 + 7 + 64 + 928": [1, 7, 64, 928], "1000 batches of 1": [1] * 1000}


def _feed(errors, latents, sizes):
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import PCEvalState
    state = PCEvalState(errors.device, n_articulators=errors.shape[1], latent_size=latents.shape[1])
    lo = 0
    for n in sizes:
        state.update(p2cp_mm=errors[lo:lo + n], latents=latents[lo:lo + n])
        lo += n
    assert lo == errors.shape[0]
    return state


@pytest.fixture(scope="module")
def split(dev):
    g = torch.Generator().manual_seed(9)
    errors = (torch.rand(ROWS, ERR_A, generator=g) * 5 + 0.1).to(dev)
    return errors, {L: torch.randn(ROWS, L, generator=g).mul(0.3).add(0.2).to(dev) for L in (1, 12, 64)}


@pytest.mark.parametrize("L", [1, 12, 64])
def test_accumulate_agrees_with_numpy_for_every_feeding_and_repeats_bit_for_bit(L, split, dev):
    errors, latents = split[0], split[1][L]
    e64, x64 = errors.cpu().numpy().astype(np.float64), latents.cpu().numpy().astype(np.float64)
    cov = np.cov(x64, rowvar=False).reshape(L, L)
    for name, sizes in FEEDINGS.items():
        a, b = _feed(errors, latents, sizes), _feed(errors, latents, sizes)
        assert torch.equal(a.errors, b.errors) and torch.equal(a.latents, b.latents), f"{name}: a repeat differs"
        assert float(a.latents[0]) == ROWS and (a.errors[0] == ROWS).all()
        figures = {"cov": _rel(a.covariance().cpu().numpy(), cov), "latent mean": _rel(a.latent_mean().cpu().numpy(), x64.mean(0))}
        stats = {k: v.cpu().numpy() for k, v in a.error_stats().items()}
        figures["error mean"] = _rel(stats["mean"], e64.mean(0))
        figures["error std"] = _rel(stats["std"], e64.std(0, ddof=1))
        print(f"L={L}, {name}: " + ", ".join(f"{k} {v:.1e}" for k, v in figures.items()))
        assert max(figures.values()) <= 1e-11, (name, figures)
        assert np.array_equal(stats["min"], e64.min(0)) and np.array_equal(stats["max"], e64.max(0)), name
        assert np.array_equal(a.covariance().cpu().numpy(), a.covariance().cpu().numpy().T), "the co-moments are not symmetric"


def test_accumulate_keeps_its_digits_when_the_mean_dwarfs_the_spread(dev):
    """Latents 0.999 + 1e-3 z: an fp64 two-pass / Chan accumulation stays near 1e-10; an fp32 accumulator or uncentred sums
    miss by orders of magnitude."""
    g = torch.Generator().manual_seed(10)
    latents = (0.999 + 1e-3 * torch.randn(ROWS, 12, generator=g)).to(dev)
    errors = torch.rand(ROWS, 1, generator=g).to(dev)
    cov = np.cov(latents.cpu().numpy().astype(np.float64), rowvar=False)
    for sizes in ([1000], [64] * 15 + [40], [1] * 1000):
        rel = _rel(_feed(errors, latents, sizes).covariance().cpu().numpy(), cov)
        print(f"ill-conditioned covariance, {len(sizes)} batches: {rel:.1e}")
        assert rel <= 1e-9


def test_accumulate_skips_the_rows_that_lengths_mask_and_either_half_may_be_absent(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import PCEvalState
    g = torch.Generator().manual_seed(11)
    B, T, A, L = 4, 7, 2, 5
    lengths = [7, 3, 1, 5]
    valid = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]
    errors, latents = torch.rand(B, T, A, generator=g), torch.randn(B, T, L, generator=g)
    errors[~valid], latents[~valid] = 1e6, -1e6   # what a padded row may hold must not count
    errors, latents = errors.to(dev), latents.to(dev)
    masked = PCEvalState(dev, A, L)
    masked.update(p2cp_mm=errors, latents=latents, lengths=lengths)
    masked.update(p2cp_mm=errors[:2], latents=latents[:2], lengths=lengths[:2])
    rows_e = torch.cat([errors[valid.to(dev)], errors[:2][valid[:2].to(dev)]])
    rows_l = torch.cat([latents[valid.to(dev)], latents[:2][valid[:2].to(dev)]])
    dense = _feed(rows_e, rows_l, [rows_e.shape[0]])
    assert float(masked.latents[0]) == rows_e.shape[0] == 26
    assert _rel(masked.covariance().cpu().numpy(), dense.covariance().cpu().numpy()) <= 1e-11
    for k, v in masked.error_stats().items():
        assert _rel(v.cpu().numpy(), dense.error_stats()[k].cpu().numpy()) <= 1e-11, k
    only_e, only_l = PCEvalState(dev, n_articulators=A), PCEvalState(dev, latent_size=L)
    only_e.update(p2cp_mm=errors, lengths=lengths)
    only_l.update(latents=latents, lengths=lengths)
    both = PCEvalState(dev, A, L)
    both.update(p2cp_mm=errors, latents=latents, lengths=lengths)
    assert torch.equal(only_e.errors, both.errors) and torch.equal(only_l.latents, both.latents)
    empty = PCEvalState(dev, A, L)
    empty.update(p2cp_mm=errors[:1], latents=latents[:1], lengths=[0])   # a batch without a valid row changes nothing
    assert not empty.errors.any() and not empty.latents.any()


def test_accumulate_refuses_more_than_64_latents(dev):
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import PCEvalState
    latents = torch.rand(8, 65, device=dev)
    state = torch.zeros(1 + 65 + 65 * 65, dtype=torch.float64, device=dev)
    rc = _lib.lib().as_pc_eval_accumulate(None, 0, None, _lib.ptr(latents), 65, _lib.ptr(state), 8, None, 0, _lib.stream_ptr())
    assert rc == AS_ERR_UNSUPPORTED and b"65" in _lib.lib().as_last_error()
    torch.cuda.synchronize()
    assert not state.any(), "nothing may be launched"
    with pytest.raises(RuntimeError, match="at most 64"):
        PCEvalState(dev, latent_size=65).update(latents=latents)


def test_median_rows_is_pandas_median(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import median_rows
    g = torch.Generator().manual_seed(12)
    for n in (1, 2, 37, 38):
        x = torch.rand(n, 3, generator=g)
        assert np.array_equal(median_rows(x.to(dev)).cpu().numpy(), np.median(x.numpy().astype(np.float64), axis=0)), n


# ------------------------------------------------------------------------------------------------ 3. loops against the fixture
class _Frames(torch.utils.data.Dataset):
    """The fixture's frames with the item layout of PrincipalComponentsAutoencoderDataset2 and the generator's frame names."""

    def __init__(self, g, prefix, arts):
        self.frames, self.weights = torch.from_numpy(g[prefix + "frames"]), torch.from_numpy(g[prefix + "weights"])
        self.normalize = _normalize(g, prefix, arts)

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return f"sub{1 + i // 20}_S{1 + i % 3}_{i:04d}", self.frames[i].clone(), self.weights[i], "a"


def test_run_multiart_autoencoder_test_matches_reference_fixture(fx, dev, tmp_path):
    """37 frames in batches of 8 (the last holds 5): info 1e-5, every covariance file 1e-5 (the reference's fp32 torch.cov)."""
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import run_multiart_autoencoder_test
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    from artspeech_amd.settings import DATASET_CONFIG
    arts = [str(a) for a in fx["small.articulators"]]
    comps = {str(a): int(k) for a, k in zip(fx["small.comps_names"], fx["small.comps"])}
    m = MultiArticulatorAutoencoder(in_features=fx["small.frames"].shape[-1], indices_dict=comps, hidden_features=10)
    m.load_state_dict(_sd(fx, "small.w."), strict=True)
    m.to(dev)
    loader = torch.utils.data.DataLoader(_Frames(fx, "small.", arts), batch_size=8, shuffle=False)
    crit = RegularizedLatentsMSELoss2(0.1, m.indices_dict)
    cfg = DATASET_CONFIG["artspeech2"]
    info = run_multiart_autoencoder_test(0, m, loader, crit, cfg, plots_dir=str(tmp_path / "blocks"), indices_dict=m.indices_dict,
                                         device=dev)
    assert set(info) == {"loss"} and abs(info["loss"] - float(fx["small.loss"])) <= 1e-5 * abs(float(fx["small.loss"])), info
    assert sorted(os.listdir(tmp_path / "blocks")) == sorted(f"covariance_matrix_{a}.npy" for a in comps)
    for a in comps:
        got = np.load(tmp_path / "blocks" / f"covariance_matrix_{a}.npy")
        assert got.dtype == np.float32 and _rel(got, fx[f"small.cov.{a}"]) <= 1e-5, a
    info = run_multiart_autoencoder_test(0, m, loader, crit, cfg, plots_dir=str(tmp_path / "whole"), device=dev,
                                         fn_metrics={"seven": lambda outputs, inputs: torch.tensor(7.0)})
    assert info["seven"] == 7.0 and abs(info["loss"] - float(fx["small.loss"])) <= 1e-5 * abs(float(fx["small.loss"]))
    assert os.listdir(tmp_path / "whole") == ["covariance_matrix.npy"]
    assert _rel(np.load(tmp_path / "whole" / "covariance_matrix.npy"), fx["small.cov"]) <= 1e-5
    with pytest.raises(NotImplementedError, match="plots"):
        run_multiart_autoencoder_test(0, m, loader, crit, cfg, outputs_dir=str(tmp_path / "frames"), device=dev)


def _read_csv(path):
    with open(path) as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_evaluate_autoencoder_matches_reference_fixture(fx, dev, tmp_path, monkeypatch):
    """The four tables of the reference's evaluate_autoencoder (2e-3) and the nomogram shapes (the decoders' denormalised outputs)."""
    sys.path.insert(0, ROOT)
    import test_principal_components_autoencoder as TE
    from artspeech_amd.helpers import make_indices_dict
    from artspeech_amd.settings import DATASET_CONFIG
    arts = [str(a) for a in fx["full.articulators"]]
    comps = {str(a): int(k) for a, k in zip(fx["full.comps_names"], fx["full.comps"])}
    torch.save(_sd(fx, "full.enc."), tmp_path / "enc.pt")
    torch.save(_sd(fx, "full.dec."), tmp_path / "dec.pt")
    dataset = _Frames(fx, "full.", arts)
    monkeypatch.setattr(TE, "_make_dataset", lambda *a, **k: dataset)
    params = {"in_features": 100, "indices_dict": make_indices_dict(comps), "hidden_features": 10}
    save_to = tmp_path / "eval"
    TE.evaluate_autoencoder("artspeech2", "unused", DATASET_CONFIG["artspeech2"], 8, {}, params, str(tmp_path / "enc.pt"),
                            str(tmp_path / "dec.pt"), str(save_to))
    L = fx["full.latents"].shape[1]
    header, rows = _read_csv(save_to / "latent_space.csv")
    assert header == [str(c) for c in fx["full.latent_columns"]] == [str(i) for i in range(1, L + 1)]
    assert _rel(np.array(rows, dtype=np.float64), fx["full.latent_space"]) <= 2e-3
    errors = np.load(save_to / "reconstruction_errors.npy")
    assert errors.dtype == np.float32 and _rel(errors, fx["full.errors"]) <= 2e-3
    header, rows = _read_csv(save_to / "reconstruction_errors.csv")
    assert header == ["subject", "sequence", "frame"] + arts
    assert np.array_equal(np.array([r[:3] for r in rows]), fx["full.errors_csv_names"])
    assert _rel(np.array([r[3:] for r in rows], dtype=np.float64), fx["full.errors_csv"]) <= 2e-3
    header, rows = _read_csv(save_to / "reconstruction_errors_agg.csv")
    assert header == ["index"] + arts and [r[0] for r in rows] == [str(s) for s in fx["full.agg_index"]]
    agg = np.array([r[1:] for r in rows], dtype=np.float64)
    for name, got, want in zip(fx["full.agg_index"], agg, fx["full.agg"]):
        assert _rel(got, want) <= 2e-3, name
    # the aggregate is that of the written errors: numpy fp64 of reconstruction_errors.npy, 1e-6
    m = Y.moments(errors)
    for name, got in zip(("mean", "std", "median", "min", "max"), agg):
        assert _rel(got, m[name]) <= 1e-6, name
    nomograms = np.load(save_to / "plots" / "nomograms.npy")
    assert nomograms.shape == (L, 21, len(arts), 2, 50) and nomograms.dtype == np.float32
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder
    dec = MultiDecoder(params["indices_dict"], 100, 10)
    dec.load_state_dict(_sd(fx, "full.dec."))
    dec.to(dev)
    z = torch.zeros(21, L, device=dev)
    z[:, 3] = torch.from_numpy(np.arange(-1, 1.01, 0.1)).float().to(dev)
    with torch.no_grad():
        want = dec(z).reshape(21, len(arts), 2, 50) * torch.from_numpy(fx["full.norm_std"]).to(dev) + torch.from_numpy(fx["full.norm_mean"]).to(dev)
    assert _rel(nomograms[3], want.cpu().numpy()) <= 1e-6


def test_run_phoneme_to_principal_components_test_matches_reference_fixture(fx, dev, tmp_path):
    """4 sentences of lengths 9, 5, 5, 1 in batches of 2 with outputs_dir: info 1e-5, the dumped contours of the 9-frame sentence
    1e-5 absolute (upper incisor injected at its sorted position), its tract variables 1e-4, and the batch's targets untouched."""
    from artspeech_amd.phoneme_to_articulation.principal_components.dataset import pad_sequence_collate_fn
    from artspeech_amd.phoneme_to_articulation.principal_components.evaluation import run_phoneme_to_principal_components_test
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.metrics import DecoderMeanP2CPDistance2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import PrincipalComponentsArtSpeech
    from artspeech_amd.settings import DATASET_CONFIG
    import types
    arts = [str(a) for a in fx["full.articulators"]]
    comps = {str(a): int(k) for a, k in zip(fx["full.comps_names"], fx["full.comps"])}
    V, E, H = (int(v) for v in fx["sent.cfg"])
    torch.save(_sd(fx, "full.enc."), tmp_path / "enc.pt")
    torch.save(_sd(fx, "full.dec."), tmp_path / "dec.pt")
    items = []
    for i in range(4):
        p = f"sent.in{i}."
        items.append((f"sent{i}", torch.from_numpy(fx[p + "tokens"]), torch.from_numpy(fx[p + "targets"]), [str(s) for s in fx[p + "phonemes"]],
                      torch.from_numpy(fx[p + "mask"]), torch.from_numpy(fx[p + "ref"]), [str(s) for s in fx[p + "frames"]],
                      torch.from_numpy(fx[p + "voicing"])))
    batches = [pad_sequence_collate_fn(items[:2]), pad_sequence_collate_fn(items[2:])]
    targets_before = [b[2].clone() for b in batches]
    norm = _normalize(fx, "sent.", arts)

    class Loader:
        dataset = types.SimpleNamespace(articulators=arts, normalize=norm)

        def __iter__(self):
            return iter(batches)

    model = PrincipalComponentsArtSpeech(V, comps, embed_dim=E, hidden_size=H)
    model.load_state_dict(_sd(fx, "sent.w."), strict=True)
    model.to(dev)
    denorm = {a: n.inverse for a, n in norm.items()}
    b1, b2, b3 = (float(v) for v in fx["sent.betas"])
    crit = AutoencoderLoss2(comps, [str(s) for s in fx["sent.TVs"]], 100, 10, tmp_path / "enc.pt", tmp_path / "dec.pt", dev,
                            denormalize_fn=denorm, beta1=b1, beta2=b2, beta3=b3)
    metric = DecoderMeanP2CPDistance2(DATASET_CONFIG["artspeech2"], tmp_path / "dec.pt", comps,
                                      {"in_features": 100, "hidden_features": 10}, denorm, dev)
    info = run_phoneme_to_principal_components_test(3, model, Loader(), crit, fn_metrics={"p2cp_mean": metric},
                                                    outputs_dir=str(tmp_path / "out"), decode_transform=crit.decode, device=dev)
    assert set(info) == {"loss", "p2cp_mean"}
    for key in ("loss", "p2cp_mean"):
        want = float(fx[f"sent.{key}"])
        print(f"{key}: {info[key]!r} against {want!r}")
        assert abs(info[key] - want) <= 1e-5 * abs(want), key
    assert all(torch.equal(a, b[2]) for a, b in zip(targets_before, batches)), "the batch's targets were modified"
    assert sorted(os.listdir(tmp_path / "out" / "3")) == [str(s) for s in fx["sent.sentence_dirs"]]
    sdir = tmp_path / "out" / "3" / "sent0"
    assert sorted(os.listdir(sdir / "contours")) == [str(s) for s in fx["sent.contour_files"]]
    tv_arts = [str(a) for a in fx["sent.tv_articulators"]]
    frames0 = items[0][6]
    pred = np.stack([[np.load(sdir / "contours" / f"{fr}_{a}.npy") for a in tv_arts] for fr in frames0])
    true = np.stack([[np.load(sdir / "contours" / f"{fr}_{a}_true.npy") for a in tv_arts] for fr in frames0])
    assert pred.dtype == np.float32 and pred.shape == fx["sent.contours_pred"].shape
    assert np.abs(pred - fx["sent.contours_pred"]).max() <= 1e-5 and np.abs(true - fx["sent.contours_true"]).max() <= 1e-5
    i_ref = tv_arts.index("upper-incisor")
    assert np.array_equal(pred[:, i_ref], fx["sent.in0.ref"][:, 0]) and np.array_equal(true[:, i_ref], fx["sent.in0.ref"][:, 0])
    header, rows = _read_csv(sdir / "phonemes.csv")
    assert [header] + rows == fx["sent.phonemes_csv"].tolist()
    header, rows = _read_csv(sdir / "tract_variables.csv")
    assert header == [str(c) for c in fx["sent.tv_columns"]]
    assert [r[header.index("frame")] for r in rows] == [str(s) for s in fx["sent.tv_frames"]]
    num = [str(c) for c in fx["sent.tv_numeric_columns"]]
    got = np.array([[float(r[header.index(c)]) for c in num] for r in rows])
    # the points of closest approach are contour points: equal to 1e-4 means the same closest-point indices
    assert np.abs(got - fx["sent.tv_values"]).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ 4. entry points, end to end
@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """Both trainers for one epoch on small synthetic splits; the autoencoder's best_* feed the method's trainer."""
    sys.path.insert(0, ROOT)
    import train_phoneme_to_principal_components as TP
    import train_principal_components_autoencoder as TA
    tmp = tmp_path_factory.mktemp("pc_eval")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_pc_autoencoder_synthetic.yaml")))
    cfg.update(results_dir=str(tmp / "ae"), n_epochs=1, train_seq_dict={"num_frames": 256}, valid_seq_dict={"num_frames": 64},
               test_seq_dict={"num_frames": 100})
    ae = TA.main(**cfg)
    pcfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_pc_based_synthetic.yaml")))
    pcfg.update(results_dir=str(tmp / "method"), num_epochs=1, encoder_state_dict_filepath=str(tmp / "ae" / "best_encoders.pt"),
                decoder_state_dict_filepath=str(tmp / "ae" / "best_decoders.pt"), train_seq_dict={"num_sentences": 8},
                valid_seq_dict={"num_sentences": 4}, test_seq_dict={"num_sentences": 4}, synthetic={"min_len": 20, "max_len": 30})
    method = TP.main(**pcfg)
    return tmp, ae, method


def test_trainers_close_with_the_test_functions(trained):
    tmp, ae, method = trained
    assert set(ae["test"]) == {"loss", "p2cp_mm"} and all(np.isfinite(v) for v in ae["test"].values())
    assert set(method["test"]) == {"loss", "p2cp_mean"} and all(np.isfinite(v) for v in method["test"].values())
    comps = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_pc_autoencoder_synthetic.yaml")))["model_params"]["indices_dict"]
    for a, k in comps.items():
        assert np.load(tmp / "ae" / f"covariance_matrix_{a}.npy").shape == (k, k), a


def test_autoencoder_entry_point_end_to_end(trained, dev):
    import test_principal_components_autoencoder as TE
    tmp = trained[0]
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "test_pc_autoencoder_synthetic.yaml")))
    cfg.update(encoders_filepath=str(tmp / "ae" / "best_encoders.pt"), decoders_filepath=str(tmp / "ae" / "best_decoders.pt"),
               save_to=str(tmp / "ae_test"), seq_dict={"num_frames": 101}, batch_size=32)
    info = TE.run(cfg)
    save_to = tmp / "ae_test"
    assert json.load(open(save_to / "test_results.json")) == info and set(info) == {"loss"} and np.isfinite(info["loss"])
    comps = cfg["model_params"]["indices_dict"]
    arts, L = sorted(comps), sum(comps.values())
    for a, k in comps.items():
        cov = np.load(save_to / "plots" / f"covariance_matrix_{a}.npy")
        assert cov.shape == (k, k) and np.isfinite(cov).all() and (np.diag(cov) > 0).all(), a
    header, rows = _read_csv(save_to / "latent_space.csv")
    assert header == [str(i) for i in range(1, L + 1)] and np.array(rows, dtype=np.float64).shape == (101, L)
    errors = np.load(save_to / "reconstruction_errors.npy")
    assert errors.shape == (101, len(arts)) and errors.dtype == np.float32 and (errors > 0).all()
    header, rows = _read_csv(save_to / "reconstruction_errors.csv")
    assert header == ["subject", "sequence", "frame"] + arts and len(rows) == 101
    assert rows[5][:3] == ["synthetic", "S1", "00005"]
    assert _rel(np.array([r[3:] for r in rows], dtype=np.float64), errors) <= 1e-6
    import pandas as pd
    df = pd.read_csv(save_to / "reconstruction_errors.csv")
    want = df.agg({a: ["mean", "std", "median", "min", "max"] for a in arts}).reset_index()
    got = pd.read_csv(save_to / "reconstruction_errors_agg.csv")
    assert list(got.columns) == list(want.columns) == ["index"] + arts and list(got["index"]) == list(want["index"])
    assert _rel(got[arts].to_numpy(np.float64), want[arts].to_numpy(np.float64)) <= 1e-6
    nomograms = np.load(save_to / "plots" / "nomograms.npy")
    assert nomograms.shape == (L, 21, len(arts), 2, 50) and np.isfinite(nomograms).all()
    # component 0 belongs to the first articulator of the dict alone: only that channel moves along its 21 steps
    first = arts.index(next(iter(comps)))
    moves = np.abs(nomograms[0] - nomograms[0, :1]).max(axis=(0, 2, 3)) > 0
    assert moves[first] and not np.delete(moves, first).any()


@pytest.mark.parametrize("kind", ["AE", "PCA"])
def test_method_entry_point_end_to_end(kind, trained, dev):
    import test_phoneme_to_principal_components as TM
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder, MultiEncoder
    tmp = trained[0]
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "test_pc_based_synthetic.yaml")))
    enc_path, dec_path = str(tmp / "ae" / "best_encoders.pt"), str(tmp / "ae" / "best_decoders.pt")
    if kind == "PCA":   # an SVD-built projection of the same widths, like the trainers' PCA test
        comps, kw = cfg["indices_dict"], cfg["autoencoder_kwargs"]
        enc = MultiEncoder(comps, kw["in_features"], kw["hidden_features"], encoder_cls="PCA")
        dec = MultiDecoder(comps, kw["in_features"], kw["hidden_features"], decoder_cls="PCA")
        data = torch.rand(400, kw["in_features"], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        _, S, Vh = torch.linalg.svd(data - data.mean(0), full_matrices=False)
        with torch.no_grad():
            for a, n in comps.items():
                enc.encoders[a].eigenvectors.copy_(Vh[:n].float())
                enc.encoders[a].eigenvalues.copy_((S[:n] ** 2 / 399).float())
                dec.decoders[a].eigenvectors.copy_(Vh[:n].float())
        enc_path, dec_path = str(tmp / "pca_enc.pt"), str(tmp / "pca_dec.pt")
        torch.save(enc.state_dict(), enc_path)
        torch.save(dec.state_dict(), dec_path)
    save_to = tmp / f"method_test_{kind}"
    cfg.update(state_dict_filepath=str(tmp / "method" / "best_model.pt"), encoder_state_dict_filepath=enc_path,
               decoder_state_dict_filepath=dec_path, encoder_type=kind, decoder_type=kind, save_to=str(save_to),
               seq_dict={"num_sentences": 3}, batch_size=2, synthetic={"min_len": 20, "max_len": 30})
    info = TM.main(**cfg)
    assert json.load(open(save_to / "test_results.json")) == info and set(info) == {"loss"} and np.isfinite(info["loss"])
    sentences = sorted(os.listdir(save_to / "test_outputs" / "0"))
    assert sentences == [f"synthetic_{i:05d}" for i in range(3)]
    tv_arts = sorted(list(cfg["indices_dict"]) + ["upper-incisor"])
    for s in sentences:
        sdir = save_to / "test_outputs" / "0" / s
        header, rows = _read_csv(sdir / "phonemes.csv")
        assert header == ["sentence", "frame", "phoneme"] and 20 <= len(rows) <= 30
        assert len(os.listdir(sdir / "contours")) == 2 * len(tv_arts) * len(rows)
        contour = np.load(sdir / "contours" / f"{rows[0][1]}_tongue.npy")
        assert contour.shape == (2, 50) and contour.dtype == np.float32 and np.isfinite(contour).all()
        tv_header, tv_rows = _read_csv(sdir / "tract_variables.csv")
        assert tv_header[:3] == ["sentence", "frame", "phoneme"] and "TTCD_pred" in tv_header and len(tv_rows) == len(rows)
