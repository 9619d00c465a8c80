"""GPU checks of the contour preparation (csrc/contours.hip): as_prepare_contours against the fixture recorded from the
reference's own TailClipper and prepare_articulator_array (tests/golden/make_golden_contours.py) and, for the shapes the fixture
does not hold, against the index-arithmetic restatement tests/contours_ref.py that the host tests hold to that fixture -- bit for
bit everywhere; as_column_mean_std against numpy fp64; the statistics script and ArtSpeechDataset(device=...) end to end."""
import os
import random
import types

import numpy as np
import pytest
import torch
import yaml

import contours_ref as Y
from conftest import ROOT, WORST, load_golden
from test_contours_host import fixture_inputs

pytestmark = pytest.mark.gpu

TIE_FRAMES = [69, 74, 80]   # tongue, lower lip, upper lip: a point on the threshold (make_golden_contours.py's construction order)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_golden("contours")


@pytest.fixture(scope="module")
def cfg():
    from artspeech_amd.settings import DATASET_CONFIG
    return DATASET_CONFIG["artspeech2"]


def same_bits(got, want, what):
    """bit-equal float32 arrays; a NaN in one is a NaN in the other (its payload is not compared)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other places"
    differ = int((got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan]).sum())
    assert differ == 0, f"{what}: {differ} of {got.size} elements differ in their bits"


def write_tree(root, fx, frames, subject="S0", sequence="seq"):
    """the contour files of some fixture frames in pixel units, every other file in (2, N) orientation"""
    arts = [str(a) for a in fx["articulators"]]
    directory = os.path.join(root, subject, sequence, "inference_contours")
    os.makedirs(directory, exist_ok=True)
    for f in frames:
        named = {name: fx["raw"][f, a] for a, name in enumerate(arts)}
        named["lower-incisor"], named["epiglottis"] = fx["lower_incisor"][f], fx["epiglottis"][f]
        for i, (name, points) in enumerate(sorted(named.items())):
            pixels = points.astype(np.float64) * 136     # exact, and / 136 in float64 gives the float32 value back
            np.save(os.path.join(directory, f"{f:04d}_{name}.npy"), pixels.T if (f + i) % 2 else pixels)
    return [f"{f:04d}" for f in frames]


def normalize_dict(fx, arts):
    from artspeech_amd.phoneme_to_articulation.transforms import Normalize
    return {a: Normalize(torch.from_numpy(fx["norm_mean"][i]), torch.from_numpy(fx["norm_std"][i])) for i, a in enumerate(arts)}


# ------------------------------------------------------------------------------------------------ 1. the fixture
def test_fixture_batched(fx, dev, cfg):
    from artspeech_amd.phoneme_to_articulation import prepare_contours
    from artspeech_amd.phoneme_to_articulation.tail_clipper import clip_tails_batched
    arts, raw, refs, kinds, thr = fixture_inputs(fx)
    raw_d, refs_d = torch.from_numpy(raw).to(dev), torch.from_numpy(refs).to(dev)
    _, want_counts = Y.clip_batched(raw, refs, kinds, thr)
    clipped, counts = clip_tails_batched(raw_d, refs_d, arts, cfg)
    assert clipped.shape == (96, 5, 50, 2) and counts.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    clipped = clipped.cpu().numpy()
    for k, name in enumerate(fx["clipped_articulators"]):
        same_bits(clipped[:, arts.index(str(name))], fx["clipped"][:, k], f"clip_{name}_tails")
    for a, kind in enumerate(kinds):
        if kind == 0:
            same_bits(clipped[:, a], raw[:, a], f"{arts[a]} passes through")
    targets, references, counts = prepare_contours(raw_d, refs_d, arts, cfg)
    same_bits(targets.cpu().numpy(), fx["prepared"], "prepared")
    same_bits(references.cpu().numpy(), fx["references"], "references")
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    targets, references, _ = prepare_contours(raw_d, refs_d, arts, cfg, normalize=normalize_dict(fx, arts))
    same_bits(targets.cpu().numpy(), fx["prepared_norm"], "prepared, normalised")
    same_bits(references.cpu().numpy(), fx["references"], "references (never normalised)")
    targets, _, counts = prepare_contours(raw_d, refs_d, arts, cfg, clip_tails=False)
    same_bits(targets[:, arts.index("tongue")].cpu().numpy(), fx["unclipped_tongue"], "clip_tails=False")
    assert (counts == 50).all()


def test_fixture_single_frame_methods_on_host_tensors(fx, cfg):
    from artspeech_amd.phoneme_to_articulation import TailClipper
    arts, raw, refs, _, _ = fixture_inputs(fx)
    clipper = TailClipper(cfg)
    for f in range(raw.shape[0]):
        named = {name.replace("-", "_"): torch.from_numpy(refs[f, i]) for i, name in enumerate(Y.REFERENCES)}
        for k, name in enumerate(fx["clipped_articulators"]):
            method = getattr(clipper, f"clip_{str(name).replace('-', '_')}_tails")
            out = method(torch.from_numpy(raw[f, arts.index(str(name))]), **named)   # every reference given: the unused are ignored
            assert out.device.type == "cpu" and out.shape == (50, 2) and out.dtype == torch.float32
            same_bits(out.numpy(), fx["clipped"][f, k], f"frame {f} clip_{name}_tails")
    out = clipper.clip_tongue_tails(torch.from_numpy(raw[0, arts.index("tongue")]).cuda(), torch.from_numpy(refs[0, 0]), torch.from_numpy(refs[0, 2]))
    assert out.is_cuda, "a device tensor comes back on its device"
    empty = {name.replace("-", "_"): torch.from_numpy(fx["empty_refs"][i]) for i, name in enumerate(Y.REFERENCES)}
    with pytest.raises(RuntimeError, match="no point"):
        clipper.clip_tongue_tails(torch.from_numpy(fx["empty_raw"][arts.index("tongue")]), **empty)
    with pytest.raises(RuntimeError, match="no point"):
        clipper.clip_upper_lip_tails(torch.from_numpy(fx["empty_raw"][arts.index("upper-lip")]), **empty)


def test_fixture_prepare_articulator_array_from_files(fx, cfg, tmp_path):
    from artspeech_amd.phoneme_to_articulation import InputLoaderMixin
    arts = [str(a) for a in fx["articulators"]]
    frames = sorted(set(range(0, 96, 4)) | set(TIE_FRAMES))
    names = write_tree(str(tmp_path), fx, frames)
    normalize = normalize_dict(fx, arts)
    for f, frame_id in zip(frames, names):
        for a, name in enumerate(arts):
            arr, ref = InputLoaderMixin.prepare_articulator_array(str(tmp_path), "S0", "seq", frame_id, name, cfg)
            assert arr.shape == ref.shape == (2, 50) and arr.device.type == "cpu"
            same_bits(arr.numpy(), fx["prepared"][f, a], f"frame {f} {name}")
            same_bits(ref.numpy(), fx["references"][f, 0], f"frame {f} reference")
            arr, _ = InputLoaderMixin.prepare_articulator_array(str(tmp_path), "S0", "seq", frame_id, name, cfg, normalize_fn=normalize[name])
            same_bits(arr.numpy(), fx["prepared_norm"][f, a], f"frame {f} {name} normalised")
    # a callable that is no Normalize is applied to the result
    arr, _ = InputLoaderMixin.prepare_articulator_array(str(tmp_path), "S0", "seq", names[0], "tongue", cfg, normalize_fn=lambda x: x * 2)
    same_bits(arr.numpy(), fx["prepared"][frames[0], arts.index("tongue")] * np.float32(2), "callable")
    # clip_tails=False reads the upper incisor only
    os.remove(tmp_path / "S0" / "seq" / "inference_contours" / f"{names[0]}_epiglottis.npy")
    arr, _ = InputLoaderMixin.prepare_articulator_array(str(tmp_path), "S0", "seq", names[0], "tongue", cfg, clip_tails=False)
    same_bits(arr.numpy(), fx["unclipped_tongue"][frames[0]], "clip_tails=False")


# ------------------------------------------------------------------------------------------------ 2. launch geometry
def draw(F, arts, seed, N=50):
    """frames in the fixture's mixed scale: the upper lip's and the upper incisor's y in pixels"""
    rng = np.random.RandomState(seed)
    raw = rng.rand(F, len(arts), N, 2).astype(np.float32)
    refs = rng.rand(F, 3, N, 2).astype(np.float32)
    refs[:, 0, :, 1] = (0.15 + 0.85 * rng.rand(F, 1) - 0.1 * rng.rand(F, N)).astype(np.float32)
    refs[:, 2, :, 1] = (0.1 + 0.8 * rng.rand(F, 1) + 0.1 * rng.rand(F, N)).astype(np.float32)
    refs[:, 1, :, 1] = (2 + 17 * rng.rand(F, 1) + rng.rand(F, N)).astype(np.float32)
    if "upper-lip" in arts:
        raw[:, arts.index("upper-lip"), :, 1] *= 20
    return raw, refs


GEOMETRY_ARTS = {1: ["tongue"], 3: ["lower-lip", "tongue", "upper-lip"], 5: ["lower-lip", "pharynx", "tongue", "upper-lip", "vocal-folds"]}


@pytest.mark.parametrize("A", [1, 3, 5])
@pytest.mark.parametrize("F", [1, 3, 5, 67])
def test_tile_counts_that_do_not_fill_a_block(F, A, dev, cfg):
    from artspeech_amd.phoneme_to_articulation import prepare_contours
    from artspeech_amd.phoneme_to_articulation.tail_clipper import clip_tails_batched
    from artspeech_amd.phoneme_to_articulation.transforms import Normalize
    arts = GEOMETRY_ARTS[A]
    raw, refs = draw(F, arts, 100 * F + A)
    rng = np.random.RandomState(7)
    mean, std = rng.rand(A, 2, 50).astype(np.float32), (0.5 + rng.rand(A, 2, 50)).astype(np.float32)
    kinds, thr = Y.kinds_of(arts), Y.thresholds(cfg)
    raw_d, refs_d = torch.from_numpy(raw).to(dev), torch.from_numpy(refs).to(dev)
    want_t, want_r, want_c = Y.prepare(raw, refs, kinds, thr, mean, std)
    normalize = {a: Normalize(torch.from_numpy(mean[i]), torch.from_numpy(std[i])) for i, a in enumerate(arts)}
    targets, references, counts = prepare_contours(raw_d, refs_d, arts, cfg, normalize=normalize, check=False)
    same_bits(targets.cpu().numpy(), want_t, "targets")
    same_bits(references.cpu().numpy(), want_r, "references")
    assert np.array_equal(counts.cpu().numpy(), want_c)
    clipped, counts = clip_tails_batched(raw_d, refs_d, arts, cfg)
    same_bits(clipped.cpu().numpy(), Y.clip_batched(raw, refs, kinds, thr)[0], "clipped")
    assert np.array_equal(counts.cpu().numpy(), want_c)


def test_non_contiguous_inputs(dev, cfg):
    from artspeech_amd.phoneme_to_articulation import prepare_contours
    arts = GEOMETRY_ARTS[3]
    raw, refs = draw(6, arts, 5)
    raw_d = torch.from_numpy(np.ascontiguousarray(raw.transpose(0, 1, 3, 2))).to(dev).permute(0, 1, 3, 2)     # channel-major storage
    refs_wide = torch.zeros(6, 5, 50, 2, device=dev)
    refs_wide[:, ::2] = torch.from_numpy(refs).to(dev)
    refs_d = refs_wide[:, ::2]
    assert not raw_d.is_contiguous() and not refs_d.is_contiguous()
    targets, references, counts = prepare_contours(raw_d, refs_d, arts, cfg, check=False)
    want_t, want_r, want_c = Y.prepare(raw, refs, Y.kinds_of(arts), Y.thresholds(cfg))
    same_bits(targets.cpu().numpy(), want_t, "targets")
    same_bits(references.cpu().numpy(), want_r, "references")
    assert np.array_equal(counts.cpu().numpy(), want_c)


@pytest.mark.parametrize("N", [1, 50, 100])
def test_without_a_clipped_articulator_any_point_count_works(N, dev, cfg):
    from artspeech_amd.phoneme_to_articulation import prepare_contours
    rng = np.random.RandomState(N)
    mean, std = rng.rand(2, 2, N).astype(np.float32), (0.5 + rng.rand(2, 2, N)).astype(np.float32)
    for arts, clip_tails in ((["pharynx", "vocal-folds"], True), (["tongue", "upper-lip"], False)):
        raw, refs = draw(7, arts, N, N=N)
        want_t, want_r, _ = Y.prepare(raw, refs, [0, 0], Y.thresholds(cfg), mean, std)
        from artspeech_amd.phoneme_to_articulation.transforms import Normalize
        normalize = {a: Normalize(torch.from_numpy(mean[i]), torch.from_numpy(std[i])) for i, a in enumerate(arts)}
        targets, references, counts = prepare_contours(torch.from_numpy(raw).to(dev), torch.from_numpy(refs).to(dev), arts, cfg,
                                                       normalize=normalize, clip_tails=clip_tails)
        same_bits(targets.cpu().numpy(), want_t, f"targets N={N}")
        same_bits(references.cpu().numpy(), want_r, f"references N={N}")
        assert (counts == N).all()


# ------------------------------------------------------------------------------------------------ 3. emptied contours
def test_emptied_contour(fx, dev, cfg):
    from artspeech_amd.phoneme_to_articulation import prepare_contours
    arts, raw, refs, kinds, thr = fixture_inputs(fx)
    raw3 = np.stack([raw[0], fx["empty_raw"], raw[TIE_FRAMES[0]]])
    refs3 = np.stack([refs[0], fx["empty_refs"], refs[TIE_FRAMES[0]]])
    raw_d, refs_d = torch.from_numpy(raw3).to(dev), torch.from_numpy(refs3).to(dev)
    with pytest.raises(RuntimeError, match=r"'tongue' in frame 1 \(2 emptied"):
        prepare_contours(raw_d, refs_d, arts, cfg)
    targets, references, counts = prepare_contours(raw_d, refs_d, arts, cfg, check=False)
    targets, counts = targets.cpu().numpy(), counts.cpu().numpy()
    t, ul = arts.index("tongue"), arts.index("upper-lip")
    assert counts[1, t] == 0 and counts[1, ul] == 0 and (counts[[0, 2]] > 0).all()
    assert np.isnan(targets[1, t]).all() and np.isnan(targets[1, ul]).all()
    want_t, want_r, want_c = Y.prepare(raw3, refs3, kinds, thr)
    same_bits(targets, want_t, "every other row")
    same_bits(targets[[0, 2]], fx["prepared"][[0, TIE_FRAMES[0]]], "the neighbouring frames")
    same_bits(references.cpu().numpy(), want_r, "references")
    assert np.array_equal(counts, want_c)
    prepare_contours(raw_d, refs_d, arts, cfg, clip_tails=False)   # nothing is clipped, nothing is empty


def test_clipping_another_point_count_is_refused(dev, cfg):
    from artspeech_amd.phoneme_to_articulation import prepare_contours
    raw, refs = draw(2, ["pharynx", "tongue"], 1, N=40)
    with pytest.raises(RuntimeError, match="defined for 50 points per contour, got 40"):
        prepare_contours(torch.from_numpy(raw).to(dev), torch.from_numpy(refs).to(dev), ["pharynx", "tongue"], cfg)
    with pytest.raises(ValueError, match="refs must be"):
        prepare_contours(torch.from_numpy(raw).to(dev), torch.from_numpy(refs[:, :2]).to(dev), ["pharynx", "tongue"], cfg)


# ------------------------------------------------------------------------------------------------ 4. statistics
def within_one_ulp(got, want64, what, slack=0.0):
    """|got - want| <= one float32 ulp of want (+ slack), element-wise: fp64 accumulation, one rounding"""
    got = np.asarray(got, np.float64)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    ratio = float(np.max(np.abs(got - want64) / (ulp + slack)))
    print(f"{what}: worst |got - fp64| / bound = {ratio:.3f}")
    WORST[f"contour statistics {what} / ulp bound"] = max(WORST.get(f"contour statistics {what} / ulp bound", 0.0), ratio)
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("cols", [1, 100, 1000])
@pytest.mark.parametrize("rows", [1, 2, 3, 64, 65, 257, 4099])
def test_contour_statistics_against_fp64(rows, cols, dev):
    from artspeech_amd.phoneme_to_articulation import contour_statistics
    rng = np.random.RandomState(rows + cols)
    x = (0.3 + 0.2 * rng.randn(rows, cols)).astype(np.float32)
    if cols > 2:
        x[:, 1] = np.float32(0.7)                                           # a constant column
        x[:, 2] = (1e3 + 1e-3 * rng.randn(rows)).astype(np.float32)         # mean 1e3, spread 1e-3
    xd = torch.from_numpy(x).to(dev)
    mean, std = contour_statistics(xd)
    mean2, std2 = contour_statistics(xd)
    assert mean.shape == std.shape == (cols,) and mean.dtype == std.dtype == torch.float32
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    assert mean.tobytes() == mean2.cpu().numpy().tobytes() and std.tobytes() == std2.cpu().numpy().tobytes(), "two calls differ"
    want_mean, want_std = Y.column_stats_fp64(x)
    within_one_ulp(mean, want_mean, "mean")
    if rows == 1:
        assert np.isnan(std).all() and mean.tobytes() == x[0].tobytes()
        return
    assert not np.isnan(std).any()
    within_one_ulp(std, want_std, "std")
    if cols > 2:
        assert std[1] == 0.0 and mean[1] == np.float32(0.7), "a constant column has std exactly 0"
    # a trailing shape is kept
    if cols == 100:
        m3, s3 = contour_statistics(xd.reshape(rows, 2, 50))
        assert m3.shape == s3.shape == (2, 50) and m3.cpu().numpy().tobytes() == mean.tobytes() and s3.cpu().numpy().tobytes() == std.tobytes()


def test_contour_statistics_against_the_fixture(fx, dev):
    """|device - torch's recorded value| <= |torch's value - fp64| + 1 ulp, per articulator as the reference's script reduces"""
    from artspeech_amd.phoneme_to_articulation import contour_statistics
    prepared = torch.from_numpy(fx["prepared"]).to(dev)
    for a in range(prepared.shape[1]):
        mean, std = (t.cpu().numpy() for t in contour_statistics(prepared[:, a]))   # a strided slice
        assert mean.shape == std.shape == (2, 50)
        want_mean, want_std = Y.column_stats_fp64(fx["prepared"][:, a])
        within_one_ulp(mean, want_mean, "fixture mean")
        within_one_ulp(std, want_std, "fixture std")
        for got, ref, want in ((mean, fx["stats_mean"][a], want_mean), (std, fx["stats_std"][a], want_std)):
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - ref) <= np.abs(ref - want) + ulp).all()


# ------------------------------------------------------------------------------------------------ 5. the script
def test_statistics_script_end_to_end(dev, cfg, tmp_path):
    import calculate_normalization_statistics as script
    from artspeech_amd.phoneme_to_articulation import SyntheticRawContours, contour_statistics, prepare_contours
    with open(os.path.join(ROOT, "configs", "normalization_statistics_synthetic.yaml")) as f:
        config = yaml.safe_load(f)
    config.update(save_to=str(tmp_path / "all"), sequences_dict={"num_frames": 300})
    info = script.main(**config, seed=0)
    arts = config["articulators"]
    assert info["num_frames"] == 300 and sorted(os.listdir(tmp_path / "all")) == sorted(f"{a}_{w}.npy" for a in arts for w in ("mean", "std"))
    data = SyntheticRawContours(300, arts, seed=0)

    def expect(chosen):
        targets, _, _ = prepare_contours(data.raw[chosen].to(dev), data.refs[chosen].to(dev), arts, cfg)
        return [tuple(t.cpu().numpy() for t in contour_statistics(targets[:, i])) for i in range(len(arts))]

    for (mean, std), a in zip(expect(list(range(300))), arts):
        got_mean, got_std = np.load(tmp_path / "all" / f"{a}_mean.npy"), np.load(tmp_path / "all" / f"{a}_std.npy")
        assert got_mean.shape == got_std.shape == (2, 50) and got_mean.dtype == got_std.dtype == np.float32
        assert got_mean.tobytes() == mean.tobytes() and got_std.tobytes() == std.tobytes()
        assert (got_std > 0).all()
    config.update(save_to=str(tmp_path / "sampled"), num_samples=100)
    assert script.main(**config, seed=3)["num_frames"] == 100
    data = SyntheticRawContours(300, arts, seed=3)
    chosen = random.Random(3).sample(list(range(300)), 100)
    for (mean, std), a in zip(expect(chosen), arts):
        assert np.load(tmp_path / "sampled" / f"{a}_mean.npy").tobytes() == mean.tobytes()
        assert np.load(tmp_path / "sampled" / f"{a}_std.npy").tobytes() == std.tobytes()


# ------------------------------------------------------------------------------------------------ 6. the data set
def test_artspeech_dataset_on_the_device_equals_the_per_frame_path(fx, dev, tmp_path, monkeypatch):
    import sys
    import torch.utils.data
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.dataset import ArtSpeechDataset, HBMResidentDataset
    arts = [str(a) for a in fx["articulators"]]
    sentences = [("S0", "seq1", [0, 1, 64, 69, 74]), ("S0", "seq2", [80, 5, 95])]
    data = []
    for subject, sequence, frames in sentences:
        frame_ids = write_tree(str(tmp_path), fx, frames, subject, sequence)
        data.append({"has_all": True, "subject": subject, "sequence": sequence, "frame_ids": frame_ids, "sentence_name": f"{subject}_{sequence}",
                     "phonemes": [f"ph{i % 3:02d}" for i in range(len(frames))]})

    class Collector:
        def __init__(self, datadir):
            assert datadir == str(tmp_path)

        def collect_data(self, sequences):
            return data + [{"has_all": False}]

    monkeypatch.setitem(sys.modules, "database_collector", types.SimpleNamespace(DATABASE_COLLECTORS={"artspeech2": Collector}))
    vocabulary = {"<blank>": 0, "<unk>": 1, "ph00": 2, "ph01": 3}
    args = (str(tmp_path), "artspeech2", [("S0", "seq1"), ("S0", "seq2")], vocabulary, arts)
    for clip_tails in (True, False):
        host = ArtSpeechDataset(*args, clip_tails=clip_tails, voiced_tokens=["ph01"])
        device = ArtSpeechDataset(*args, clip_tails=clip_tails, voiced_tokens=["ph01"], device=dev)
        assert len(host) == len(device) == 2
        for i, (_, _, frames) in enumerate(sentences):
            a, b = host[i], device[i]
            assert b[2].device == dev and b[4].device == dev and a[2].device.type == "cpu"
            assert a[0] == b[0] and a[3] == b[3] and a[6] == b[6] and torch.equal(a[1], b[1]) and torch.equal(a[7], b[7])
            same_bits(b[2].cpu().numpy(), a[2].numpy(), "targets")
            same_bits(b[4].cpu().numpy(), a[4].numpy(), "references")
            assert a[2].shape == (len(frames), 5, 2, 50) and a[4].shape == (len(frames), 1, 2, 50)
            if clip_tails:
                same_bits(a[2].numpy(), fx["prepared"][frames], "targets against the fixture")
                same_bits(a[4].numpy(), fx["references"][frames], "references against the fixture")
    resident = HBMResidentDataset(device, dev)     # the device items fill the resident data set as they are
    assert len(resident) == 2
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="num_workers=0"):
        device[0]
