"""GPU checks of the result tables: as_segment_corr (csrc/report.hip) against the fp64 restatement tests/report_fp64.py; the
fixture recorded from the reference's own report_phoneme_to_articulation.py (tests/golden/make_golden_report.py) through
report_from_results_dir; the in-memory path of the test script's pass against the file path, byte for byte; run_test with and
without report_dir."""
import csv
import filecmp
import os

import numpy as np
import pytest
import torch
import yaml

import report_fp64 as Y
from conftest import ROOT, WORST, load_golden
from test_report_host import _degenerate_case, restated

pytestmark = pytest.mark.gpu

FILES = ("tract_variables.csv", "error_report_full.csv", "error_report_agg.csv", "TV_corr_report.csv")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return load_golden("report")


@pytest.fixture(scope="module")
def to_mm():
    from artspeech_amd.settings import DATASET_CONFIG
    cfg = DATASET_CONFIG["artspeech2"]
    return cfg.RES * cfg.PIXEL_SPACING


# ------------------------------------------------------------------------------------------------ 1. as_segment_corr
def _check_corr(a, b, seg_first, scale, dev, what):
    """corr and summary within 1e-11 absolute of the restatement, NaN at the same places, min / max elements of corr bit for
    bit, two runs bit-identical.  Returns (corr, summary) as numpy."""
    from artspeech_amd.phoneme_to_articulation.report import segment_correlation
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    sd = torch.from_numpy(np.asarray(seg_first, np.int64)).to(dev)
    corr, summary = (t.cpu().numpy() for t in segment_correlation(ad, bd, sd, scale))
    corr2, summary2 = (t.cpu().numpy() for t in segment_correlation(ad, bd, sd, scale))
    assert corr.tobytes() == corr2.tobytes() and summary.tobytes() == summary2.tobytes(), f"{what}: two runs differ"
    want, want_summary = Y.segment_corr(a, b, seg_first, scale)
    assert corr.shape == want.shape and summary.shape == want_summary.shape == (5, a.shape[1])
    assert np.array_equal(np.isnan(corr), np.isnan(want)), (what, corr, want)
    assert np.array_equal(np.isnan(summary), np.isnan(want_summary)), (what, summary, want_summary)
    err = max(float(np.nanmax(np.abs(corr - want), initial=0.0)), float(np.nanmax(np.abs(summary - want_summary), initial=0.0)))
    print(f"{what}: max |got - fp64| = {err:.3e}")
    WORST[f"segment corr {what} / 1e-11"] = max(WORST.get(f"segment corr {what} / 1e-11", 0.0), err / 1e-11)
    assert err <= 1e-11, (what, err)
    for k in range(a.shape[1]):
        if summary[0, k] > 0:
            assert summary[3, k].tobytes() in [c.tobytes() for c in corr[:, k]] and summary[3, k] == np.nanmin(corr[:, k])
            assert summary[4, k].tobytes() in [c.tobytes() for c in corr[:, k]] and summary[4, k] == np.nanmax(corr[:, k])
    return corr, summary


def _values(rows, K, seed):
    """20 + z, z ~ N(0, 1), rounded to float32: an uncentred or float32 accumulation is visible at this magnitude."""
    rng = np.random.RandomState(seed)
    return (20 + rng.randn(rows, K)).astype(np.float32), (20 + rng.randn(rows, K)).astype(np.float32)


@pytest.mark.parametrize("K", [4, 1])
def test_segment_corr_every_segment_length(K, dev, to_mm):
    """Segments of 1, 2, 3, 63, 64, 65 and 130 rows in one call: the empty and tiny cases, both sides of the wave width and a
    second pass of the lane loop."""
    lengths = [1, 2, 3, 63, 64, 65, 130]
    seg_first = np.concatenate([[0], np.cumsum(lengths)])
    a, b = _values(int(seg_first[-1]), K, 10 + K)
    b = (0.6 * a + 0.4 * b).astype(np.float32)   # correlated, not perfectly
    corr, summary = _check_corr(a, b, seg_first, to_mm, dev, f"lengths K={K}")
    assert np.isnan(corr[0]).all() and not np.isnan(corr[1:]).any() and (summary[0] == 6).all()
    assert (np.abs(corr[1, :]) > 1 - 1e-9).all(), "two rows correlate perfectly"


def _butterfly_mean_7(x):
    """The kernel's mean of 7 equal values: one per lane, added by the xor butterfly (4, 2, 1)."""
    return (((x + x) + (x + x)) + ((x + x) + x)) / 7.0


def test_segment_corr_constant_column(dev):
    """One segment whose target column holds one value, chosen so that the two-pass formula in the kernel's own order of
    addition would answer rounding noise: NaN all the same, like pandas; the prediction's other column is unaffected."""
    scale = 1.6
    v = next(np.float32(c) for c in (0.7, 1.1, 0.61, 0.3, 0.9) if _butterfly_mean_7(float(np.float32(c)) * scale) != float(np.float32(c)) * scale)
    a, b = _values(7 + 9, 2, 3)
    a[:7, 0] = v
    corr, summary = _check_corr(a, b, [0, 7, 16], scale, dev, "constant column")
    assert np.isnan(corr[0, 0]) and not np.isnan(corr[0, 1]) and not np.isnan(corr[1]).any()
    assert summary[0].tolist() == [1, 2] and np.isnan(summary[2, 0])
    b[7:, 1] = b[7, 1]      # the other side, in the other segment
    corr, summary = _check_corr(a, b, [0, 7, 16], scale, dev, "constant column")
    assert np.isnan(corr[1, 1]) and summary[0].tolist() == [1, 1]


def test_segment_corr_uncovered_rows_and_empty_segment(dev, to_mm):
    """Segments need not cover the table: the rows before the first segment, after the last one and -- the gap between two
    segments that S + 1 boundaries can express -- those of a segment a second call leaves out are NaN, which no coefficient
    shows; an empty segment in the middle is NaN and is not counted."""
    a, b = _values(40, 4, 4)
    a[:3], a[33:], b[:3], b[33:] = np.nan, np.nan, np.nan, np.nan
    corr, summary = _check_corr(a, b, [3, 12, 12, 20, 33], to_mm, dev, "uncovered rows")
    assert np.isnan(corr[1]).all() and not np.isnan(corr[[0, 2, 3]]).any() and (summary[0] == 3).all()
    a[12:20], b[12:20] = np.nan, np.nan    # the gap: rows 12..19 belong to no segment of these two calls
    left, _ = _check_corr(a, b, [3, 12], to_mm, dev, "uncovered rows")
    right, _ = _check_corr(a, b, [20, 33], to_mm, dev, "uncovered rows")
    assert left.tobytes() == corr[0:1].tobytes() and right.tobytes() == corr[3:4].tobytes(), "a coefficient depends on its own rows only"


@pytest.mark.parametrize("K", [4, 1])
def test_segment_corr_no_segment_and_one_segment(K, dev, to_mm):
    a, b = _values(9, K, 5)
    corr, summary = _check_corr(a, b, [0], to_mm, dev, "S=0")
    assert corr.shape == (0, K) and (summary[0] == 0).all() and np.isnan(summary[1:]).all()
    corr, summary = _check_corr(a, b, [0, 9], to_mm, dev, "S=1")
    assert (summary[0] == 1).all() and np.isnan(summary[2]).all(), "std of one coefficient is NaN"
    assert summary[1].tobytes() == corr[0].tobytes() == summary[3].tobytes() == summary[4].tobytes()


@pytest.mark.parametrize("with_regular", [True, False])
def test_segment_corr_degenerate_sentences(with_regular, dev):
    """The host test's degenerate groups (a 1-frame sentence, a constant prediction, a constant target whose mean is not
    representable) through the kernel: NaN where pandas has NaN; with only such sentences count is 0 and the summary all NaN."""
    _, target, pred, seg_first = _degenerate_case(with_regular)
    corr, summary = _check_corr(target[:, None].copy(), pred[:, None].copy(), seg_first, 1.6, dev, "degenerate sentences")
    assert np.isnan(corr[:3]).all() and np.isnan(corr).sum() == 3
    assert summary[0, 0] == (3 if with_regular else 0) and np.isnan(summary[1:, 0]).all() == (not with_regular)


# ------------------------------------------------------------------------------------------------ 2. the fixture, from files
def _rebuild_tree(fx, root, only=None):
    """The results tree the reference's test pass left, from the fixture: per-sentence tract_variables.csv and contour dumps."""
    names = [str(n) for n in fx["sentence_dirs"]]
    channels = [str(a) for a in fx["tv_articulators"]]
    for name, text in zip(names, fx["tv_text"]):
        if only is not None and name not in only:
            continue
        os.makedirs(os.path.join(root, "test_outputs", "0", name, "contours"))
        with open(os.path.join(root, "test_outputs", "0", name, "tract_variables.csv"), "w", newline="") as f:
            f.write(str(text))
    for i, (name, frame) in enumerate(zip(fx["sentence"], fx["frame"])):
        if only is not None and str(name) not in only:
            continue
        for c, art in enumerate(channels):
            stem = os.path.join(root, "test_outputs", "0", str(name), "contours", f"{frame}_{art}")
            np.save(stem + ".npy", fx["pred"][i, c])
            np.save(stem + "_true.npy", fx["true"][i, c])


def _read_csv(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _num(cells):
    return np.array([float(c) if c != "" else np.nan for c in cells])


@pytest.fixture(scope="module")
def fixture_report(fx, dev, tmp_path_factory):
    from artspeech_amd.phoneme_to_articulation.report import report_from_results_dir
    root = str(tmp_path_factory.mktemp("report_fixture"))
    _rebuild_tree(fx, root)
    paths = report_from_results_dir(str(fx["database_name"]), root, [str(a) for a in fx["articulators"]], dev).write(root)
    return root, paths


def test_fixture_text_columns_and_headers(fx, fixture_report):
    root, paths = fixture_report
    assert sorted(paths) == sorted(FILES) and all(os.path.dirname(p) == root for p in paths.values())
    full, agg, corr = (_read_csv(paths[f]) for f in FILES[1:])
    with open(paths["error_report_full.csv"]) as f:
        assert f.readline().rstrip("\n") == str(fx["full_header"])
    with open(paths["error_report_agg.csv"]) as f:
        assert [f.readline().rstrip("\n") for _ in range(2)] == [str(line) for line in fx["agg_header"]]
    with open(paths["TV_corr_report.csv"]) as f:
        assert f.readline().rstrip("\n") == str(fx["corr_header"])
    assert [r[:4] for r in full[1:]] == [[str(c) for c in r] for r in fx["full_keys"]]
    assert [r[0] for r in agg[2:]] == [str(a) for a in fx["agg_names"]] and [r[0] for r in corr[1:]] == list(Y.TVS)
    # the collected table: the header once, then the rows of the per-sentence files as they are, in directory order
    with open(paths["tract_variables.csv"], newline="") as f:
        lines = f.read().splitlines()
    texts = [str(t).splitlines() for t in fx["tv_text"]]
    assert lines == [texts[0][0]] + [row for t in texts for row in t[1:]]


def test_fixture_correlations(fx, fixture_report):
    corr = np.array([_num(r[1:]) for r in _read_csv(fixture_report[1]["TV_corr_report.csv"])[1:]])
    err = float(np.abs(corr - fx["corr_values"]).max())
    WORST["report fixture TV_corr / 1e-11"] = err / 1e-11
    assert err <= 1e-11, err


def test_fixture_error_columns(fx, fixture_report):
    """Per frame within 1e-6 relative of the fp64 restatement (the bound the metric kernels are held to) and within
    2 x (the reference's own recorded deviation from fp64) + 1e-6 x max of the reference's values, per column; the aggregate rows
    within the latter."""
    y = restated(fx)
    full = np.array([_num(r[4:]) for r in _read_csv(fixture_report[1]["error_report_full.csv"])[1:]])
    agg = np.array([_num(r[1:]) for r in _read_csv(fixture_report[1]["error_report_agg.csv"])[2:]])
    rel = np.abs(full - y["full"]["values"]) / np.abs(y["full"]["values"])
    print(f"per frame: max relative error against fp64 per column {rel.max(axis=0)}")
    WORST["report fixture per-frame / fp64 1e-6"] = float(rel.max()) / 1e-6
    assert rel.max() <= 1e-6, rel.max(axis=0)
    for what, got, ref, dev_ in (("full", full, fx["full_values"], fx["full_dev"]), ("agg", agg, fx["agg_values"], fx["agg_dev"])):
        scale = np.abs(ref).max(axis=0)
        bound = 2 * dev_ * scale + 1e-6 * scale
        ratio = float((np.abs(got - ref).max(axis=0) / bound).max())
        print(f"{what}: worst |got - reference| / (2 x reference's deviation + 1e-6 max) = {ratio:.3e}")
        WORST[f"report fixture {what} / reference bound"] = ratio
        assert ratio <= 1.0, (what, ratio)
    assert not np.isnan(agg).any()


def test_one_row_groups_have_no_std(fx, dev, tmp_path):
    """Only the 1-frame sentence: every articulator's group has one row, so std is an empty field (NaN) while mean = min = max;
    no sentence has a correlation, so TV_corr_report.csv holds empty fields only."""
    from artspeech_amd.phoneme_to_articulation.report import report_from_results_dir
    _rebuild_tree(fx, str(tmp_path), only={"sent3"})
    paths = report_from_results_dir("artspeech2", str(tmp_path), [str(a) for a in fx["articulators"]], dev).write(str(tmp_path))
    agg = _read_csv(paths["error_report_agg.csv"])[2:]
    assert len(agg) == 5
    for row in agg:
        for m in range(4):
            mean, std, mn, mx = row[1 + 4 * m: 5 + 4 * m]
            assert std == "" and mean == mn == mx != ""
    assert [r[1:] for r in _read_csv(paths["TV_corr_report.csv"])[1:]] == [[""] * 4] * 4
    assert len(_read_csv(paths["error_report_full.csv"])) == 1 + 5


def test_missing_contour_and_bad_frame_id(fx, dev, tmp_path):
    from artspeech_amd.phoneme_to_articulation.report import report_from_results_dir
    _rebuild_tree(fx, str(tmp_path), only={"sent3"})
    sdir = tmp_path / "test_outputs" / "0" / "sent3"
    os.rename(sdir / "contours" / "0000_tongue_true.npy", sdir / "contours" / "kept.npy")
    with pytest.raises(FileNotFoundError, match="0000_tongue_true.npy"):
        report_from_results_dir("artspeech2", str(tmp_path), ["tongue"], dev)
    os.rename(sdir / "contours" / "kept.npy", sdir / "contours" / "0000_tongue_true.npy")
    text = (sdir / "tract_variables.csv").read_text()
    (sdir / "tract_variables.csv").write_text(text.replace("sent3,0000,", "sent3,0000a,"))
    with pytest.raises(ValueError, match="0000a"):
        report_from_results_dir("artspeech2", str(tmp_path), ["tongue"], dev)


# ------------------------------------------------------------------------------------------------ 3. both paths
def test_test_script_and_report_script_write_the_same_files(dev, tmp_path, monkeypatch):
    """test_phoneme_to_articulation.main, its run_test given report_dir=save_to, writes the four files from the frames of its own
    pass; report_phoneme_to_articulation.main reads the same pass back from its dumps: byte-identical.  (The test scripts are
    kept as they are, so the key that would pass report_dir is set here, on the function main() calls.)"""
    import functools
    import report_phoneme_to_articulation as report_cli
    import test_phoneme_to_articulation as cli
    with open(os.path.join(ROOT, "configs", "test_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    memory = tmp_path / "memory"
    cfg.update(test_seq_dict={"num_sentences": 3}, batch_size=2, save_to=str(memory), synthetic={"min_len": 5, "max_len": 9},
               model_kwargs={"embed_dim": 16, "hidden_size": 32})
    monkeypatch.setattr(cli, "run_test", functools.partial(cli.run_test, report_dir=str(memory)))
    cli.main(**cfg)
    assert all(os.path.exists(memory / f) for f in FILES)
    files = tmp_path / "files"
    os.makedirs(files)
    os.symlink(memory / "test_outputs", files / "test_outputs")
    with open(os.path.join(ROOT, "configs", "report_synthetic.yaml")) as f:
        report_cfg = yaml.safe_load(f)
    assert report_cfg["articulators"] == cfg["articulators"]
    report_cfg["results_dir"] = str(files)
    report_cli.main(**report_cfg)
    for f in FILES:
        assert filecmp.cmp(memory / f, files / f, shallow=False), f"{f} differs between the two paths"
    full = _read_csv(memory / "error_report_full.csv")
    n_frames = sum(len(_read_csv(memory / "test_outputs" / "0" / s / "phonemes.csv")) - 1 for s in os.listdir(memory / "test_outputs" / "0"))
    assert len(full) == 1 + n_frames * len(cfg["articulators"]) and 15 <= n_frames <= 27


def _tree(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out


def test_report_dir_none_changes_nothing(dev, tmp_path):
    """run_test on one loader with and without report_dir: equal info dicts, the same per-sentence files; the four tables appear
    only where they were asked for."""
    from torch.utils.data import DataLoader
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.dataset import SyntheticArtSpeechDataset, pad_sequence_collate_fn
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.evaluation import run_test
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech
    from artspeech_amd.phoneme_to_articulation.metrics import EuclideanDistance
    from artspeech_amd.training import build_vocabulary
    arts = ["lower-lip", "pharynx", "soft-palate-midline", "tongue", "upper-lip"]
    vocabulary = build_vocabulary(None)
    dataset = SyntheticArtSpeechDataset(3, vocabulary, arts, min_len=4, max_len=8, seed=2)
    loader = DataLoader(dataset, batch_size=2, shuffle=False, collate_fn=pad_sequence_collate_fn)
    torch.manual_seed(0)
    model = ArtSpeech(len(vocabulary), len(arts), embed_dim=16, hidden_size=32).to(dev)
    plain = run_test(0, model, loader, EuclideanDistance("none"), str(tmp_path / "plain"), arts, device=dev)
    told = run_test(0, model, loader, EuclideanDistance("none"), str(tmp_path / "told"), arts, device=dev,
                    report_dir=str(tmp_path / "tables"))
    assert plain == told
    a, b = _tree(tmp_path / "plain"), _tree(tmp_path / "told")
    assert a == b and any(k.endswith("tract_variables.csv") for k in a)
    assert sorted(os.listdir(tmp_path / "tables")) == sorted(FILES)
