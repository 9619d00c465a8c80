"""Host checks of the result tables (no GPU): the fp64 restatement tests/report_fp64.py against the fixture recorded from the
reference's own report_phoneme_to_articulation.py (tests/golden/make_golden_report.py) and against pandas on degenerate groups;
the contract of the entry script, its config and the new symbol; the CSV writer's header rows."""
import csv
import importlib
import inspect
import os

import numpy as np
import pytest
import yaml

import report_fp64 as Y
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def fx():
    return load_golden("report")


def tv_values(fx):
    """(pred, target) (rows, 4) in the fixture's arrival order, from the text of the per-sentence tract_variables.csv."""
    rows = {(r["sentence"], r["frame"]): r for text in fx["tv_text"] for r in csv.DictReader(str(text).splitlines())}
    return [np.array([[float(rows[str(s), str(f)][f"{tv}_{key}"]) for tv in Y.TVS] for s, f in zip(fx["sentence"], fx["frame"])])
            for key in ("pred", "target")]


def restated(fx):
    arts, channels = [str(a) for a in fx["articulators"]], [str(a) for a in fx["tv_articulators"]]
    ch = [channels.index(a) for a in arts]
    tv_pred, tv_target = tv_values(fx)
    return Y.report(list(fx["sentence"]), list(fx["frame"]), list(fx["phoneme"]), fx["pred"][:, ch], fx["true"][:, ch], tv_pred,
                    tv_target, arts, float(fx["to_mm"]))


def test_restatement_reproduces_the_references_reports(fx):
    """Text columns and row order equal; correlations and their summary to 1e-11 absolute with the NaN in the same places; the
    error columns within the deviation recorded at generation time (the reference's float32 cdist against direct float64
    differences), itself below 1e-3."""
    y = restated(fx)
    keys = fx["full_keys"]
    assert [str(k) for k in keys[:, 0]] == y["full"]["sentence_name"] and [int(k) for k in keys[:, 1]] == y["full"]["frame"]
    assert [str(k) for k in keys[:, 2]] == y["full"]["phoneme"] and [str(k) for k in keys[:, 3]] == y["full"]["articulator"]
    assert [str(a) for a in fx["agg_names"]] == y["agg"]["articulator"] == sorted(str(a) for a in fx["articulators"])
    assert [str(s) for s in fx["sentence_dirs"]] == y["sentences"] and tuple(str(t) for t in fx["corr_names"]) == Y.TVS
    assert fx["full_dev"].max() <= 1e-3 and fx["agg_dev"].max() <= 1e-3
    for what, ref, got, dev in (("full", fx["full_values"], y["full"]["values"], fx["full_dev"]),
                                ("agg", fx["agg_values"], y["agg"]["values"], fx["agg_dev"])):
        ratio = np.abs(ref - got).max(axis=0) / np.abs(got).max(axis=0)
        print(f"{what}: reference / fp64 deviation per column {ratio}")
        assert (ratio <= dev * (1 + 1e-9)).all(), (what, ratio, dev)
    assert np.array_equal(np.isnan(fx["corr_sentences"]), np.isnan(y["corr"]))
    assert np.isnan(y["corr"]).sum() == 4, "the 1-frame sentence, and only it, has no correlation"
    assert np.nanmax(np.abs(fx["corr_sentences"] - y["corr"])) <= 1e-11
    assert not np.isnan(fx["corr_values"]).any() and np.abs(fx["corr_values"] - y["corr_report"]).max() <= 1e-11


def _pandas_corr(sentences, target, pred, scale):
    """The reference's expression (:143-153, :258-280) for one tract variable: per-sentence coefficients and their summary."""
    import pandas as pd
    df = pd.DataFrame({"sentence": sentences, "t": np.asarray(target, np.float64), "p": np.asarray(pred, np.float64)})
    df["t"], df["p"] = df["t"] * scale, df["p"] * scale
    c = df.groupby("sentence")[["t", "p"]].corr().reset_index()
    c = c[c.level_1 == "t"][["sentence", "p"]]
    return c["p"].to_numpy(), np.array([c["p"].mean(), c["p"].std(), c["p"].min(), c["p"].max()])


def _degenerate_case(with_regular):
    rng = np.random.RandomState(5)
    groups = [("a", rng.rand(1), rng.rand(1)),                                       # one frame
              ("b", rng.rand(5), np.full(5, 0.7)),                                    # constant prediction
              ("c", np.full(7, 0.7), rng.rand(7))]                                    # constant target: 7 x fl32(0.7) x 1.6 / 7 is inexact
    if with_regular:
        groups += [("d", rng.rand(6), rng.rand(6)), ("e", rng.rand(2), rng.rand(2)), ("f", rng.rand(70), rng.rand(70))]
    sentences = [n for n, t, _ in groups for _ in t]
    target = np.concatenate([t for _, t, _ in groups]).astype(np.float32)
    pred = np.concatenate([p for _, _, p in groups]).astype(np.float32)
    seg_first = np.concatenate([[0], np.cumsum([len(t) for _, t, _ in groups])])
    return sentences, target, pred, seg_first


@pytest.mark.parametrize("with_regular", [True, False])
def test_degenerate_groups_agree_with_pandas(with_regular):
    """A 1-frame sentence, a constant prediction and a constant target whose mean is not representable are NaN in pandas and in
    the restatement, at the same positions, none skipped; with only such sentences the whole summary is NaN."""
    sentences, target, pred, seg_first = _degenerate_case(with_regular)
    scale = 1.6
    want, want_summary = _pandas_corr(sentences, target, pred, scale)
    x = target[6:13].astype(np.float64) * scale
    assert (x == x[0]).all() and (x - x.sum() / 7 != 0).all(), "the constant column's centred values must be rounding noise for the case to bite"
    corr, summary = Y.segment_corr(target[:, None], pred[:, None], seg_first, scale)
    assert np.array_equal(np.isnan(want), np.isnan(corr[:, 0])), (want, corr[:, 0])
    assert np.isnan(want[:3]).all() and np.isnan(want).sum() == 3
    assert np.array_equal(np.isnan(want_summary), np.isnan(summary[1:, 0])), (want_summary, summary[:, 0])
    assert summary[0, 0] == (3 if with_regular else 0)
    if with_regular:
        assert np.abs(want[3:] - corr[3:, 0]).max() <= 1e-11 and np.abs(want_summary - summary[1:, 0]).max() <= 1e-11
    else:
        assert np.isnan(summary[1:, 0]).all()


def test_script_contract():
    """main's leading keywords are the reference's, every key of the synthetic config is one of main's parameters, the script
    imports without a device."""
    import torch
    script = importlib.import_module("report_phoneme_to_articulation")
    params = list(inspect.signature(script.main).parameters)
    assert params[:3] == ["database_name", "results_dir", "articulators"]
    assert not torch.cuda.is_initialized()
    with open(os.path.join(ROOT, "configs", "report_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= set(params) and cfg["results_dir"] == "results/test_synthetic"
    with open(os.path.join(ROOT, "configs", "test_synthetic.yaml")) as f:
        test_cfg = yaml.safe_load(f)
    assert cfg["results_dir"] == test_cfg["save_to"] and cfg["articulators"] == test_cfg["articulators"]


def test_symbol_is_declared_bound_and_built():
    from artspeech_amd import _lib, build
    with open(os.path.join(ROOT, "include", "artspeech_hip.h")) as f:
        header = f.read()
    assert "int as_segment_corr(const float* a, const float* b, int64_t rows, int32_t K, double scale" in header
    assert "report_phoneme_to_articulation.py:256-285" in header
    res, args = _lib.PROTOTYPES["as_segment_corr"]
    assert len(args) == 10
    assert "report.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "report.hip"))


def test_test_loops_take_report_dir():
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.evaluation import run_test
    from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import test as mean_contour_test
    from artspeech_amd.phoneme_to_articulation.transformer.evaluation import run_transformer_test
    for fn in (run_test, run_transformer_test, mean_contour_test):
        assert inspect.signature(fn).parameters["report_dir"].default is None


def test_agg_writer_reproduces_the_fixtures_text(fx, tmp_path):
    """The two header rows pandas writes for the grouped table, an empty field for NaN, and -- fed the fixture's parsed values --
    the reference's file byte for byte."""
    from artspeech_amd.phoneme_to_articulation.report import write_error_report_agg
    path = str(tmp_path / "agg.csv")
    write_error_report_agg(path, [str(a) for a in fx["agg_names"]], fx["agg_values"])
    with open(path, newline="") as f:
        text = f.read()
    assert text.splitlines()[:2] == [str(line) for line in fx["agg_header"]]
    assert text == str(fx["agg_text"])
    values = np.array(fx["agg_values"][:1])
    values[0, 1] = values[0, 5] = np.nan
    write_error_report_agg(path, ["only"], values)
    with open(path, newline="") as f:
        cells = list(csv.reader(f))[2]
    assert cells[0] == "only" and cells[2] == "" and cells[6] == "" and "" not in cells[3:6]
