"""Fixture of the result tables, produced by the reference's own report_phoneme_to_articulation.py on a results tree that the
reference's own save_outputs / tract_variables (phoneme_to_articulation/__init__.py) wrote from seeded contours.  Run from the
repository root with the reference checkout at make_golden.REF:

    python tests/golden/make_golden_report.py

Writes tests/golden/report.npz.  Uses make_golden.py's name-only shims (funcy.lfilter among them) plus a ``seaborn`` whose
color_palette returns six tuples and an empty ``matplotlib.pyplot``; the script's plot_tract_variables_for_sentence is stubbed to
a no-op.

The tree: 4 sentences of 9, 5, 5 and 1 frames, the five tract-variable articulators plus the injected upper incisor, N = 50; the
targets are the predictions plus noise, so the correlations are neither 0 nor 1.  Sentences arrive out of name order, the frames
of one sentence out of frame order, and one sentence's frames straddle 9999 / 10000 (integer order differs from text order); the
report is asked for the articulators in an unsorted order.  The 1-frame sentence has no correlation (NaN).

Stored: the contours, ids, frames and phonemes in arrival order, the text of the per-sentence tract_variables.csv files, the text,
header rows and parsed values of the three reports, the per-sentence correlations from the reference's pandas expression, and the
reference's largest deviation from the fp64 restatement tests/report_fp64.py per metric column (max |ref - fp64| / max |fp64|;
asserted <= 1e-3 here: N = 50 sends torch.cdist down its matmul path)."""
import csv
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import report_fp64 as Y  # noqa: E402
from make_golden import _load, _shim, save  # noqa: E402
from make_golden_pc_training import load_reference  # noqa: E402

TV_ARTS = ["lower-lip", "pharynx", "soft-palate-midline", "tongue", "upper-incisor", "upper-lip"]   # sorted: the channels
REPORT_ARTS = ["tongue", "lower-lip", "upper-lip", "soft-palate-midline", "pharynx"]               # as asked for: unsorted
N = 50
SEED = 171
SENTENCES = [   # (name, first frame, arrival order of its frames)
    ("sent2", 9997, [0, 1, 2, 3, 4, 5, 6, 7, 8]),
    ("sent0", 12, [3, 0, 4, 1, 2]),
    ("sent3", 0, [0]),
    ("sent1", 100, [0, 1, 2, 3, 4]),
]


def load_report_script():
    settings = load_reference()[0]
    plt = _shim("matplotlib.pyplot")
    _shim("matplotlib", pyplot=plt)
    _shim("seaborn", color_palette=lambda *a, **k: [(0.1 * i, 0.1 * i, 0.1 * i) for i in range(6)])
    _shim("ujson", dump=json.dump, load=json.load)
    sys.modules["vt_tools"].COLORS = {}
    _shim("vt_shape_gen")
    _shim("vt_shape_gen.helpers", load_articulator_array=None)
    _shim("vt_tools.bs_regularization", regularize_Bsplines=None)
    _shim("phoneme_to_articulation.tail_clipper", TailClipper=None)
    _load("tract_variables", "tract_variables.py")
    ref_init = _load("ref_p2a_init_for_report", "phoneme_to_articulation/__init__.py")
    _load("metrics", "metrics.py")
    script = _load("ref_report_script", "report_phoneme_to_articulation.py")
    script.plot_tract_variables_for_sentence = lambda *a, **k: None
    return settings, ref_init, script


def _read(path):
    with open(path, newline="") as f:
        return f.read()


def main():
    settings, ref_init, script = load_report_script()
    g = torch.Generator().manual_seed(SEED)
    inc = TV_ARTS.index("upper-incisor")
    rows = {"sentence": [], "frame": [], "phoneme": [], "pred": [], "true": []}
    with tempfile.TemporaryDirectory() as results_dir:
        base = os.path.join(results_dir, "test_outputs", "0")
        for name, first, arrival in SENTENCES:
            length = len(arrival)
            pred = torch.rand(1, length, len(TV_ARTS), 2, N, generator=g)
            true = pred + 0.05 * torch.randn(1, length, len(TV_ARTS), 2, N, generator=g)
            true[:, :, inc] = pred[:, :, inc]
            frames = [["%04d" % (first + j) for j in arrival]]
            phonemes = [[f"ph{int(t)}" for t in torch.randint(0, 9, (length,), generator=g)]]
            ref_init.save_outputs([name], frames, pred, true, [length], phonemes, TV_ARTS, base, False)
            ref_init.tract_variables([name], frames, pred, true, [length], phonemes, TV_ARTS, base)
            rows["sentence"] += [name] * length
            rows["frame"] += frames[0]
            rows["phoneme"] += phonemes[0]
            rows["pred"].append(pred[0].numpy())
            rows["true"].append(true[0].numpy())
        script.main("artspeech2", results_dir, list(REPORT_ARTS))
        names = sorted(os.listdir(base))
        tv_text = [_read(os.path.join(base, n, "tract_variables.csv")) for n in names]
        text = {k: _read(os.path.join(results_dir, f)) for k, f in (("full", "error_report_full.csv"), ("agg", "error_report_agg.csv"),
                                                                     ("corr", "TV_corr_report.csv"))}
        # the per-sentence coefficients behind TV_corr_report.csv: the script's own expression (:143-153, :258-267)
        df = pd.concat([pd.read_csv(os.path.join(base, n, "tract_variables.csv")) for n in names]).sort_values(["sentence", "frame"])
        cfg = settings.DATASET_CONFIG["artspeech2"]
        to_mm = cfg.RES * cfg.PIXEL_SPACING
        corr_sentences = np.full((len(names), 4), np.nan)
        for j, tv in enumerate(Y.TVS):
            df[f"{tv}_pred"], df[f"{tv}_target"] = df[f"{tv}_pred"] * to_mm, df[f"{tv}_target"] * to_mm
            c = df.groupby("sentence")[[f"{tv}_target", f"{tv}_pred"]].corr().reset_index()
            c = c[c.level_1 == f"{tv}_target"][["sentence", f"{tv}_pred"]]
            assert list(c.sentence) == names
            corr_sentences[:, j] = c[f"{tv}_pred"].to_numpy()

    pred, true = np.concatenate(rows["pred"]), np.concatenate(rows["true"])
    full = list(csv.reader(text["full"].splitlines()))
    agg = list(csv.reader(text["agg"].splitlines()))
    corr = list(csv.reader(text["corr"].splitlines()))
    num = lambda cells: [float(c) if c != "" else np.nan for c in cells]   # noqa: E731
    full_values = np.array([num(r[4:]) for r in full[1:]])
    agg_values = np.array([num(r[1:]) for r in agg[2:]])
    corr_values = np.array([num(r[1:]) for r in corr[1:]])

    tv_rows = [r for t in tv_text for r in csv.DictReader(t.splitlines())]
    assert [r["sentence"] for r in tv_rows] == sorted(rows["sentence"])
    lookup = {(r["sentence"], r["frame"]): r for r in tv_rows}
    tvs = {key: np.array([[float(lookup[s, f][f"{tv}_{key}"]) for tv in Y.TVS] for s, f in zip(rows["sentence"], rows["frame"])])
           for key in ("pred", "target")}
    ch = [TV_ARTS.index(a) for a in REPORT_ARTS]
    yard = Y.report(rows["sentence"], rows["frame"], rows["phoneme"], pred[:, ch], true[:, ch], tvs["pred"], tvs["target"], REPORT_ARTS,
                    to_mm)
    assert [r[0] for r in full[1:]] == yard["full"]["sentence_name"] and [int(r[1]) for r in full[1:]] == yard["full"]["frame"]
    assert [r[2] for r in full[1:]] == yard["full"]["phoneme"] and [r[3] for r in full[1:]] == yard["full"]["articulator"]
    assert [r[0] for r in agg[2:]] == yard["agg"]["articulator"]
    full_dev = np.abs(full_values - yard["full"]["values"]).max(axis=0) / np.abs(yard["full"]["values"]).max(axis=0)
    agg_dev = np.abs(agg_values - yard["agg"]["values"]).max(axis=0) / np.abs(yard["agg"]["values"]).max(axis=0)
    assert full_dev.max() <= 1e-3 and agg_dev.max() <= 1e-3, (full_dev, agg_dev, "change SEED, not the bound")
    corr_dev = float(np.nanmax(np.abs(corr_sentences - yard["corr"])))
    report_dev = float(np.nanmax(np.abs(corr_values - yard["corr_report"])))
    assert np.array_equal(np.isnan(corr_sentences), np.isnan(yard["corr"])) and corr_dev <= 1e-11 and report_dev <= 1e-11

    checks = dict(seed=SEED, full_dev=[float(v) for v in full_dev], agg_dev_max=float(agg_dev.max()), corr_dev=corr_dev,
                  corr_report_dev=report_dev, mean_corr=[float(v) for v in corr_values[:, 0]])
    save("report", pred=pred.astype(np.float32), true=true.astype(np.float32), tv_articulators=np.array(TV_ARTS),
         articulators=np.array(REPORT_ARTS), sentence=np.array(rows["sentence"]), frame=np.array(rows["frame"]),
         phoneme=np.array(rows["phoneme"]), to_mm=np.float64(to_mm), database_name=np.array("artspeech2"),
         sentence_dirs=np.array(names), tv_text=np.array(tv_text),
         full_text=np.array(text["full"]), agg_text=np.array(text["agg"]), corr_text=np.array(text["corr"]),
         full_header=np.array(text["full"].splitlines()[0]), agg_header=np.array(text["agg"].splitlines()[:2]),
         corr_header=np.array(text["corr"].splitlines()[0]),
         full_keys=np.array([r[:4] for r in full[1:]]), full_values=full_values,
         agg_names=np.array([r[0] for r in agg[2:]]), agg_values=agg_values,
         corr_names=np.array([r[0] for r in corr[1:]]), corr_values=corr_values, corr_sentences=corr_sentences,
         full_dev=full_dev, agg_dev=agg_dev, checks=np.array(json.dumps(checks)))
    print(json.dumps(checks, indent=1))


if __name__ == "__main__":
    main()
