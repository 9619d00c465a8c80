"""Result tables of a test pass of the model-free path on MI355X (reference: report_phoneme_to_articulation.py:128-285).

The reference reloads two ``.npy`` files per frame and articulator, measures one frame at a time on the host and groups in pandas.
Here the per-frame point-to-closest-point and mean Euclidean distances come from the device functions of ``artspeech_amd/metrics.py``
for a whole batch of frames, the per-articulator statistics from ``as_pc_eval_accumulate`` over the retained per-frame table, and
the per-sentence correlation of each tract variable with its summary from ``as_segment_corr`` (csrc/report.hip); the tables cross
to the host once, when the files are written:

  tract_variables.csv      the rows of the per-sentence files, as they are, in sentence-directory order
  error_report_full.csv    sentence_name, frame, phoneme, articulator, p2cp, p2cp_mm, euclidean, euclidean_mm
  error_report_agg.csv     mean / std / min / max of the four metric columns per articulator (sorted)
  TV_corr_report.csv       mean / std / min / max over the sentences of the correlation of LA, TTCD, TBCD and VEL

``ErrorReport`` is fed either by a test loop while it runs (``report_dir`` of run_test, run_transformer_test and the mean-contour
``test``: nothing is read back from disk) or by ``report_from_results_dir`` from the files a test pass has left.  The plots of the
reference (tract variables over time per sentence) are not ported: matplotlib and seaborn are not part of this engine."""
import csv
import os

import numpy as np
import torch

from .. import _lib
from .. import metrics as root_metrics
from ..settings import DATASET_CONFIG
from ..tract_variables import TV_NAMES

METRICS = ("p2cp", "p2cp_mm", "euclidean", "euclidean_mm")
STATS = ("mean", "std", "min", "max")
FILES = ("tract_variables.csv", "error_report_full.csv", "error_report_agg.csv", "TV_corr_report.csv")


def segment_correlation(a, b, seg_first, scale=1.0):
    """Pearson's r of the columns of ``a`` and ``b`` (rows, K) float32 inside every segment: segment s owns the rows
    [seg_first[s], seg_first[s + 1]) (int64 (S + 1,); segments need not cover all rows), every value is x * scale in float64.
    Device tensors only.  Returns (corr (S, K), summary (5, K) = count | mean | std | min | max of the finite corr), float64 on
    the device; NaN where pandas answers NaN (fewer than 2 rows, a constant column)."""
    for name, t in (("a", a), ("b", b), ("seg_first", seg_first)):
        _lib.require_gpu(t, name)
    if a.dim() != 2 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"segment_correlation expects two (rows, K) float32 tensors, got {tuple(a.shape)} {a.dtype} and "
                         f"{tuple(b.shape)} {b.dtype}")
    if seg_first.dim() != 1 or seg_first.numel() < 1 or seg_first.dtype != torch.int64:
        raise ValueError("segment_correlation: seg_first is an int64 vector of S + 1 row numbers")
    a, b, seg_first = a.contiguous(), b.contiguous(), seg_first.contiguous()
    rows, K = a.shape
    S = seg_first.numel() - 1
    corr = torch.empty((S, K), dtype=torch.float64, device=a.device)
    summary = torch.empty((5, K), dtype=torch.float64, device=a.device)
    _lib.call("as_segment_corr", a, b, rows, K, float(scale), seg_first, S, corr, summary)
    return corr, summary


def _cell(v):
    """A CSV field as pandas writes it: an empty field for NaN."""
    return "" if isinstance(v, float) and v != v else v


def write_error_report_agg(path, articulators, values):
    """error_report_agg.csv: the two header rows of ``groupby("articulator").agg({metric: [mean, std, min, max]})
    .reset_index().to_csv(index=False)``, then one row per articulator; values[i] holds METRICS x STATS."""
    with open(path, "w", newline="") as f:
        writer = csv.writer(f, lineterminator="\n")
        writer.writerow(["articulator", *(m for m in METRICS for _ in STATS)])
        writer.writerow(["", *(s for _ in METRICS for s in STATS)])
        for art, row in zip(articulators, values):
            writer.writerow([art, *(_cell(float(v)) for v in row)])


class ErrorReport:
    """The per-frame table of a test pass, retained on the device, and the reference's four files from it.

    ``articulators`` fixes the rows of a frame in error_report_full.csv; ``channels`` names the channels of the tensors given to
    add() when their order differs (the data sets sort their articulators)."""

    def __init__(self, articulators, dataset_config, device, channels=None):
        self.articulators, self.device = list(articulators), device
        channels = self.articulators if channels is None else list(channels)
        self.columns = [channels.index(a) for a in self.articulators]
        self.n_channels = len(channels)
        self.to_mm = dataset_config.RES * dataset_config.PIXEL_SPACING
        self.sentences, self.frames, self.phonemes = [], [], []
        self.errors, self.tv_pred, self.tv_target = [], [], []      # device: (frames, 2 A) and (frames, 4) per add()
        self.tv_text = {}                                            # sentence -> [header, rows] of its tract_variables.csv

    def add(self, outputs, targets, lengths, sentences_ids, frame_ids, phonemes, tv=None, metrics=None):
        """outputs, targets (B, T, channels, 2, N) on the device; frames t < lengths[b] are retained.  ``tv`` = (pred, target,
        texts): the tract variables (B, T, 4) float32 on the device and the text of each sentence's tract_variables.csv;
        either every call brings it or none.  ``metrics`` = (p2cp, euclidean) (B, T, channels) where the caller has them."""
        B, T = outputs.shape[:2]
        if outputs.shape[2] != self.n_channels:
            raise ValueError(f"ErrorReport.add: {outputs.shape[2]} channels, expected {self.n_channels}")
        if (tv is None) != (not self.tv_text) and self.sentences:
            raise ValueError("ErrorReport.add: tract variables must come with every call or with none")
        if metrics is None:
            with torch.no_grad():
                metrics = root_metrics.p2cp_distance(outputs, targets), root_metrics.euclidean_distance(outputs, targets)
        keep = []
        for b, (sid, length) in enumerate(zip(sentences_ids, lengths)):
            for t in range(int(length)):
                try:
                    frame = int(frame_ids[b][t])
                except ValueError:
                    raise ValueError(f"sentence {sid}: frame id {frame_ids[b][t]!r} is not an integer") from None
                keep.append(b * T + t)
                self.sentences.append(str(sid))
                self.frames.append(frame)
                self.phonemes.append(phonemes[b][t])
        keep = torch.tensor(keep, dtype=torch.int64).to(self.device, non_blocking=True)
        cols = torch.tensor(self.columns, dtype=torch.int64).to(self.device, non_blocking=True)
        table = torch.cat([m.detach().float().reshape(B * T, -1).index_select(1, cols) for m in metrics], dim=1)
        self.errors.append(table.index_select(0, keep))
        if tv is not None:
            pred, target, texts = tv
            self.tv_pred.append(pred.detach().float().reshape(B * T, 4).index_select(0, keep))
            self.tv_target.append(target.detach().float().reshape(B * T, 4).index_select(0, keep))
            for sid, text in zip(sentences_ids, texts):
                lines = text.splitlines()
                self.tv_text.setdefault(str(sid), [lines[0], []])[1].extend(lines[1:])   # a sentence may arrive in parts

    def tables(self):
        """Everything write() puts into files, computed on the device and copied to the host once: a dict with ``order`` (into
        the retained frames: sentences by name, frames by integer value), ``sentences`` (sorted names), ``errors`` (rows, A, 2)
        p2cp | euclidean in that order, ``agg`` (A, 16) METRICS x STATS in the order of self.articulators, and with tract
        variables ``corr`` (S, 4) and ``corr_report`` (4, 4) TV x STATS."""
        R, A = len(self.sentences), len(self.articulators)
        if R == 0:
            raise ValueError("ErrorReport: no frames were added")
        order = sorted(range(R), key=lambda i: (self.sentences[i], self.frames[i]))
        names = sorted(set(self.sentences))
        first = {}
        for row, i in enumerate(order):
            first.setdefault(self.sentences[i], row)
        seg_first = [first[n] for n in names] + [R]
        order_dev = torch.tensor(order, dtype=torch.int64).to(self.device, non_blocking=True)
        errors = torch.cat(self.errors).index_select(0, order_dev).contiguous()                  # (R, 2 A) float32
        state = torch.zeros(5, 2 * A, dtype=torch.float64, device=self.device)
        _lib.call("as_pc_eval_accumulate", errors, 2 * A, state, None, 0, None, R, None, 0)
        parts = [errors.double().flatten(), state.flatten()]
        if self.tv_text:
            seg = torch.tensor(seg_first, dtype=torch.int64).to(self.device, non_blocking=True)
            corr, summary = segment_correlation(torch.cat(self.tv_target).index_select(0, order_dev),
                                                torch.cat(self.tv_pred).index_select(0, order_dev), seg, self.to_mm)
            parts += [corr.flatten(), summary.flatten()]
        host = torch.cat(parts).cpu().numpy()                                                    # the one copy
        errors, host = host[:R * 2 * A].reshape(R, 2, A).transpose(0, 2, 1), host[R * 2 * A:]
        state, host = host[:10 * A].reshape(5, 2, A), host[10 * A:]
        n, mean, m2, mn, mx = state
        with np.errstate(invalid="ignore", divide="ignore"):
            std = np.where(n > 1, np.sqrt(m2 / (n - 1)), np.nan)
        px = np.stack([mean, std, mn, mx], axis=-1)                                              # (2, A, 4) in pixels
        agg = np.stack([px[0], px[0] * self.to_mm, px[1], px[1] * self.to_mm], axis=1)           # (A, 4 metrics, 4 stats)
        out = {"order": order, "sentences": names, "errors": errors, "agg": agg.reshape(A, 16)}
        if self.tv_text:
            S = len(names)
            out["corr"] = host[:4 * S].reshape(S, 4)
            out["corr_report"] = host[4 * S:].reshape(5, 4)[1:].T.copy()
        return out

    def write(self, results_dir):
        """Write the four files (the two error reports only when no tract variables were given).  Returns their paths."""
        t = self.tables()
        os.makedirs(results_dir, exist_ok=True)
        paths = {name: os.path.join(results_dir, name) for name in FILES}
        if not self.tv_text:
            del paths["tract_variables.csv"], paths["TV_corr_report.csv"]
        to_mm = self.to_mm
        with open(paths["error_report_full.csv"], "w", newline="") as f:
            writer = csv.writer(f, lineterminator="\n")   # DataFrame.to_csv(index=False) layout
            writer.writerow(["sentence_name", "frame", "phoneme", "articulator", *METRICS])
            for row, i in enumerate(t["order"]):
                for a, art in enumerate(self.articulators):
                    p2cp, euclid = float(t["errors"][row, a, 0]), float(t["errors"][row, a, 1])
                    writer.writerow([self.sentences[i], self.frames[i], self.phonemes[i], art, p2cp, p2cp * to_mm, euclid,
                                     euclid * to_mm])
        by_name = sorted(range(len(self.articulators)), key=lambda a: self.articulators[a])
        write_error_report_agg(paths["error_report_agg.csv"], [self.articulators[a] for a in by_name], t["agg"][by_name])
        if self.tv_text:
            with open(paths["tract_variables.csv"], "w", newline="") as f:
                f.write(self.tv_text[t["sentences"][0]][0] + "\n")
                for name in t["sentences"]:
                    f.writelines(line + "\n" for line in self.tv_text[name][1])
            with open(paths["TV_corr_report.csv"], "w", newline="") as f:
                writer = csv.writer(f, lineterminator="\n")
                writer.writerow(["TV", *STATS])
                for tv, row in zip(TV_NAMES, t["corr_report"]):
                    writer.writerow([tv, *(_cell(float(v)) for v in row)])
        return paths


def read_sentence(sentence_dir, articulators):
    """What a test pass left for one sentence, on the host: (text of tract_variables.csv, frames, phonemes, pred, true
    (1, F, A, 2, N) float32, tv_pred, tv_target (1, F, 4) float32), or None for a table without rows."""
    name = os.path.basename(sentence_dir)
    with open(os.path.join(sentence_dir, "tract_variables.csv"), newline="") as f:
        text = f.read()
    rows = list(csv.DictReader(text.splitlines()))
    if not rows:
        return None
    frames, phonemes = [r["frame"] for r in rows], [r["phoneme"] for r in rows]
    pred, true = [], []
    for frame in frames:
        try:
            stem = "%04d" % int(frame)
        except ValueError:
            raise ValueError(f"sentence {name}: frame id {frame!r} is not an integer") from None
        for art in articulators:
            for suffix, into in (("", pred), ("_true", true)):
                path = os.path.join(sentence_dir, "contours", f"{stem}_{art}{suffix}.npy")
                if not os.path.exists(path):
                    raise FileNotFoundError(f"sentence {name}: contour {path} is missing")
                into.append(np.load(path).astype(np.float32, copy=False))
    shape = (1, len(frames), len(articulators), *pred[0].shape)
    tv = [torch.tensor([[float(r[f"{v}_{key}"]) for v in TV_NAMES] for r in rows], dtype=torch.float32).view(1, -1, 4)
          for key in ("pred", "target")]
    return text, frames, phonemes, torch.from_numpy(np.stack(pred).reshape(shape)), torch.from_numpy(np.stack(true).reshape(shape)), *tv


def report_from_results_dir(database_name, results_dir, articulators, device=None):
    """The ErrorReport of the files a test pass has left under ``results_dir/test_outputs/0/<sentence>/``: the frames, phonemes and
    tract variables of ``tract_variables.csv`` and the contours ``contours/%04d_<articulator>.npy`` / ``..._true.npy`` of the
    articulators asked for (reference :135-239), uploaded one sentence at a time.  A missing contour raises FileNotFoundError, a
    frame id that is not an integer ValueError.  The tract variables enter the device tables as float32 (what the test loops
    wrote).  The per-sentence plots of the reference are not produced."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    articulators = list(articulators)
    report = ErrorReport(articulators, DATASET_CONFIG[database_name], device)
    base = os.path.join(results_dir, "test_outputs", "0")
    for name in sorted(os.listdir(base)):
        if not os.path.isdir(os.path.join(base, name)):
            continue
        sentence = read_sentence(os.path.join(base, name), articulators)
        if sentence is None:
            continue
        text, frames, phonemes, outputs, targets, tv_pred, tv_target = sentence
        report.add(outputs.to(device), targets.to(device), [len(frames)], [name], [frames], [phonemes],
                   tv=(tv_pred.to(device), tv_target.to(device), [text]))
    return report
