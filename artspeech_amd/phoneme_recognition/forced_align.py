"""CTC forced alignment on the HIP library (as_ctc_align): the Viterbi path of a known label sequence through the recogniser's
emissions, expanded on the device into one phoneme token per frame -- the sequences the phoneme-to-articulation models consume,
which the reference takes from hand-made TextGrids (generate_vocal_tract_shape_v2.py:135-158; it has no alignment of its own).

``forced_align`` is the kernel call; ``Alignment.segments`` turns one utterance's filled spans into (token, start, end, score) in
seconds; ``phonetic_sequence`` is the reference's get_repeated_phoneme over such segments (host); ``FrameAgreement`` and
``align_test`` compare the filled per-frame tokens with a per-frame truth (``acoustic_target`` / ``articulatory_target``).  This is
not align.py, which is the edit-distance alignment of decoded predictions."""
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib
from . import emission_args as args

_MAX_FRAMES = 8192  # the per-frame scratch of one utterance lives in LDS


@dataclass
class Alignment:
    """What as_ctc_align writes, on the device: score (B,) float32, feasible (B,) bool = isfinite(score); frame_index,
    frame_token, frame_filled (B, T) int32 (-1 past an utterance's frames, and everywhere without an alignment); spans
    (B, max L, 2) int32 (first frame, last frame + 1) of every target entry's own frames; span_score (B, max L) float32, the
    mean log-probability of the entry's label over them."""
    score: torch.Tensor
    feasible: torch.Tensor
    frame_index: torch.Tensor
    frame_token: torch.Tensor
    frame_filled: torch.Tensor
    spans: torch.Tensor
    span_score: torch.Tensor

    def segments(self, b, frame_rate):
        """[(token, start_s, end_s, score)] of utterance b: every target entry with the frames it fills (its own and the blank
        frames it absorbs: those after it, and for entry 0 the leading ones), in seconds at ``frame_rate`` frames per second.
        Empty without an alignment.  Copies that utterance's rows to the host."""
        filled = self.frame_filled[b].cpu().numpy()
        tokens = self.frame_token[b].cpu().numpy()
        spans = self.spans[b].cpu().numpy()
        scores = self.span_score[b].cpu().numpy()
        out = []
        for j, first, last in filled_runs(filled):
            out.append((int(tokens[spans[j][0]]), first / frame_rate, last / frame_rate, float(scores[j])))
        return out


def filled_runs(filled):
    """[(entry, first frame, last frame + 1)] of one frame_filled row (host): the runs of its entries, -1 frames left out."""
    filled = np.asarray(filled)
    n = int((filled >= 0).sum())   # the -1 frames are a suffix (or the whole row)
    if n == 0:
        return []
    cuts = np.flatnonzero(np.diff(filled[:n])) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [n]])
    return [(int(filled[s]), int(s), int(e)) for s, e in zip(starts, ends)]


def forced_align(emissions, targets, input_lengths, target_lengths, blank=0, logits=False):
    """The best CTC alignment of ``targets`` to ``emissions`` for every utterance, as an ``Alignment``.

    emissions: (B, T, C) float32 on the device, any strided view whose class stride is 1 (the permuted (T, B, C) tensor of the
    loss costs no copy); log-probabilities, or raw scores with ``logits=True`` (normalised inside the kernel).  targets: padded
    (B, S) with -1 padding, or 1-D concatenated, as ``ctc_loss`` takes them; lengths: one entry per utterance.  One kernel launch,
    nothing synchronises beyond reading the lengths that the caller passed on the host."""
    _lib.require_gpu(emissions, "emissions")
    x, T, B, Cn, st, sb = args.emissions(emissions, "forced_align", False)
    dev = x.device
    _, il = args.lengths(input_lengths, B, "forced_align", "input_lengths", T=T, device=dev)
    tl_h, tl = args.lengths(target_lengths, B, "forced_align", "target_lengths", host=True, device=dev)
    if T > _MAX_FRAMES:
        raise ValueError(f"forced_align (HIP): {T} frames exceed the supported {_MAX_FRAMES}")
    targets, tstride, max_l = args.ctc_targets(targets, tl_h, B, "forced_align", blank, Cn, dev)
    score = torch.empty(B, device=dev, dtype=torch.float32)
    frames = torch.empty(3, B, T, device=dev, dtype=torch.int32)
    spans = torch.empty(B, max_l, 2, device=dev, dtype=torch.int32)
    span_score = torch.empty(B, max_l, device=dev, dtype=torch.float32)
    if B == 0 or T == 0:
        score.fill_(float("-inf"))
        score[tl == 0] = 0.0
        frames.fill_(-1), spans.fill_(-1), span_score.fill_(float("nan"))
    else:
        wsn = int(_lib.call("as_ctc_align_workspace_bytes", T, B, max_l))
        ws = torch.empty(wsn, device=dev, dtype=torch.uint8) if wsn else None
        _lib.call("as_ctc_align", x, st, sb, T, B, Cn, int(logits), targets, tstride, il, tl, max_l, int(blank), ws, wsn, score,
                  frames[0], frames[1], frames[2], spans if max_l else None, span_score if max_l else None)
    return Alignment(score, torch.isfinite(score), frames[0], frames[1], frames[2], spans, span_score)


def filled_tokens(alignment, targets, target_lengths=None):
    """(B, T) int64 on the device: the token of every frame with blanks absorbed, targets[b][frame_filled[b][t]], -1 where
    frame_filled is -1.  targets as given to forced_align (1-D concatenated targets need ``target_lengths``)."""
    filled = alignment.frame_filled.to(torch.int64)
    dev = filled.device
    targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int64)
    if filled.shape[0] == 0 or targets.numel() == 0:
        return torch.full_like(filled, -1)
    if targets.dim() == 1:
        tl = torch.as_tensor(target_lengths).reshape(-1).to(device=dev, dtype=torch.int64)
        offsets = torch.cumsum(tl, 0) - tl
        tok = targets[(filled.clamp(min=0) + offsets[:, None]).clamp(max=targets.numel() - 1)]
    else:
        tok = torch.gather(targets, 1, filled.clamp(min=0, max=targets.shape[1] - 1))
    return torch.where(filled >= 0, tok, torch.full_like(tok, -1))


def phonetic_sequence(tokens, start_times, end_times, framerate):
    """The reference's get_repeated_phoneme over a list of intervals (generate_vocal_tract_shape_v2.py:135-139, bit for bit): token
    i repeated int("%.0f" % ((end - start) / (1 / framerate))) times -- Python's round-half-even of the frame count."""
    period = 1 / framerate
    out = []
    for token, start, end in zip(tokens, start_times, end_times):
        out.extend([token] * int("%.0f" % ((end - start) / period)))
    return out


def _frame_agreement_counts(al, targets, input_lengths, target_lengths, truth, truth_lengths):
    """(agreeing frames, compared frames, feasible utterances, sum of score / frames over the feasible ones) of an Alignment
    against a per-frame truth, device scalars."""
    dev = al.score.device
    tokens = filled_tokens(al, targets, target_lengths)
    truth = torch.as_tensor(truth).to(device=dev, dtype=torch.int64)
    n = torch.minimum(torch.as_tensor(input_lengths).reshape(-1).to(dev), torch.as_tensor(truth_lengths).reshape(-1).to(dev))
    n = torch.where(al.feasible, n, torch.zeros_like(n))   # an utterance without an alignment has no frames to compare
    T = min(tokens.shape[1], truth.shape[1])
    valid = torch.arange(T, device=dev)[None, :] < n[:, None]
    agree = ((tokens[:, :T] == truth[:, :T]) & valid).sum()
    frames = torch.as_tensor(input_lengths).reshape(-1).to(device=dev, dtype=torch.float32).clamp(min=1)
    per_frame = torch.where(al.feasible, al.score / frames, torch.zeros_like(al.score)).sum()
    return agree, valid.sum(), al.feasible.sum(), per_frame


class FrameAgreement:
    """The share of frames on which the forced alignment's filled token equals a per-frame truth, as a metric of the
    ``fn_metrics`` call form ``(emissions, targets, input_lengths, target_lengths)``.  The truth travels beside the call:
    ``set_truth(batch[truth_key], batch[truth_key + "_length"])`` before it (``align_test`` is the loop that needs no such step:
    it reads the truth from the batch itself).  Emissions are
    probabilities (what run_test hands its metrics) unless ``log_probs=True``; counted on the device, one number copied back."""

    def __init__(self, blank, truth_key="articulatory_target", log_probs=False):
        self.blank, self.truth_key, self.log_probs = blank, truth_key, log_probs
        self._truth = None

    def set_truth(self, truth, truth_lengths):
        self._truth = (truth, truth_lengths)

    def __call__(self, emissions, targets, input_lengths, target_lengths):
        if self._truth is None:
            raise ValueError(f"FrameAgreement: no truth set; call set_truth(batch[{self.truth_key!r}], its lengths) first")
        _lib.require_gpu(emissions, "emissions")
        logp = emissions if self.log_probs else torch.log(emissions)
        al = forced_align(logp, targets, input_lengths, target_lengths, self.blank)
        agree, frames, _, _ = _frame_agreement_counts(al, targets, input_lengths, target_lengths, *self._truth)
        return float(agree) / max(int(frames), 1)


def align_test(model, dataloader, target, truth, feature=None, use_voicing=False, device=None, blank=0, on_batch=None):
    """Align ``batch[target]`` to the model's outputs for every batch and compare the filled per-frame tokens with ``batch[truth]``
    over min(input length, truth length) frames, counted on the device.  The model's raw outputs go to the kernel as logits.
    Returns {"frame_agreement": agreeing / compared frames, "feasible_fraction": utterances with an alignment / all,
    "mean_score_per_frame": the mean over those utterances of score / frames}.  ``on_batch(batch, alignment, first utterance
    index)`` sees every batch's Alignment (the entry script writes its files from there)."""
    from . import Feature
    feature = Feature.MELSPEC if feature is None else feature
    if device is None:
        device = torch.device("cuda")
    model.eval()
    totals = torch.zeros(4, device=device, dtype=torch.float64)
    utterances = 0
    with torch.no_grad():
        for batch in dataloader:
            inputs = batch[feature.value].to(device)
            input_lengths = batch[f"{feature.value}_length"]
            targets = batch[target.value].to(device)
            target_lengths = batch[f"{target.value}_length"]
            voicing = batch["voicing"].to(device) if use_voicing else None
            outputs = model(inputs, voicing)
            input_lengths = torch.as_tensor(input_lengths).reshape(-1).clamp(max=outputs.shape[1])
            al = forced_align(outputs, targets, input_lengths, target_lengths, blank, logits=True)
            counts = _frame_agreement_counts(al, targets, input_lengths, target_lengths, batch[truth.value],
                                             batch[f"{truth.value}_length"])
            totals += torch.stack([c.to(torch.float64) for c in counts])
            if on_batch is not None:
                on_batch(batch, al, utterances)
            utterances += int(outputs.shape[0])
    agree, frames, feasible, per_frame = totals.tolist()
    return {"frame_agreement": agree / max(frames, 1.0), "feasible_fraction": feasible / max(utterances, 1),
            "mean_score_per_frame": per_frame / max(feasible, 1.0)}
