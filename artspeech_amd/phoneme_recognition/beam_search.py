"""CTC beam search on the HIP library (as_ctc_beam_search): the N most probable labellings of every utterance with their scores,
what the reference decodes CTC emissions with through ``torchaudio.models.decoder.ctc_decoder(lexicon=None, ...)``
(test_phoneme_recognition.py:84-91) -- flashlight's lexicon-free decoder with a zero language model.  Best-path decoding
(``decode_top1``) returns the single best alignment; this search sums (``log_add=True``) or maximises over the alignments of
every labelling it keeps, and returns alternatives.  tests/ctc_beam_fp64.py is the contract; DESIGN.md section 4n states it, the
two differences from flashlight (no silence at the ends of a result, identical labellings merged) and the limits."""
from dataclasses import dataclass

import torch

from .. import _lib
from . import emission_args as args

MAX_BEAM = 64      # live prefixes of one utterance (as_ctc_beam_search)
MAX_CLASSES = 128
MAX_FRAMES = 8192
_MODES = {"scores": 0, "probs": 1, "logits": 2}


@dataclass
class BeamResult:
    """What as_ctc_beam_search writes, on the device: tokens (B, nbest, T) int32 padded with -1; counts (B, nbest) int32; scores
    (B, nbest) float32, best first, -inf where there is no hypothesis; num_hyps (B,) int32."""
    tokens: torch.Tensor
    counts: torch.Tensor
    scores: torch.Tensor
    num_hyps: torch.Tensor


def ctc_beam_search(emissions, lengths=None, blank=0, beam_size=50, beam_size_token=None, beam_threshold=50.0, nbest=1, log_add=False,
                    sil=-1, sil_score=0.0, input="scores"):
    """The ``nbest`` best labellings of every utterance as a ``BeamResult``.

    emissions: (B, T, C) float32 on the device, any strided view whose class stride is 1 (the permuted (T, B, C) tensor of the
    loss costs no copy).  ``input``: "scores" adds the values as they are (log-probabilities, usually), "probs" takes their log
    inside the kernel (log(0) = -inf), "logits" their row log-softmax.  lengths: one entry per utterance, or None for all T
    frames.  beam_size: hypotheses kept per frame; beam_size_token: classes considered per frame (None: all); beam_threshold:
    contributions further than this below the frame's best are dropped; log_add: merge the alignments of a labelling by
    logaddexp rather than max; sil / sil_score: a class whose emissions get sil_score added (-1: none).  One kernel launch."""
    _lib.require_gpu(emissions, "emissions")
    x, T, B, Cn, st, sb = args.emissions(emissions, "ctc_beam_search", False, detach=True)
    if input not in _MODES:
        raise ValueError(f"ctc_beam_search: input must be one of {sorted(_MODES)}, got {input!r}")
    dev = x.device
    beam_size, nbest = int(beam_size), int(nbest)
    K = Cn if beam_size_token is None else int(beam_size_token)
    if not 1 <= beam_size <= MAX_BEAM:
        raise ValueError(f"ctc_beam_search (HIP): beam_size {beam_size} outside the supported 1 to {MAX_BEAM}")
    if not 2 <= Cn <= MAX_CLASSES:
        raise ValueError(f"ctc_beam_search (HIP): {Cn} classes outside the supported 2 to {MAX_CLASSES}")
    if not 1 <= K <= Cn:
        raise ValueError(f"ctc_beam_search: beam_size_token {K} outside 1 to the {Cn} classes")
    if T > MAX_FRAMES:
        raise ValueError(f"ctc_beam_search (HIP): {T} frames exceed the supported {MAX_FRAMES}")
    if nbest < 1:
        raise ValueError(f"ctc_beam_search: nbest {nbest} must be at least 1")
    if not 0 <= blank < Cn:
        raise ValueError(f"ctc_beam_search: blank {blank} outside [0, {Cn})")
    if not -1 <= sil < Cn:
        raise ValueError(f"ctc_beam_search: sil {sil} outside [-1, {Cn})")
    if not float(beam_threshold) >= 0.0:
        raise ValueError(f"ctc_beam_search: beam_threshold {beam_threshold} must be at least 0")
    if lengths is not None:
        _, lengths = args.lengths(lengths, B, "ctc_beam_search", device=dev)
    tokens = torch.empty(B, nbest, T, device=dev, dtype=torch.int32)
    counts = torch.empty(B, nbest, device=dev, dtype=torch.int32)
    scores = torch.empty(B, nbest, device=dev, dtype=torch.float32)
    num_hyps = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0 or T == 0:   # no frames: the empty labelling with score 0
        tokens.fill_(-1), counts.zero_(), scores.fill_(float("-inf")), num_hyps.fill_(1)
        scores[:, :1] = 0.0
    else:
        wsn = int(_lib.call("as_ctc_beam_workspace_bytes", T, B, Cn, beam_size))
        ws = torch.empty(wsn, device=dev, dtype=torch.uint8)
        _lib.call("as_ctc_beam_search", x, st, sb, T, B, Cn, _MODES[input], lengths, int(blank), int(sil),
                  float(sil_score), beam_size, K, float(beam_threshold), int(bool(log_add)), nbest, tokens, counts, scores, num_hyps,
                  ws, wsn)
    return BeamResult(tokens, counts, scores, num_hyps)
