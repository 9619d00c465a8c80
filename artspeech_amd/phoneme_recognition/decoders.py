"""Decoders of the recogniser's emissions (reference ``phoneme_recognition/decoders.py``).  Both return torchaudio's
``ctc_decoder`` result shape: one list of hypotheses per utterance, best first, each with a ``tokens`` sequence of indices.

* ``TopKDecoder``: the reference's own (top-1 per frame, repeats collapsed, blank dropped when it has one).
* ``GreedyCTCDecoder``: best-path CTC decoding -- argmax per frame over the first ``lengths[b]`` frames, collapse repeats, drop
  blank.  It stands in for torchaudio's lexicon-free beam-search ``ctc_decoder``, which the reference uses for CTC and which this
  engine does not depend on.

Both also have ``decode_device(emissions, lengths)``: the same decoding by the as_decode_top1 kernel, emissions and result on the
device -- ``(tokens (B, T) int32 padded with -1, counts (B,) int32)`` -- which is what the metrics and the matrices consume.
"""
from collections import namedtuple

import torch

Hypothesis = namedtuple("Hypothesis", ["tokens"])


class TopKDecoder:
    def __init__(self, tokens, sil_token=None, blank_token=None, unk_word=None, **kwargs):
        self.num_tokens = len(tokens)
        self.sil_token, self.blank_token, self.unk_word = sil_token, blank_token, unk_word

    def filter_blank(self, indices):
        if self.blank_token is None:
            return indices
        return [i for i in indices if i != self.blank_token]

    def __call__(self, emissions, lengths):
        top = torch.topk(emissions, k=1, dim=-1).indices.squeeze(dim=-1)
        return [[Hypothesis(tokens=self.filter_blank(torch.unique_consecutive(t)))] for t in top]

    uses_lengths = False   # like the reference's, it decodes every frame, padding included

    @property
    def blank_index(self):
        return -1 if self.blank_token is None else int(self.blank_token)

    def decode_device(self, emissions, lengths=None):
        from .align import decode_top1
        return decode_top1(emissions, None, self.blank_index)


class GreedyCTCDecoder:
    """tokens: the vocabulary's token names in index order; blank_token: the blank's name (or index)."""

    def __init__(self, tokens, blank_token=None, sil_token=None, unk_word=None, lexicon=None, **kwargs):
        tokens = list(tokens)
        self.tokens = tokens
        if isinstance(blank_token, int):
            self.blank = blank_token
        else:
            self.blank = tokens.index(blank_token) if blank_token in tokens else 0

    def __call__(self, emissions, lengths=None):
        """emissions (B, T, C) -> [[Hypothesis(tokens=LongTensor)] per utterance]."""
        best = emissions.detach().argmax(dim=-1).cpu()
        out = []
        for b in range(best.shape[0]):
            seq = best[b, : int(lengths[b])] if lengths is not None else best[b]
            seq = torch.unique_consecutive(seq)
            out.append([Hypothesis(tokens=seq[seq != self.blank])])
        return out

    uses_lengths = True

    @property
    def blank_index(self):
        return self.blank

    def decode_device(self, emissions, lengths=None):
        from .align import decode_top1
        return decode_top1(emissions, lengths, self.blank)
