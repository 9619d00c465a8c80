"""Decoders of the recogniser's emissions (reference ``phoneme_recognition/decoders.py``).  All return torchaudio's
``ctc_decoder`` result shape: one list of hypotheses per utterance, best first, each with a ``tokens`` sequence of indices.

* ``TopKDecoder``: the reference's own (top-1 per frame, repeats collapsed, blank dropped when it has one).
* ``GreedyCTCDecoder``: best-path CTC decoding -- argmax per frame over the first ``lengths[b]`` frames, collapse repeats, drop
  blank.  It stands in for torchaudio's lexicon-free beam-search ``ctc_decoder``, which the reference uses for CTC and which this
  engine does not depend on.

* ``BeamSearchCTCDecoder``: that beam search itself (beam_search.ctc_beam_search, the as_ctc_beam_search kernel) under
  torchaudio's parameter names: up to ``nbest`` hypotheses with scores.  Lexicon-free and without a language model only.

All have ``decode_device(emissions, lengths)``: the same decoding of the best hypothesis on the device (as_decode_top1, or
as_ctc_beam_search), emissions and result there -- ``(tokens (B, T) int32 padded with -1, counts (B,) int32)`` -- which is
what the metrics and the matrices consume.
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


ScoredHypothesis = namedtuple("ScoredHypothesis", ["tokens", "score"])


class BeamSearchCTCDecoder:
    """CTC beam search over prefixes on the device, under the names and defaults of ``torchaudio.models.decoder.ctc_decoder``
    (the reference builds it with ``lexicon=None``: test_phoneme_recognition.py:84-91).  ``lexicon`` and ``lm`` must stay None.

    tokens: the vocabulary's token names in index order; blank_token / sil_token: a name or an index (a sil_token outside the
    vocabulary means no silence class; it only matters with ``sil_score`` != 0).  Unlike torchaudio's, a result carries no
    silence token at its ends, and identical labellings are merged.

    ``input`` says what the emissions are.  ``run_test`` hands decoders the softmax of the outputs, as the reference does; the
    reference's decoder adds those probabilities as if they were log-probabilities.  "probs" (the default) decodes them
    properly, by their log; "scores" adds the values as they are, which on probabilities is the reference's arithmetic and on
    log-probabilities the proper search; "logits" takes the log-softmax of raw outputs."""

    def __init__(self, tokens, blank_token, sil_token=None, unk_word=None, lexicon=None, lm=None, nbest=1, beam_size=50,
                 beam_size_token=None, beam_threshold=50, sil_score=0, log_add=False, input="probs"):
        if lexicon is not None or lm is not None:
            raise NotImplementedError("BeamSearchCTCDecoder: only the lexicon-free search without a language model is built "
                                      "(lexicon=None, lm=None)")
        tokens = list(tokens)
        self.tokens = tokens
        self.blank = self._index(tokens, blank_token, 0)
        self.sil = self._index(tokens, sil_token, -1)
        self.unk_word = unk_word
        self.nbest, self.beam_size, self.beam_size_token = int(nbest), int(beam_size), beam_size_token
        self.beam_threshold, self.sil_score, self.log_add, self.input = float(beam_threshold), float(sil_score), bool(log_add), input

    @staticmethod
    def _index(tokens, token, default):
        if isinstance(token, int):
            return token
        return tokens.index(token) if token in tokens else default

    def search(self, emissions, lengths=None, nbest=None):
        """The ``BeamResult`` (device tensors) of ``ctc_beam_search`` with this decoder's parameters."""
        from .beam_search import ctc_beam_search
        return ctc_beam_search(emissions, lengths, blank=self.blank, beam_size=self.beam_size, beam_size_token=self.beam_size_token,
                               beam_threshold=self.beam_threshold, nbest=self.nbest if nbest is None else nbest,
                               log_add=self.log_add, sil=self.sil, sil_score=self.sil_score, input=self.input)

    def __call__(self, emissions, lengths=None):
        """emissions (B, T, C) on the device -> [[ScoredHypothesis(tokens=LongTensor, score=float), ...] per utterance], best first,
        up to nbest.  One copy of the result to the host."""
        res = self.search(emissions, lengths)
        tokens, counts, scores, found = res.tokens.cpu(), res.counts.cpu(), res.scores.cpu(), res.num_hyps.cpu()
        return [[ScoredHypothesis(tokens=tokens[b, k, : int(counts[b, k])].to(torch.int64), score=float(scores[b, k]))
                 for k in range(int(found[b]))] for b in range(tokens.shape[0])]

    uses_lengths = True

    @property
    def blank_index(self):
        return self.blank

    def decode_device(self, emissions, lengths=None):
        """(tokens (B, T) int32 padded with -1, counts (B,) int32) of the best hypothesis; an utterance without one decodes to
        nothing."""
        res = self.search(emissions, lengths, nbest=1)
        return res.tokens[:, 0], res.counts[:, 0]
