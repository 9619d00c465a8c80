####################################################################################################
#
# Test the DeepSpeech2 phoneme recogniser with a choice of decoder on the MI355X engine:
#   python decode_phoneme_recognition.py --config cfg.yaml
# test_phoneme_recognition.py with one more YAML key: the keyword arguments of main() are that
# script's, in its order, plus `decoder`.  Without the key, or with `decoder: {name: greedy}`, it
# calls that script's main(): the test pass with best-path CTC decoding.  With
# `decoder: {name: beam, nbest: ..., beam_size: ..., log_add: ..., ...}` (the other keys are
# BeamSearchCTCDecoder's, torchaudio's ctc_decoder names) the predictions are the best hypotheses
# of the CTC beam search on the device (as_ctc_beam_search), which is what the reference's
# test_phoneme_recognition.py:84-91 decodes with.  Writes info_test.json, substitution_matrix.npy
# and confusion_matrix.npy to save_dir as that script does and, with nbest > 1, hypotheses.json:
# per utterance of the split, in order, the token names and scores of the N best labellings.  The
# split is walked once and every batch searched once: the metrics, the substitution counts and
# hypotheses.json are served from that one search.
#
####################################################################################################
import argparse
import json
import logging
import os
from functools import partial

import torch
import yaml
from torch.utils.data import DataLoader

from artspeech_amd.helpers import set_seeds
from artspeech_amd.phoneme_recognition import BLANK, SIL, UNKNOWN, Criterion, DeepSpeech2, Feature, Target, run_test
from artspeech_amd.phoneme_recognition.datasets import collate_fn
from artspeech_amd.phoneme_recognition.decoders import BeamSearchCTCDecoder, GreedyCTCDecoder
from artspeech_amd.phoneme_recognition.metrics import EditDistance, WordInfoLost
from artspeech_amd.training import load_json
import test_phoneme_recognition
from train_phoneme_recognition import _make_dataset, build_vocabulary


def decoder_block(decoder):
    """(name, parameters) of a config's `decoder:` block; None is {name: greedy}."""
    params = dict(decoder or {})
    name = params.pop("name", "greedy")
    if name not in ("greedy", "beam"):
        raise ValueError(f"decode_phoneme_recognition: decoder name {name!r} is neither 'greedy' nor 'beam'")
    if name == "greedy" and params:
        raise ValueError(f"decode_phoneme_recognition: the greedy decoder takes no parameters, got {sorted(params)}")
    return name, params


def make_decoder(decoder, tokens):
    """The decoder of a config's `decoder:` block: None or {name: greedy} -> best path, built as test_phoneme_recognition.py
    builds it; {name: beam, ...} -> the beam search, one search per batch, with the block's other keys as
    BeamSearchCTCDecoder's keyword arguments."""
    name, params = decoder_block(decoder)
    if name == "greedy":
        return GreedyCTCDecoder(tokens=tokens, sil_token=SIL, blank_token=BLANK, unk_word=UNKNOWN)
    return RecordingBeamDecoder(tokens=tokens, sil_token=SIL, blank_token=BLANK, unk_word=UNKNOWN, **params)


class RecordingBeamDecoder(BeamSearchCTCDecoder):
    """BeamSearchCTCDecoder that searches every batch once: run_test hands the same emissions tensor to each metric and to the
    substitution counts, so the first ``decode_device`` of a batch runs the search with ``nbest`` and keeps its result, the
    others are served from it (the held reference keeps the tensor, and so its identity, alive).  ``batches`` collects every
    batch's BeamResult in order: the N best of the whole split from the one test pass."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.batches = []
        self._last = None   # (emissions, lengths, (tokens, counts) of the best hypothesis)

    def decode_device(self, emissions, lengths=None):
        key = None if lengths is None else tuple(int(n) for n in lengths)
        if self._last is None or self._last[0] is not emissions or self._last[1] != key:
            res = self.search(emissions, lengths)
            # the best hypothesis as decode_device's consumers take it: dense rows, not a stride-nbest view
            self._last = (emissions, key, (res.tokens[:, 0].contiguous(), res.counts[:, 0].contiguous()))
            self.batches.append(res)
        return self._last[2]

    def hypotheses(self):
        """Per utterance, in order: [{"tokens": [names], "score": float}], best first."""
        out = []
        for res in self.batches:
            tokens, counts, scores, found = res.tokens.cpu(), res.counts.cpu(), res.scores.cpu(), res.num_hyps.cpu()
            for b in range(tokens.shape[0]):
                out.append([{"tokens": [self.tokens[int(k)] for k in tokens[b, n, : int(counts[b, n])]], "score": float(scores[b, n])}
                            for n in range(int(found[b]))])
        return out


def main(database_name, datadir, batch_size, seq_dict, vocab_filepath, pretrained, feature, loss, model_params, target,
         state_dict_filepath, plot_target=None, voicing_filepath=None, num_workers=0, save_dir=None, seed=0, synthetic=None,
         decoder=None):
    arguments = {k: v for k, v in locals().items() if k != "decoder"}
    if decoder_block(decoder)[0] == "greedy":   # best path: that script's own pass, so the two cannot drift apart
        return test_phoneme_recognition.main(**arguments)
    criterion = Criterion[loss]
    if criterion != Criterion.CTC:
        raise NotImplementedError(f"decode_phoneme_recognition: loss {loss!r} is not supported; only CTC is ported")
    if pretrained:
        raise NotImplementedError("decode_phoneme_recognition: pretrained (the LibriSpeech checkpoint) is not supported")
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    feature = Feature(feature)
    target = Target(target)
    plot_target = Target(plot_target) if plot_target else None

    vocabulary = build_vocabulary(vocab_filepath, criterion)
    voiced_tokens = load_json(voicing_filepath)
    tokens = [k for k, _ in sorted(vocabulary.items(), key=lambda t: t[1])]
    decoder = make_decoder(decoder, tokens)

    model = DeepSpeech2(num_classes=len(vocabulary), **model_params)
    model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
    model.to(device)
    print(f"\nDeepSpeech2 -- {model.total_parameters} parameters\n")

    dataset = _make_dataset(datadir, database_name, seq_dict, vocabulary, feature, voiced_tokens, synthetic, seed + 2)
    dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, worker_init_fn=set_seeds,
                            collate_fn=partial(collate_fn, features_names=[feature]))
    metrics = {"edit_distance": EditDistance(decoder), "word_info_lost": WordInfoLost(decoder)}
    info_test = run_test(model=model, dataloader=dataloader, fn_metrics=metrics, decoder=decoder, device=device, feature=feature,
                         target=target, plot_target=plot_target, use_voicing=voicing_filepath is not None, save_dir=save_dir)
    if save_dir is not None:
        with open(os.path.join(save_dir, "info_test.json"), "w") as f:
            json.dump(info_test, f, indent=2)
        if getattr(decoder, "nbest", 1) > 1:   # collected during that one pass
            with open(os.path.join(save_dir, "hypotheses.json"), "w") as f:
                json.dump(decoder.hypotheses(), f, indent=2)
    return info_test


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="config_filepath")
    args = parser.parse_args()
    with open(args.config_filepath) as f:
        cfg = yaml.safe_load(f)
    print(json.dumps(main(**cfg), indent=2))
