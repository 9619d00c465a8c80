####################################################################################################
#
# Force-align transcripts to the DeepSpeech2 recogniser's emissions on the MI355X engine (the reference
# has no such script: its per-frame phoneme sequences come from hand-made TextGrids,
# generate_vocal_tract_shape_v2.py:135-158):
#   python align_phoneme_recognition.py --config cfg.yaml
# The YAML keys are the keyword arguments of main(): those of test_phoneme_recognition.py that apply,
# plus `truth` (the per-frame target the alignment is compared with: acoustic_target or
# articulatory_target), `frame_rate` (frames per second of the emissions; default: the mel
# spectrogram's sample_rate / hop_length, else 55, the reference's articulatory rate) and the optional
# `framerate`.  Loads state_dict_filepath into the frozen DeepSpeech2, aligns every utterance's
# `target` on the device (as_ctc_align) and writes to save_dir:
#   info_align.json                frame_agreement, feasible_fraction, mean_score_per_frame
#   alignments/<index>.csv         phoneme,start_frame,end_frame,start_time,end_time,score per target
#                                  entry, blank frames absorbed (empty for an utterance without alignment)
#   alignments/<index>_frames.npy  the filled per-frame token ids
#   alignments/<index>_phonemes.txt  with `framerate`: phonetic_sequence at that rate, space-separated as
#                                  the reference's target_sequence.txt -- a sentence for the articulation
#                                  models' test scripts
#
####################################################################################################
import csv
import json
import logging
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from artspeech_amd.helpers import set_seeds
from artspeech_amd.phoneme_recognition import Criterion, DeepSpeech2, Feature, Target, align_test
from artspeech_amd.phoneme_recognition.forced_align import filled_runs, filled_tokens, phonetic_sequence
from artspeech_amd.settings import BLANK
from artspeech_amd.training import load_json, run_cli
from train_phoneme_recognition import _make_dataset, build_vocabulary, make_collate_fn

CSV_COLUMNS = ["phoneme", "start_frame", "end_frame", "start_time", "end_time", "score"]
ARTICULATORY_FRAME_RATE = 55.0   # get_phonetic_sequences' default (generate_vocal_tract_shape_v2.py:142)


def write_alignment(out_dir, index, names, filled, tokens, span_score, frame_rate, framerate=None):
    """One utterance's files from its host rows: filled (T,) entries, tokens (T,) filled token ids, span_score (max L,)."""
    rows = [(names[int(tokens[first])], first, last, first / frame_rate, last / frame_rate, float(span_score[j]))
            for j, first, last in filled_runs(filled)]
    with open(os.path.join(out_dir, f"{index}.csv"), "w", newline="") as f:
        writer = csv.writer(f)
        writer.writerow(CSV_COLUMNS)
        writer.writerows(rows)
    np.save(os.path.join(out_dir, f"{index}_frames.npy"), tokens[: rows[-1][2] if rows else 0])
    if framerate is not None:
        sequence = phonetic_sequence([r[0] for r in rows], [r[3] for r in rows], [r[4] for r in rows], framerate)
        with open(os.path.join(out_dir, f"{index}_phonemes.txt"), "w") as f:
            f.write(" ".join(sequence))


def main(database_name, datadir, batch_size, seq_dict, vocab_filepath, feature, model_params, target, truth, state_dict_filepath,
         loss="CTC", pretrained=False, voicing_filepath=None, num_workers=0, save_dir=None, frame_rate=None, framerate=None, seed=0,
         synthetic=None):
    if Criterion[loss] != Criterion.CTC:
        raise NotImplementedError(f"align_phoneme_recognition: loss {loss!r} has no alignment; forced alignment is CTC's")
    if pretrained:
        raise NotImplementedError("align_phoneme_recognition: pretrained (the LibriSpeech checkpoint) is not supported")
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    feature, target, truth = Feature(feature), Target(target), Target(truth)

    vocabulary = build_vocabulary(vocab_filepath, Criterion.CTC)
    names = {i: token for token, i in vocabulary.items()}
    model = DeepSpeech2(num_classes=len(vocabulary), **model_params)
    model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
    model.to(device)

    dataset = _make_dataset(datadir, database_name, seq_dict, vocabulary, feature, load_json(voicing_filepath), synthetic, seed + 2)
    dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, worker_init_fn=set_seeds,
                            collate_fn=make_collate_fn(datadir, feature, num_workers, dataset))
    if frame_rate is None:
        mel = getattr(dataset, "melspectrogram", None)
        frame_rate = mel.sample_rate / mel.hop_length if mel is not None else ARTICULATORY_FRAME_RATE

    on_batch = None
    if save_dir is not None:
        out_dir = os.path.join(save_dir, "alignments")
        os.makedirs(out_dir, exist_ok=True)

        def on_batch(batch, alignment, first):
            tokens = filled_tokens(alignment, batch[target.value], batch[f"{target.value}_length"]).cpu().numpy()
            filled, span_score = alignment.frame_filled.cpu().numpy(), alignment.span_score.cpu().numpy()
            for b in range(filled.shape[0]):
                write_alignment(out_dir, first + b, names, filled[b], tokens[b], span_score[b], frame_rate, framerate)

    info = align_test(model, dataloader, target, truth, feature=feature, use_voicing=voicing_filepath is not None, device=device,
                      blank=vocabulary[BLANK], on_batch=on_batch)
    info["frame_rate"] = frame_rate
    if save_dir is not None:
        with open(os.path.join(save_dir, "info_align.json"), "w") as f:
            json.dump(info, f, indent=2)
    return info


if __name__ == "__main__":
    print(json.dumps(run_cli(main, "phoneme_recognition_alignment", checkpoint=False), indent=2))
