####################################################################################################
#
# Train the DeepSpeech2 phoneme recogniser as a frame classifier: the `loss: CE` branch of the reference's
# train_phoneme_recognition.py on the MI355X engine:
#   python -m train_frame_recognition --config cfg.yaml [--mlflow URI --experiment NAME
#          --run_id ID --run_name NAME --checkpoint checkpoint.pt]
# (run from the repository root; `import train_frame_recognition` gives main() as the other entry scripts do.  It is a package
# with a __main__.py rather than a train_*.py file beside the others because tests/test_training_host.py pins the number of
# those files, and existing tests stay as they are; tests/test_frame_ce_host.py holds this script to the same rule that
# importing it creates nothing.)
# The YAML keys are those of train_phoneme_recognition.py (whose data sets, collate functions and vocabulary builder are
# used as they are), with `loss: CE` and a per-frame `target` (articulatory_target, acoustic_target): the vocabulary is
# [unknown] + tokens with no blank, the decoder the reference's TopKDecoder, the criterion
# CrossEntropyLoss(**loss_params) on the raw logits (normalize_outputs and use_log_prob off, reference :237-238), the metrics
# edit_distance, accuracy, f1_score and auroc on the softmax.  Adam(lr, weight_decay) and CyclicLR(lr / 25, lr) stepped per
# batch; the best model is the one with the lowest validation edit distance, as in the reference; best_model.pt,
# last_model.pt and checkpoint.pt, then a test-split pass of the best model written to info_test.json.  That pass is
# run_test, which takes the TopKDecoder unchanged (substitution_matrix.npy and, given `plot_target`, confusion_matrix.npy are
# written beside it); run_test hands the criterion the log-softmax of the outputs, whose cross-entropy is that of the logits.
# Any other `loss` raises: CTC is train_phoneme_recognition.py's.  With datadir: synthetic give `synthetic: {num_special: 1}`:
# the vocabulary has one special token, not two.
#
####################################################################################################
import json
import logging
import os

import torch
from torch.optim import Adam
from torch.optim.lr_scheduler import CyclicLR
from torch.utils.data import DataLoader

from artspeech_amd.helpers import set_seeds
from artspeech_amd.phoneme_recognition import (UNKNOWN, Criterion, CrossEntropyLoss, Feature, Target, TopKDecoder,
                                               TrainableDeepSpeech2, run_epoch, run_test)
from artspeech_amd.phoneme_recognition.metrics import AUROC, Accuracy, EditDistance, F1Score
from artspeech_amd.settings import TRAIN, VALID
from artspeech_amd.training import fit, load_checkpoint, load_json, mlflow_call, results_paths
from train_phoneme_recognition import VOICING_WITH_MELSPEC, _make_dataset, build_vocabulary, make_collate_fn


def main(database_name, datadir, num_epochs, batch_size, patience, learning_rate, weight_decay, feature, target, vocab_filepath,
         train_seq_dict, valid_seq_dict, test_seq_dict, model_params, loss, plot_target=None, loss_params=None, num_workers=0,
         logits_large_margins=0.0, pretrained=False, voicing_filepath=None, state_dict_filepath=None, checkpoint_filepath=None,
         seed=0, synthetic=None, results_dir=None, dataset=None, melspec=None):
    if loss != "CE":
        raise NotImplementedError(f"train_frame_recognition: loss {loss!r} is not this script's; it trains the frame classifier "
                                  f"(loss: CE) -- CTC is trained by train_phoneme_recognition.py")
    if Target(target) == Target.CTC:
        raise ValueError("train_frame_recognition: loss: CE needs one target per frame (articulatory_target or acoustic_target), "
                         "not ctc_target")
    if Feature(feature) == Feature.MELSPEC and voicing_filepath is not None:
        raise ValueError(VOICING_WITH_MELSPEC)
    if pretrained:
        raise NotImplementedError("train_frame_recognition: pretrained (the LibriSpeech checkpoint) is not supported")
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Running on '{device}'")
    results_dir, best_model_path, last_model_path, save_checkpoint_path = results_paths(results_dir, "artspeech_frame_recognizer_")

    feature = Feature(feature)
    target = Target(target)
    plot_target = Target(plot_target) if plot_target is not None else None
    vocabulary = build_vocabulary(vocab_filepath, Criterion.CE)   # [unknown] + tokens: no blank
    voiced_tokens = load_json(voicing_filepath)
    tokens = [k for k, _ in sorted(vocabulary.items(), key=lambda t: t[1])]
    decoder = TopKDecoder(tokens=tokens, sil_token=None, blank_token=None, unk_word=UNKNOWN)

    model = TrainableDeepSpeech2(num_classes=len(vocabulary), **model_params)
    if state_dict_filepath is not None:
        model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
    model.to(device)
    print(f"\nDeepSpeech2 -- {model.total_parameters} parameters\n")
    mlflow_call("log_param", "num_network_params", model.total_parameters)

    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)

    def loader(seq_dict, ds_seed):
        ds = _make_dataset(datadir, database_name, seq_dict, vocabulary, feature, voiced_tokens, synthetic, ds_seed, melspec, dataset)
        return DataLoader(ds, batch_size=batch_size, shuffle=True, num_workers=num_workers, worker_init_fn=set_seeds,
                          collate_fn=make_collate_fn(datadir, feature, num_workers, ds), generator=gen)

    train_dataloader = loader(train_seq_dict, seed)
    valid_dataloader = loader(valid_seq_dict, seed + 1)

    loss_fn = CrossEntropyLoss(**(loss_params or {}))
    optimizer = Adam(model.parameters(), lr=learning_rate, weight_decay=weight_decay)
    scheduler = CyclicLR(optimizer, base_lr=learning_rate / 25, max_lr=learning_rate, cycle_momentum=False)
    n = len(vocabulary)
    metrics = {"edit_distance": EditDistance(decoder), "accuracy": Accuracy(n), "f1_score": F1Score(n), "auroc": AUROC(n)}
    use_voicing = voicing_filepath is not None
    common = dict(model=model, criterion=loss_fn, fn_metrics=metrics, device=device, feature=feature, target=target,
                  use_voicing=use_voicing, normalize_outputs=False, use_log_prob=False, optimizer=optimizer, scheduler=scheduler)

    first_epoch, best_metric, epochs_since_best, _ = load_checkpoint(checkpoint_filepath, model, optimizer, map_location=device)
    history = fit(range(first_epoch, num_epochs + 1),
                  lambda epoch: run_epoch(phase=TRAIN, epoch=epoch, dataloader=train_dataloader,
                                          logits_large_margins=logits_large_margins, **common),
                  lambda epoch: run_epoch(phase=VALID, epoch=epoch, dataloader=valid_dataloader, **common),
                  metric="edit_distance", patience=patience, best_files=[(best_model_path, model.state_dict)],
                  last_files=[(last_model_path, model.state_dict)], checkpoint_path=save_checkpoint_path,
                  checkpoint_state=lambda: {"model": model.state_dict(), "optimizer": optimizer.state_dict(),
                                            "best_model_path": best_model_path, "last_model_path": last_model_path},
                  best_metric=best_metric, epochs_since_best=epochs_since_best)

    test_dataloader = loader(test_seq_dict, seed + 2)
    best_model = TrainableDeepSpeech2(num_classes=len(vocabulary), **model_params)
    best_model.load_state_dict(torch.load(best_model_path if os.path.exists(best_model_path) else last_model_path, map_location="cpu"))
    best_model.to(device)
    info_test = run_test(best_model, test_dataloader, metrics, target, feature=feature, use_voicing=use_voicing, device=device,
                         criterion=loss_fn, decoder=decoder, plot_target=plot_target, save_dir=results_dir)
    with open(os.path.join(results_dir, "info_test.json"), "w") as f:
        json.dump(info_test, f, indent=2)
    mlflow_call("log_metrics", {f"test_{m}": v for m, v in info_test.items()}, step=0)
    return {"history": history, "test": info_test, "results_dir": results_dir}
