"""What the entry scripts (train_*.py, test_*.py) share on the host: optional mlflow, vocabulary and synthetic sizing,
results directory, checkpoint resume, the epoch loop with model selection and early stopping, and the command line.
Host only: nothing here loads the HIP library or touches a device, so a script's main() holds what is specific to
its method (model, data, loss, optimizer, metrics, closing test pass) and hands the rest to fit()."""
import argparse
import json
import logging
import os
import random
import shutil
import tempfile

import numpy as np
import torch
import yaml

from artspeech_amd.settings import BLANK, UNKNOWN

try:  # mlflow is optional here (absent from the MI355X image): same flags, no-op logging
    import mlflow
except ImportError:  # pragma: no cover
    mlflow = None

_TEMPORARY = []   # results directories made by results_paths(None, ...): run_cli removes the ones of its own run


def mlflow_call(fn, *args, **kwargs):
    if mlflow is not None:
        return getattr(mlflow, fn)(*args, **kwargs)


def load_json(filepath):
    """The JSON document of `filepath`, or None without one (vocab_filepath, voicing_filepath)."""
    if filepath is None:
        return None
    with open(filepath) as f:
        return json.load(f)


def build_vocabulary(vocab_filepath, default_tokens=(BLANK, UNKNOWN)):
    """{token: index}: the default tokens first, then the JSON list; without a file, 43 synthetic phoneme names."""
    tokens = load_json(vocab_filepath)
    if tokens is None:
        tokens = [f"ph{i:02d}" for i in range(43)]
    return {token: i for i, token in enumerate([*default_tokens, *tokens])}


def synthetic_size(seq_dict, synthetic, key, default):
    """(n, options): the size of a synthetic split is seq_dict[key], else synthetic[key], else default; options is
    `synthetic` without that key (the data set's remaining keyword arguments)."""
    options = dict(synthetic or {})
    n = options.pop(key, default)
    if isinstance(seq_dict, dict):
        n = seq_dict.get(key, n)
    return n, options


def results_paths(results_dir, prefix, names=("best_model.pt", "last_model.pt", "checkpoint.pt")):
    """[results_dir, *files in it]; the directory is created, a fresh temporary one (mkdtemp(prefix)) when None."""
    if results_dir is None:
        results_dir = tempfile.mkdtemp(prefix=prefix)
        _TEMPORARY.append(results_dir)
    os.makedirs(results_dir, exist_ok=True)
    return [results_dir, *(os.path.join(results_dir, name) for name in names)]


def load_checkpoint(path, model, optimizer, scheduler=None, map_location="cpu"):
    """Restore a checkpoint.pt written by fit(): (first epoch to run, best_metric, epochs_since_best, the checkpoint).
    Without a path nothing is loaded: a fresh run, (1, inf, 0, {})."""
    if path is None:
        return 1, np.inf, 0, {}
    checkpoint = torch.load(path, map_location=map_location)
    model.load_state_dict(checkpoint["model"])
    optimizer.load_state_dict(checkpoint["optimizer"])
    if scheduler is not None:
        scheduler.load_state_dict(checkpoint["scheduler"])
    epoch, best_metric, epochs_since_best = checkpoint["epoch"] + 1, checkpoint["best_metric"], checkpoint["epochs_since_best"]
    logging.info(f"Loaded checkpoint -- training from epoch {epoch}, best metric {best_metric} seen {epochs_since_best} epochs ago.")
    return epoch, best_metric, epochs_since_best, checkpoint


def fit(epochs, train_epoch, valid_epoch, *, metric, patience, best_files, last_files, checkpoint_path, checkpoint_state,
        best_metric=np.inf, epochs_since_best=0, plateau=None, rank=0):
    """The epoch loop of every trainer.  Per epoch: train_epoch(epoch), valid_epoch(epoch) (the info dicts), plateau.step on the
    validation loss, strict improvement of valid[metric] selects the best model; best_files (on improvement) and last_files,
    lists of (path, state_fn), then the checkpoint (checkpoint_state() plus epoch and the two counters) are written by rank 0;
    stops once the best lies more than `patience` epochs back.  Returns [{"epoch", "train", "valid"}, ...]."""
    history = []
    for epoch in epochs:
        train, valid = train_epoch(epoch), valid_epoch(epoch)
        history.append({"epoch": epoch, "train": train, "valid": valid})
        if plateau is not None:
            plateau.step(valid["loss"])
        improved = valid[metric] < best_metric
        if improved:
            best_metric, epochs_since_best = valid[metric], 0
        else:
            epochs_since_best += 1
        if rank == 0:
            mlflow_call("log_metrics", {f"train_{k}": v for k, v in train.items()}, step=epoch)
            mlflow_call("log_metrics", {f"valid_{k}": v for k, v in valid.items()}, step=epoch)
            for path, state_fn in (*(best_files if improved else ()), *last_files):
                torch.save(state_fn(), path)
                mlflow_call("log_artifact", path)
            torch.save({**checkpoint_state(), "epoch": epoch, "best_metric": float(best_metric),
                        "epochs_since_best": epochs_since_best}, checkpoint_path)
            mlflow_call("log_artifact", checkpoint_path)
            print(f"epoch {epoch}: train loss {train['loss']:.5f}  valid loss {valid['loss']:.5f}  {metric} {valid[metric]:.4f}  "
                  f"best {best_metric:.4f}, {epochs_since_best} epochs ago", flush=True)
        if epochs_since_best > patience:
            break
    return history


def cli_parser(experiment, checkpoint=True):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", dest="config_filepath")
    parser.add_argument("--mlflow", dest="mlflow_tracking_uri", default=None)
    parser.add_argument("--experiment", dest="experiment_name", default=experiment)
    parser.add_argument("--run_id", dest="run_id", default=None)
    parser.add_argument("--run_name", dest="run_name", default=None)
    if checkpoint:
        parser.add_argument("--checkpoint", dest="checkpoint_filepath", default=None)
    return parser


def run_cli(main, experiment, checkpoint=True, argv=None):
    """A trainer's __main__: the reference's flags, seeds 0, main(**YAML keys[, checkpoint_filepath], seed=0); a temporary
    results directory made during the run is removed.  Returns what main() returns."""
    args = cli_parser(experiment, checkpoint).parse_args(argv)
    seed = 0
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    with open(args.config_filepath) as f:
        cfg = yaml.safe_load(f)
    if mlflow is not None and args.mlflow_tracking_uri is not None:
        mlflow.set_tracking_uri(args.mlflow_tracking_uri)
        mlflow.set_experiment(args.experiment_name)
    if checkpoint:
        cfg["checkpoint_filepath"] = args.checkpoint_filepath
    cfg.setdefault("seed", seed)
    made = len(_TEMPORARY)
    try:
        return main(**cfg)
    finally:
        while len(_TEMPORARY) > made:
            shutil.rmtree(_TEMPORARY.pop(), ignore_errors=True)
