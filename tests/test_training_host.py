"""artspeech_amd/training.py, the host-side harness the entry scripts share (no GPU, no library): the epoch loop with model
selection and early stopping, checkpoint resume, synthetic sizing, vocabulary, the command line; and two properties of the
scripts themselves: importing one creates nothing, and an error inside run_epoch's batch loop is the error that comes out."""
import importlib
import os
import sys
import tempfile

import pytest
import torch
import yaml

from conftest import ROOT
from artspeech_amd import training as T

SCRIPTS = sorted(f[:-3] for f in os.listdir(ROOT) if f.startswith(("train_", "test_")) and f.endswith(".py"))


class _Plateau:
    def __init__(self, log):
        self.log = log

    def step(self, loss):
        self.log.append(("plateau", loss))


def _drive(tmp_path, values, epochs, n_files=1, plateau=False, **kw):
    """fit() over stub epochs whose validation metric follows `values`; returns (history, log, infos): the log holds
    (what, epoch) for every state function fit called (= every file it wrote), in order, and ("plateau", loss)."""
    log, infos, now = [], [], {}
    values = list(values)

    def train_epoch(epoch):
        now["epoch"] = epoch
        return {"loss": 100.0 + epoch}

    def valid_epoch(epoch):
        log.append(("valid", epoch))
        return {"loss": 10.0 + epoch, "m": values.pop(0)}

    def state(what, extra=None):
        def fn():
            log.append((what, now["epoch"]))
            return {"what": what, "epoch": now["epoch"], **(extra or {})}
        return fn

    def wrap(fn):
        def call(epoch):
            infos.append(fn(epoch))
            return infos[-1]
        return call

    best = [(str(tmp_path / f"best{i}.pt"), state(f"best{i}")) for i in range(n_files)]
    last = [(str(tmp_path / f"last{i}.pt"), state(f"last{i}")) for i in range(n_files)]
    extra = {"model": {"w": torch.ones(2)}, "optimizer": {"o": 1}, "scheduler": {"s": 2}, **{f"best{i}_path": p for i, (p, _) in enumerate(best)},
             **{f"last{i}_path": p for i, (p, _) in enumerate(last)}}
    history = T.fit(epochs, wrap(train_epoch), wrap(valid_epoch), metric="m", patience=1, best_files=best, last_files=last,
                    checkpoint_path=str(tmp_path / "checkpoint.pt"), checkpoint_state=state("checkpoint", extra),
                    plateau=_Plateau(log) if plateau else None, **kw)
    return history, log, infos


def _epochs_of(log, what):
    return [epoch for w, epoch in log if w == what]


def test_fit_selects_saves_and_stops(tmp_path):
    history, log, infos = _drive(tmp_path, [5, 4, 4, 6, 3], range(1, 6))
    assert [h["epoch"] for h in history] == [1, 2, 3, 4]             # the second epoch without a strict improvement ends it
    assert _epochs_of(log, "best0") == [1, 2]
    assert _epochs_of(log, "last0") == _epochs_of(log, "checkpoint") == [1, 2, 3, 4]
    ckpt = torch.load(tmp_path / "checkpoint.pt")
    assert (ckpt["epoch"], ckpt["best_metric"], ckpt["epochs_since_best"]) == (4, 4.0, 2) and type(ckpt["best_metric"]) is float
    assert all(h["train"] is infos[2 * i] and h["valid"] is infos[2 * i + 1] for i, h in enumerate(history)) and len(infos) == 8
    assert torch.load(tmp_path / "best0.pt")["epoch"] == 2 and torch.load(tmp_path / "last0.pt")["epoch"] == 4
    # within an epoch: best, then last, then the checkpoint
    assert [w for w, e in log if e == 2 and w != "valid"] == ["best0", "last0", "checkpoint"]


def test_a_tie_is_no_improvement(tmp_path):
    history, log, _ = _drive(tmp_path, [3, 3, 3], range(1, 4))
    assert _epochs_of(log, "best0") == [1] and [h["epoch"] for h in history] == [1, 2, 3]
    assert torch.load(tmp_path / "checkpoint.pt")["epochs_since_best"] == 2


class _Loads:
    def __init__(self):
        self.loaded = None

    def load_state_dict(self, state):
        self.loaded = state


def test_resume_continues_the_count(tmp_path, caplog):
    _drive(tmp_path, [5, 4, 4, 6, 3], range(1, 6))
    model, optimizer, scheduler = _Loads(), _Loads(), _Loads()
    with caplog.at_level("INFO"):
        first, best_metric, epochs_since_best, ckpt = T.load_checkpoint(str(tmp_path / "checkpoint.pt"), model, optimizer, scheduler)
    assert (first, best_metric, epochs_since_best) == (5, 4.0, 2) and ckpt["best0_path"] == str(tmp_path / "best0.pt")
    assert torch.equal(model.loaded["w"], torch.ones(2)) and optimizer.loaded == {"o": 1} and scheduler.loaded == {"s": 2}
    assert "Loaded checkpoint -- training from epoch 5, best metric 4.0 seen 2 epochs ago." in caplog.text
    unstepped = _Loads()                                              # no scheduler: the key is not read
    T.load_checkpoint(str(tmp_path / "checkpoint.pt"), _Loads(), unstepped)
    assert unstepped.loaded == {"o": 1}
    assert T.load_checkpoint(None, None, None) == (1, float("inf"), 0, {})
    history, log, _ = _drive(tmp_path, [3.5, 9], range(first, 7), best_metric=best_metric, epochs_since_best=epochs_since_best)
    assert [h["epoch"] for h in history] == [5, 6] and _epochs_of(log, "best0") == [5]
    ckpt = torch.load(tmp_path / "checkpoint.pt")
    assert (ckpt["epoch"], ckpt["best_metric"], ckpt["epochs_since_best"]) == (6, 3.5, 1)
    # without the improvement the resumed counter ends the run at once: 2 epochs ago already, patience 1
    history, _, _ = _drive(tmp_path, [4, 1], range(5, 7), best_metric=4.0, epochs_since_best=2)
    assert [h["epoch"] for h in history] == [5]


def test_plateau_steps_once_per_epoch_on_the_validation_loss_before_the_comparison(tmp_path):
    _, log, _ = _drive(tmp_path, [5, 4, 6], range(1, 4), plateau=True)
    assert [x for w, x in log if w == "plateau"] == [11.0, 12.0, 13.0]
    assert [w for w, _ in log][:5] == ["valid", "plateau", "best0", "last0", "checkpoint"]
    _, log, _ = _drive(tmp_path, [5, 4, 6], range(1, 4))
    assert not [w for w, _ in log if w == "plateau"]


def test_other_ranks_write_nothing(tmp_path):
    history, log, _ = _drive(tmp_path, [5, 4, 4, 6, 3], range(1, 6), rank=1)
    assert [h["epoch"] for h in history] == [1, 2, 3, 4] and [h["valid"]["m"] for h in history] == [5, 4, 4, 6]
    assert {w for w, _ in log} == {"valid"} and os.listdir(tmp_path) == []


def test_pairs_of_files(tmp_path):
    _drive(tmp_path, [5, 6], range(1, 3), n_files=2)
    assert sorted(os.listdir(tmp_path)) == ["best0.pt", "best1.pt", "checkpoint.pt", "last0.pt", "last1.pt"]
    ckpt = torch.load(tmp_path / "checkpoint.pt")
    assert set(ckpt) == {"epoch", "best_metric", "epochs_since_best", "what", "model", "optimizer", "scheduler", "best0_path", "best1_path",
                         "last0_path", "last1_path"}
    assert torch.load(tmp_path / "best1.pt") == {"what": "best1", "epoch": 1} and torch.load(tmp_path / "last1.pt")["epoch"] == 2


def test_synthetic_size_has_one_precedence():
    synthetic = {"num_sentences": 7, "min_len": 5}
    assert T.synthetic_size({"num_sentences": 3}, synthetic, "num_sentences", 64) == (3, {"min_len": 5})
    assert T.synthetic_size({}, synthetic, "num_sentences", 64) == (7, {"min_len": 5})
    assert T.synthetic_size(None, synthetic, "num_sentences", 64) == (7, {"min_len": 5})
    assert T.synthetic_size(["s1"], {"min_len": 5}, "num_sentences", 64) == (64, {"min_len": 5})
    assert T.synthetic_size(None, None, "num_frames", 256) == (256, {})
    assert T.synthetic_size({"num_frames": 8}, None, "num_frames", 256) == (8, {})
    assert synthetic == {"num_sentences": 7, "min_len": 5}            # the caller's dict is left alone


def test_build_vocabulary(tmp_path):
    from artspeech_amd.settings import BLANK, UNKNOWN
    voc = T.build_vocabulary(None)
    assert len(voc) == 45 and list(voc)[:3] == [BLANK, UNKNOWN, "ph00"] and list(voc.values()) == list(range(45))
    path = tmp_path / "vocab.json"
    path.write_text('["a", "b", "c"]')
    assert T.build_vocabulary(str(path)) == {BLANK: 0, UNKNOWN: 1, "a": 2, "b": 3, "c": 4}
    assert T.build_vocabulary(str(path), default_tokens=(UNKNOWN,)) == {UNKNOWN: 0, "a": 1, "b": 2, "c": 3}
    assert T.load_json(None) is None and T.load_json(str(path)) == ["a", "b", "c"]
    # the scripts' wrappers keep their rules
    import train_phoneme_recognition as R
    import train_phoneme_wise_mean_contour as M
    assert R.build_vocabulary(str(path), R.Criterion.CTC) == {BLANK: 0, UNKNOWN: 1, "a": 2, "b": 3, "c": 4}
    assert R.build_vocabulary(str(path), R.Criterion.CE) == {UNKNOWN: 0, "a": 1, "b": 2, "c": 3}
    assert M.build_vocabulary(str(path)) == {UNKNOWN: 0, "a": 1, "b": 2, "c": 3} and M.build_vocabulary(None) == voc


@pytest.mark.parametrize("fails", [False, True])
def test_run_cli(tmp_path, monkeypatch, fails):
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path / "tmp"))
    os.makedirs(tmp_path / "tmp")
    config = tmp_path / "cfg.yaml"
    config.write_text(yaml.safe_dump({"num_epochs": 3, "train_seq_dict": {"num_sentences": 4}}))
    seen = {}

    def main(**kwargs):
        seen.update(kwargs, torch_seed=torch.initial_seed(), results_dir=T.results_paths(None, "cli_")[0],
                    given=T.results_paths(str(tmp_path / "given"), "cli_")[1])
        assert os.path.isdir(seen["results_dir"]) and os.path.dirname(seen["results_dir"]) == str(tmp_path / "tmp")
        if fails:
            raise RuntimeError("main failed")
        return "result"

    argv = ["--config", str(config), "--checkpoint", "ckpt.pt", "--mlflow", "uri", "--experiment", "e", "--run_id", "r", "--run_name", "n"]
    if fails:
        with pytest.raises(RuntimeError, match="main failed"):
            T.run_cli(main, "experiment", argv=argv)
    else:
        assert T.run_cli(main, "experiment", argv=argv) == "result"
    assert {k: seen[k] for k in ("num_epochs", "train_seq_dict", "checkpoint_filepath", "seed", "torch_seed")} == {
        "num_epochs": 3, "train_seq_dict": {"num_sentences": 4}, "checkpoint_filepath": "ckpt.pt", "seed": 0, "torch_seed": 0}
    assert not os.path.exists(seen["results_dir"]) and os.listdir(tmp_path / "tmp") == []
    assert os.path.isdir(tmp_path / "given") and seen["given"] == str(tmp_path / "given" / "best_model.pt")   # a named one stays
    seen.clear()
    if not fails:                                                     # the form without --checkpoint passes no such keyword
        T.run_cli(main, "experiment", checkpoint=False, argv=["--config", str(config)])
        assert "checkpoint_filepath" not in seen and seen["seed"] == 0
        with pytest.raises(SystemExit):
            T.run_cli(main, "experiment", checkpoint=False, argv=["--config", str(config), "--checkpoint", "ckpt.pt"])


@pytest.mark.parametrize("script", SCRIPTS)
def test_importing_a_script_creates_nothing(script, tmp_path, monkeypatch):
    assert len(SCRIPTS) == 13
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    for name in SCRIPTS:                                              # a fresh import of the script and of the scripts it imports
        monkeypatch.delitem(sys.modules, name, raising=False)
    module = importlib.import_module(script)
    assert callable(module.main)
    assert os.listdir(tmp_path) == []
    assert not hasattr(module, "TMP_DIR") and not hasattr(module, "RESULTS_DIR")


class _FailingModel:
    defer_token_check = False

    def __init__(self):
        self.checked = 0

    def train(self):
        pass

    def check_tokens(self):
        self.checked += 1

    def __call__(self, sentence, lengths):
        assert self.defer_token_check is True
        raise RuntimeError("first")


class _Optimizer:
    def zero_grad(self):
        pass


def test_an_error_in_the_batch_loop_is_the_error_that_propagates():
    import train_phoneme_to_articulation as tr
    from artspeech_amd.settings import TRAIN
    model = _FailingModel()
    batch = (["s0"], torch.zeros(1, 3, dtype=torch.long), torch.zeros(1, 3, 2, 2, 5), torch.tensor([3]), None, None, None, None)
    with pytest.raises(RuntimeError, match="first"):
        tr.run_epoch(TRAIN, 1, model, [batch], _Optimizer(), None, device=torch.device("cpu"))
    assert model.checked == 0 and model.defer_token_check is False and not getattr(model, "_pending_ws", [])
