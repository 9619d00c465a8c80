"""Host-side pieces of the forced alignment (no GPU): the new entry points are declared, bound and exported, the sizing call, the
reference's repeat rule, the refusal of CPU tensors, both configs against main()'s parameters, and the fp64 restatement itself
against an exhaustive search."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch
import yaml

import forced_align_fp64 as F
from conftest import ROOT

NEW_SYMBOLS = ["as_ctc_align_workspace_bytes", "as_ctc_align"]


def test_new_symbols_are_declared_bound_and_exported():
    from artspeech_amd import _lib
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in the header"
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    assert "ctc_align.hip" in __import__("artspeech_amd.build", fromlist=["SOURCES"]).SOURCES
    from artspeech_amd.phoneme_recognition import forced_align
    from artspeech_amd.phoneme_recognition.forced_align import forced_align as same
    assert forced_align is same


def test_workspace_size_needs_no_device():
    from artspeech_amd import _lib
    L = _lib.lib()
    assert L.as_ctc_align_workspace_bytes(64, 4, 16) == 0            # T, B, max target length: the table fits LDS
    assert L.as_ctc_align_workspace_bytes(1024, 4, 512) > 0
    assert L.as_ctc_align_workspace_bytes(1024, 4, 512) == 4 * 1024 * 260   # 2 bits per state, rows padded to 4 bytes
    assert L.as_ctc_align_workspace_bytes(200, 32, 100) == 0        # the recogniser-evaluation shape


def test_phonetic_sequence_is_the_references_repeat_rule():
    from artspeech_amd.phoneme_recognition.forced_align import phonetic_sequence
    assert phonetic_sequence(["a"], [0.0], [0.05], 50) == ["a", "a"]            # 2.5 frames: "%.0f" rounds half to even
    assert phonetic_sequence(["a"], [0.0], [0.07], 50) == ["a"] * 4             # 3.5 -> "4"
    assert phonetic_sequence(["a", "b", "c"], [0.0, 0.1, 0.1], [0.1, 0.1, 0.2], 55) == ["a"] * 6 + ["c"] * 6   # 5.5 -> "6", 0 frames
    assert phonetic_sequence([3, 7], [0.0, 1.0], [1.0, 1.5], 10) == [3] * 10 + [7] * 5
    assert phonetic_sequence([], [], [], 55) == []


def test_filled_runs():
    from artspeech_amd.phoneme_recognition.forced_align import filled_runs
    assert filled_runs([0, 0, 1, 1, 1, 3, -1, -1]) == [(0, 0, 2), (1, 2, 5), (3, 5, 6)]
    assert filled_runs([-1, -1]) == [] and filled_runs([]) == [] and filled_runs([2]) == [(2, 0, 1)]


def test_cpu_tensors_are_refused():
    from artspeech_amd.phoneme_recognition.forced_align import FrameAgreement, forced_align
    em = torch.rand(2, 5, 4).log()
    with pytest.raises(RuntimeError, match="no CPU path"):
        forced_align(em, torch.tensor([[1, 2], [3, -1]]), [5, 5], [2, 1])
    metric = FrameAgreement(0)
    with pytest.raises(ValueError, match="truth"):
        metric(em, torch.tensor([[1, 2], [3, -1]]), [5, 5], [2, 1])
    metric.set_truth(torch.zeros(2, 5, dtype=torch.long), [5, 5])
    with pytest.raises(RuntimeError, match="no CPU path"):
        metric(em, torch.tensor([[1, 2], [3, -1]]), [5, 5], [2, 1])


@pytest.mark.parametrize("name, train, truth", [("align_recognizer_acoustic_synthetic", "train_recognizer_acoustic_synthetic", "acoustic_target"),
                                                ("align_recognizer_synthetic", "train_recognizer_synthetic", "articulatory_target")])
def test_configs_parse_and_read_the_trainers_model(name, train, truth):
    import align_phoneme_recognition as A   # imports cleanly: nothing runs at import
    with open(os.path.join(ROOT, "configs", name + ".yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "configs", train + ".yaml")) as f:
        trainer = yaml.safe_load(f)
    params = inspect.signature(A.main).parameters
    assert set(cfg) <= set(params), set(cfg) - set(params)
    assert cfg["truth"] == truth and cfg["target"] == "ctc_target"
    assert cfg["state_dict_filepath"] == os.path.join(trainer["results_dir"], "best_model.pt")
    for key in ("model_params", "feature", "datadir", "loss"):
        assert cfg[key] == trainer[key], key
    assert cfg["seq_dict"] == trainer["test_seq_dict"]
    assert A.CSV_COLUMNS == ["phoneme", "start_frame", "end_frame", "start_time", "end_time", "score"]
    with pytest.raises(NotImplementedError, match="CTC"):
        A.main(**dict(cfg, loss="CE"))


def test_write_alignment_files(tmp_path):
    import align_phoneme_recognition as A
    names = {0: "_", 1: "a", 2: "b"}
    filled = np.array([0, 0, 0, 1, 1, -1], np.int32)
    tokens = np.array([1, 1, 1, 2, 2, -1], np.int64)
    A.write_alignment(str(tmp_path), 7, names, filled, tokens, np.array([-0.5, -0.25], np.float32), 50.0, framerate=100)
    lines = open(tmp_path / "7.csv").read().split()
    assert lines == ["phoneme,start_frame,end_frame,start_time,end_time,score", "a,0,3,0.0,0.06,-0.5", "b,3,5,0.06,0.1,-0.25"]
    assert np.array_equal(np.load(tmp_path / "7_frames.npy"), [1, 1, 1, 2, 2])
    assert open(tmp_path / "7_phonemes.txt").read().split() == ["a"] * 6 + ["b"] * 4
    A.write_alignment(str(tmp_path), 8, names, np.full(4, -1, np.int32), np.full(4, -1, np.int64), np.zeros(0, np.float32), 50.0)
    assert open(tmp_path / "8.csv").read().split() == ["phoneme,start_frame,end_frame,start_time,end_time,score"]
    assert np.load(tmp_path / "8_frames.npy").size == 0 and not (tmp_path / "8_phonemes.txt").exists()


def test_oracle_finds_the_optimum_and_float32_agrees_on_the_grid():
    """The restatement against an exhaustive search over all state sequences (tiny cases), and the float32 run against the
    float64 run on inputs that are multiples of 1/8 in [-16, 0], where every sum is exact: the same path and score, ties included."""
    rng = np.random.default_rng(0)
    infeasible = 0
    for _ in range(120):
        C, L, Tb = 3, int(rng.integers(0, 4)), int(rng.integers(0, 6))
        lp = -rng.integers(0, 129, size=(Tb, C)) / 8.0
        tg = [int(v) for v in rng.integers(1, C, size=L)]
        score, states = F.viterbi(lp, tg, 0)
        s32, p32 = F.viterbi(lp.astype(np.float32), tg, 0, np.float32)
        assert p32 == states and float(s32) == float(score)
        best = -np.inf
        for cand in itertools.product(range(2 * L + 1), repeat=Tb):
            if F.is_valid_path(list(cand), tg, 0):
                best = max(best, F.rescore(lp, tg, 0, list(cand)))
        if states is None:
            infeasible += 1
            assert best == -np.inf
            continue
        assert best == score == F.rescore(lp, tg, 0, states) and F.is_valid_path(states, tg, 0)
        fi = F.expand(states, lp, tg, 0, Tb + 1, L + 1)[0]
        assert F.states_from_frame_index(fi[:Tb]) == states and fi[Tb] == -1
    assert infeasible > 5
    # the tie rules on hand-made cases of all-equal emissions: the label state ends the path, and stay is preferred on the way back
    assert F.viterbi(np.zeros((3, 2)), [1], 0)[1] == [1, 1, 1]
    assert F.viterbi(np.zeros((2, 3)), [1, 2], 0)[1] == [1, 3]
