"""Host-side pieces of recogniser training (no GPU): the trainer's config contract, the collate function, greedy CTC decoding,
the edit distance, TrainableDeepSpeech2's state_dict / seeded initialisation and its refusals."""
import inspect
import os

import pytest
import torch
import yaml

from conftest import ROOT


def test_config_keys_are_main_arguments():
    import train_phoneme_recognition as T
    params = set(inspect.signature(T.main).parameters)
    with open(os.path.join(ROOT, "configs", "train_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) <= params, set(cfg) - params
    assert cfg["loss"] == "CTC" and cfg["loss_params"] == {"zero_infinity": True} and cfg["logits_large_margins"] == 0.0005
    with open(os.path.join(ROOT, "configs", "train_pc_based_recognizer_synthetic.yaml")) as f:
        pc = yaml.safe_load(f)
    mp = dict(cfg["model_params"])
    assert mp.pop("dropout") == 0.1
    assert mp == pc["recognizer_params"]
    assert len(T.build_vocabulary(None, T.Criterion.CTC)) == 45


def test_collate_pads_with_minus_one_and_reports_lengths():
    from artspeech_amd.phoneme_recognition import Feature
    from artspeech_amd.phoneme_recognition.datasets import SyntheticPhonemeRecognitionDataset, collate_fn
    vocab = {"<blank>": 0, "<unk>": 1, **{f"ph{i:02d}": i + 2 for i in range(5)}}
    ds = SyntheticPhonemeRecognitionDataset(3, vocab, min_len=6, max_len=15, voiced_tokens=["ph00"], seed=3)
    items = [ds[i] for i in range(3)]
    b = collate_fn(items, [Feature.VOCAL_TRACT])
    T = max(it["vocal_tract_length"] for it in items)
    assert b["vocal_tract"].shape == (3, 2, 500, T)
    for i, it in enumerate(items):
        n, L = it["vocal_tract_length"], it["ctc_target_length"]
        assert int(b["vocal_tract_length"][i]) == n and int(b["ctc_target_length"][i]) == L
        assert torch.equal(b["vocal_tract"][i, :, :, :n], it["vocal_tract"])
        assert (b["vocal_tract"][i, :, :, n:] == -1).all() and (b["ctc_target"][i, L:] == -1).all() and (b["voicing"][i, n:] == -1).all()
        assert torch.equal(it["ctc_target"], torch.unique_consecutive(it["articulatory_target"]))
        assert (it["articulatory_target"] >= 2).all()
        assert torch.equal(it["voicing"], (it["articulatory_target"] == 2).float())


def test_greedy_decoder_and_edit_distance_known_answers():
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder, TopKDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance, word_error_rate
    dec = GreedyCTCDecoder(["<blank>", "a", "b", "c"], blank_token="<blank>")
    frames = torch.tensor([[1, 1, 0, 2, 2, 0, 0, 3, 3, 1]])
    em = torch.nn.functional.one_hot(frames, 4).float()
    assert dec(em, torch.tensor([9]))[0][0].tokens.tolist() == [1, 2, 3]
    assert dec(em, torch.tensor([10]))[0][0].tokens.tolist() == [1, 2, 3, 1]
    assert TopKDecoder(["<blank>", "a", "b", "c"], blank_token=0)(em, None)[0][0].tokens == [1, 2, 3, 1]
    assert word_error_rate(["1 2 3"], ["1 3"]) == 0.5
    ed = EditDistance(dec)
    assert ed(em, torch.tensor([[1, 3, -1]]), torch.tensor([9]), torch.tensor([2])) == 0.5
    assert word_error_rate(["1 2", "4"], ["1 2 3", "4 5"]) == 2 / 5


def test_trainable_model_state_dict_and_seeded_init():
    from artspeech_amd.phoneme_recognition import DeepSpeech2, TrainableDeepSpeech2
    kw = dict(in_channels=2, num_residual_layers=2, num_rnn_layers=2, rnn_hidden_size=16, num_classes=9, num_features=12,
              adapter_out_features=10)
    torch.manual_seed(4)
    a = DeepSpeech2(**kw).state_dict()
    torch.manual_seed(4)
    b = TrainableDeepSpeech2(**kw).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_trainable_model_refuses_cpu_inputs_and_ce_loss(tmp_path):
    import train_phoneme_recognition as T
    from artspeech_amd.phoneme_recognition import TrainableDeepSpeech2
    m = TrainableDeepSpeech2(in_channels=1, num_residual_layers=1, num_rnn_layers=1, rnn_hidden_size=8, num_classes=5, num_features=6)
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(RuntimeError, match="MI355X"):
            m(torch.randn(1, 1, 6, 4))
    with pytest.raises(NotImplementedError, match="CTC"):
        T.Criterion.CE.value()
    with open(os.path.join(ROOT, "configs", "train_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    with pytest.raises(NotImplementedError, match="CTC"):
        T.main(**dict(cfg, loss="CE", results_dir=str(tmp_path)))
