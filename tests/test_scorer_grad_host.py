"""Host-side checks of the recognition term of the principal-components method: the recognizer config against the trainer's
signature, and the refusals that need no GPU."""
import inspect
import os

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recognizer_config_keys_are_main_arguments():
    import train_phoneme_to_principal_components as TP
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_pc_based_recognizer_synthetic.yaml")))
    params = inspect.signature(TP.main).parameters
    assert set(cfg) <= set(params), set(cfg) - set(params)
    required = {n for n, p in params.items() if p.default is inspect.Parameter.empty}
    assert required <= set(cfg), required - set(cfg)
    assert cfg["beta4"] > 0 and cfg["recognizer_filepath"]
    # the thesis scorer: 2 planes of 10 articulators x 50 points, adapted to 80 features
    assert cfg["recognizer_params"] == dict(in_channels=2, num_residual_layers=4, num_rnn_layers=2, rnn_hidden_size=64,
                                            num_features=500, adapter_out_features=80)
    assert len(cfg["indices_dict"]) * 50 == cfg["recognizer_params"]["num_features"]
    from artspeech_amd.phoneme_recognition import DeepSpeech2
    DeepSpeech2(num_classes=45, **cfg["recognizer_params"])   # the trainer's construction


@pytest.mark.parametrize("recognizer", [object(), torch.nn.Linear(2, 2)])
def test_autoencoder_loss2_refuses_other_recognizers(recognizer):
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    with pytest.raises(NotImplementedError, match="recognizer"):
        AutoencoderLoss2({"tongue": 2}, ["TTCD"], 10, 8, "missing_enc.pt", "missing_dec.pt", "cpu", beta4=1.0, recognizer=recognizer)


def test_scorer_input_gradient_has_no_cpu_path():
    from artspeech_amd.phoneme_recognition import DeepSpeech2
    m = DeepSpeech2(2, 1, 1, 32, num_classes=5, num_features=12).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 2, 12, 3, requires_grad=True))
