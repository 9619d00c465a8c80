"""Host tests (no GPU) of the principal-components training modules: PCA parameter keys, shapes and seeded initialisation,
encoder / decoder type resolution, the refused configurations, the kernel's LDS limit and the loud failure on CPU tensors."""
import ctypes as C

import pytest
import torch


def test_pca_keys_shapes_and_seeded_init():
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder, MultiEncoder, PCADecoder, PCAEncoder
    torch.manual_seed(0)
    e = PCAEncoder(in_features=20, num_components=4)
    torch.manual_seed(0)
    ev, vec = torch.rand(size=(4,)), torch.rand(size=(4, 20))   # the reference's torch.rand order (autoencoder.py:20-29)
    assert torch.equal(e.eigenvalues, ev) and torch.equal(e.eigenvectors, vec)
    torch.manual_seed(0)
    d = PCADecoder(out_features=20, num_components=4)
    torch.manual_seed(0)
    ev, vec = torch.rand(size=(4, 1)), torch.rand(size=(4, 20))
    assert torch.equal(d.eigenvalues, ev) and torch.equal(d.eigenvectors, vec)
    enc = MultiEncoder({"tongue": 3, "lower-lip": 2}, 20, 8, encoder_cls="PCA")
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == {
        "encoders.tongue.eigenvalues": (3,), "encoders.tongue.eigenvectors": (3, 20),
        "encoders.lower-lip.eigenvalues": (2,), "encoders.lower-lip.eigenvectors": (2, 20)}
    dec = MultiDecoder({"tongue": 3, "lower-lip": 2}, 20, 8, decoder_cls=PCADecoder)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == {
        "decoders.tongue.eigenvalues": (3, 1), "decoders.tongue.eigenvectors": (3, 20),
        "decoders.lower-lip.eigenvalues": (2, 1), "decoders.lower-lip.eigenvectors": (2, 20)}


def test_encoder_decoder_type_resolution():
    from artspeech_amd.phoneme_to_articulation.principal_components.models import (Decoder, DecoderType, Encoder, EncoderType,
                                                                                   MultiDecoder, MultiEncoder, PCADecoder,
                                                                                   PCAEncoder)
    assert EncoderType.AE.value is Encoder and EncoderType.PCA.value is PCAEncoder
    assert DecoderType.AE.value is Decoder and DecoderType.PCA.value is PCADecoder
    for cls, want in (("AE", Encoder), ("PCA", PCAEncoder), (Encoder, Encoder), (PCAEncoder, PCAEncoder)):
        assert all(type(m) is want for m in MultiEncoder({"a": 2}, 6, 4, encoder_cls=cls).encoders.values())
    for cls, want in (("AE", Decoder), ("PCA", PCADecoder), (Decoder, Decoder), (PCADecoder, PCADecoder)):
        assert all(type(m) is want for m in MultiDecoder({"a": 2}, 6, 4, decoder_cls=cls).decoders.values())
    with pytest.raises(KeyError):
        MultiEncoder({"a": 2}, 6, 4, encoder_cls="VAE")
    with pytest.raises(NotImplementedError):
        MultiDecoder({"a": 2}, 6, 4, decoder_cls=torch.nn.Linear)
    # seed-for-seed: the MLP containers draw their weights like the reference (one nn.Linear after another)
    torch.manual_seed(1)
    a = MultiEncoder({"a": 2}, 6, 4)
    torch.manual_seed(1)
    ref = [torch.nn.Linear(6, 4), torch.nn.Linear(4, 2), torch.nn.Linear(2, 2)]
    assert torch.equal(a.encoders["a"].encoder[4].weight, ref[2].weight)


def test_refused_configurations():
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import PCADecoder
    with pytest.raises(NotImplementedError, match="whiten"):
        PCADecoder(out_features=10, num_components=3, whiten=True)
    with pytest.raises(NotImplementedError, match="recognizer"):
        AutoencoderLoss2({"tongue": 2}, ["TTCD"], 10, 8, "missing_enc.pt", "missing_dec.pt", "cpu", recognizer=object())


def test_cpu_tensors_fail_loudly():
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    m = MultiArticulatorAutoencoder(10, {"tongue": 2, "lower-lip": 1}, hidden_features=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(3, 2, 10))
    with pytest.raises(RuntimeError, match="no CPU path"):
        RegularizedLatentsMSELoss2(0.1, m.indices_dict)(torch.zeros(3, 2, 10), torch.zeros(3, 3), torch.zeros(3, 2, 10))


def test_multi_mlp_lds_budget_and_unsupported_return():
    from artspeech_amd import _lib
    L = _lib.lib()
    assert L.as_multi_mlp_supported(3, 100, 50, 25, 35) == 1          # thesis sizes
    assert L.as_multi_mlp_supported(1, 100, 0, 0, 35) == 1            # PCA projection
    assert L.as_multi_mlp_supported(3, 300, 64, 32, 3) == 0           # a width beyond 256
    assert L.as_multi_mlp_supported(3, 256, 256, 128, 256) == 0       # within the widths, beyond the LDS budget
    assert L.as_multi_mlp_param_floats(3, 100, 50, 25, 35) == 50 * 100 + 50 + 25 * 50 + 25 + 35 * 25 + 35
    d = _lib.MultiMlp(groups=2, rows=10, layers=3, h1=64, h2=32, k_max=300, n_max=3, latent=6)
    assert L.as_multi_mlp_fwd(C.byref(d), None) == -2                 # AS_ERR_UNSUPPORTED, before any launch
    assert L.as_multi_mlp_bwd(C.byref(d), None) == -2
    assert b"LDS budget" in L.as_last_error()
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    assert not MultiArticulatorAutoencoder(300, {"tongue": 3}, 64).encoders._plan.supported
    assert MultiArticulatorAutoencoder(100, {"tongue": 30, "lips": 5}, 50).encoders._plan.supported


# ------------------------------------------------------------------------------------------------ reference fixtures
def _fixture():
    import os

    import numpy as np
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pc_training.npz")
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_collate_matches_reference_fixture():
    import json

    import numpy as np
    from artspeech_amd.phoneme_to_articulation.principal_components.dataset import pad_sequence_collate_fn
    g = _fixture()
    items = []
    for i in range(4):
        tokens = torch.from_numpy(g[f"col.in{i}.tokens"])
        T = len(tokens)
        items.append((f"s{i}", tokens, torch.from_numpy(g[f"col.in{i}.targets"]), [f"p{int(t)}" for t in tokens],
                      torch.from_numpy(g[f"col.in{i}.mask"]), torch.from_numpy(g[f"col.in{i}.ref"]), [f"{k:04d}" for k in range(T)],
                      torch.from_numpy(g[f"col.in{i}.voicing"])))
    out = pad_sequence_collate_fn(items)
    assert len(out) == 9
    assert list(out[0]) == g["col.ids"].tolist()
    for k, idx in (("tokens", 1), ("targets", 2), ("lengths", 3), ("mask", 5), ("ref", 6), ("voicing", 8)):
        assert out[idx].dtype == torch.from_numpy(g[f"col.{k}"]).dtype, k
        assert np.array_equal(out[idx].numpy(), g[f"col.{k}"]), k
    assert out[4] == json.loads(str(g["col.phonemes"]))
    assert out[7] == json.loads(str(g["col.frames"]))


def _script_signature(path):
    """main()'s keyword names / defaults and the argparse flags (option, dest, default) of a training script: the flags of
    the parser its `run_cli(main, experiment)` call builds (artspeech_amd/training.py)."""
    import ast
    from artspeech_amd.training import cli_parser
    tree = ast.parse(open(path).read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    names = [a.arg for a in main.args.args]
    defaults = [ast.literal_eval(d) for d in main.args.defaults]
    keys = {n: None for n in names}
    keys.update(dict(zip(names[len(names) - len(defaults):], defaults)))
    call, = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "run_cli"]
    assert call.args[0].id == "main" and not call.keywords
    parser = cli_parser(*(ast.literal_eval(a) for a in call.args[1:]))
    flags = [[a.option_strings[0], a.dest, a.default] for a in parser._actions if a.option_strings[0] != "-h"]
    return keys, flags


@pytest.mark.parametrize("which,script", [("autoencoder", "train_principal_components_autoencoder.py"),
                                          ("method", "train_phoneme_to_principal_components.py")])
def test_trainer_flags_and_main_keys_match_the_reference(which, script):
    """Same CLI flags (option, dest, default) and every main() keyword of the reference with its default; the only extra
    keys are the engine's `synthetic` / `results_dir`."""
    import json
    import os
    ref = json.loads(str(_fixture()["signatures"]))[which]
    keys, flags = _script_signature(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), script))
    assert flags == ref["flags"]
    ref_keys = dict((k, v) for k, v in ref["main"])
    assert {k: keys[k] for k in ref_keys if k in keys} == ref_keys
    assert set(keys) - set(ref_keys) == {"synthetic", "results_dir"}


def test_datasets_item_layouts_and_real_data_refusal():
    from artspeech_amd.phoneme_to_articulation.principal_components.dataset import (
        PrincipalComponentsAutoencoderDataset2, PrincipalComponentsPhonemeToArticulationDataset2,
        SyntheticPrincipalComponentsAutoencoderDataset, SyntheticPrincipalComponentsPhonemeToArticulationDataset,
        pad_sequence_collate_fn)
    with pytest.raises(NotImplementedError, match="database_collector"):
        PrincipalComponentsAutoencoderDataset2("artspeech2", "/data", [], ["tongue"])
    with pytest.raises(NotImplementedError, match="vt_shape_gen"):
        PrincipalComponentsPhonemeToArticulationDataset2("artspeech2", "/data", [], {}, ["tongue"], None)
    ds = SyntheticPrincipalComponentsAutoencoderDataset(10, ["tongue", "lower-lip"], n_samples=50)
    name, frame, weight, phoneme = ds[3]
    assert frame.shape == (2, 100) and frame.dtype == torch.float32 and weight.dim() == 0 and isinstance(phoneme, str)
    assert set(ds.normalize) == {"tongue", "lower-lip"} and ds.normalize["tongue"].mean.shape == (2, 50)
    vocab = {"<blank>": 0, "<unk>": 1, "a": 2, "l": 3, "t": 4}
    sds = SyntheticPrincipalComponentsPhonemeToArticulationDataset(5, vocab, ["tongue", "lower-lip"], {"LA": ["l"], "TTCD": ["t"]},
                                                                   n_samples=50, min_len=3, max_len=9)
    item = sds[2]
    T = len(item[1])
    assert len(item) == 8 and item[2].shape == (T, 2, 2, 50) and item[4].shape == (2, T) and item[5].shape == (T, 1, 2, 50)
    batch = pad_sequence_collate_fn([sds[i] for i in range(5)])
    assert len(batch) == 9 and batch[5].shape[:2] == (5, 2) and list(batch[3]) == sorted(batch[3].tolist(), reverse=True)
