"""generate_vocal_tract_shape.py end to end on the device, from configs written into tmp_path: the three methods with the smallest
models their constructors allow, three sentences of 12, 7 and 1 frames."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

TOKENS = ["a", "b", "c"]
SENTENCES = {"long": "a a a b b c c c a a b b", "mid": "c c b b b a a", "one": "b"}
ARTICULATORS = ["lower-lip", "tongue"]
N = 20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def run_script(cfg, tmp_path, name="cfg.yaml"):
    """python generate_vocal_tract_shape.py --config <file>, in this process"""
    import generate_vocal_tract_shape as script
    from artspeech_amd.training import run_cli
    path = tmp_path / name
    path.write_text(yaml.safe_dump(cfg, sort_keys=False))   # indices_dict assigns the latent slices in the file's order
    return run_cli(script.main, "vocal_tract_shape_synthesis", checkpoint=False, argv=["--config", str(path)])


def base_config(tmp_path, sentences=SENTENCES):
    vocab = tmp_path / "vocab.json"
    vocab.write_text(json.dumps(TOKENS))
    entries = []
    for name, text in sentences.items():
        (tmp_path / f"{name}.txt").write_text(text)
        entries.append({"name": name, "phonemes_filepath": str(tmp_path / f"{name}.txt")})
    return {"vocab_filepath": str(vocab), "articulators": list(ARTICULATORS), "sentences": entries, "batch_size": 3}


def vocabulary():
    return {"<blank>": 0, "<unk>": 1, "a": 2, "b": 3, "c": 4}


def padded_tokens(dev, sentences=SENTENCES):
    """The batch synthesize() builds: sentences by descending length, padded with 0."""
    from artspeech_amd.phoneme_to_articulation.synthesis import numerize
    order = sorted(sentences, key=lambda k: -len(sentences[k].split()))
    rows = [numerize(sentences[k].split(), vocabulary()) for k in order]
    return order, torch.nn.utils.rnn.pad_sequence(rows, batch_first=True).to(dev), [len(r) for r in rows]


def check_tree(save_to, order, lengths, want, upper_incisor=None, n=N):
    """contours.npy against ``want`` (B, T, A, 2, n) bit for bit, the per-frame files numbered from 1, target_sequence.txt."""
    for b, (name, length) in enumerate(zip(order, lengths)):
        folder = os.path.join(save_to, name)
        contours = np.load(os.path.join(folder, "contours.npy"))
        assert contours.shape == (length, 2, 2, n) and contours.dtype == np.float32
        assert np.array_equal(contours, want[b, :length]), name
        assert open(os.path.join(folder, "target_sequence.txt")).read().split() == SENTENCES[name].split()
        files = sorted(os.listdir(os.path.join(folder, "inference_contours")))
        per_frame = 2 + (upper_incisor is not None)
        assert len(files) == per_frame * length and files[0].startswith("0001_") and not any(f.startswith("0000") for f in files)
        for t in range(length):
            for a, art in enumerate(ARTICULATORS):
                frame = np.load(os.path.join(folder, "inference_contours", f"{t + 1:04d}_{art}.npy"))
                assert frame.shape == (2, n) and np.array_equal(frame, contours[t, a])
            incisor = os.path.join(folder, "inference_contours", f"{t + 1:04d}_upper-incisor.npy")
            assert os.path.exists(incisor) == (upper_incisor is not None)
            if upper_incisor is not None:
                assert np.array_equal(np.load(incisor), upper_incisor)


@pytest.fixture(scope="module")
def artspeech(dev, tmp_path_factory):
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech
    torch.manual_seed(3)
    params = {"embed_dim": 16, "hidden_size": 32, "n_samples": N}
    model = ArtSpeech(5, 2, **params)
    path = tmp_path_factory.mktemp("artspeech") / "best_model.pt"
    torch.save(model.state_dict(), path)
    return model.to(dev).eval(), params, str(path)


def test_encoder_decoder_end_to_end(dev, tmp_path, artspeech):
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    model, params, path = artspeech
    incisor = np.linspace(0.2, 0.4, 2 * N, dtype=np.float32).reshape(2, N)
    np.save(tmp_path / "incisor.npy", incisor)
    cfg = dict(base_config(tmp_path), method="encoder_decoder", state_dict_filepath=path, model_params=params,
               save_to=str(tmp_path / "out"), upper_incisor_filepath=str(tmp_path / "incisor.npy"))
    info = run_script(cfg, tmp_path)
    order, tokens, lengths = padded_tokens(dev)
    assert order == ["long", "mid", "one"] and lengths == [12, 7, 1]
    with torch.no_grad():
        outputs = model(tokens, lengths)
    want = regularize_contours(outputs, lengths=lengths)
    assert torch.all(want[1, 7:] == 0) and torch.all(want[2, 1:] == 0)
    check_tree(cfg["save_to"], order, lengths, want.cpu().numpy(), upper_incisor=incisor)
    summary = json.load(open(os.path.join(cfg["save_to"], "synthesis.json")))
    assert summary["frames"] == 20 == info["frames"] and [s["name"] for s in summary["sentences"]] == list(SENTENCES)
    assert summary["flagged_contours"] == {"zero_length": 0, "non_finite": 0} and summary["parameters"]["n_ctrl"] == 12

    # regularize_outputs: false is the model's output bit for bit; no upper-incisor file unless asked for
    raw = dict(cfg, regularize_outputs=False, save_to=str(tmp_path / "raw"))
    del raw["upper_incisor_filepath"]
    run_script(raw, tmp_path, "raw.yaml")
    check_tree(raw["save_to"], order, lengths, outputs.cpu().numpy())

    # one sentence per batch: the same contours within the project's contour bound (1e-4 relative)
    single = dict(cfg, batch_size=1, save_to=str(tmp_path / "single"), save_frames=False)
    run_script(single, tmp_path, "single.yaml")
    for name in order:
        a = np.load(os.path.join(single["save_to"], name, "contours.npy")).astype(np.float64)
        b = np.load(os.path.join(cfg["save_to"], name, "contours.npy")).astype(np.float64)
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), name
        assert not os.path.exists(os.path.join(single["save_to"], name, "inference_contours"))

    # other smoothing parameters reach the launch
    other = dict(cfg, degree=2, n_ctrl=6, smoothing=0.5, n_out=33, save_to=str(tmp_path / "other"), save_frames=False)
    run_script(other, tmp_path, "other.yaml")
    want33 = regularize_contours(outputs, 2, 6, 0.5, 33, lengths=lengths).cpu().numpy()
    assert np.array_equal(np.load(os.path.join(other["save_to"], "mid", "contours.npy")), want33[1, :7])


def test_alignment_files_are_consumed(dev, tmp_path, artspeech):
    """The <index>_phonemes.txt files of align_phoneme_recognition.py, an unknown token among them."""
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    model, params, path = artspeech
    al = tmp_path / "alignments"
    al.mkdir()
    (al / "0_phonemes.txt").write_text("a a zz b")
    (al / "1_phonemes.txt").write_text("c c")
    (al / "1.csv").write_text("phoneme,start_frame\n")
    cfg = dict(base_config(tmp_path), method="encoder_decoder", state_dict_filepath=path, model_params=params,
               save_to=str(tmp_path / "out"), alignments_dir=str(al))
    del cfg["sentences"]
    info = run_script(cfg, tmp_path)
    assert [s["name"] for s in info["sentences"]] == ["0", "1"] and info["frames"] == 6
    tokens = torch.tensor([[2, 2, 1, 3], [4, 4, 0, 0]], device=dev)   # zz -> <unk>
    with torch.no_grad():
        want = regularize_contours(model(tokens, [4, 2]), lengths=[4, 2]).cpu().numpy()
    assert np.array_equal(np.load(os.path.join(cfg["save_to"], "0", "contours.npy")), want[0])
    assert np.array_equal(np.load(os.path.join(cfg["save_to"], "1", "contours.npy")), want[1, :2])
    assert open(os.path.join(cfg["save_to"], "0", "target_sequence.txt")).read() == "a a zz b"


def test_mean_contour_end_to_end(dev, tmp_path):
    from artspeech_amd.phoneme_to_articulation.phoneme_wise_mean_contour import PhonemeWiseMeanContour, write_table
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    rng = np.random.default_rng(11)
    rows = ["a", "b", "c", "a", "b", "c", "c"]
    write_table(str(tmp_path / "table.csv"), rows, None, rng.random((len(rows), 2, 2, N), dtype=np.float32), ARTICULATORS)
    cfg = dict(base_config(tmp_path), method="mean_contour", state_dict_filepath=str(tmp_path / "table.csv"),
               model_params={"frac": 1.0}, save_to=str(tmp_path / "out"))
    run_script(cfg, tmp_path)
    table = PhonemeWiseMeanContour.from_csv(str(tmp_path / "table.csv"), device=dev)
    order, _, lengths = padded_tokens(dev)
    ids = torch.nn.utils.rnn.pad_sequence([table.numerize(SENTENCES[k].split()) for k in order], batch_first=True).to(dev)
    want = regularize_contours(table.forward(ids, lengths), lengths=lengths)
    check_tree(cfg["save_to"], order, lengths, want.cpu().numpy())


def test_autoencoder_end_to_end(dev, tmp_path):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import (MultiDecoder, PrincipalComponentsArtSpeech,
                                                                                    PrincipalComponentsArtSpeechWrapper)
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    from artspeech_amd.phoneme_to_articulation.transforms import Normalize
    torch.manual_seed(5)
    comps = {"tongue": 2, "lower-lip": 1}
    rnn_params = {"indices_dict": comps, "embed_dim": 16, "hidden_size": 32}
    dec_params = {"indices_dict": comps, "in_features": 2 * N, "hidden_features": 8}
    rnn, dec = PrincipalComponentsArtSpeech(5, **rnn_params), MultiDecoder(**dec_params)
    torch.save(rnn.state_dict(), tmp_path / "rnn.pt")
    torch.save(dec.state_dict(), tmp_path / "dec.pt")
    stats = tmp_path / "data" / "normalization_statistics"
    stats.mkdir(parents=True)
    g = torch.Generator().manual_seed(1)
    normalize = {}
    for art in ARTICULATORS:
        mean, std = torch.rand(2, N, generator=g), 0.1 + torch.rand(2, N, generator=g)
        np.save(stats / f"{art}_mean.npy", mean.numpy())
        np.save(stats / f"{art}_std.npy", std.numpy())
        normalize[art] = Normalize(mean, std).inverse
    cfg = dict(base_config(tmp_path), method="autoencoder", state_dict_filepath=str(tmp_path / "rnn.pt"), model_params=rnn_params,
               aux_state_dict_filepath=str(tmp_path / "dec.pt"), aux_model_params=dec_params, datadir=str(tmp_path / "data"),
               n_ctrl=8, save_to=str(tmp_path / "out"))
    run_script(cfg, tmp_path)
    model = PrincipalComponentsArtSpeechWrapper(rnn, dec, normalize).to(dev).eval()
    order, tokens, lengths = padded_tokens(dev)
    with torch.no_grad():
        want = regularize_contours(model(tokens, lengths), n_ctrl=8, lengths=lengths)
    check_tree(cfg["save_to"], order, lengths, want.cpu().numpy())
