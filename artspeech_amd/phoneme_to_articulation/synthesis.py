"""Vocal-tract shape synthesis (reference generate_vocal_tract_shape_v2.py and generate_vocal_tract_shape.py): per-frame phoneme
sequences and a trained model in, the ``inference_contours/`` tree out -- what scripts/shape_to_air_column.py,
SyntheticPhonemeRecognitionDataset and the area function start from.

The reference runs one forward pass per sentence and one host spline fit per (frame, articulator).  Here the sentences are sorted
by length and batched; a batch takes one forward pass of the model and one as_contour_spline launch over its (B, T, A) contours
(``regularize_contours`` with the batch's lengths).  The smoothing is this project's own definition (regularization.py): parity
with ``vt_tools.bs_regularization.regularize_Bsplines`` is unpinned.

With ``air_column`` the batch takes one more launch, as_vocal_tract_tube over its (B, T) frames (``vocal_tract_tube`` with the
batch's lengths), and every sentence gains air_column/%04d.npy and xarticul/%04d.txt (v2 :425-439).  The tube is this project's own
definition too (vocal_tract_tube.py): parity with ``vt_shape_gen.vocal_tract_tube.generate_vocal_tract_tube`` is unpinned.

Left out, with the reference's line numbers: the jpg / pdf / avi rendering (:190-241) and TextGrid parsing (:124-158, ``tgt`` is
absent: the ``<index>_phonemes.txt`` files of align_phoneme_recognition.py stand in)."""
import json
import os
import re

import numpy as np
import torch

from ..helpers import npy_to_xarticul
from ..settings import UNKNOWN
from .regularization import STATUS_NON_FINITE, STATUS_ZERO_LENGTH, regularize_contours
from .tail_clipper import UPPER_INCISOR
from .vocal_tract_tube import vocal_tract_tube

METHODS = ("encoder_decoder", "mean_contour", "autoencoder")


# ---------------------------------------------------------------------------------------------------- sentences (host)
def read_phonemes(filepath):
    """A ``target_sequence.txt``: the sentence's per-frame phonemes separated by blanks (v2 :391-392)."""
    with open(filepath) as f:
        return f.read().split()


def read_sentences(sentences=None, alignments_dir=None):
    """[(name, per-frame phonemes)]: the configured ``sentences`` ({name, phonemes_filepath}) in order, then every
    ``<index>_phonemes.txt`` of ``alignments_dir`` by index.  A file without frames (an utterance that has no alignment) is left
    out; a name given twice is an error, as it would overwrite a directory."""
    out = []
    for entry in sentences or []:
        out.append((str(entry["name"]), read_phonemes(entry["phonemes_filepath"])))
    if alignments_dir is not None:
        found = []
        for fname in os.listdir(alignments_dir):
            m = re.fullmatch(r"(\d+)_phonemes\.txt", fname)
            if m:
                found.append((int(m.group(1)), fname))
        for index, fname in sorted(found):
            out.append((str(index), read_phonemes(os.path.join(alignments_dir, fname))))
    out = [(name, tokens) for name, tokens in out if tokens]
    names = [name for name, _ in out]
    twice = sorted({n for n in names if names.count(n) > 1})
    if twice:
        raise ValueError(f"sentence name(s) given twice: {', '.join(twice)}")
    if not out:
        raise ValueError("there is no sentence to synthesise (sentences, alignments_dir or datadir: synthetic)")
    return out


def synthetic_sentences(vocabulary, articulators, seed=0, num_sentences=8, **options):
    """Seeded sentences with phoneme runs: the token strings of SyntheticSegmentedArtSpeechDataset's utterances."""
    from .phoneme_wise_mean_contour import SyntheticSegmentedArtSpeechDataset
    dataset = SyntheticSegmentedArtSpeechDataset(num_sentences, vocabulary, articulators, seed=seed, **options)
    return [(item[0], list(item[3])) for item in (dataset[i] for i in range(len(dataset)))]


def numerize(tokens, vocabulary):
    """``vocabulary.get(token, vocabulary[UNKNOWN])`` per frame (v2 :104-107)."""
    unknown = vocabulary[UNKNOWN]
    return torch.tensor([vocabulary.get(token, unknown) for token in tokens], dtype=torch.long)


def make_batches(sentences, batch_size):
    """Indices into ``sentences``, longest first (the packed recurrences want descending lengths), ``batch_size`` at a time."""
    order = sorted(range(len(sentences)), key=lambda i: -len(sentences[i][1]))
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


# ---------------------------------------------------------------------------------------------------- models
def load_denormalize(datadir, articulators, n_samples=50, seed=0):
    """{articulator: Normalize.inverse} from ``<datadir>/normalization_statistics/<articulator>_{mean,std}.npy`` (v2 :315-329,
    the files calculate_normalization_statistics.py writes); ``datadir: synthetic`` gives the synthetic data sets' seeded
    statistics."""
    from .principal_components.dataset import _normalizers
    from .transforms import Normalize
    if datadir == "synthetic":
        normalize = _normalizers(sorted(articulators), n_samples, torch.Generator().manual_seed(seed))
        return {a: n.inverse for a, n in normalize.items()}
    stats = os.path.join(datadir, "normalization_statistics")
    return {a: Normalize(torch.from_numpy(np.load(os.path.join(stats, f"{a}_mean.npy"))),
                         torch.from_numpy(np.load(os.path.join(stats, f"{a}_std.npy")))).inverse for a in articulators}


def build_model(method, vocabulary, articulators, state_dict_filepath, model_params=None, aux_state_dict_filepath=None,
                aux_model_params=None, datadir=None, seed=0, device=None):
    """The model of one of the reference's three methods (v2 :295-353) on ``device``, in eval mode, as a callable
    (tokens (B, T) on the device, lengths descending) -> (B, T, A, 2, N).  ``state_dict_filepath`` None leaves the fresh
    initialisation (encoder_decoder and autoencoder)."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    model_params, aux_model_params = dict(model_params or {}), dict(aux_model_params or {})
    if method == "encoder_decoder":
        from .encoder_decoder.models import ArtSpeech
        model = ArtSpeech(len(vocabulary), len(articulators), **model_params)
        if state_dict_filepath is not None:
            model.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
        return model.to(device).eval()
    if method == "mean_contour":
        from .phoneme_wise_mean_contour import _as_model
        table = _as_model(state_dict_filepath, device)
        weighted = bool(model_params.pop("weighted", False))
        frac, random_state = model_params.pop("frac", 0.1), model_params.pop("random_state", 0)
        if model_params:
            raise TypeError(f"mean_contour: unknown model_params {sorted(model_params)} (weighted, frac, random_state)")
        if frac is not None and frac < 1.0 and not table.sampled:   # the reference's .sample(frac=0.1, random_state=0) per token
            table = table.resample(frac, random_state)
        channels = [table.articulators.index(a) for a in articulators]
        ids = torch.tensor([table.vocabulary.get(t, -1) for t, _ in sorted(vocabulary.items(), key=lambda kv: kv[1])], device=device)

        def forward(tokens, lengths):
            mapped = ids[tokens]   # the script's vocabulary -> the table's; a token the table never saw raises there
            out = table.forward(mapped, lengths, weighted=weighted)
            return out if channels == list(range(len(table.articulators))) else out[:, :, channels]
        return forward
    if method == "autoencoder":
        from .principal_components.models import MultiDecoder, PrincipalComponentsArtSpeech, PrincipalComponentsArtSpeechWrapper
        decoder = MultiDecoder(**aux_model_params)
        if aux_state_dict_filepath is not None:
            decoder.load_state_dict(torch.load(aux_state_dict_filepath, map_location="cpu"))
        rnn = PrincipalComponentsArtSpeech(len(vocabulary), **model_params)
        if state_dict_filepath is not None:
            rnn.load_state_dict(torch.load(state_dict_filepath, map_location="cpu"))
        n_samples = aux_model_params["in_features"] // 2
        denormalize = load_denormalize(datadir, decoder.sorted_articulators, n_samples, seed)
        model = PrincipalComponentsArtSpeechWrapper(rnn, decoder, denormalize).to(device).eval()
        channels = [decoder.sorted_articulators.index(a) for a in articulators]
        if channels == list(range(len(decoder.sorted_articulators))):
            return model
        return lambda tokens, lengths: model(tokens, lengths)[:, :, channels]
    raise ValueError(f"Unavailable method '{method}' (one of {', '.join(METHODS)})")


# ---------------------------------------------------------------------------------------------------- the synthesis
def synthesize_batch(model, token_rows, regularize_outputs=True, degree=3, n_ctrl=12, smoothing=1e-3, n_out=None):
    """token_rows: id tensors sorted by descending length -> (contours (B, T, A, 2, n_out or N) on the device, zeros behind each
    sentence's length when regularised; status (B, T, A) int32 or None; lengths).  One forward pass, one spline launch."""
    lengths = [int(t.numel()) for t in token_rows]
    tokens = torch.nn.utils.rnn.pad_sequence(token_rows, batch_first=True).cuda()
    with torch.no_grad():
        outputs = model(tokens, lengths)
    if not regularize_outputs:
        return outputs, None, lengths
    contours, status = regularize_contours(outputs, degree, n_ctrl, smoothing, n_out, lengths=lengths, return_status=True)
    return contours, status, lengths


def tube_channels(contours, articulators, upper_incisor=None):
    """The contours (..., A, 2, n) and channel names that the tube is built from: the configured upper incisor joined as one more
    channel when the articulators lack one (v2 :244-267 saves it beside every frame for the same reason)."""
    articulators = list(articulators)
    if upper_incisor is None or UPPER_INCISOR in articulators:
        return contours, articulators
    incisor = torch.as_tensor(np.asarray(upper_incisor, dtype=np.float32))
    if incisor.shape != (2, contours.shape[-1]):
        raise ValueError(f"the upper incisor has {tuple(incisor.shape)} coordinates, the contours {contours.shape[-1]} points each: "
                         "give it the contours' point count (n_out)")
    incisor = incisor.to(contours.device).expand(contours.shape[:-3] + (1, 2, contours.shape[-1]))
    return torch.cat([contours.float(), incisor], dim=-3), articulators + [UPPER_INCISOR]


def save_air_columns(save_dir, air_columns, res=1.0):
    """air_columns (T, 2, 2, n_wall) float64 -> air_column/%04d.npy in ``save_air_column``'s layout and xarticul/%04d.txt,
    ``npy_to_xarticul(internal * res) + npy_to_xarticul(external * res)`` (v2 :425-439), numbered from 1."""
    air_dir, xarticul_dir = os.path.join(save_dir, "air_column"), os.path.join(save_dir, "xarticul")
    os.makedirs(air_dir, exist_ok=True)
    os.makedirs(xarticul_dir, exist_ok=True)
    for i_frame, air in enumerate(np.asarray(air_columns, dtype=np.float64), start=1):
        np.save(os.path.join(air_dir, f"{'%04d' % i_frame}.npy"), air)
        lines = npy_to_xarticul(air[0].T * res) + npy_to_xarticul(air[1].T * res)
        with open(os.path.join(xarticul_dir, f"{'%04d' % i_frame}.txt"), "w") as f:
            f.write("\n".join(lines))


def save_sentence(save_dir, tokens, contours, articulators, upper_incisor=None, save_frames=True, air_column=False, n_wall=100,
                  res=1.0):
    """One sentence's files (v2 :244-267, :391-392): target_sequence.txt, contours.npy (T, A, 2, n) and, with ``save_frames``,
    inference_contours/%04d_<articulator>.npy numbered from 1, plus the upper incisor's when given and not an articulator.
    ``air_column``: False writes nothing more; a (T, 2, 2, n_wall) array (the caller's batched launch) is written as
    air_column/ and xarticul/ (``save_air_columns``); True builds the walls of ``n_wall`` points here, one launch for the sentence."""
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "target_sequence.txt"), "w") as f:
        f.write(" ".join(tokens))
    np.save(os.path.join(save_dir, "contours.npy"), contours)
    if air_column is True:
        x, names = tube_channels(torch.as_tensor(np.asarray(contours, dtype=np.float32)).cuda(), articulators, upper_incisor)
        air_column = vocal_tract_tube(x, names, n_out=n_wall).cpu().numpy()
    if air_column is not False and air_column is not None:
        save_air_columns(save_dir, air_column, res)
    if not save_frames:
        return
    frames_dir = os.path.join(save_dir, "inference_contours")
    os.makedirs(frames_dir, exist_ok=True)
    for i_frame, frame in enumerate(contours, start=1):
        for articulator, contour in zip(articulators, frame):
            np.save(os.path.join(frames_dir, f"{'%04d' % i_frame}_{articulator}.npy"), contour)
        if upper_incisor is not None and UPPER_INCISOR not in articulators:
            np.save(os.path.join(frames_dir, f"{'%04d' % i_frame}_{UPPER_INCISOR}.npy"), upper_incisor)


def synthesize(model, sentences, vocabulary, articulators, save_to, batch_size=32, regularize_outputs=True, degree=3, n_ctrl=12,
               smoothing=1e-3, n_out=None, upper_incisor=None, save_frames=True, air_column=False, n_wall=100, res=1.0):
    """Every sentence of ``sentences`` [(name, phonemes)] through ``model`` and the smoothing, written under ``save_to/<name>/``;
    returns the summary that main() writes to synthesis.json.  ``air_column``: one vocal_tract_tube launch per batch after the
    smoothing, walls of ``n_wall`` points, air_column/ and xarticul/ (scaled by ``res``, the data set's image resolution) beside
    the contours, and the count of flagged walls in the summary."""
    flagged = {"zero_length": 0, "non_finite": 0}
    flagged_walls = {"zero_length": 0, "non_finite": 0}
    report = []
    for batch in make_batches(sentences, batch_size):
        rows = [numerize(sentences[i][1], vocabulary) for i in batch]
        contours, status, lengths = synthesize_batch(model, rows, regularize_outputs, degree, n_ctrl, smoothing, n_out)
        air = wall_status = None
        if air_column:
            x, names = tube_channels(contours, articulators, upper_incisor)
            air, wall_status = vocal_tract_tube(x, names, n_out=n_wall, lengths=lengths, return_status=True)
            air, wall_status = air.cpu().numpy(), wall_status.cpu().numpy()
        contours = contours.cpu().numpy()   # one copy per batch
        status = status.cpu().numpy() if status is not None else None
        for b, i in enumerate(batch):
            name, tokens = sentences[i]
            length = lengths[b]
            entry = {"name": name, "frames": length}
            if status is not None:
                s = status[b, :length]
                entry["zero_length"], entry["non_finite"] = int((s & STATUS_ZERO_LENGTH != 0).sum()), int((s & STATUS_NON_FINITE != 0).sum())
                flagged["zero_length"] += entry["zero_length"]
                flagged["non_finite"] += entry["non_finite"]
            if wall_status is not None:
                s = wall_status[b, :length]
                flagged_walls["zero_length"] += int((s & STATUS_ZERO_LENGTH != 0).sum())
                flagged_walls["non_finite"] += int((s & STATUS_NON_FINITE != 0).sum())
            save_sentence(os.path.join(save_to, name), tokens, contours[b, :length], articulators, upper_incisor, save_frames,
                          air[b, :length] if air is not None else False, n_wall, res)
            report.append(entry)
    position = {name: i for i, (name, _) in enumerate(sentences)}
    report.sort(key=lambda e: position[e["name"]])
    info = {"sentences": report, "frames": sum(e["frames"] for e in report), "flagged_contours": flagged if regularize_outputs else None}
    if air_column:
        info["flagged_walls"] = flagged_walls
    return info


def write_summary(save_to, info):
    with open(os.path.join(save_to, "synthesis.json"), "w") as f:
        json.dump(info, f, indent=2)
