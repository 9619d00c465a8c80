"""Data of the phoneme recogniser (reference ``phoneme_recognition/datasets.py``, ``synthetic_shapes.py``): the collate function
(:253-302), a seeded synthetic data set with the reference's item layout (synthetic_shapes.py:146-158), and the real-data class,
which needs the reference's MRI data stack and raises without it, and ``ShapeTreeRecognitionDataset``, which reads the tree that
``generate_vocal_tract_shape.py`` writes with ``air_column: true`` (the reference's synthetic_shapes.py).  For the speech signal: seeded synthetic waveforms, WAV
recordings listed in a manifest (``read_wav``, ``RecordedAcousticRecognitionDataset``), and ``acoustic_collate_fn``, which brings
a batch to the model's rate (:124-126) and computes its log-mel features on the device."""
import json
import logging
import os
import wave
from glob import glob

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import Dataset

_NEEDS_DATA_STACK = ("needs the reference's real-data stack (database_collector.DATABASE_COLLECTORS, vt_shape_gen / vt_tools and "
                     "the air-column / mel-spectrogram feature extraction), which this engine does not vendor; use datadir: synthetic")


class PhonemeRecognitionDataset(Dataset):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"PhonemeRecognitionDataset {_NEEDS_DATA_STACK}")


class SyntheticPhonemeRecognitionDataset(Dataset):
    """num_sentences seeded utterances over vocabulary ({token: index}; the first ``num_special`` indices -- blank and unknown --
    never occur).  Every token has a prototype frame (seeded by prototype_seed, the same for every split) of the vocal-tract feature (2, n_articulators * n_samples); a
    sentence is a random token sequence in which each token holds for 2 to 6 frames (between min_len and max_len frames in all),
    its frames the token's prototype plus Gaussian noise of scale ``noise``.  Items carry the reference's keys: ``vocal_tract``
    (2, A*N, T) and ``air_column`` (2, 2N, T) with their lengths, ``articulatory_target`` (the per-frame tokens), ``voicing``
    (1 where the frame's token is in voiced_tokens) and ``ctc_target = unique_consecutive(articulatory_target)``."""

    def __init__(self, num_sentences, vocabulary, n_articulators=10, n_samples=50, min_len=20, max_len=120, noise=0.3, seed=0,
                 voiced_tokens=None, num_special=2, prototype_seed=0):
        self.vocabulary = vocabulary
        self.num_sentences, self.min_len, self.max_len, self.noise = num_sentences, min_len, max_len, noise
        self.voiced = set(voiced_tokens or [])
        self.names = {i: tok for tok, i in vocabulary.items()}
        self.token_ids = sorted(i for i in vocabulary.values() if i >= num_special)
        V = max(vocabulary.values()) + 1
        gp = torch.Generator().manual_seed(prototype_seed)   # shared by every split: the splits differ in their sentences only
        self.prototypes = torch.randn(V, 2, n_articulators * n_samples, generator=gp)
        self.air_prototypes = torch.randn(V, 2, 2 * n_samples, generator=gp)
        g = torch.Generator().manual_seed(seed)
        self._seeds = torch.randint(0, 2 ** 31 - 1, (num_sentences,), generator=g).tolist()

    def __len__(self):
        return self.num_sentences

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self._seeds[index])
        T = int(torch.randint(self.min_len, self.max_len + 1, (1,), generator=g))
        ids = torch.tensor(self.token_ids)
        frames = []
        while len(frames) < T:
            tok = int(ids[torch.randint(0, len(ids), (1,), generator=g)])
            frames += [tok] * int(torch.randint(2, 7, (1,), generator=g))
        sentence = torch.tensor(frames[:T], dtype=torch.long)
        vt = self.prototypes[sentence] + self.noise * torch.randn(T, *self.prototypes.shape[1:], generator=g)   # (T, 2, A*N)
        air = self.air_prototypes[sentence] + self.noise * torch.randn(T, *self.air_prototypes.shape[1:], generator=g)
        voicing = torch.tensor([self.names[int(t)] in self.voiced for t in sentence], dtype=torch.float)
        ctc_target = torch.unique_consecutive(sentence)
        return {
            "air_column": air.permute(1, 2, 0).contiguous(),
            "air_column_length": T,
            "vocal_tract": vt.permute(1, 2, 0).contiguous(),
            "vocal_tract_length": T,
            "articulatory_target": sentence,
            "articulatory_target_length": T,
            "voicing": voicing,
            "ctc_target": ctc_target,
            "ctc_target_length": len(ctc_target),
        }


class ShapeTreeRecognitionDataset(Dataset):
    """The reference's ``synthetic_shapes.SyntheticPhonemeRecognitionDataset`` (that name is taken here by the seeded data set
    above): the recogniser's data read from synthesised shapes, ``<datadir>/<subject>/<sentence>/`` with target_sequence.txt,
    air_column/<frame>.npy and inference_contours/<frame>_<articulator>.npy -- the tree of ``generate_vocal_tract_shape.py`` with
    ``air_column: true``, or of ``shape_to_air_column.py``.  Same constructor arguments (:39-47); the frame ids come from
    air_column/*.npy (:58-62) and a sequence without frames is skipped with a warning (:69-71).  Items carry the reference's nine
    keys (:146-158): ``air_column`` (2, 2 Nw, T) and ``vocal_tract`` (2, A N, T) over the sorted articulators, float32.  The
    articulators are the reference's ten (:24-35) unless ``articulators`` names others; the point count is read from the files
    (the reference fixes 50, :112)."""
    ARTICULATORS = ("arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate-midline",
                    "thyroid-cartilage", "tongue", "upper-lip", "vocal-folds")

    def __init__(self, database_name, datadir, vocabulary, sequences, voiced_tokens=None, articulators=None, **kwargs):
        from ..settings import DATASET_CONFIG
        self.datadir = datadir
        self.database_config = DATASET_CONFIG[database_name]
        self.articulators = sorted(articulators or self.ARTICULATORS)
        self.vocabulary = vocabulary
        self.voiced_tokens = voiced_tokens or []
        self.data = self._collect_data(sequences)

    def __len__(self):
        return len(self.data)

    def get_frame_ids(self, subject, sentence_name):
        filepaths = glob(os.path.join(self.datadir, subject, sentence_name, "air_column", "*.npy"))
        return sorted(os.path.basename(f).split(".")[0] for f in filepaths)

    def _collect_data(self, sequences):
        data = []
        for subject, sentence_name in sequences:
            frame_ids = self.get_frame_ids(subject, sentence_name)
            if len(frame_ids) == 0:
                logging.warning(f"Skipping {subject}/{sentence_name} - Empty frame sequence")
                continue
            with open(os.path.join(self.datadir, subject, sentence_name, "target_sequence.txt")) as f:
                phonemes = f.read().strip().split()
            data.append({"subject": subject, "sentence_name": sentence_name, "phonemes": phonemes, "frame_ids": frame_ids})
        return data

    def __getitem__(self, index):
        item = self.data[index]
        sequence_dir = os.path.join(self.datadir, item["subject"], item["sentence_name"])
        frame_ids, phonemes = item["frame_ids"], item["phonemes"]
        sentence = torch.tensor([self.vocabulary.get(p, 0) for p in phonemes], dtype=torch.long)   # :93-96: unknown -> 0
        air = np.stack([np.load(os.path.join(sequence_dir, "air_column", f"{f}.npy")) for f in frame_ids])   # (T, walls, 2, Nw)
        shapes = np.stack([np.stack([np.load(os.path.join(sequence_dir, "inference_contours", f"{f}_{a}.npy"))
                                     for a in self.articulators]) for f in frame_ids])                       # (T, A, 2, N)
        air = torch.from_numpy(air).float().permute(2, 1, 3, 0)        # (2, walls, Nw, T), :129-131
        shapes = torch.from_numpy(shapes).float().permute(2, 1, 3, 0)  # (2, A, N, T), :133-135
        voicing = torch.tensor([p in self.voiced_tokens for p in phonemes], dtype=torch.float)
        ctc_target = torch.unique_consecutive(sentence)
        return {
            "air_column": air.reshape(2, -1, len(frame_ids)),
            "air_column_length": len(frame_ids),
            "vocal_tract": shapes.reshape(2, -1, len(frame_ids)),
            "vocal_tract_length": len(frame_ids),
            "articulatory_target": sentence,
            "articulatory_target_length": len(sentence),
            "voicing": voicing,
            "ctc_target": ctc_target,
            "ctc_target_length": len(ctc_target),
        }


class SyntheticAcousticRecognitionDataset(Dataset):
    """num_sentences seeded utterances of synthetic speech over vocabulary, for ``feature: melspec``.  Every token has a prototype
    of three sinusoids (frequencies between 200 Hz and 0.45 sample_rate and amplitudes seeded by prototype_seed, the same for every
    split); a sentence of min_seconds to max_seconds is a random token sequence in which each token is held for 60 to 200 ms,
    and its waveform is the tokens' prototypes over their intervals plus white noise of scale ``noise``.  Items carry the
    waveform (``waveform`` (n,) float32, ``waveform_length``, ``audio_duration`` = n / sample_rate) and the reference's label keys:
    ``phonemes_with_time`` [(token name, start, end) in seconds] with ``phoneme_tokens`` (their ids), ``articulatory_target``
    (the token of every frame at ``framerate``) with ``voicing``, and ``ctc_target = unique_consecutive`` of the token
    sequence.  No spectrogram: the features of a batch are computed on the device by ``acoustic_collate_fn``; with the
    attribute ``melspectrogram`` set, items carry that transform (key ``melspectrogram``) and ``collate_fn(batch, [Feature.MELSPEC])``
    does the same.  With ``orig_sample_rate`` the waveforms are generated at that rate instead (``sample_rate`` of the data set
    and the key ``sample_rate`` of its items then name it; durations and labels stay in seconds, and the prototypes stay below
    0.45 of the lower of the two rates), and ``acoustic_collate_fn`` resamples them to the transform's rate on the device."""

    def __init__(self, num_sentences, vocabulary, sample_rate=16000, min_seconds=0.5, max_seconds=2.0, framerate=50, noise=0.01,
                 seed=0, voiced_tokens=None, num_special=2, prototype_seed=0, orig_sample_rate=None):
        self.vocabulary = vocabulary
        if orig_sample_rate is not None:   # recordings at a foreign rate: generated there, resampled on the device while collating
            if int(orig_sample_rate) != orig_sample_rate or orig_sample_rate < 1:
                raise ValueError(f"SyntheticAcousticRecognitionDataset: orig_sample_rate {orig_sample_rate} must be a positive integer")
            self.orig_sample_rate = int(orig_sample_rate)
            lower_rate, sample_rate = min(sample_rate, self.orig_sample_rate), self.orig_sample_rate
        else:
            self.orig_sample_rate, lower_rate = None, sample_rate
        self.num_sentences, self.sample_rate, self.framerate, self.noise = num_sentences, sample_rate, framerate, noise
        self.min_samples, self.max_samples = int(round(min_seconds * sample_rate)), int(round(max_seconds * sample_rate))
        self.voiced = set(voiced_tokens or [])
        self.names = {i: tok for tok, i in vocabulary.items()}
        self.token_ids = sorted(i for i in vocabulary.values() if i >= num_special)
        V = max(vocabulary.values()) + 1
        gp = torch.Generator().manual_seed(prototype_seed)   # shared by every split
        self.melspectrogram = None   # features.MelSpectrogram that collate_fn launches on this data set's batches (set by the owner)
        # below 0.45 of the lower of the two rates: the prototypes survive the resampler's low-pass
        self.frequencies = 200.0 + (0.45 * lower_rate - 200.0) * torch.rand(V, 3, generator=gp, dtype=torch.float64)
        self.amplitudes = (0.1 + 0.3 * torch.rand(V, 3, generator=gp, dtype=torch.float64))
        g = torch.Generator().manual_seed(seed)
        self._seeds = torch.randint(0, 2 ** 31 - 1, (num_sentences,), generator=g).tolist()

    def __len__(self):
        return self.num_sentences

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self._seeds[index])
        sr = self.sample_rate
        n = int(torch.randint(self.min_samples, self.max_samples + 1, (1,), generator=g))
        ids = torch.tensor(self.token_ids)
        lo, hi = max(1, int(0.06 * sr)), max(2, int(0.2 * sr))
        tokens, bounds, at = [], [0], 0
        while at < n:
            tokens.append(int(ids[torch.randint(0, len(ids), (1,), generator=g)]))
            at = min(n, at + int(torch.randint(lo, hi + 1, (1,), generator=g)))
            bounds.append(at)
        time = torch.arange(n, dtype=torch.float64) / sr
        token_of_sample = torch.repeat_interleave(torch.tensor(tokens), torch.tensor(bounds).diff())
        phase = 2.0 * torch.pi * self.frequencies[token_of_sample] * time[:, None]                       # (n, 3)
        signal = (self.amplitudes[token_of_sample] * torch.sin(phase)).sum(dim=1)
        waveform = (signal + self.noise * torch.randn(n, generator=g, dtype=torch.float64)).float()
        duration = n / sr
        phonemes_with_time = [(self.names[tok], bounds[i] / sr, bounds[i + 1] / sr) for i, tok in enumerate(tokens)]
        T = max(1, int(duration * self.framerate))
        centres = ((torch.arange(T, dtype=torch.float64) + 0.5) / self.framerate * sr).long().clamp(max=n - 1)
        sentence = token_of_sample[centres]
        voicing = torch.tensor([self.names[int(t)] in self.voiced for t in sentence], dtype=torch.float)
        ctc_target = torch.unique_consecutive(torch.tensor(tokens, dtype=torch.long))
        item = {} if self.melspectrogram is None else {"melspectrogram": self.melspectrogram}
        if self.orig_sample_rate is not None:
            item["sample_rate"] = sr
        return {
            **item,
            "waveform": waveform,
            "waveform_length": n,
            "audio_duration": duration,
            "phonemes_with_time": phonemes_with_time,
            "phoneme_tokens": tokens,
            "articulatory_target": sentence,
            "articulatory_target_length": T,
            "voicing": voicing,
            "ctc_target": ctc_target,
            "ctc_target_length": len(ctc_target),
        }


def read_wav(path):
    """(samples (n,) int16, sample_rate) of a 16-bit PCM WAV file, read with the standard library's ``wave``: the first channel of
    a multi-channel file (the reference treats the signal as mono).  Any other sample width raises.  The samples stay int16 --
    what the file holds and half the upload; the resampler and ``acoustic_collate_fn`` read them as value / 32768, which is
    the float32 torchaudio.load returns."""
    with wave.open(str(path), "rb") as f:
        channels, sample_width, rate, frames = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if sample_width != 2:
            raise ValueError(f"read_wav: {path} holds {8 * sample_width}-bit samples; only 16-bit PCM is read")
        data = f.readframes(frames)
    samples = np.frombuffer(data, dtype="<i2").reshape(-1, channels)[:, 0]
    return torch.from_numpy(samples.astype(np.int16)), rate


def write_wav(path, samples, sample_rate):
    """Write (n,) samples as a mono 16-bit PCM WAV file with the standard library's ``wave`` and return ``path``.  int16 samples go
    out as they are, so ``read_wav(write_wav(path, x, rate))`` gives x back; floating-point samples are read as full scale = 1:
    round(value x 32768) to the nearest, halves to even, clipped to [-32768, 32767] (read_wav's value / 32768, inverted).
    ``sample_rate`` must be a whole number of Hz, which is all the format holds."""
    samples = torch.as_tensor(samples).detach().cpu().reshape(-1)
    if samples.dtype != torch.int16:
        if not samples.dtype.is_floating_point:
            raise ValueError(f"write_wav: samples are int16 or floating point, got {samples.dtype}")
        if not bool(torch.isfinite(samples).all()):
            raise ValueError(f"write_wav: {path}: non-finite samples")
        samples = torch.round(samples.double() * 32768.0).clamp(-32768, 32767).to(torch.int16)
    if int(sample_rate) != sample_rate or sample_rate <= 0:
        raise ValueError(f"write_wav: a WAV file holds a whole positive sample rate, got {sample_rate}")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(samples.numpy().astype("<i2").tobytes())
    return path


class RecordedAcousticRecognitionDataset(Dataset):
    """Recordings with phoneme intervals, for ``feature: melspec``: ``manifest`` is a JSON file (or the list itself) of
    ``{"audio_filepath": a 16-bit PCM WAV, relative paths taken from the manifest's folder, "phonemes": [[token, start, end], ...]}``
    with the times in seconds.  Items carry the keys of SyntheticAcousticRecognitionDataset plus ``sample_rate`` (the file's):
    ``waveform`` is int16 (read_wav), ``phoneme_tokens`` are ``vocabulary.get(token, unknown)``, ``articulatory_target`` is the
    token of every frame centre at ``framerate`` (the unknown token where no interval covers it), ``ctc_target`` the
    ``unique_consecutive`` token sequence.  The files are read per item; ``acoustic_collate_fn`` resamples a batch to the
    transform's rate on the device."""

    def __init__(self, manifest, vocabulary, framerate=50, voiced_tokens=None, unknown_token="<unk>"):
        self.vocabulary, self.framerate, self.unknown = vocabulary, framerate, vocabulary[unknown_token]
        self.voiced = set(voiced_tokens or [])
        self.names = {i: tok for tok, i in vocabulary.items()}
        self.melspectrogram = None   # as in SyntheticAcousticRecognitionDataset
        folder = ""
        if isinstance(manifest, (str, os.PathLike)):
            folder = os.path.dirname(os.path.abspath(manifest))
            with open(manifest) as f:
                manifest = json.load(f)
        self.entries = []
        for entry in manifest:
            if "audio_filepath" not in entry or "phonemes" not in entry:
                raise ValueError(f"RecordedAcousticRecognitionDataset: a manifest entry needs audio_filepath and phonemes, got {sorted(entry)}")
            spans = [(str(tok), float(start), float(end)) for tok, start, end in entry["phonemes"]]
            self.entries.append((os.path.join(folder, entry["audio_filepath"]), spans))

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, index):
        path, spans = self.entries[index]
        waveform, sr = read_wav(path)
        n = len(waveform)
        if n == 0:
            raise ValueError(f"RecordedAcousticRecognitionDataset: {path} holds no samples")
        duration = n / sr
        tokens = [self.vocabulary.get(tok, self.unknown) for tok, _, _ in spans]
        T = max(1, int(duration * self.framerate))
        sentence = torch.full((T,), self.unknown, dtype=torch.long)
        centres = (torch.arange(T, dtype=torch.float64) + 0.5) / self.framerate
        for (_, start, end), tok in zip(spans, tokens):
            sentence[(centres >= start) & (centres < end)] = tok
        voicing = torch.tensor([self.names[int(t)] in self.voiced for t in sentence], dtype=torch.float)
        ctc_target = torch.unique_consecutive(torch.tensor(tokens, dtype=torch.long))
        item = {} if self.melspectrogram is None else {"melspectrogram": self.melspectrogram}
        return {
            **item,
            "waveform": waveform,
            "waveform_length": n,
            "sample_rate": sr,
            "audio_duration": duration,
            "phonemes_with_time": spans,
            "phoneme_tokens": tokens,
            "articulatory_target": sentence,
            "articulatory_target_length": T,
            "voicing": voicing,
            "ctc_target": ctc_target,
            "ctc_target_length": len(ctc_target),
        }


def resample_to_model_rate(batch, sample_rate, device):
    """(batch in launch order, waveforms (B, m_max) float32 on the device, lengths (B,) int64 on the host) of items whose
    ``sample_rate`` is not all the model's: the items are ordered by their rate (a stable sort, so a batch of one rate keeps
    its order), the rows of each rate are padded and uploaded together -- int16 as int16 -- and one ``Resample.resample_batch``
    launch per distinct foreign rate writes them into its rows of the one padded buffer; rows already at the model's rate
    are copied there.  Everything runs on the current stream, ahead of the log-mel launch on the same buffer."""
    from .features import resampled_length, resampler
    batch = sorted(batch, key=lambda item: item.get("sample_rate", sample_rate))
    rates = [int(item.get("sample_rate", sample_rate)) for item in batch]
    lengths = torch.tensor([item["waveform_length"] if r == sample_rate else resampled_length(item["waveform_length"], r, sample_rate)
                            for item, r in zip(batch, rates)], dtype=torch.long)
    waves = torch.empty(len(batch), int(lengths.max()), dtype=torch.float32, device=device)
    at = 0
    while at < len(batch):
        end = at + rates[at:].count(rates[at])
        rows = [item["waveform"] for item in batch[at:end]]
        if len({row.dtype for row in rows}) > 1 or rows[0].dtype != torch.int16:
            rows = [row.float() / 32768.0 if row.dtype == torch.int16 else row.float() for row in rows]
        group = pad_sequence(rows, batch_first=True, padding_value=0).to(device)
        if rates[at] == sample_rate:
            waves[at:end, :group.shape[1]] = group.float() / 32768.0 if group.dtype == torch.int16 else group
            waves[at:end, group.shape[1]:] = 0.0
        else:
            resampler(rates[at], sample_rate).resample_batch(group, [item["waveform_length"] for item in batch[at:end]], out=waves[at:end])
        at = end
    return batch, waves, lengths


def acoustic_target(phonemes_with_time, tokens, melspec_length, audio_duration):
    """Reference :213-220: zeros of melspec_length; per (phoneme, start, end) the frames
    [int(start L / duration), int(end L / duration)) take the phoneme's token (tokens[i] for the i-th interval)."""
    target = torch.zeros(melspec_length, dtype=torch.long)
    for (_, start_time, end_time), token in zip(phonemes_with_time, tokens):
        start_spec = int((start_time * melspec_length) / audio_duration)
        end_spec = int((end_time * melspec_length) / audio_duration)
        target[start_spec:end_spec] = token
    return target


def acoustic_collate_fn(batch, melspectrogram, device=None, vocabulary=None, unknown_token="<unk>"):
    """The reference's collate_fn(batch, [Feature.MELSPEC]) for items that carry waveforms: the waveforms are padded and uploaded
    once, ``melspectrogram.log_mel_batch`` (features.MelSpectrogram) computes the (B, 2, n_mels, T) log-mel batch with its -1
    padding on the device, and the acoustic targets follow from the frame counts.  Same keys, dtypes and padding as collate_fn;
    ``melspec`` is on the device.  With ``vocabulary`` the token of an interval is ``vocabulary.get(phoneme, unknown)`` as in the
    reference (:215), for any item with ``phonemes_with_time``; without it the item's own ``phoneme_tokens`` are taken.  Items
    whose ``sample_rate`` is not the transform's are resampled on the device first (``resample_to_model_rate``: the batch is
    ordered by rate, one launch per distinct rate, then the one log-mel launch on the same stream); without such an item the
    calls are the ones made before, and int16 waveforms (``read_wav``) are read as value / 32768.  It
    launches a kernel, so it runs in the main process: the DataLoader gets num_workers=0 (a worker process raises)."""
    if torch.utils.data.get_worker_info() is not None:
        raise ValueError("acoustic_collate_fn computes its features on the device while collating: num_workers must be 0")
    from . import Feature, Target
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("artspeech_amd: acoustic_collate_fn computes the mel spectrogram on an MI355X device; there is no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
    if any(item.get("sample_rate", melspectrogram.sample_rate) != melspectrogram.sample_rate for item in batch):
        # recordings at a foreign rate (reference :124-126): resampled on the device, then the same one log-mel launch
        batch, waves, lengths = resample_to_model_rate(batch, melspectrogram.sample_rate, device)
    else:
        waves = pad_sequence([item["waveform"] for item in batch], batch_first=True, padding_value=0.0)
        lengths = torch.tensor([item["waveform_length"] for item in batch], dtype=torch.long)
        waves = waves.to(device).float() / 32768.0 if waves.dtype == torch.int16 else waves.to(device)   # int16: read_wav's samples
    feats, feat_lengths = melspectrogram.log_mel_batch(waves, lengths, channels=2)
    out = {Feature.MELSPEC.value: feats, f"{Feature.MELSPEC.value}_length": feat_lengths}
    def tokens(item):
        if vocabulary is None:
            return item["phoneme_tokens"]
        return [vocabulary.get(phoneme, vocabulary[unknown_token]) for phoneme, _, _ in item["phonemes_with_time"]]

    targets = [acoustic_target(item["phonemes_with_time"], tokens(item), int(L), item["audio_duration"])
               for item, L in zip(batch, feat_lengths)]
    out[Target.ACOUSTIC.value] = pad_sequence(targets, batch_first=True, padding_value=-1)
    out[f"{Target.ACOUSTIC.value}_length"] = feat_lengths.clone()
    for tgt in (Target.ARTICULATORY, Target.CTC):
        out[tgt.value] = pad_sequence([item[tgt.value] for item in batch], batch_first=True, padding_value=-1)
        out[f"{tgt.value}_length"] = torch.tensor([item[f"{tgt.value}_length"] for item in batch], dtype=torch.long)
    out["voicing"] = pad_sequence([item["voicing"] for item in batch], batch_first=True, padding_value=-1)
    return out


def collate_fn(batch, features_names):
    """Reference :253-302: features (C, D, T) padded with -1 along time into (B, C, D, T); articulatory targets, voicing and CTC
    targets padded with -1; lengths as int64 tensors."""
    from . import Feature, Target
    if Feature.MELSPEC in features_names and "waveform" in batch[0]:   # waveform items: the feature is computed here, on the device
        if list(features_names) != [Feature.MELSPEC] or batch[0].get("melspectrogram") is None:
            raise ValueError("collate_fn: waveform items collate as [Feature.MELSPEC] alone and carry their MelSpectrogram "
                             "(SyntheticAcousticRecognitionDataset.melspectrogram); or call acoustic_collate_fn")
        return acoustic_collate_fn(batch, batch[0]["melspectrogram"])
    out = {}
    for feature_name in features_names:
        feats = pad_sequence([item[feature_name.value].permute(2, 0, 1) for item in batch], batch_first=True, padding_value=-1)
        out[feature_name.value] = feats.permute(0, 2, 3, 1)
        out[f"{feature_name.value}_length"] = torch.tensor([item[f"{feature_name.value}_length"] for item in batch], dtype=torch.long)
    if Feature.MELSPEC in features_names:
        out[Target.ACOUSTIC.value] = pad_sequence([item[Target.ACOUSTIC.value] for item in batch], batch_first=True, padding_value=-1)
        out[f"{Target.ACOUSTIC.value}_length"] = torch.tensor([item[f"{Target.ACOUSTIC.value}_length"] for item in batch],
                                                              dtype=torch.long)
    for tgt in (Target.ARTICULATORY, Target.CTC):
        out[tgt.value] = pad_sequence([item[tgt.value] for item in batch], batch_first=True, padding_value=-1)
        out[f"{tgt.value}_length"] = torch.tensor([item[f"{tgt.value}_length"] for item in batch], dtype=torch.long)
    out["voicing"] = pad_sequence([item["voicing"] for item in batch], batch_first=True, padding_value=-1)
    return out
