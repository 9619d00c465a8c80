####################################################################################################
#
# Speech from synthesised vocal-tract shapes on the MI355X engine:
#   python vocal_tract_speech.py --config cfg.yaml
# The YAML keys are the keyword arguments of main().  The script works on the tree that
# generate_vocal_tract_shape.py writes with `air_column: true`: for every
# <datadir>/<subject>/<sequence>/ it reads the frames' air_column/%04d.npy and target_sequence.txt, and runs
#   tube_from_air_columns   per sequence: the ragged tube sections (vocal_tract_formants.py)
#   synthesize_speech       ONCE for all sequences: equal_sections -> frication_control -> one
#                           as_vt_glottal_source launch -> one as_vt_waveguide launch
#   Resample                optionally, to `model_sample_rate`, one launch for the batch
# Voicing comes from the config's `voiced_tokens`: a frame whose phoneme is one of them is voiced.
# S = round(sample_rate / FRAMERATE) samples per frame; the true rate S x FRAMERATE is what is written
# and reported (44100 Hz at 50 frames per second: S = 882, exactly 44100).
# Per sequence: speech.wav (16-bit PCM; the whole batch is scaled by one factor, `output_gain`, or so
# that its peak is 0.9 of full scale) and speech.json (parameters, K, tract lengths in cm, status, peak,
# clipped samples).  At the tree's root: manifest.json in RecordedAcousticRecognitionDataset's format,
# the phoneme intervals being the runs of target_sequence.txt at the data set's FRAMERATE.
# The reference has no acoustic stage; the definition is this project's own (include/artspeech_hip.h).
#
####################################################################################################
import json
import logging
import os
from glob import glob
from itertools import groupby

import numpy as np
import torch

from artspeech_amd.area_function import build_semipolar_grid
from artspeech_amd.phoneme_recognition.datasets import write_wav
from artspeech_amd.phoneme_recognition.features import resampler
from artspeech_amd.phoneme_to_articulation.synthesis import read_phonemes
from artspeech_amd.settings import DATASET_CONFIG
from artspeech_amd.training import run_cli
from artspeech_amd.vocal_tract_synthesis import (FALL, MIN_AREA, MU, R_GLOTTIS, R_LIPS, RISE, SOUND_SPEED, STATUS_CLOSED,
                                                 STATUS_NON_FINITE, synthesize_speech)
from vocal_tract_formants import tube_from_air_columns


def phoneme_intervals(phonemes, framerate):
    """[[token, start, end], ...] in seconds: the runs of the per-frame phonemes, frame t covering [t, t + 1) / framerate."""
    out, at = [], 0
    for token, run in groupby(phonemes):
        n = len(list(run))
        out.append([token, at / framerate, (at + n) / framerate])
        at += n
    return out


def main(datadir, database_name, grid, voiced_tokens, alpha=np.pi, beta=2.0, sample_rate=44100, model_sample_rate=None,
         f0_start=120.0, f0_end=90.0, amplitude=1.0, aspiration=0.05, frication=0.1, critical_area=0.2, rise=RISE, fall=FALL,
         r_g=R_GLOTTIS, r_l=R_LIPS, mu=MU, min_area=MIN_AREA, radiation="difference", c=SOUND_SPEED, output_gain=None, seed=0):
    config = DATASET_CONFIG[database_name]
    to_cm = config.RES * config.PIXEL_SPACING / 10.0   # contour unit -> mm (settings.py) -> cm
    framerate = config.FRAMERATE
    S = max(1, int(round(sample_rate / framerate)))
    fs = S * framerate
    semipolar_grid = build_semipolar_grid(**grid)
    device = torch.device("cuda", torch.cuda.current_device())
    voiced = set(voiced_tokens)
    sequences = []
    for sequence_dir in sorted(filter(os.path.isdir, glob(os.path.join(datadir, "*", "*")))):
        filepaths = sorted(glob(os.path.join(sequence_dir, "air_column", "*.npy")))
        if not filepaths:
            continue
        phonemes = read_phonemes(os.path.join(sequence_dir, "target_sequence.txt"))
        if len(phonemes) != len(filepaths):
            raise ValueError(f"{sequence_dir}: {len(filepaths)} air columns for {len(phonemes)} phonemes in target_sequence.txt")
        air = torch.from_numpy(np.stack([np.load(f) for f in filepaths]).astype(np.float64)).to(device)
        areas, lengths, counts = tube_from_air_columns(air, semipolar_grid, to_cm, alpha, beta)
        sequences.append((sequence_dir, phonemes, areas, lengths, counts))
    if not sequences:
        return {"sequences": [], "sample_rate": fs, "samples_per_frame": S}
    B, T, Kr = len(sequences), max(len(s[1]) for s in sequences), max(s[2].shape[1] for s in sequences)
    areas = torch.zeros((B, T, Kr), dtype=torch.float64, device=device)
    lengths = torch.zeros_like(areas)
    counts = torch.zeros((B, T), dtype=torch.int32, device=device)
    voicing = torch.zeros((B, T), dtype=torch.float64, device=device)
    frames = torch.tensor([len(s[1]) for s in sequences], dtype=torch.int32, device=device)
    for b, (_, phonemes, a, l, n) in enumerate(sequences):
        areas[b, :a.shape[0], :a.shape[1]], lengths[b, :a.shape[0], :a.shape[1]], counts[b, :a.shape[0]] = a, l, n
        voicing[b, :len(phonemes)] = torch.tensor([float(p in voiced) for p in phonemes], dtype=torch.float64)
    wave = synthesize_speech(areas, lengths, counts, voicing, frames, S, framerate, c=c, f0_start=f0_start, f0_end=f0_end,
                             amplitude=amplitude, aspiration=aspiration, frication=frication, critical_area=critical_area, seed=seed,
                             rise=rise, fall=fall, r_g=r_g, r_l=r_l, mu=mu, min_area=min_area, radiation=radiation)
    samples, n_samples, rate = wave.samples, wave.n_samples.cpu(), fs
    if model_sample_rate is not None and int(model_sample_rate) != fs:
        samples, n_samples = resampler(fs, int(model_sample_rate)).resample_batch(samples, n_samples)
        rate = int(model_sample_rate)
    finite = torch.nan_to_num(samples, nan=0.0, posinf=0.0, neginf=0.0)
    peaks = finite.abs().amax(1)
    scale = float(output_gain) if output_gain is not None else 0.9 / max(float(peaks.max()), 1e-30)
    scaled = finite * scale
    clipped = ((scaled >= 32767.0 / 32768.0) | (scaled < -1.0)).sum(1).cpu().tolist()
    scaled, peaks, status = scaled.cpu(), peaks.cpu().tolist(), wave.status.cpu().tolist()
    parameters = dict(database_name=database_name, grid=grid, alpha=float(alpha), beta=float(beta), to_cm=to_cm, framerate=framerate,
                      samples_per_frame=S, synthesis_sample_rate=fs, sample_rate=rate, voiced_tokens=sorted(voiced), f0_start=f0_start,
                      f0_end=f0_end, amplitude=amplitude, aspiration=aspiration, frication=frication, critical_area=critical_area,
                      rise=rise, fall=fall, r_g=r_g, r_l=r_l, mu=mu, min_area=min_area, radiation=radiation, c=c, output_scale=scale,
                      seed=seed)
    report, manifest = [], []
    tract, sections, replaced = wave.tract_length.cpu().tolist(), wave.sections.cpu().tolist(), wave.replaced.cpu().tolist()
    for b, (sequence_dir, phonemes, *_) in enumerate(sequences):
        n = int(n_samples[b])
        write_wav(os.path.join(sequence_dir, "speech.wav"), scaled[b, :n], rate)
        entry = {"sequence": os.path.relpath(sequence_dir, datadir), "frames": len(phonemes), "samples": n, "sections": sections[b],
                 "tract_length_cm": dict(zip(("min", "mean", "max"), tract[b])), "replaced_frames": replaced[b],
                 "status": {"closed": bool(status[b] & STATUS_CLOSED), "non_finite": bool(status[b] & STATUS_NON_FINITE)},
                 "peak": peaks[b], "clipped": clipped[b]}
        with open(os.path.join(sequence_dir, "speech.json"), "w") as f:
            json.dump({"parameters": parameters, **entry}, f, indent=1)
        manifest.append({"audio_filepath": os.path.join(entry["sequence"], "speech.wav"), "phonemes": phoneme_intervals(phonemes, framerate)})
        report.append(entry)
        logging.info(f"{entry['sequence']}: {n} samples at {rate} Hz, K = {sections[b]}, status {entry['status']}")
    with open(os.path.join(datadir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    return {"sequences": report, "sample_rate": rate, "synthesis_sample_rate": fs, "samples_per_frame": S,
            "manifest": os.path.join(datadir, "manifest.json")}


if __name__ == "__main__":
    print(json.dumps(run_cli(main, "vocal_tract_speech", checkpoint=False), indent=2))
