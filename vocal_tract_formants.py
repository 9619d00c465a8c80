####################################################################################################
#
# Formants of synthesised vocal-tract shapes on the MI355X engine:
#   python vocal_tract_formants.py --config cfg.yaml
# The YAML keys are the keyword arguments of main().  The script works on the tree that
# generate_vocal_tract_shape.py writes with `air_column: true`: for every
# <datadir>/<subject>/<sequence>/air_column/ it reads the frames' %04d.npy air columns and runs, on the
# device and once per sequence,
#   intersect_semipolar_grid_batched  the walls' sections on Maeda's semipolar grid (`grid`: the keyword
#                                     arguments of build_semipolar_grid; the grid is built once)
#   area_function_batched             the area function along the mid line (`alpha`, `beta`)
#   tube_sections                     areas in cm^2 and lengths in cm; one contour unit is
#                                     RES * PIXEL_SPACING millimetres of the data set
#   formants                          as_vt_acoustics: the transfer function's denominator on the grid
#                                     f0 + j df and its first n_formants minima, refined
# and writes formants.npy (frames, n_formants) in Hz, formant_levels.npy in dB, formants.csv and
# formants.json (the parameters and how many frames carry each status) into the sequence's directory.
# A grid line that crosses neither wall gives no section, so frames differ in their number of sections:
# the sections are packed to the front and the kernel reads each frame's own count.
# The reference has no acoustic stage; the definition is this project's own (include/artspeech_hip.h).
#
####################################################################################################
import csv
import json
import logging
import os
from glob import glob

import numpy as np
import torch

from artspeech_amd.area_function import area_function_batched, build_semipolar_grid, intersect_semipolar_grid_batched
from artspeech_amd.settings import DATASET_CONFIG
from artspeech_amd.training import run_cli
from artspeech_amd.vocal_tract_acoustics import (AIR_DENSITY, MIN_AREA, SOUND_SPEED, STATUS_CLOSED, STATUS_NON_FINITE, formants,
                                                 tube_sections)


def tube_from_air_columns(air, grid, to_cm, alpha=np.pi, beta=2.0):
    """air (frames, 2, 2, Nw) float64 on the GPU, grid (n_lines, grid_res, 2) -> (areas, lengths) (frames, n_lines - 1) in cm^2
    and cm and counts (frames,) int32: the sections of the grid lines that cross a wall, in grid order and packed to the front;
    frame n has counts[n] tube sections (one less than its lines; -1 for a frame that no line crosses).  Behind a frame's last
    line its last section point repeats, so the unused sections have length zero and are never read."""
    flags, p_int, p_ext = intersect_semipolar_grid_batched(air, grid)
    keep = (flags & 3) != 0
    lines = keep.sum(1)
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)
    position = torch.minimum(torch.arange(keep.shape[1], device=air.device)[None, :], (lines - 1).clamp(min=0)[:, None])
    index = order.gather(1, position)[..., None].expand(-1, -1, 2)
    sections = torch.stack([p_int.gather(1, index).transpose(1, 2), p_ext.gather(1, index).transpose(1, 2)], dim=1)
    dists, fx = area_function_batched(sections, alpha, beta)
    areas, lengths = tube_sections(dists, fx, to_cm)
    return areas, lengths, (lines - 1).to(torch.int32)


def main(datadir, database_name, grid, alpha=np.pi, beta=2.0, f0=10.0, df=10.0, n_freq=500, radiation="piston", n_formants=5,
         rounds=3, c=SOUND_SPEED, rho=AIR_DENSITY, min_area=MIN_AREA, seed=0):
    config = DATASET_CONFIG[database_name]
    to_cm = config.RES * config.PIXEL_SPACING / 10.0   # contour unit -> mm (settings.py) -> cm
    semipolar_grid = build_semipolar_grid(**grid)
    device = torch.device("cuda", torch.cuda.current_device())
    parameters = dict(database_name=database_name, grid=grid, alpha=float(alpha), beta=float(beta), to_cm=to_cm, f0=f0, df=df,
                      n_freq=n_freq, radiation=radiation, n_formants=n_formants, rounds=rounds, c=c, rho=rho, min_area=min_area)
    report = []
    for sequence_dir in sorted(filter(os.path.isdir, glob(os.path.join(datadir, "*", "*")))):
        filepaths = sorted(glob(os.path.join(sequence_dir, "air_column", "*.npy")))
        if not filepaths:
            continue
        air = torch.from_numpy(np.stack([np.load(f) for f in filepaths]).astype(np.float64)).to(device)
        areas, lengths, counts = tube_from_air_columns(air, semipolar_grid, to_cm, alpha, beta)
        result = formants(areas, lengths, counts, f0=f0, df=df, n_freq=n_freq, radiation=radiation, c=c, rho=rho, min_area=min_area,
                          n_formants=n_formants, rounds=rounds)
        freq, level, found, status = (t.cpu().numpy() for t in result)
        np.save(os.path.join(sequence_dir, "formants.npy"), freq)
        np.save(os.path.join(sequence_dir, "formant_levels.npy"), level)
        with open(os.path.join(sequence_dir, "formants.csv"), "w", newline="") as f:
            writer = csv.writer(f)
            writer.writerow(["frame", "sections", "status", "found"] + [f"F{k + 1}" for k in range(n_formants)])
            for filepath, n, s, k, row in zip(filepaths, counts.cpu().tolist(), status, found, freq):
                writer.writerow([os.path.basename(filepath)[:-len(".npy")], n, s, k] + [f"{v:.6f}" for v in row])
        entry = {"sequence": os.path.relpath(sequence_dir, datadir), "frames": len(filepaths),
                 "status": {"ok": int((status == 0).sum()), "closed": int(((status & STATUS_CLOSED) != 0).sum()),
                            "non_finite": int(((status & STATUS_NON_FINITE) != 0).sum())},
                 "found": {str(k): int((found == k).sum()) for k in range(n_formants + 1)}}
        with open(os.path.join(sequence_dir, "formants.json"), "w") as f:
            json.dump({"parameters": parameters, **entry}, f, indent=1)
        report.append(entry)
        logging.info(f"{entry['sequence']}: {entry['frames']} frames, status {entry['status']}")
    return {"sequences": report, "frames": sum(e["frames"] for e in report)}


if __name__ == "__main__":
    print(json.dumps(run_cli(main, "vocal_tract_formants", checkpoint=False), indent=2))
