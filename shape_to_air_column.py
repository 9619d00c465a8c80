####################################################################################################
#
# Air columns from saved contours on the MI355X engine (reference scripts/shape_to_air_column.py):
#   python shape_to_air_column.py --config cfg.yaml
# The YAML keys are the keyword arguments of main(): datadir, database_name, overwrite (true), n_wall
# (100) and, optionally, internal / external: the chains of articulators that make the two walls
# (default: INTERNAL_WALL and EXTERNAL_WALL of artspeech_amd/phoneme_to_articulation/vocal_tract_tube.py,
# this project's own definition of the reference's generate_vocal_tract_tube).  For every
# <datadir>/<subject>/<sequence>/inference_contours/ the frames that have a <frame>_<articulator>.npy for
# every articulator of the two chains are read, their walls are built in ONE launch per sequence, and
# air_column/<frame>.npy is written in the (2 walls, 2, n_wall) float64 layout.  Like the reference
# (:77-80) the coordinates are divided by the data set's RES.
# Quirk: the reference's overwrite check (:63) tests isfile(isfile(...)), which is never true, so it
# always overwrites; here overwrite: false does what it says and leaves existing files alone.
#
####################################################################################################
import json
import logging
import os
from glob import glob

import numpy as np
import torch

from artspeech_amd.phoneme_to_articulation.vocal_tract_tube import EXTERNAL_WALL, INTERNAL_WALL, _as_contour, vocal_tract_tube
from artspeech_amd.settings import DATASET_CONFIG
from artspeech_amd.training import run_cli


def frame_table(contours_dir):
    """{frame id: {articulator: filepath}} of the <frame>_<articulator>.npy files of one inference_contours/ (:54-56, :66-72)."""
    table = {}
    for filepath in glob(os.path.join(contours_dir, "*_*.npy")):
        frame_id, articulator = os.path.basename(filepath)[:-len(".npy")].split("_", 1)
        table.setdefault(frame_id, {})[articulator] = filepath
    return table


def select_frames(table, needed, save_dir, overwrite=True):
    """The sorted frame ids that have every articulator of ``needed`` (:74-75) and, with ``overwrite`` false, no air column yet."""
    frames = []
    for frame_id in sorted(table):
        if not all(articulator in table[frame_id] for articulator in needed):
            continue
        if not overwrite and os.path.isfile(os.path.join(save_dir, f"{frame_id}.npy")):
            continue
        frames.append(frame_id)
    return frames


def build_walls(contours, articulators, internal, external, n_wall):
    """contours (F, A, 2, N) float32 on the host -> air columns (F, 2, 2, n_wall) float64 on the host: one launch."""
    device = torch.device("cuda", torch.cuda.current_device())
    return vocal_tract_tube(torch.from_numpy(contours).to(device), articulators, internal, external, n_out=n_wall).cpu().numpy()


def main(datadir, database_name, overwrite=True, n_wall=100, internal=None, external=None, seed=0):
    res = np.float32(DATASET_CONFIG[database_name].RES)
    internal = tuple(internal) if internal is not None else INTERNAL_WALL
    external = tuple(external) if external is not None else EXTERNAL_WALL
    needed = sorted(set(internal) | set(external))
    report = []
    for sequence_dir in sorted(filter(os.path.isdir, glob(os.path.join(datadir, "*", "*")))):
        contours_dir = os.path.join(sequence_dir, "inference_contours")
        if not os.path.isdir(contours_dir):
            continue
        save_dir = os.path.join(sequence_dir, "air_column")
        os.makedirs(save_dir, exist_ok=True)
        table = frame_table(contours_dir)
        frames = select_frames(table, needed, save_dir, overwrite)
        entry = {"sequence": os.path.relpath(sequence_dir, datadir), "frames": len(table), "written": len(frames)}
        report.append(entry)
        if not frames:
            continue
        contours = [[_as_contour(table[frame_id][articulator]) for articulator in needed] for frame_id in frames]
        if len({c.shape for frame in contours for c in frame}) != 1:
            raise ValueError(f"{contours_dir}: the contours of one sequence have one point count")
        air_columns = build_walls(np.asarray(contours, dtype=np.float32) / res, needed, internal, external, n_wall)
        for frame_id, air_column in zip(frames, air_columns):
            np.save(os.path.join(save_dir, f"{frame_id}.npy"), air_column)
        logging.info(f"{entry['sequence']}: {len(frames)} of {len(table)} frames")
    return {"sequences": report, "written": sum(e["written"] for e in report)}


if __name__ == "__main__":
    print(json.dumps(run_cli(main, "shape_to_air_column", checkpoint=False), indent=2))
