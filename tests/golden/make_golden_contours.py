"""Fixture of the contour preparation, produced by the reference's own TailClipper (phoneme_to_articulation/tail_clipper.py),
InputLoaderMixin.prepare_articulator_array (phoneme_to_articulation/__init__.py) and the reduction of its statistics script
(scripts/calculate_normalization_statistics.py:73-75).  Run on the CPU from the repository root with the reference checkout at
make_golden.REF:

    python tests/golden/make_golden_contours.py

Writes tests/golden/contours.npz.  Uses make_golden.py's name-only shims plus the three articulator names the clipper imports
from ``vt_tools`` and empty ``vt_shape_gen.helpers`` / ``vt_tools.bs_regularization``; ``cached_load_articulator_array`` is
replaced by a lookup into the fixture's own arrays, keyed by the file name the reference asks for.

96 frames x 5 articulators (lower-lip, pharynx, tongue, upper-incisor, upper-lip), N = 50, database artspeech2:
  * frames 0..63 are seeded draws: contours U(0, 1); the heights of the lower incisor and the epiglottis are spread over the whole
    range so that the kept counts vary; the upper lip's and the upper incisor's y are at PIXEL scale (0..20), where the upper lip's
    margins (10 / PIXEL_SPACING and 5 / PIXEL_SPACING, not divided by RES in the reference) cut;
  * frames 64..95 are constructed: for each clipped kind a frame per kept count 50, 49, 26, 25 and 1 (the lower lip always keeps
    the 25 points of a half, so its frames stop at 25) and one frame with points whose y equals the threshold bit for bit (the
    comparison is strict: they are dropped); the remaining frames repeat the seeded recipe.
Stored: raw contours and the two references that are not articulators; the three methods' outputs; prepare_articulator_array's
contours without and with Normalize and its reference arrays; the statistics of the prepared contours from the reference's torch
expressions; the kept counts of the restatement tests/contours_ref.py, which is asserted equal to every recorded array bit for
bit here.  Asserted too: the reference raised on no frame, and each kind's counts include 50, a value <= 25 and (tongue, upper
lip) 1.  A separate pair of frames records that the reference raises on an emptied tongue and on an emptied upper lip."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import contours_ref as Y  # noqa: E402
from make_golden import REF, _load, _shim, install_shims, save  # noqa: E402

ARTS = ["lower-lip", "pharynx", "tongue", "upper-incisor", "upper-lip"]
N = 50
SEED = 2110
DATABASE = "artspeech2"
N_SEEDED, N_FRAMES = 64, 96


def load_reference():
    install_shims()
    sys.path.insert(0, REF)
    vt = sys.modules["vt_tools"]
    vt.LOWER_INCISOR, vt.EPIGLOTTIS = "lower-incisor", "epiglottis"
    _shim("vt_tools.bs_regularization", regularize_Bsplines=None)
    _shim("vt_shape_gen")
    _shim("vt_shape_gen.helpers", load_articulator_array=None)
    settings = _load("settings", "settings.py")
    _load("tract_variables", "tract_variables.py")
    pkg = types.ModuleType("phoneme_to_articulation")
    pkg.__path__ = [os.path.join(REF, "phoneme_to_articulation")]
    sys.modules["phoneme_to_articulation"] = pkg
    clipper = _load("phoneme_to_articulation.tail_clipper", "phoneme_to_articulation/tail_clipper.py")
    transforms = _load("phoneme_to_articulation.transforms", "phoneme_to_articulation/transforms.py")
    init = _load("ref_p2a_init_for_contours", "phoneme_to_articulation/__init__.py")
    return settings, clipper, transforms, init


def seeded_frame(rng):
    """raw (5, 50, 2), lower incisor (50, 2), epiglottis (50, 2)"""
    raw = rng.rand(len(ARTS), N, 2)
    raw[ARTS.index("upper-incisor"), :, 1] = 3 + 17 * rng.rand() + rng.rand(N) - 1      # pixel scale, last point anywhere in 2..20
    raw[ARTS.index("upper-lip"), :, 1] = 20 * rng.rand(N)
    li, ep = rng.rand(N, 2), rng.rand(N, 2)
    li[:, 1] = 0.15 + 0.85 * rng.rand() - 0.1 * rng.rand(N)
    ep[:, 1] = 0.1 + 0.8 * rng.rand() + 0.1 * rng.rand(N)
    return raw.astype(np.float32), li.astype(np.float32), ep.astype(np.float32)


def constructed_frame(rng, kind, count, thr):
    """a seeded frame whose articulator of `kind` keeps exactly `count` points (count None: the tie frame)"""
    raw, li, ep = seeded_frame(rng)
    first = np.arange(N) < 25
    if kind == "tongue":
        li[:, 1] = np.float32(0.5) - (0.2 * rng.rand(N)).astype(np.float32)
        li[7, 1] = 0.5
        ep[:, 1] = np.float32(0.4) + (0.2 * rng.rand(N)).astype(np.float32)
        ep[11, 1] = 0.4
        y = raw[ARTS.index("tongue"), :, 1]
        if count is None:
            y[:] = np.where(rng.rand(N) < 0.5, 0.1, 0.9)
            y[3], y[30] = np.float32(0.4) + thr[0], 0.5          # on the thresholds of their halves: dropped
            y[4], y[31] = np.nextafter(y[3], np.float32(0)), np.nextafter(np.float32(0.5), np.float32(0))   # just inside: kept
        else:
            y[:] = 0.9
            y[rng.permutation(N)[:count]] = 0.1
    elif kind == "upper-lip":
        ui = raw[ARTS.index("upper-incisor")]
        ui[-1, 1] = 10.0
        y = raw[ARTS.index("upper-lip"), :, 1]
        if count is None:
            y[:] = np.where(rng.rand(N) < 0.5, 15.0, 1.0)
            y[3], y[30] = np.float32(10.0) - thr[3], np.float32(10.0) - thr[2]
            y[4], y[31] = np.nextafter(y[3], np.float32(100)), np.nextafter(y[30], np.float32(100))
        else:
            y[:] = 1.0
            y[rng.permutation(N)[:count]] = 15.0
    else:
        li[:, 1] = np.float32(0.5) - (0.2 * rng.rand(N)).astype(np.float32)
        li[7, 1] = 0.5
        y = raw[ARTS.index("lower-lip"), :, 1]
        y[:] = 0.1
        if count is None:
            y[:] = np.where(rng.rand(N) < 0.5, 0.1, 0.9)
            y[first] = np.where(rng.rand(25) < 0.5, 0.1, 0.9)
            y[30], y[3] = np.float32(0.5) + thr[1], 0.5           # stage 1 drops 30; 3 survives the resampling and stage 2 drops it
            y[31] = np.nextafter(y[30], np.float32(0))
        else:
            y[rng.permutation(25)[:N - count]] = 0.51             # between the incisor's top and its margin: only stage 2 drops them
    return raw, li, ep


def main():
    settings, clipper_mod, transforms, init = load_reference()
    cfg = settings.DATASET_CONFIG[DATABASE]
    thr = Y.thresholds(cfg)
    rng = np.random.RandomState(SEED)
    frames = [seeded_frame(rng) for _ in range(N_SEEDED)]
    tie_frame = {}
    for kind in ("tongue", "lower-lip", "upper-lip"):
        for count in (50, 49, 26, 25, 1, None):
            if kind == "lower-lip" and count == 1:
                continue
            if count is None:
                tie_frame[kind] = len(frames)
            frames.append(constructed_frame(rng, kind, count, thr))
    frames += [seeded_frame(rng) for _ in range(N_FRAMES - len(frames))]
    raw = np.stack([f[0] for f in frames])
    li, ep = np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])
    refs = np.stack([li, raw[:, ARTS.index("upper-incisor")], ep], axis=1)
    assert raw.shape == (N_FRAMES, 5, N, 2) and refs.shape == (N_FRAMES, 3, N, 2)

    # ---- the three methods
    clipper = clipper_mod.TailClipper(cfg)
    assert clipper_mod.TailClipper.TAIL_CLIP_REFERENCES == Y.REFERENCES
    clipped = raw.copy()
    for f in range(N_FRAMES):
        named = {name.replace("-", "_"): torch.from_numpy(refs[f, i]) for i, name in enumerate(Y.REFERENCES)}
        for kind in Y.KINDS:
            method = getattr(clipper, f"clip_{kind.replace('-', '_')}_tails")
            clipped[f, ARTS.index(kind)] = method(torch.from_numpy(raw[f, ARTS.index(kind)]), **named).numpy()   # raises on no frame

    # ---- prepare_articulator_array over a lookup instead of files
    table = {}
    for f in range(N_FRAMES):
        for a, name in enumerate(ARTS):
            table[f"{f:04d}_{name}.npy"] = raw[f, a]
        table[f"{f:04d}_lower-incisor.npy"], table[f"{f:04d}_epiglottis.npy"] = li[f], ep[f]
    asked = []

    def lookup(filepath, norm_value):
        assert norm_value == cfg.RES
        asked.append(filepath)
        return torch.from_numpy(table[os.path.basename(filepath)].copy())

    init.cached_load_articulator_array = lookup
    norm_mean = (0.2 + 0.6 * rng.rand(len(ARTS), 2, N)).astype(np.float32)
    norm_std = (0.5 + rng.rand(len(ARTS), 2, N)).astype(np.float32)
    prepared = np.empty((N_FRAMES, len(ARTS), 2, N), np.float32)
    prepared_norm, prepared_unclipped = np.empty_like(prepared), np.empty_like(prepared)
    references = np.empty((N_FRAMES, 1, 2, N), np.float32)
    for f in range(N_FRAMES):
        for a, name in enumerate(ARTS):
            args = ("data", "S0", "seq", f"{f:04d}", name, cfg)
            arr, ref = init.InputLoaderMixin.prepare_articulator_array(*args)
            prepared[f, a], references[f, 0] = arr.numpy(), ref.numpy()
            normalize = transforms.Normalize(torch.from_numpy(norm_mean[a]), torch.from_numpy(norm_std[a]))
            arr_n, ref_n = init.InputLoaderMixin.prepare_articulator_array(*args, normalize_fn=normalize)
            prepared_norm[f, a] = arr_n.numpy()
            assert ref_n.numpy().tobytes() == ref.numpy().tobytes()
            arr_u, _ = init.InputLoaderMixin.prepare_articulator_array(*args, clip_tails=False)
            prepared_unclipped[f, a] = arr_u.numpy()
    assert asked[0] == os.path.join("data", "S0", "seq", "inference_contours", "0000_lower-lip.npy")

    # ---- the statistics script's reduction of the prepared contours
    stacked = torch.from_numpy(prepared)
    stats_mean = np.stack([stacked[:, a].mean(axis=0).numpy() for a in range(len(ARTS))])
    stats_std = np.stack([stacked[:, a].std(axis=0).numpy() for a in range(len(ARTS))])

    # ---- the restatement equals all of it, bit for bit; its counts cover what the issue of this fixture asks for
    kinds = Y.kinds_of(ARTS)
    y_clipped, counts = Y.clip_batched(raw, refs, kinds, thr)
    assert y_clipped.tobytes() == clipped.tobytes()
    for got, want in ((Y.prepare(raw, refs, kinds, thr), (prepared, references)),
                      (Y.prepare(raw, refs, kinds, thr, norm_mean, norm_std), (prepared_norm, references)),
                      (Y.prepare(raw, refs, [0] * len(ARTS), thr), (prepared_unclipped, references))):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    for kind, lowest in (("tongue", 1), ("lower-lip", 25), ("upper-lip", 1)):
        seen = set(counts[:, ARTS.index(kind)].tolist())
        assert {50, 49, 26, 25, lowest} <= seen and 0 not in seen, (kind, sorted(seen))
        assert len(set(counts[:N_SEEDED, ARTS.index(kind)].tolist())) >= 8, (kind, "the seeded frames' counts do not vary")
    for kind, at in (("tongue", (3, 30)), ("upper-lip", (3, 30)), ("lower-lip", (30,))):   # the tie frames: the points on a threshold are gone
        f = tie_frame[kind]
        pts = raw[f, ARTS.index(kind)]
        for i in at:
            assert not (clipped[f, ARTS.index(kind)] == pts[i]).all(axis=1).any(), (kind, f, i)
        assert (clipped[f, ARTS.index(kind)] == pts[at[-1] + 1]).all(axis=1).any(), (kind, f, "the point just inside is kept")

    # ---- the reference raises on an emptied tongue and an emptied upper lip
    e_raw, e_li, e_ep = seeded_frame(rng)
    e_li[:, 1], e_ep[:, 1] = 0.2, 0.1
    e_raw[ARTS.index("tongue"), :, 1] = 0.9
    e_raw[ARTS.index("upper-incisor"), -1, 1] = 19.0
    e_raw[ARTS.index("upper-lip"), :, 1] = 2.0
    e_refs = np.stack([e_li, e_raw[ARTS.index("upper-incisor")], e_ep])
    raised = []
    for kind in ("tongue", "upper-lip"):
        named = {name.replace("-", "_"): torch.from_numpy(e_refs[i]) for i, name in enumerate(Y.REFERENCES)}
        try:
            getattr(clipper, f"clip_{kind.replace('-', '_')}_tails")(torch.from_numpy(e_raw[ARTS.index(kind)]), **named)
            raised.append("")
        except Exception as exc:  # noqa: BLE001
            raised.append(type(exc).__name__)
    assert all(raised), raised
    e_counts = Y.clip_batched(e_raw[None], e_refs[None], kinds, thr)[1][0].tolist()
    assert e_counts[1::2] == [50, 50] and e_counts[2::2] == [0, 0] and e_counts[0] >= 25, e_counts

    save("contours", articulators=np.array(ARTS), database_name=np.array(DATABASE), raw=raw, lower_incisor=li, epiglottis=ep,
         clipped=clipped[:, [ARTS.index(k) for k in Y.KINDS]], clipped_articulators=np.array(list(Y.KINDS)),
         prepared=prepared, prepared_norm=prepared_norm, references=references, norm_mean=norm_mean, norm_std=norm_std,
         unclipped_tongue=prepared_unclipped[:, ARTS.index("tongue")], stats_mean=stats_mean, stats_std=stats_std, counts=counts,
         empty_raw=e_raw, empty_refs=e_refs, empty_raised=np.array(raised))
    assert os.path.getsize(os.path.join(HERE, "contours.npz")) <= 1000000


if __name__ == "__main__":
    main()
