"""Tail clipping of the tongue and the lips (reference: phoneme_to_articulation/tail_clipper.py:7-128) on the MI355X.

``TailClipper`` keeps the reference's names and signatures: three ``clip_*_tails(contour, **references)`` methods that take one
(50, 2) tensor on any device and return the clipped, resampled (50, 2) contour on the same device; like ``area_function`` they
compute on the GPU for host inputs.  ``clip_tails_batched`` is the form the engine uses: all frames and articulators of a corpus
in one launch of ``as_prepare_contours`` (csrc/contours.hip), one wave per (frame, articulator).

The reference's quirks are kept: halves are ``[:25]`` and ``[25:]`` of the current point list, comparisons are strict, the
resampling is ``F.interpolate(size=50)`` in nearest mode, and the upper lip's margins are ``10 / PIXEL_SPACING`` and
``5 / PIXEL_SPACING`` WITHOUT the division by ``RES`` that the tongue's and the lower lip's carry -- on RES-normalised contours
(coordinates in [0, 1], margins of 6.2 and 3.1) the upper lip therefore keeps every point.  Inputs are finite: what ``argmax`` /
``argmin`` answer for NaN is not reproduced."""
import torch

from .. import _lib

LOWER_INCISOR, UPPER_INCISOR, EPIGLOTTIS = "lower-incisor", "upper-incisor", "epiglottis"
CLIP_POINTS = 50
CLIP_KINDS = {"tongue": 1, "lower-lip": 2, "upper-lip": 3}   # the kinds of as_prepare_contours; every other articulator: 0


def clip_thresholds(dataset_config):
    """The four margins of the reference's expressions as Python floats (double), in the order of as_prepare_contours; the
    binding rounds each once to float32, as torch does with a Python scalar next to a float32 tensor."""
    spacing, res = dataset_config.PIXEL_SPACING, dataset_config.RES
    return (10 / spacing / res, 5 / spacing / res, 10 / spacing, 5 / spacing)


def clip_kinds(articulators, clip_tails=True):
    """[kind per articulator]: the articulators for which the reference's TailClipper has a ``clip_<name>_tails`` method."""
    return [CLIP_KINDS.get(a, 0) if clip_tails else 0 for a in articulators]


def launch_prepare_contours(raw, refs, kinds, dataset_config, mean=None, std=None, point_major=False):
    """One as_prepare_contours launch.  raw (F, A, N, 2), refs (F, 3, N, 2) float32 on the GPU (made contiguous here), kinds a
    list of A ints, mean / std (A, 2, N) or None.  Returns (out, ref_out (None when point_major), counts int32 (F, A)) without synchronising."""
    _lib.require_gpu(raw, "raw")
    _lib.require_gpu(refs, "refs")
    raw = raw.to(torch.float32).contiguous()
    refs = refs.to(device=raw.device, dtype=torch.float32).contiguous()
    if raw.dim() != 4 or raw.shape[-1] != 2 or raw.shape[0] < 1 or raw.shape[1] < 1 or raw.shape[2] < 1:
        raise ValueError(f"raw must be (frames, articulators, points, 2) and not empty, got {tuple(raw.shape)}")
    F, A, N, _ = raw.shape
    if tuple(refs.shape) != (F, 3, N, 2):
        raise ValueError(f"refs must be {(F, 3, N, 2)} (lower incisor, upper incisor, epiglottis), got {tuple(refs.shape)}")
    if len(kinds) != A:
        raise ValueError(f"{len(kinds)} kinds for {A} articulators")
    kinds_dev = torch.tensor(list(kinds), dtype=torch.int32).to(raw.device) if any(kinds) else None
    if (mean is None) != (std is None):
        raise ValueError("mean and std come together")
    if mean is not None:
        mean = mean.to(device=raw.device, dtype=torch.float32).contiguous()
        std = std.to(device=raw.device, dtype=torch.float32).contiguous()
        if tuple(mean.shape) != (A, 2, N) or tuple(std.shape) != (A, 2, N):
            raise ValueError(f"mean and std must be {(A, 2, N)}, got {tuple(mean.shape)} and {tuple(std.shape)}")
    out = torch.empty((F, A, N, 2) if point_major else (F, A, 2, N), dtype=torch.float32, device=raw.device)
    ref_out = torch.empty((F, 1, 2, N), dtype=torch.float32, device=raw.device) if not point_major else None
    counts = torch.empty((F, A), dtype=torch.int32, device=raw.device)
    tongue, lower_lip, upper_lip_front, upper_lip_back = clip_thresholds(dataset_config)
    with torch.cuda.device(raw.device):
        _lib.call("as_prepare_contours", raw, refs, kinds_dev, F, A, N, tongue, lower_lip, upper_lip_front, upper_lip_back, mean, std, int(point_major),
                  out, ref_out, counts)
    return out, ref_out, counts


def raise_on_empty(counts, articulators, frame_names=None):
    """RuntimeError naming the first (frame, articulator) whose contour kept no point -- where the reference raises inside
    F.interpolate.  Reads the counts back: one synchronisation."""
    empty = (counts == 0).nonzero()
    if empty.shape[0]:
        f, a = (int(v) for v in empty[0])
        frame = frame_names[f] if frame_names is not None else f
        raise RuntimeError(f"tail clipping left no point of articulator '{articulators[a]}' in frame {frame} "
                           f"({empty.shape[0]} emptied contours in all)")


def clip_tails_batched(raw, refs, articulators, dataset_config):
    """raw (F, A, 50, 2), refs (F, 3, 50, 2) on the GPU, articulators the A names -> (clipped (F, A, 50, 2), counts int32
    (F, A)): what the reference's clip_*_tails methods return for every frame (articulators without a method pass through), and
    the number of points each kept before its last resampling.  An emptied contour has count 0 and a NaN row."""
    out, _, counts = launch_prepare_contours(raw, refs, clip_kinds(articulators), dataset_config, point_major=True)
    return out, counts


class TailClipper:
    TAIL_CLIP_REFERENCES = [LOWER_INCISOR, UPPER_INCISOR, EPIGLOTTIS]

    def __init__(self, dataset_config):
        self.dataset_config = dataset_config

    def _clip(self, name, contour, **references):
        if not torch.cuda.is_available():
            raise RuntimeError("artspeech_amd TailClipper needs an MI355X device; there is no CPU path")
        contour = torch.as_tensor(contour)
        if tuple(contour.shape) != (CLIP_POINTS, 2):
            raise ValueError(f"a contour of ({CLIP_POINTS}, 2) points is clipped, got {tuple(contour.shape)}")
        dev = contour.device if contour.is_cuda else torch.device("cuda", torch.cuda.current_device())
        refs = torch.zeros((1, 3, CLIP_POINTS, 2), dtype=torch.float32, device=dev)
        for i, ref_name in enumerate(self.TAIL_CLIP_REFERENCES):
            ref = references.get(ref_name.replace("-", "_"))
            if ref is not None:
                refs[0, i] = torch.as_tensor(ref).to(device=dev, dtype=torch.float32)
        out, counts = clip_tails_batched(contour.to(device=dev, dtype=torch.float32)[None, None], refs, [name], self.dataset_config)
        if int(counts[0, 0]) == 0:
            raise RuntimeError(f"tail clipping left no point of the {name} contour (the reference fails in F.interpolate here)")
        return out[0, 0].to(contour.device)

    def clip_tongue_tails(self, tongue, lower_incisor, epiglottis, **kwargs):
        return self._clip("tongue", tongue, lower_incisor=lower_incisor, epiglottis=epiglottis)

    def clip_lower_lip_tails(self, lower_lip, lower_incisor, **kwargs):
        return self._clip("lower-lip", lower_lip, lower_incisor=lower_incisor)

    def clip_upper_lip_tails(self, upper_lip, upper_incisor, **kwargs):
        return self._clip("upper-lip", upper_lip, upper_incisor=upper_incisor)
