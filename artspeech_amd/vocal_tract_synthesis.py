"""Speech from the tube on the device (csrc/vt_synth.hip): a glottal source (as_vt_glottal_source) drives a time-domain
Kelly-Lochbaum waveguide whose sections vary in time (as_vt_waveguide), one launch each for a whole batch.  The reference has no
acoustic stage: the definition is this project's own, an ASSUMPTION whose parity with any other synthesiser is unpinned; the
header (include/artspeech_hip.h) states it in full.  In short, float64 throughout:

- B utterances of T frame slots, ``frames[b]`` of them used, S samples per frame: the sample rate is S x the frame rate, and a
  per-frame control is read per sample by linear interpolation towards the next used frame (the last one is held);
- the source is a Rosenberg pulse train on the running phase of f0 plus aspiration noise;
- the ladder has K_b <= 64 sections of c / fs each, section 0 the glottis and K_b - 1 the lips; its reflection coefficients
  k_j = (A_j - A_{j+1}) / (A_j + A_{j+1}) are formed per frame and interpolated per sample; frication noise may be injected at
  one section per frame; the lips' output is differenced (``radiation="difference"``) or not (``"none"``).

Status bits per utterance: ``STATUS_CLOSED`` (an area below ``min_area``, computed as ``min_area``: a closure, not an error) and
``STATUS_NON_FINITE`` (a non-finite control, area, source sample or gain in a used frame: the utterance's samples are NaN).
Left out: a nasal branch, wall vibration and frequency-dependent losses, a two-mass glottis, more than 64 sections, and pitch or
prosody models beyond a linear declination."""
from collections import namedtuple

import torch

from . import _lib
from .vocal_tract_acoustics import MIN_AREA, SOUND_SPEED, STATUS_CLOSED, STATUS_NON_FINITE  # noqa: F401  (one meaning, one name)

MAX_SECTIONS = 64
RISE, FALL = 0.40, 0.16                   # the Rosenberg pulse's opening and closing parts of a period
R_GLOTTIS, R_LIPS, MU = 0.75, -0.85, 0.999   # plausible, but this project's own
RADIATION = {"none": 0, "difference": 1}

EqualSections = namedtuple("EqualSections", ["areas", "sections", "tract_length", "replaced"])
Waveguide = namedtuple("Waveguide", ["out64", "out32", "status"])
Waveform = namedtuple("Waveform", ["samples", "n_samples", "sample_rate", "status", "sections", "tract_length", "replaced"])


def _control(x, name, B, T, device):
    """A per-frame control as the kernels read it: (B, T) float64, contiguous, on the device; a number is spread over the frames."""
    if not isinstance(x, torch.Tensor):
        return torch.full((B, T), float(x), dtype=torch.float64, device=device)
    _lib.require_gpu(x, name)
    if tuple(x.shape) != (B, T):
        raise ValueError(f"{name} is (B, T) = ({B}, {T}), got {tuple(x.shape)}")
    return _lib.contiguous(x.detach().to(torch.float64))


def _frames(frames, B, device):
    frames = torch.as_tensor(frames).to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    if frames.numel() != B:
        raise ValueError(f"frames {tuple(frames.shape)} for {B} utterances")
    return frames


def _output(out, dtype, B, pitch, device, name):
    """An output of (B, pitch): allocated (True), left out (False / None) or the caller's own tensor, written in place."""
    if out is None or out is False:
        return None
    if out is True:
        return torch.empty((B, pitch), dtype=dtype, device=device)
    _lib.require_gpu(out, name)
    if out.dtype != dtype or tuple(out.shape) != (B, pitch) or not out.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of (B, pitch) = ({B}, {pitch}), got {out.dtype} {tuple(out.shape)}")
    return out


def equal_sections(areas, lengths, counts, frames, sample_rate, c=SOUND_SPEED):
    """The ragged sections of ``tube_from_air_columns`` as the ladder's equal ones.  areas, lengths (B, T, Kr) float64 on the GPU in
    cm^2 and cm, counts (B, T) sections used per frame, frames (B,) -> ``EqualSections(areas (B, T, Kmax), sections (B,) int32,
    tract_length (B, 3), replaced (B,))``:

    - a frame t < frames[b] is valid when it has at least one section and its used areas and lengths are finite, the lengths > 0;
    - K_b = clamp(round(mean tract length over the valid frames x sample_rate / c), 2, 64), halves to even;
    - every frame is cut into K_b slices of its OWN length; a slice takes the area of the section that holds its midpoint
      (the number of section ends at or below the midpoint, at most the last section).  The ladder's sections are c / fs long:
      the frame-to-frame variation of the tract's length is dropped; ``tract_length`` holds its min, mean and max over the
      valid frames in cm (NaN without a valid frame);
    - a frame that is not valid takes the nearest earlier valid frame's areas, or the first valid one's at the start;
      ``replaced`` counts them.  Without any valid frame the utterance's areas are NaN and the ladder reports it.
    Columns K_b .. Kmax - 1 and frames t >= frames[b] hold 0 and are never read.  Torch ops in float64: glue, not a hot path."""
    _lib.require_gpu(areas, "areas")
    _lib.require_gpu(lengths, "lengths")
    areas, lengths = areas.to(torch.float64), lengths.to(torch.float64)
    if areas.dim() != 3 or areas.shape != lengths.shape:
        raise ValueError(f"equal_sections needs areas and lengths of one shape (B, T, K), got {tuple(areas.shape)} and {tuple(lengths.shape)}")
    B, T, Kr = areas.shape
    dev = areas.device
    counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int64).reshape(B, T).clamp(max=Kr)
    frames = _frames(frames, B, dev).to(torch.int64).clamp(0, T)
    used = torch.arange(Kr, device=dev)[None, None, :] < counts[..., None]
    fine = (torch.isfinite(areas) & torch.isfinite(lengths) & (lengths > 0)) | ~used
    valid = fine.all(-1) & (counts >= 1) & (torch.arange(T, device=dev)[None, :] < frames[:, None])
    ends = torch.where(used, lengths, torch.zeros_like(lengths)).cumsum(-1)
    total = ends[..., -1] if Kr else torch.zeros((B, T), dtype=torch.float64, device=dev)
    n_valid = valid.sum(1)
    nan = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    masked = torch.where(valid, total, torch.zeros_like(total))
    mean = torch.where(n_valid > 0, masked.sum(1) / n_valid.clamp(min=1), nan)
    low = torch.where(n_valid > 0, torch.where(valid, total, torch.full_like(total, float("inf"))).amin(1), nan)
    high = torch.where(n_valid > 0, torch.where(valid, total, torch.full_like(total, -float("inf"))).amax(1), nan)
    sections = torch.round(torch.nan_to_num(mean, nan=0.0) * float(sample_rate) / float(c)).clamp(2, MAX_SECTIONS).to(torch.int64)
    Kmax = int(sections.max()) if B else 2
    mid = (torch.arange(Kmax, device=dev, dtype=torch.float64)[None, None, :] + 0.5) * (total / sections[:, None])[..., None]
    index = torch.searchsorted(ends.contiguous(), mid.contiguous(), right=True)
    index = torch.minimum(index, (counts - 1).clamp(min=0)[..., None])
    sliced = areas.gather(2, index) if Kr else torch.zeros((B, T, Kmax), dtype=torch.float64, device=dev)
    at = torch.arange(T, device=dev)[None, :].expand(B, T)
    earlier = torch.where(valid, at, torch.full_like(at, -1)).cummax(1).values
    first = valid.to(torch.int8).argmax(1)[:, None].expand(B, T)
    source = torch.where(earlier >= 0, earlier, first)
    sliced = sliced.gather(1, source[..., None].expand(B, T, Kmax))
    sliced = torch.where((n_valid > 0)[:, None, None], sliced, torch.full_like(sliced, float("nan")))
    keep = (torch.arange(Kmax, device=dev)[None, None, :] < sections[:, None, None]) & (at < frames[:, None])[..., None]
    sliced = torch.where(keep, sliced, torch.zeros_like(sliced))
    replaced = ((at < frames[:, None]) & ~valid).sum(1)
    return EqualSections(sliced.contiguous(), sections.to(torch.int32), torch.stack([low, mean, high], 1), replaced)


def frication_control(areas_eq, sections, gain, critical_area=0.2, min_area=MIN_AREA):
    """Where and how strongly to inject frication noise, per frame, from the narrowest interior section (1 .. K_b - 2; the glottis
    and the lips' section are not looked at): A_min at the lowest index m among equals, q = gain max(0, 1 - A_min /
    critical_area), q = 0 at a closure (A_min < min_area) and without an interior section.  -> (inject_section (B, T) int32:
    min(m + 1, K_b - 1) where q > 0, else -1; inject_gain (B, T) float64: q).  ``gain`` is a number or (B, T).  A NaN area gives
    no injection: the ladder reports it."""
    _lib.require_gpu(areas_eq, "areas_eq")
    B, T, Kmax = areas_eq.shape
    dev = areas_eq.device
    sections = torch.as_tensor(sections).to(device=dev, dtype=torch.int64).reshape(B)
    j = torch.arange(Kmax, device=dev)[None, None, :]
    interior = (j >= 1) & (j <= sections[:, None, None] - 2)
    a = torch.where(interior & ~torch.isnan(areas_eq), areas_eq.to(torch.float64), torch.full_like(areas_eq, float("inf"), dtype=torch.float64))
    a_min = a.amin(-1)
    m = (a == a_min[..., None]).to(torch.int8).argmax(-1)   # the lowest index among equals
    gain = _control(gain, "gain", B, T, dev)
    q = gain * (1.0 - a_min / float(critical_area)).clamp(min=0.0)
    q = torch.where(torch.isfinite(a_min) & (a_min >= float(min_area)), q, torch.zeros_like(q))
    where = torch.minimum(m + 1, (sections - 1)[:, None].expand(B, T))
    where = torch.where(q > 0, where, torch.full_like(where, -1))
    return where.to(torch.int32).contiguous(), q.contiguous()


def glottal_source(f0, voiced_amp, asp_amp, frames, samples_per_frame, sample_rate, seed=0, rise=RISE, fall=FALL, pitch=None,
                   out=True):
    """f0 (Hz), voiced_amp, asp_amp (B, T) on the GPU (or numbers), frames (B,) -> (source (B, pitch) float64, status (B,) int32):
    one as_vt_glottal_source launch.  ``pitch`` >= T x samples_per_frame is the rows' pitch (T x samples_per_frame by default)."""
    _lib.require_gpu(f0, "f0")
    B, T = f0.shape
    dev = f0.device
    S = int(samples_per_frame)
    pitch = T * S if pitch is None else int(pitch)
    f0 = _control(f0, "f0", B, T, dev)
    voiced_amp = _control(voiced_amp, "voiced_amp", B, T, dev)
    asp_amp = _control(asp_amp, "asp_amp", B, T, dev)
    frames = _frames(frames, B, dev)
    source = _output(out, torch.float64, B, pitch, dev, "out")
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    if B > 0:   # an empty batch launches nothing (and an empty tensor has no address to hand over)
        with torch.cuda.device(dev):
            _lib.call("as_vt_glottal_source", f0, voiced_amp, asp_amp, frames, B, T, S, float(sample_rate), int(seed) & (2 ** 64 - 1),
                      float(rise), float(fall), source, pitch, status)
    return source, status


def waveguide(areas, sections, frames, samples_per_frame, source, inject_section=None, inject_gain=None, seed=0, r_g=R_GLOTTIS,
              r_l=R_LIPS, mu=MU, min_area=MIN_AREA, radiation="difference", out64=True, out32=True):
    """areas (B, T, Kmax) cm^2 on the GPU (any strides), sections (B,), frames (B,), source (B, pitch) float64 ->
    ``Waveguide(out64 (B, pitch) float64, out32 (B, pitch) float32, status (B,) int32)``: one as_vt_waveguide launch.  ``out64`` /
    ``out32`` are True (allocate), False (leave out) or a tensor of (B, pitch) to write into.  A section count outside 1 .. 64
    or an injection section outside 1 .. K_b - 1 (-1: none) raises before anything is launched."""
    if radiation not in RADIATION and radiation not in (0, 1):
        raise ValueError(f"radiation is one of {sorted(RADIATION)}, got {radiation!r}")
    _lib.require_gpu(areas, "areas")
    _lib.require_gpu(source, "source")
    if areas.dim() != 3 or source.dim() != 2 or source.shape[0] != areas.shape[0]:
        raise ValueError(f"waveguide needs areas (B, T, Kmax) and source (B, pitch), got {tuple(areas.shape)} and {tuple(source.shape)}")
    areas = areas.detach()
    if areas.dtype != torch.float64:
        areas = areas.to(torch.float64)
    B, T, Kmax = areas.shape
    dev = areas.device
    S = int(samples_per_frame)
    source = _lib.contiguous(source.detach().to(torch.float64))
    pitch = source.shape[1]
    sections = torch.as_tensor(sections).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if sections.numel() != B:
        raise ValueError(f"sections {tuple(sections.shape)} for {B} utterances")
    frames = _frames(frames, B, dev)
    if (inject_section is None) != (inject_gain is None):
        raise ValueError("inject_section and inject_gain come together")
    if inject_section is not None:
        inject_section = torch.as_tensor(inject_section).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(inject_section.shape) != (B, T):
            raise ValueError(f"inject_section is (B, T) = ({B}, {T}), got {tuple(inject_section.shape)}")
        inject_gain = _control(inject_gain, "inject_gain", B, T, dev)
    out64 = _output(out64, torch.float64, B, pitch, dev, "out64")
    out32 = _output(out32, torch.float32, B, pitch, dev, "out32")
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call("as_vt_waveguide", areas, areas.stride(0), areas.stride(1), areas.stride(2), sections, frames, B, T, Kmax, S,
                      source, inject_section, inject_gain, int(seed) & (2 ** 64 - 1), float(r_g), float(r_l), float(mu),
                      float(min_area), RADIATION.get(radiation, radiation), out64, out32, pitch, status)
    return Waveguide(out64, out32, status)


def synthesize_speech(areas, lengths, counts, voicing, frames, samples_per_frame, framerate, c=SOUND_SPEED, f0=None, f0_start=120.0,
                      f0_end=90.0, amplitude=1.0, aspiration=0.05, frication=0.1, critical_area=0.2, seed=0, rise=RISE, fall=FALL,
                      r_g=R_GLOTTIS, r_l=R_LIPS, mu=MU, min_area=MIN_AREA, radiation="difference"):
    """From the tube's ragged sections to sound: ``equal_sections`` -> ``frication_control`` -> ``glottal_source`` ->
    ``waveguide``.  areas, lengths (B, T, Kr), counts (B, T), voicing (B, T) in [0, 1], frames (B,) ->
    ``Waveform(samples float32 (B, T S), n_samples (B,), sample_rate, status (B,), sections, tract_length, replaced)``.
    voiced_amp = amplitude x voicing, asp_amp = aspiration x (1 - voicing); without ``f0`` (B, T) the pitch declines linearly from
    ``f0_start`` to ``f0_end`` Hz over each utterance's frames.  The sample rate is samples_per_frame x framerate.  An area of
    exactly 0 (walls that touch) is a closure here, not the defect that ``waveguide`` reports for a non-positive area."""
    S = int(samples_per_frame)
    fs = S * float(framerate)
    eq = equal_sections(areas, lengths, counts, frames, fs, c)
    B, T, _ = eq.areas.shape
    dev = eq.areas.device
    frames = _frames(frames, B, dev)
    voicing = _control(voicing, "voicing", B, T, dev)
    if f0 is None:
        along = torch.arange(T, device=dev, dtype=torch.float64)[None, :] / (frames.to(torch.float64)[:, None] - 1).clamp(min=1)
        f0 = float(f0_start) + (float(f0_end) - float(f0_start)) * along.clamp(max=1)
    # The area function gives exactly 0 where the walls touch: a closure.  The ladder takes a non-positive area for a defect of
    # its input (status bit 1), so a 0 goes in as half the closure threshold: flagged STATUS_CLOSED and computed as min_area.
    eq = eq._replace(areas=torch.where(eq.areas == 0, torch.full_like(eq.areas, 0.5 * float(min_area)), eq.areas))
    where, gain = frication_control(eq.areas, eq.sections, frication, critical_area, min_area)
    source, s_status = glottal_source(f0, float(amplitude) * voicing, float(aspiration) * (1.0 - voicing), frames, S, fs, seed, rise, fall)
    out = waveguide(eq.areas, eq.sections, frames, S, source, where, gain, seed, r_g, r_l, mu, min_area, radiation, out64=False)
    return Waveform(out.out32, frames.to(torch.int64).clamp(0, T) * S, fs, out.status | s_status, eq.sections, eq.tract_length,
                    eq.replaced)
