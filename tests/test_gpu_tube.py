"""as_vocal_tract_tube on the device against the numpy restatement (tests/tube_fp64.py).

Junctions and status are compared exactly: both sides form the squared distances with the same float32 operations.  Wall lengths
and coordinates are compared within 2 P 2^-53 max(L, 1), P and L taken from the restatement wall by wall: the two paths differ only
in the order of at most P float64 additions (a wave scan against a sequential cumsum), and a lerp carries an error in s into the
position unamplified."""
import os

import numpy as np
import pytest
import torch

import tube_fp64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def names(A):
    return [f"a{i}" for i in range(A)]


def chains(k_int, k_ext):
    """Channel indices: the internal wall follows the even channels, the external wall the odd ones (R.random_frames)."""
    return [2 * k for k in range(k_int)], [2 * k + 1 for k in range(k_ext)]


def run(x, k_int, k_ext, M, **kw):
    from artspeech_amd.phoneme_to_articulation.vocal_tract_tube import vocal_tract_tube
    A = x.shape[-3]
    i, e = chains(k_int, k_ext)
    n = names(A)
    return vocal_tract_tube(x, n, [n[a] for a in i], [n[a] for a in e], n_out=M, return_status=True, return_junctions=True,
                            return_length=True, **kw)


def assert_parity(got, ref, what):
    air, status, junc, length = (t.cpu().numpy() for t in got)
    r_air, r_status, r_junc, r_length, r_P = ref
    assert np.array_equal(junc, r_junc), what
    assert np.array_equal(status, r_status), what
    ok = r_status == 0
    tol = R.bound(r_P, np.where(ok, r_length, 1.0))
    err_len = np.abs(length - r_length)[ok]
    err = np.abs(air - r_air).reshape(air.shape[:-2] + (-1,)).max(-1)
    print(f"{what}: max length error {err_len.max() if err_len.size else 0:.3e}, max coordinate error "
          f"{err[ok].max() if ok.any() else 0:.3e}, smallest bound {tol[ok].min() if ok.any() else 0:.3e}")
    assert (err_len <= tol[ok]).all(), what
    assert (err[ok] <= tol[ok]).all(), what
    zero = r_status == R.STATUS_ZERO_LENGTH
    assert np.array_equal(air[zero], r_air[zero]) and (length[zero] == 0).all()
    bad = r_status == R.STATUS_NON_FINITE
    assert np.isnan(air[bad]).all() and np.isnan(length[bad]).all()


# (frames, N, k_int, k_ext, M): every N of {2, 3, 50, 63, 64, 65, 128}, K of {1, 2, 6, 8}, M of {2, 63, 64, 65, 100, 1024} and frame
# count of {1, 3, 4, 5, 9} (around the four-wave workgroup) at least once
PARITY_CASES = [(1, 2, 1, 2, 2), (3, 3, 2, 6, 63), (4, 50, 6, 6, 100), (5, 63, 8, 1, 64), (9, 64, 2, 8, 65), (3, 65, 6, 2, 1024),
                (5, 128, 8, 8, 1024), (4, 128, 1, 6, 2), (9, 50, 6, 6, 100)]


@pytest.mark.parametrize("F,N,k_int,k_ext,M", PARITY_CASES, ids=lambda v: str(v))
def test_parity_with_the_restatement(dev, F, N, k_int, k_ext, M):
    rng = np.random.default_rng(F * 1000 + N + M)
    x = R.random_frames(rng, F, 2 * max(k_int, k_ext), N)
    got = run(torch.from_numpy(x).to(dev), k_int, k_ext, M)
    assert got[0].shape == (F, 2, 2, M) and got[0].dtype == torch.float64
    assert_parity(got, R.tube(x, *chains(k_int, k_ext), M), f"tube F={F} N={N} K={k_int},{k_ext} M={M}")


def test_ties_repeated_points_and_zero_length_segments(dev):
    """Coordinates on the 1/8 grid: many equal distances (the first minimum in row-major order decides), repeated points and
    segments of zero length."""
    rng = np.random.default_rng(11)
    x = (rng.integers(0, 12, (7, 8, 2, 20)) / 8.0).astype(np.float32)
    x[2, :, :, 5:12] = x[2, :, :, 5:6]            # runs of repeated points
    x[4, 0::2] = x[4, 0:1, :, 0:1]                # the internal chain: all points coincident
    ref = R.tube(x, *chains(4, 3), 65)
    assert ref[1][4, 0] == R.STATUS_ZERO_LENGTH and (ref[1] == 0).sum() == 13
    got = run(torch.from_numpy(x).to(dev), 4, 3, 65)
    assert_parity(got, ref, "tube on the 1/8 grid")
    first = torch.from_numpy(x[4, 0, :, 0].astype(np.float64)).to(dev)
    assert torch.equal(got[0][4, 0], first[:, None].expand(2, 65))


def test_non_finite_points_flag_their_wall_only(dev):
    rng = np.random.default_rng(12)
    x = R.random_frames(rng, 5, 8, 50)
    clean = run(torch.from_numpy(x).to(dev), 3, 3, 100)
    y = x.copy()
    y[1, 2, 0, 17] = np.nan        # internal chain of frame 1
    y[3, 5, 1, 49] = np.inf        # external chain of frame 3
    y[2, 6, 0, 3] = np.nan         # channels 6 and 7 are in neither chain
    y[2, 7, 1, 0] = -np.inf
    got = run(torch.from_numpy(y).to(dev), 3, 3, 100)
    air, status, junc, length = got
    want = np.zeros((5, 2), np.int32)
    want[1, 0] = want[3, 1] = R.STATUS_NON_FINITE
    assert status.cpu().numpy().tolist() == want.tolist()
    for f, w in ((1, 0), (3, 1)):
        assert torch.isnan(air[f, w]).all() and torch.all(junc[f, w] == -1) and torch.isnan(length[f, w])
    keep = torch.from_numpy(want == 0).to(dev)
    for a, b in zip(got, clean):
        assert torch.equal(a[keep], b[keep])   # every other wall, frame 2 included: the bits of the clean launch
    assert_parity(got, R.tube(y, *chains(3, 3), 100), "tube beside non-finite walls")


@pytest.fixture(scope="module")
def batch():
    """(B, T, A) = (3, 4, 12) contours of 50 points and their restatement with six-contour chains, shared and left unchanged."""
    x = R.random_frames(np.random.default_rng(7), 12, 12, 50)
    return x.reshape(3, 4, 12, 2, 50), R.tube(x, *chains(6, 6), 100)


def test_model_layout_with_nan_behind_every_row(dev, batch):
    x, ref = batch
    wide = torch.full((3, 4, 12, 2, 57), float("nan"), device=dev)
    wide[..., :50] = torch.from_numpy(x).to(dev)
    view = wide[..., :50]
    assert not view.is_contiguous()
    got = run(view, 6, 6, 100)
    assert got[0].shape == (3, 4, 2, 2, 100) and got[1].shape == (3, 4, 2) and got[2].shape == (3, 4, 2, 7, 2)
    assert_parity([t.flatten(0, 1) for t in got], ref, "tube (B, T, A, 2, N) view")


def test_raw_contour_layout_goes_in_without_a_copy(dev, batch, monkeypatch):
    from artspeech_amd import _lib
    x, ref = batch
    raw = torch.full((12, 12, 53, 2), float("nan"), device=dev)
    raw[:, :, :50] = torch.from_numpy(x.reshape(12, 12, 2, 50)).to(dev).permute(0, 1, 3, 2)
    view = raw[:, :, :50].permute(0, 1, 3, 2)
    assert view.stride() == (12 * 53 * 2, 53 * 2, 1, 2)
    seen = []
    real = _lib.call

    def spy(name, *args, **kw):
        seen.append((name, args[0].data_ptr(), args[1:5]))
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, "call", spy)
    got = run(view, 6, 6, 100)
    assert seen == [("as_vocal_tract_tube", raw.data_ptr(), (12 * 53 * 2, 53 * 2, 1, 2))]
    assert_parity(got, ref, "tube (F, A, N, 2) view")
    swapped = view.permute(1, 0, 2, 3)[:, None].expand(12, 2, 12, 2, 50)   # no one stride walks (12, 2): copied once
    seen.clear()
    from artspeech_amd.phoneme_to_articulation.vocal_tract_tube import vocal_tract_tube
    vocal_tract_tube(swapped, names(12), ["a0"], ["a1"])
    assert len(seen) == 1 and seen[0][1] != raw.data_ptr()


def test_output_wider_than_m_keeps_its_tail(dev, batch):
    import ctypes
    from artspeech_amd import _lib
    x, ref = batch
    flat = torch.from_numpy(x.reshape(12, 12, 2, 50)).to(dev)
    air = torch.full((12, 2, 2, 108), 7.5, dtype=torch.float64, device=dev)
    i, e = chains(6, 6)
    table = (ctypes.c_int32 * 16)(*(i + [-1, -1] + e + [-1, -1]))
    _lib.call("as_vocal_tract_tube", flat, flat.stride(0), flat.stride(1), flat.stride(2), flat.stride(3), 12, 12, 50, table, 6, 6,
              None, 0, 100, air, 108, None, None, None)
    assert torch.all(air[..., 100:] == 7.5)
    tol = R.bound(ref[4], ref[3])[:, :, None, None]
    assert (np.abs(air[..., :100].cpu().numpy() - ref[0]) <= tol).all()


def test_lengths_zero_padded_frames_and_only_those(dev, batch):
    x, ref = batch
    xd = torch.from_numpy(x).to(dev).clone()
    xd[1, 2:] = float("nan")   # padded frames are not read: their NaN does not count as a non-finite wall
    lengths = [4, 2, 1]
    got = run(xd, 6, 6, 100, lengths=lengths)
    full = run(torch.from_numpy(x).to(dev), 6, 6, 100)
    for b, n in enumerate(lengths):
        for g, f in zip(got, full):
            assert torch.equal(g[b, :n], f[b, :n])          # valid frames: the bits of the launch without lengths
        air, status, junc, length = (t[b, n:] for t in got)
        assert torch.all(air == 0) and torch.all(status == 0) and torch.all(junc == -1) and torch.all(length == 0)
    x2 = x.reshape(12, 12, 2, 50)
    assert_parity([t.flatten(0, 1) for t in got], R.tube(x2, *chains(6, 6), 100, lengths=lengths, T=4), "tube with lengths")
    with pytest.raises(ValueError, match="B, T, A"):
        run(xd[0], 6, 6, 100, lengths=[4])


def test_two_launches_give_equal_bits_and_a_frame_alone_equals_it_in_a_batch(dev):
    x = torch.from_numpy(R.random_frames(np.random.default_rng(3), 131, 12, 50)).to(dev)
    a, b = run(x, 6, 6, 100), run(x, 6, 6, 100)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    for s, t in zip(run(x[77:78], 6, 6, 100), a):
        assert torch.equal(s, t[77:78])


def test_reversed_contours_give_equal_bits(dev):
    """N even, so that neither end rule meets its tie: a chain's wall does not depend on how its contours are stored."""
    rng = np.random.default_rng(5)
    x = R.random_frames(rng, 6, 12, 50)
    y = x.copy()
    flip = rng.random((6, 12)) < 0.5
    y[flip] = y[flip][..., ::-1]
    a, b = run(torch.from_numpy(x).to(dev), 6, 6, 100), run(torch.from_numpy(y).to(dev), 6, 6, 100)
    assert flip.any() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert not torch.equal(a[2], b[2])   # the junction indices do follow the storage order


def test_reference_call_form(dev, batch, tmp_path):
    from artspeech_amd.phoneme_to_articulation import vocal_tract_tube as V
    x, _ = batch
    frame = x[1, 2]
    order = list(V.INTERNAL_WALL) + [a for a in V.EXTERNAL_WALL if a not in V.INTERNAL_WALL]   # 11 articulators
    arrays = {a: frame[i] for i, a in enumerate(order)}
    want = V.vocal_tract_tube(torch.from_numpy(np.stack([arrays[a] for a in sorted(arrays)])).to(dev), sorted(arrays)).cpu().numpy()
    internal, external = V.generate_vocal_tract_tube(arrays)
    assert internal.shape == (100, 2) and external.dtype == np.float64
    assert np.array_equal(internal.T, want[0]) and np.array_equal(external.T, want[1])
    files = {}
    for k, (a, c) in enumerate(arrays.items()):
        files[a] = str(tmp_path / f"{a}.npy")
        np.save(files[a], c.T if k % 2 else c)   # (N, 2) and (2, N) files alike
    internal, external = V.generate_vocal_tract_tube(files)
    assert np.array_equal(internal.T, want[0]) and np.array_equal(external.T, want[1])
    halved = V.generate_vocal_tract_tube(arrays, norm_value=2.0, n_out=33)
    scaled = V.vocal_tract_tube(torch.from_numpy(np.stack([arrays[a] for a in sorted(arrays)]) / np.float32(2)).to(dev), sorted(arrays),
                                n_out=33).cpu().numpy()
    assert np.array_equal(halved[0].T, scaled[0]) and np.array_equal(halved[1].T, scaled[1])
    with pytest.raises(ValueError, match="none of its articulators"):
        V.generate_vocal_tract_tube({"tongue": frame[0]})


def test_limits_are_refused_and_nothing_is_launched(dev):
    from artspeech_amd.phoneme_to_articulation.vocal_tract_tube import vocal_tract_tube
    n = names(10)
    for bad in (torch.rand(2, 10, 2, 1, device=dev), torch.rand(2, 10, 2, 129, device=dev)):
        with pytest.raises(RuntimeError, match="points per contour"):
            vocal_tract_tube(bad, n, n[:2], n[2:4])
    x = torch.rand(2, 10, 2, 50, device=dev)
    for kw in (dict(n_out=1), dict(n_out=1025)):
        with pytest.raises(RuntimeError, match="output points"):
            vocal_tract_tube(x, n, n[:2], n[2:4], **kw)
    with pytest.raises(ValueError, match="at most 8"):
        vocal_tract_tube(x, n, n[:9], n[2:4])
    with pytest.raises(ValueError, match="none of its articulators"):
        vocal_tract_tube(x, n, ["tongue"], n[2:4])
    with pytest.raises(RuntimeError, match="MI355X"):
        vocal_tract_tube(x.cpu(), n, n[:2], n[2:4])


def test_end_to_end_concentric_arcs_give_the_radial_gap(dev):
    """vocal_tract_tube -> intersect_semipolar_grid_batched -> area_function_batched at B = 3, T = 15 on two concentric half
    circles (radius 1 and 1.5, exact up to float32 rounding) cut into chains of six.  The grid lines are rays from the centre.
    A ray meets a polyline inscribed in a circle of radius r between r cos(dtheta / 2) and r, dtheta the largest angular step;
    the wall is a polyline (the outputs, dtheta_2 apart) inscribed in a polyline (the contours' points, dtheta_1 apart) inscribed
    in the circle, so each section point lies within r ((1 - cos(dtheta_1 / 2)) + (1 - cos(dtheta_2 / 2))) below its circle, and
    the section distance within the sum of the two walls' errors (and 1e-6 for the float32 points) of the radial gap 0.5."""
    from artspeech_amd.area_function import area_function_batched, intersect_semipolar_grid_batched
    B, T, N, M, K = 3, 15, 50, 100, 6
    x = R.random_frames(np.random.default_rng(21), B * T, 2 * K, N, noise=0.0).reshape(B, T, 2 * K, 2, N)
    lengths = [15, 9, 4]
    air, status, junc, length = run(torch.from_numpy(x).to(dev), K, K, M, lengths=lengths)
    valid = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(dev)
    assert torch.all(status == 0) and torch.all(length[valid][:, 0] >= 3.13) and torch.all(length[valid][:, 1] >= 1.5 * 3.13)
    margin = 0.05
    inside = np.linspace(margin, np.pi - margin, 40)
    outside = np.array([-0.6, -0.3, -0.1])           # rays below the half plane: they cross neither arc
    phi = np.concatenate([inside, outside])
    rad = np.linspace(0.5, 2.0, 20)
    grid = np.stack([np.cos(phi)[:, None] * rad, np.sin(phi)[:, None] * rad], axis=-1)
    flags, p_int, p_ext = intersect_semipolar_grid_batched(air[valid], grid)
    assert torch.all(flags[:, :40] & 3 == 3) and torch.all(flags[:, 40:] & 3 == 0)
    sections = torch.stack([p_int[:, :40].transpose(1, 2), p_ext[:, :40].transpose(1, 2)], dim=1)   # the air-column layout
    dists, fx = area_function_batched(sections)   # fx = pi (section distance / 2)^2; dists runs along the mid line
    span = np.pi / (K - (K - 1) * 0.25)
    dtheta_1, dtheta_2 = span / (N - 1), np.pi / (M - 1)
    sag = (1 - np.cos(dtheta_1 / 2)) + (1 - np.cos(dtheta_2 / 2))
    tol = (1.0 + 1.5) * sag + 1e-6
    gap = torch.linalg.norm(p_ext[:, :40] - p_int[:, :40], dim=-1)
    err = float((gap - 0.5).abs().max())
    err_fx = float((2 * torch.sqrt(fx / np.pi) - 0.5).abs().max())
    print(f"end to end: max |section distance - 0.5| = {err:.3e} (from fx: {err_fx:.3e}), chord bound {tol:.3e}")
    assert err <= tol and err_fx <= tol + 1e-12
    assert torch.all(dists[:, 1:] > dists[:, :-1])
    radius = torch.linalg.norm(p_int[:, :40], dim=-1)
    assert torch.all(radius <= 1 + 1e-6) and torch.all(radius >= 1 - sag - 1e-6)


def test_synthesize_writes_air_columns_and_xarticul(dev, tmp_path):
    """synthesize(..., air_column=True) with a freshly initialised encoder_decoder model on four short sentences: the air columns
    equal the restatement applied to the saved inference_contours/ (the configured upper incisor among them), the Xarticul files
    parse back, and air_column=False leaves the listing as it was."""
    from artspeech_amd.helpers import xarticul_to_npy
    from artspeech_amd.phoneme_to_articulation import synthesis as S
    from artspeech_amd.phoneme_to_articulation import vocal_tract_tube as V
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech
    torch.manual_seed(9)
    articulators = sorted(["lower-lip", "pharynx", "soft-palate-midline", "tongue", "upper-lip", "vocal-folds"])
    N = 20
    model = ArtSpeech(5, len(articulators), embed_dim=16, hidden_size=32, n_samples=N).to(dev).eval()
    vocabulary = {"<blank>": 0, "<unk>": 1, "a": 2, "b": 3, "c": 4}
    sentences = [("s1", "a a a b b c c c a".split()), ("s2", "c c b".split()), ("s3", ["b"]), ("s4", "a b c a b".split())]
    incisor = np.stack([np.linspace(0.45, 0.55, N), np.linspace(0.7, 0.6, N)]).astype(np.float32)
    info = S.synthesize(model, sentences, vocabulary, articulators, str(tmp_path / "with"), batch_size=3, upper_incisor=incisor,
                        air_column=True, res=136)
    assert info["frames"] == 18 and info["flagged_walls"] == {"zero_length": 0, "non_finite": 0}
    names = articulators + ["upper-incisor"]
    chains = [V.chain_indices(names, V.INTERNAL_WALL), V.chain_indices(names, V.EXTERNAL_WALL)]
    assert [len(c) for c in chains] == [3, 5]   # no arytenoid cartilage among them; the joined upper incisor is
    for name, tokens in sentences:
        folder = tmp_path / "with" / name
        assert sorted(os.listdir(folder)) == ["air_column", "contours.npy", "inference_contours", "target_sequence.txt", "xarticul"]
        assert sorted(os.listdir(folder / "air_column")) == [f"{t + 1:04d}.npy" for t in range(len(tokens))]
        assert sorted(os.listdir(folder / "xarticul")) == [f"{t + 1:04d}.txt" for t in range(len(tokens))]
        saved = np.stack([np.stack([np.load(folder / "inference_contours" / f"{t + 1:04d}_{a}.npy") for a in names])
                          for t in range(len(tokens))])
        want, status, _, length, P = R.tube(saved, chains[0], chains[1], 100)
        assert (status == 0).all()
        for t in range(len(tokens)):
            air = np.load(folder / "air_column" / f"{t + 1:04d}.npy")
            assert air.shape == (2, 2, 100) and air.dtype == np.float64
            assert (np.abs(air - want[t]).reshape(2, -1).max(-1) <= R.bound(P[t], length[t])).all(), (name, t)
            rows = xarticul_to_npy(folder / "xarticul" / f"{t + 1:04d}.txt")
            assert rows.shape == (201, 2) and rows[100].tolist() == [-1, -1]
            assert np.array_equal(rows[:100], air[0].T * 136) and np.array_equal(rows[101:], air[1].T * 136)
    info = S.synthesize(model, sentences, vocabulary, articulators, str(tmp_path / "without"), batch_size=3, upper_incisor=incisor)
    assert "flagged_walls" not in info
    for name, _ in sentences:
        assert sorted(os.listdir(tmp_path / "without" / name)) == ["contours.npy", "inference_contours", "target_sequence.txt"]
        assert np.array_equal(np.load(tmp_path / "without" / name / "contours.npy"), np.load(tmp_path / "with" / name / "contours.npy"))
    with pytest.raises(ValueError, match="point count"):
        S.synthesize(model, sentences, vocabulary, articulators, str(tmp_path / "bad"), upper_incisor=incisor[:, :7], air_column=True)
