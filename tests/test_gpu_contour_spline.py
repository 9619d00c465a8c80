"""as_contour_spline on the device against the numpy float64 restatement (tests/contour_spline_fp64.py) rounded to float32.

Tolerance of the parity: |got - ref| <= 2^-23 max|ref|, one float32 ulp of the largest coordinate.  The two float64 solves differ
by about cond * 2^-52 <= 1e8 * 2.2e-16 = 2.2e-8 relative (tests/test_contour_spline_host.py asserts the condition numbers of every
matrix used here), under half of float32's half-ulp, so at most a rounding flip of one ulp is left."""
import numpy as np
import pytest
import torch

import contour_spline_fp64 as R
from conftest import WORST

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def launch(x, N, K, d, lam, M, lengths=None, T=0, A=0, out=None, status=None, strides=None, n=None):
    """The raw entry point on a tensor whose contours lie (n, 2, N) unless ``strides`` = (contour, coordinate, point)."""
    from artspeech_amd import _lib
    n = x.shape[0] if n is None else n
    strides = strides or (x.stride(0), x.stride(1), x.stride(2))
    if out is None:
        out = torch.empty(n, 2, M, dtype=torch.float32, device=x.device)
    _lib.call("as_contour_spline", x, strides[0], strides[1], strides[2], n, N, K, d, lam, M, lengths, T, A, out, out.stride(1), status)
    return out


def assert_parity(got, ref64, what):
    ref = ref64.astype(np.float32).astype(np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got.astype(np.float64) - ref).max())
    WORST[what] = max(WORST.get(what, 0.0), err / scale)
    print(f"{what}: max|got - ref| / max|ref| = {err / scale:.3e} ({err / scale / ULP:.2f} ulp)")
    assert err <= ULP * scale, f"{what}: {err / scale / ULP:.2f} float32 ulp of max|ref|"


@pytest.mark.parametrize("n,N,K,d,M,lam", R.PARITY_CASES, ids=lambda v: str(v))
def test_parity_with_the_float64_restatement(dev, n, N, K, d, M, lam):
    K = d + 1 if K is None else K
    x = R.case_contours(n, N)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    got = launch(torch.from_numpy(x).to(dev), N, K, d, lam, M, status=status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert_parity(got.cpu().numpy(), R.smooth_batch(x, d, K, lam, M), f"contour_spline n={n} N={N} K={K} d={d} M={M} lam={lam:g}")


@pytest.fixture(scope="module")
def batch():
    """(B, T, A) = (3, 4, 2) contours of 50 points and their restatement with the package's defaults, shared and left unchanged."""
    d, K, lam = R.DEFAULTS
    x = R.case_contours(24, 50, seed=7).reshape(3, 4, 2, 2, 50)
    return x, R.smooth_batch(x, d, K, lam)


def test_model_layout_with_nan_behind_every_row(dev, batch):
    """(B, T, A, 2, N) as a view of a wider buffer whose padding is NaN: a read past a row would poison the result."""
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    x, ref = batch
    wide = torch.full((3, 4, 2, 2, 57), float("nan"), device=dev)
    wide[..., :50] = torch.from_numpy(x).to(dev)
    view = wide[..., :50]
    assert not view.is_contiguous()
    got, status = regularize_contours(view, return_status=True)
    assert got.shape == (3, 4, 2, 2, 50) and int(status.abs().sum()) == 0
    assert_parity(got.cpu().numpy(), ref, "contour_spline (B, T, A, 2, N) view")


def test_raw_contour_layout_goes_in_without_a_copy(dev, batch):
    """(F, A, N, 2) raw contours, NaN behind every row, as the permuted view (F, A, 2, N): point stride 2, coordinate stride 1."""
    from artspeech_amd.phoneme_to_articulation import regularization as G
    x, ref = batch
    raw = torch.full((12, 2, 53, 2), float("nan"), device=dev)
    raw[:, :, :50] = torch.from_numpy(x.reshape(12, 2, 2, 50)).to(dev).permute(0, 1, 3, 2)
    view = raw[:, :, :50].permute(0, 1, 3, 2)
    assert view.stride() == (2 * 53 * 2, 53 * 2, 1, 2) and G._contour_stride(view) == 53 * 2
    got = G.regularize_contours(view)
    assert_parity(got.cpu().numpy(), ref.reshape(12, 2, 2, 50), "contour_spline (F, A, N, 2) view")
    swapped = view.permute(1, 0, 2, 3)   # (A, F, 2, N): no one stride walks the leading dimensions, so it is copied once
    assert G._contour_stride(swapped) is None
    assert torch.equal(G.regularize_contours(swapped), got.permute(1, 0, 2, 3))


def test_output_wider_than_m_keeps_its_tail(dev, batch):
    x, ref = batch
    d, K, lam = R.DEFAULTS
    flat = torch.from_numpy(x.reshape(24, 2, 50)).to(dev)
    out = torch.full((24, 2, 40), 7.5, device=dev)
    launch(flat, 50, K, d, lam, 33, out=out)
    assert torch.all(out[..., 33:] == 7.5) and torch.isfinite(out[..., :33]).all()
    assert_parity(out[..., :33].cpu().numpy(), R.smooth_batch(x.reshape(24, 2, 50), d, K, lam, 33), "contour_spline pitched output")


def test_lengths_zero_padded_frames_and_only_those(dev, batch):
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    x, ref = batch
    xd = torch.from_numpy(x).to(dev).clone()
    xd[1, 2:] = float("nan")   # padded frames are not read: their NaN does not count as a non-finite contour
    lengths = [4, 2, 1]
    got, status = regularize_contours(xd, lengths=lengths, return_status=True)
    full = regularize_contours(torch.from_numpy(x).to(dev))
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, :n], full[b, :n])          # valid frames: the bits of the launch without lengths
        assert torch.all(got[b, n:] == 0) and torch.all(status[b] == 0)
    with pytest.raises(ValueError, match="B, T, A"):
        regularize_contours(xd[0], lengths=[4])


def test_degenerate_contours(dev, batch):
    from artspeech_amd.phoneme_to_articulation.regularization import STATUS_NON_FINITE, STATUS_ZERO_LENGTH, regularize_contours
    x, ref = batch
    xd = torch.from_numpy(x.reshape(24, 2, 50)).to(dev).clone()
    p0 = torch.tensor([0.1234567, 0.7654321], device=dev)
    xd[3] = p0[:, None]                       # zero length
    xd[5, 1, 17] = float("nan")               # one NaN coordinate
    xd[6, 0, 49] = float("inf")
    xd[8, :, 10:30] = xd[8, :, 10:11]         # twenty repeated points
    got, status = regularize_contours(xd, n_out=65, return_status=True)
    status = status.cpu().numpy()
    want = np.zeros(24, np.int32)
    want[3], want[5], want[6] = STATUS_ZERO_LENGTH, STATUS_NON_FINITE, STATUS_NON_FINITE
    assert status.tolist() == want.tolist()
    assert torch.equal(got[3], p0[:, None].expand(2, 65))      # p_0, bit for bit
    assert torch.isnan(got[5]).all() and torch.isnan(got[6]).all()
    keep = [i for i in range(24) if i not in (3, 5, 6)]
    assert torch.isfinite(got[keep]).all()                     # a NaN poisons its own row only
    d, K, lam = R.DEFAULTS
    xh = xd.cpu().numpy()
    assert np.linalg.cond(R.normal_matrix(xh[8].T, K, d, lam)) <= 1e8
    assert_parity(got[keep].cpu().numpy(), R.smooth_batch(xh[keep], d, K, lam, 65), "contour_spline beside degenerate rows")


def test_limits_are_refused_and_nothing_is_launched(dev):
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_contours
    x = torch.rand(2, 2, 50, device=dev)
    sentinel = torch.full((2, 2, 50), -3.0, device=dev)
    for kw in (dict(n_ctrl=3), dict(n_ctrl=33), dict(n_out=1), dict(n_out=1025), dict(degree=0), dict(degree=4), dict(smoothing=0.0),
               dict(smoothing=float("nan")), dict(smoothing=float("inf"))):
        with pytest.raises(RuntimeError, match="as_contour_spline"):
            regularize_contours(x, **kw)
    for bad in (torch.rand(2, 2, 1, device=dev), torch.rand(2, 2, 257, device=dev)):
        with pytest.raises(RuntimeError, match="points per contour"):
            regularize_contours(bad)
    with pytest.raises(RuntimeError, match="as_contour_spline"):
        launch(x, 50, 12, 3, 0.0, 50, out=sentinel)
    torch.cuda.synchronize()
    assert torch.all(sentinel == -3.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        regularize_contours(x.cpu())


def test_two_launches_give_equal_bits_and_a_contour_alone_equals_it_in_a_batch(dev):
    x = torch.from_numpy(R.case_contours(257, 50)).to(dev)
    d, K, lam = R.DEFAULTS
    a = launch(x, 50, K, d, lam, 50)
    b = launch(x, 50, K, d, lam, 50)
    assert torch.equal(a, b)
    assert torch.equal(launch(x[200:201], 50, K, d, lam, 50), a[200:201])


def test_reference_call_form(dev, batch):
    from artspeech_amd.phoneme_to_articulation.regularization import regularize_Bsplines
    x, ref = batch
    reg_x, reg_y = regularize_Bsplines(x[0, 0, 0].T, 3)
    assert isinstance(reg_x, np.ndarray) and reg_x.shape == (50,) and reg_y.shape == (50,)
    assert_parity(np.stack([reg_x, reg_y]), ref[0, 0, 0], "regularize_Bsplines")
