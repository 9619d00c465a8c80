"""The split-arithmetic head kernels at the smallest shape that reaches their 64-row main loops: rows = 3021, A = 11.

The 64-row loop of s6_main_loop (csrc/lin_f32.hip) is only taken when ceil(rows / 64) x heads >= 512; the small head-stack
tests of test_gpu_parity.py (1536 and 37 rows, 3 heads) run 32-row tiles only.  At 3021 rows and 11 heads

    lin_s6_kernel (Linear 1, 2, dx3, dx2)   46 tiles of 64 rows per head, then three of 32 rows, the last one ragged (13 rows)
    lin_out_s6_kernel (output layer)        47 tiles of 64 rows per head, then one ragged tile of 32 rows
    lin_s6_plain_kernel (dx1)               47 + 1 likewise, 8 k-chunks of 352 = 11 k-tiles (three passes of the loop + two tail tiles)

H in {128, 96, 64} gives Linear 1 four, three and two k-tiles (every nk mod 3), N in {50, 40} lets dx3 reduce over 128 or 96.

Input rows 2944 + i (i < 77) are copies of rows i, in x and in d(out).  Every output row depends on its own input row only,
and the 64-row and the 32-row loop issue the same products in the same order per row: the copies' results must be equal
BITWISE although rows 0-76 sit in 64-row tiles and rows 2944-3020 (for lin_s6_kernel) in 32-row tiles.  The forward is also
checked against the fp64 oracle (the file's assert_close; no ReLU decision enters a forward value's tolerance)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import T_, assert_close
from oracle import artspeech_oracle as O

pytestmark = pytest.mark.gpu

ROWS, A, COPIES, FIRST_COPY = 3021, 11, 77, 2944


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("N", [50, 40])
@pytest.mark.parametrize("H", [128, 96, 64])
def test_rows_in_64_row_and_32_row_tiles_agree_bitwise(dev, H, N):
    """Setup as test_gpu_parity._head_stack_vs_oracle: as_head_fwd then as_head_bwd in the split arithmetic on a NaN-filled
    workspace, non-trivial LayerNorm affines."""
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import _build_views, _numel
    L = _lib.lib()
    assert L.as_get_matrix_arith() == 1, "the split arithmetic is the library's default"
    dims = _lib.Dims(1, A, 1, H, N, 1)
    lay = _lib.layout(dims)
    rng = np.random.RandomState(7)
    views = {k: v for k, v in _build_views(dims, lay).items() if k.startswith("predictors.")}
    flat = torch.zeros(lay.total)
    params = {}
    for k, (off, shape) in views.items():
        n = _numel(shape)
        if k.endswith((".linear.0.weight", ".linear.3.weight", ".linear.6.weight")):
            v = rng.uniform(0.7, 1.3, n)
        elif k.endswith((".linear.0.bias", ".linear.3.bias", ".linear.6.bias")):
            v = rng.uniform(-0.2, 0.2, n)
        else:
            fan = shape[-1] if len(shape) > 1 else 256
            v = rng.uniform(-1, 1, n) / np.sqrt(fan)
        params[k] = v.astype(np.float32).reshape(shape)
        flat[off:off + n] = torch.from_numpy(params[k]).reshape(-1)
    x = rng.randn(ROWS, H).astype(np.float32)
    dsig = (rng.randn(ROWS, A, 2, N) * 1e-3).astype(np.float32)
    x[FIRST_COPY:] = x[:COPIES]
    dsig[FIRST_COPY:] = dsig[:COPIES]
    flat_d, x_d, dsig_d = flat.to(dev), T_(x, dev), T_(dsig, dev)
    out = torch.full((ROWS, A, 2, N), float("nan"), device=dev)
    ws = torch.full((L.as_head_workspace_floats(C.byref(dims), ROWS),), float("nan"), device=dev)
    _lib.check(L.as_head_fwd(C.byref(dims), C.byref(lay), _lib.ptr(flat_d), _lib.ptr(x_d), ROWS, _lib.ptr(out), _lib.ptr(ws), 1, _lib.stream_ptr()))
    G = torch.zeros_like(flat_d)
    dx = torch.full((ROWS, H), float("nan"), device=dev)
    _lib.check(L.as_head_bwd(C.byref(dims), C.byref(lay), _lib.ptr(flat_d), _lib.ptr(out), _lib.ptr(dsig_d), ROWS, _lib.ptr(dx), _lib.ptr(G),
                             _lib.ptr(ws), _lib.stream_ptr()))
    torch.cuda.synchronize()
    out_h, dx_h, G_h = out.cpu().numpy(), dx.cpu().numpy(), G.cpu().numpy()
    assert np.isfinite(out_h).all() and np.isfinite(dx_h).all() and np.isfinite(G_h).all()
    n_out = int((out_h[FIRST_COPY:].view(np.uint32) != out_h[:COPIES].view(np.uint32)).sum())
    n_dx = int((dx_h[FIRST_COPY:].view(np.uint32) != dx_h[:COPIES].view(np.uint32)).sum())
    print(f"H={H} N={N}: elements that differ between a row and its copy: out {n_out} of {COPIES * A * 2 * N}, dx {n_dx} of {COPIES * H}")
    assert n_out == 0, f"{n_out} contour values differ between rows 0-76 (64-row tiles) and their copies"
    assert n_dx == 0, f"{n_dx} input-gradient values differ between rows 0-76 (64-row tiles) and their copies"
    for a in range(A):
        p = {k[len(f"predictors.{a}."):]: v.astype(np.float64) for k, v in params.items() if k.startswith(f"predictors.{a}.")}
        pre, _ = O.predictor_fwd(x[:COPIES].astype(np.float64), p)
        assert_close(out_h[:COPIES, a], 1 / (1 + np.exp(-pre)), what=f"H={H} N={N}: head {a} out")
