"""The short-reduction head kernels (csrc/lin_f32.hip: lin_s6_lnf_shared_kernel for Linear 1 at H <= 128,
lin_s6_lnb_short_kernel for dx3) against the kernels they replace, selected by as_set_head_short_k.

Both routes issue, for every accumulator, the same matrix instructions on the same operands in the same order, so as_head_fwd +
as_head_bwd must give the same `out`, `dx` and gradient buffer BIT FOR BIT with the switch on and off.  Setup as
test_gpu_head_tiles.py: the split arithmetic, a NaN-filled workspace, non-trivial LayerNorm affines.

    rows = 333     32-row tiles only, ten whole ones and a ragged one of 13 rows; H in {32, 64, 96, 128} gives Linear 1 one to four
                   k-tiles, N in {8, 40, 50} gives dx3 one, three and four; A in {1, 3, 11}: one head per workgroup of Linear 1
    H = 160        Linear 1 on the old kernel with the switch in either position
    rows = 3021    the shape at which 64-row tiles first appear (dx3: 46 per head, then three of 32 rows, the last ragged;
                   Linear 1: 47 per head group + a ragged one of 32, ten groups, the last of two heads); rows 2944 + i are copies
                   of rows i and must agree bitwise with them, heads 0 and 10 have identical parameters and must give
                   identical contours; the forward is checked against the fp64 oracle
    rows = 6413    Linear 1 with two and three heads per workgroup (five groups)"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import T_, assert_close
from oracle import artspeech_oracle as O

pytestmark = pytest.mark.gpu

COPIES = 77          # the last COPIES rows of a problem with copies repeat its first COPIES rows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture()
def switch():
    from artspeech_amd import _lib
    L = _lib.lib()
    assert L.as_get_matrix_arith() == 1, "the split arithmetic is the library's default"
    yield L.as_set_head_short_k
    L.as_set_head_short_k(1)


def _problem(rows, A, H, N, copies=False, equal_heads=False):
    from artspeech_amd import _lib
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import _build_views, _numel
    dims = _lib.Dims(1, A, 1, H, N, 1)
    lay = _lib.layout(dims)
    rng = np.random.RandomState(7)
    views = {k: v for k, v in _build_views(dims, lay).items() if k.startswith("predictors.")}
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
    if equal_heads:
        for k in list(params):
            if k.startswith(f"predictors.{A - 1}."):
                params[k] = params["predictors.0." + k[len(f"predictors.{A - 1}."):]].copy()
    flat = torch.zeros(lay.total)
    for k, (off, shape) in views.items():
        flat[off:off + _numel(shape)] = torch.from_numpy(params[k]).reshape(-1)
    x = rng.randn(rows, H).astype(np.float32)
    dsig = (rng.randn(rows, A, 2, N) * 1e-3).astype(np.float32)
    if copies:
        x[rows - COPIES:] = x[:COPIES]
        dsig[rows - COPIES:] = dsig[:COPIES]
    return dims, lay, params, flat, x, dsig


def _run(dev, prob, rows, A, H, N):
    from artspeech_amd import _lib
    L = _lib.lib()
    dims, lay, _, flat, x, dsig = prob
    flat_d, x_d, dsig_d = flat.to(dev), T_(x, dev), T_(dsig, dev)
    out = torch.full((rows, A, 2, N), float("nan"), device=dev)
    ws = torch.full((L.as_head_workspace_floats(C.byref(dims), rows),), float("nan"), device=dev)
    _lib.check(L.as_head_fwd(C.byref(dims), C.byref(lay), _lib.ptr(flat_d), _lib.ptr(x_d), rows, _lib.ptr(out), _lib.ptr(ws), 1, _lib.stream_ptr()))
    G = torch.zeros_like(flat_d)
    dx = torch.full((rows, H), float("nan"), device=dev)
    _lib.check(L.as_head_bwd(C.byref(dims), C.byref(lay), _lib.ptr(flat_d), _lib.ptr(out), _lib.ptr(dsig_d), rows, _lib.ptr(dx), _lib.ptr(G),
                             _lib.ptr(ws), _lib.stream_ptr()))
    torch.cuda.synchronize()
    res = out.cpu().numpy(), dx.cpu().numpy(), G.cpu().numpy()
    assert all(np.isfinite(r).all() for r in res)
    return res


def _differ(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def _on_off(dev, switch, rows, A, H, N, **kw):
    prob = _problem(rows, A, H, N, **kw)
    switch(1)
    on = _run(dev, prob, rows, A, H, N)
    switch(0)
    off = _run(dev, prob, rows, A, H, N)
    switch(1)
    n = [_differ(a, b) for a, b in zip(on, off)]
    print(f"rows={rows} A={A} H={H} N={N}: elements that differ between switch on and off: out {n[0]}, dx {n[1]}, gradients {n[2]}")
    assert n == [0, 0, 0], f"switch on and off differ in {n} elements of (out, dx, gradients)"
    return prob, on


@pytest.mark.parametrize("N", [50, 40, 8])
@pytest.mark.parametrize("H", [32, 64, 96, 128])
@pytest.mark.parametrize("A", [1, 3, 11])
def test_small_shapes_agree_bitwise_with_the_long_reduction_kernels(dev, switch, A, H, N):
    _on_off(dev, switch, 333, A, H, N)


@pytest.mark.parametrize("A", [3, 11])
def test_wider_trunk_takes_the_old_kernel_either_way(dev, switch, A):
    _on_off(dev, switch, 333, A, 160, 50)


@pytest.mark.parametrize("H,N", [(128, 50), (96, 40)])
def test_64_row_tiles_row_copies_and_equal_heads(dev, switch, H, N):
    rows, A = 3021, 11
    prob, (out, dx, _) = _on_off(dev, switch, rows, A, H, N, copies=True, equal_heads=True)
    n_out = _differ(out[rows - COPIES:], out[:COPIES])
    n_dx = _differ(dx[rows - COPIES:], dx[:COPIES])
    assert n_out == 0, f"{n_out} contour values differ between rows 0-76 and their copies"
    assert n_dx == 0, f"{n_dx} input-gradient values differ between rows 0-76 and their copies"
    n_eq = _differ(out[:, 0], out[:, A - 1])
    assert n_eq == 0, f"{n_eq} contour values differ between heads 0 and {A - 1}, which have identical parameters"
    if (H, N) == (128, 50):
        params, x = prob[2], prob[4]
        for a in range(A):
            p = {k[len(f"predictors.{a}."):]: v.astype(np.float64) for k, v in params.items() if k.startswith(f"predictors.{a}.")}
            pre, _ = O.predictor_fwd(x[:COPIES].astype(np.float64), p)
            assert_close(out[:COPIES, a], 1 / (1 + np.exp(-pre)), what=f"H={H} N={N}: head {a} out")


def test_linear_1_head_groups_of_two_and_three(dev, switch):
    """6413 rows (the benchmark's 6400 and a ragged tile): 101 row tiles x 5 groups of 2, 2, 2, 2 and 3 heads -- the smallest row
    count at which a workgroup of Linear 1 runs more than two heads over its image is 47 x 64; this is the size that is timed."""
    rows, A = 6413, 11
    _, (out, dx, _) = _on_off(dev, switch, rows, A, 128, 50, copies=True, equal_heads=True)
    assert _differ(out[rows - COPIES:], out[:COPIES]) == 0
    assert _differ(dx[rows - COPIES:], dx[:COPIES]) == 0
    assert _differ(out[:, 0], out[:, A - 1]) == 0
