"""The row-contiguous criterion epilogue of the heads' output layer (csrc/lin_f32.hip: criterion_rows_f4, taken when
2 * n_samples is a multiple of 4 and out, d(out) and the targets are 16-byte aligned) against the point-per-lane epilogue it
replaces (criterion_rows), selected by as_set_lin_out_row_epilogue.

Both run the same expressions on the same operands for every point and add a lane's distances in the same frame order, so
TrainStep.forward_backward must leave the same `out`, `dout` and gradients BIT FOR BIT and the same loss with the switch off
and on -- in the split arithmetic (lin_out_s6_kernel, 4 waves) and in the exact one (lin_out_kernel, 8 waves).

Shape as test_gpu_train.py's criterion test: V = 45, A = 4, B = 8, lengths [T, 97, 64, 63, 40, 33, 8, 1] (clipped to T),
targets padded to T + 3 frames.

    n_samples  N    T
    50         100  101   the workload's row: 25 chunks; 808 frames per head = twelve 64-row tiles, a full and an 8-row 32-row tile
    64         128  101   the full column tile; the targets' half tile is exactly 16 KB
    2          4    40    one chunk per row
    6          12   33    N / 2 is no multiple of 4: the x | y boundary lies inside a chunk
    25         50   40    N % 4 != 0: the host declines, both runs take the old path

and at n_samples = 50: targets in a view offset by one float (the host declines; values equal the aligned run's), and
zero distances (out copied into the targets at a few valid points: NaNs in d(out) must match bit for bit)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, A, B = 45, 4, 8
CASES = [(50, 101), (64, 101), (2, 40), (6, 33), (25, 40)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture()
def switch():
    from artspeech_amd import _lib
    L = _lib.lib()
    yield L.as_set_lin_out_row_epilogue
    L.as_set_lin_out_row_epilogue(1)


@pytest.fixture(params=[1, 0], ids=["split", "exact_fp32"])
def matrix_arith(request):
    """both matrix arithmetics; the default (1 = split) is restored afterwards"""
    from artspeech_amd import _lib
    L = _lib.lib()
    keep = L.as_get_matrix_arith()
    L.as_set_matrix_arith(request.param)
    yield request.param
    L.as_set_matrix_arith(keep)


def _problem(dev, n_samp, T):
    from artspeech_amd.engine import TrainStep
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech
    lengths = torch.tensor([T, 97, 64, 63, 40, 33, 8, 1], dtype=torch.int32).clamp(max=T)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(1, V, (B, T), generator=g)
    tgt = torch.rand(B, T + 3, A, 2, n_samp, generator=g)    # targets padded beyond T: tgt_T > T
    for b, l in enumerate(lengths):
        x[b, l:] = 0
    torch.manual_seed(2)
    model = ArtSpeech(V, A, n_samples=n_samp).to(dev)
    step = TrainStep(model, B, T, optimizer=False)
    assert step.fuse_loss
    scale = 1.0 / (float(lengths.sum()) * A * n_samp)
    return step, x.to(dev), lengths.to(dev), tgt.to(dev), scale


def _run(prob, switch, on, tgt=None):
    step, x, ld, tgt0, scale = prob
    switch(on)
    step.out.fill_(float("nan"))
    step.dout.fill_(float("nan"))
    step.forward_backward(x, ld, tgt0 if tgt is None else tgt, scale)
    torch.cuda.synchronize()
    return step.out.clone(), step.dout.clone(), step.grads.clone(), float(step.loss)


def _same(a, b, what):
    n = [int((p.view(torch.int32) != q.view(torch.int32)).sum()) for p, q in zip(a[:3], b[:3])]
    print(f"{what}: elements that differ: out {n[0]}, dout {n[1]}, gradients {n[2]}; loss {a[3]!r} | {b[3]!r}")
    assert torch.equal(a[0], b[0]), f"{what}: contours differ"
    assert torch.equal(a[1], b[1]), f"{what}: d loss / d(pre-sigmoid) differs"
    assert torch.equal(a[2], b[2]), f"{what}: gradients differ"
    assert a[3] == b[3], f"{what}: loss {a[3]!r} != {b[3]!r}"


@pytest.mark.parametrize("n_samp,T", CASES)
def test_row_epilogue_equals_the_point_per_lane_epilogue_bit_for_bit(dev, switch, matrix_arith, n_samp, T):
    prob = _problem(dev, n_samp, T)
    off = _run(prob, switch, 0)
    on = _run(prob, switch, 1)
    assert all(bool(torch.isfinite(r).all()) for r in off[:3]) and off[3] == off[3] and off[3] > 0
    _same(off, on, f"n_samples={n_samp} T={T} arith={matrix_arith}, switch off | on")


def test_targets_aligned_to_4_bytes_only_take_the_old_path(dev, switch, matrix_arith):
    prob = _problem(dev, 50, 101)
    tgt = prob[3]
    buf = torch.empty(tgt.numel() + 1, device=dev)
    view = buf[1:].view(tgt.shape)
    view.copy_(tgt)
    assert view.data_ptr() % 16 == 4 and tgt.data_ptr() % 16 == 0
    aligned = _run(prob, switch, 1)
    _same(aligned, _run(prob, switch, 0, view), "aligned targets, switch on | targets offset by one float, switch off")
    _same(aligned, _run(prob, switch, 1, view), "aligned targets, switch on | targets offset by one float, switch on")


def test_zero_distance_gives_the_same_nans(dev, switch, matrix_arith):
    prob = _problem(dev, 50, 101)
    out = _run(prob, switch, 0)[0]
    tgt = prob[3].clone()
    T = out.shape[1]
    # (utterance, frame, head, point): valid frames of several tiles, first and last point, both ends of an utterance
    spots = [(0, 0, 0, 0), (0, T - 1, 3, 49), (1, 96, 1, 24), (2, 63, 2, 25), (5, 32, 0, 7), (7, 0, 3, 49)]
    for b, t, a, p in spots:
        tgt[b, t, a, :, p] = out[b, t, a, :, p]
    off = _run(prob, switch, 0, tgt)
    on = _run(prob, switch, 1, tgt)
    for b, t, a, p in spots:
        assert bool(torch.isnan(off[1][b, t, a, :, p]).all()), "d(out) at zero distance is NaN, as torch autograd's"
    assert torch.equal(off[0], on[0]), "contours differ"
    assert torch.equal(off[1].view(torch.int32), on[1].view(torch.int32)), "d loss / d(pre-sigmoid) differs as bits"
    assert off[3] == on[3] and off[3] == off[3] and abs(off[3]) < float("inf"), (off[3], on[3])
