"""Training the DeepSpeech2 recogniser on the engine (train_phoneme_recognition.py): the CTC kernel against torch's own CTC in
float64, the convolution / LayerNorm parameter-gradient kernels, TrainableDeepSpeech2's gradients against the reference fixture
and an fp64 restatement (with and without dropout), its consistency with the frozen scorer, and the trainer end to end."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from conftest import ROOT, WORST, assert_grad_close, load_golden
from recognizer_fp64 import DeepSpeech2F64, engine_masks

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def _lib():
    from artspeech_amd import _lib
    return _lib


# --------------------------------------------------------------------------------------------------------------- CTC
def _ctc_case(B, T, C, L_max, seed, min_in=None, repeats=False, zero_len=False, blank=0, lengths=None):
    """repeats: True repeats the label pairs (2k, 2k+1), "across" the pairs (2k-1, 2k); blank: the class the labels avoid (labels
    then include class 0); lengths: the target lengths, instead of drawn ones."""
    g = torch.Generator().manual_seed(seed)
    tl = torch.randint(0 if zero_len else 1, L_max + 1, (B,), generator=g)
    if zero_len:
        tl[0] = 0
    tl[-1] = L_max
    if lengths is not None:
        tl = torch.tensor(lengths)
    tgts = torch.randint(1, C, (B, L_max), generator=g)
    if blank:   # the C - 1 classes other than blank
        tgts = tgts - 1
        tgts = tgts + (tgts >= blank)
    if repeats == "across":
        tgts[:, 2::2] = tgts[:, 1::2][:, : tgts[:, 2::2].shape[1]]
    elif repeats:
        tgts[:, 1::2] = tgts[:, 0::2][:, : tgts[:, 1::2].shape[1]]
    for b in range(B):
        tgts[b, tl[b]:] = -1
    need = torch.tensor([int(l) + int((tgts[b, 1:l] == tgts[b, : max(l - 1, 0)]).sum()) for b, l in enumerate(tl.tolist())])
    lo = need if min_in is None else torch.full((B,), min_in)
    il = torch.stack([torch.randint(int(min(lo[b], T)), T + 1, (1,), generator=g)[0] for b in range(B)])
    il[0] = T
    x = torch.randn(T, B, C, generator=g) * 2
    return x, tgts, il, tl


def _check_ctc(x32, tgts, il, tl, dev, reduction, zero_infinity, logits, one_d=False, permuted=False, label="", blank=0):
    from artspeech_amd.phoneme_recognition.ctc import ctc_loss
    T, B, C = x32.shape
    t_in = torch.cat([tgts[b, : tl[b]] for b in range(B)]) if one_d else tgts
    # float64 truth and torch's own float32 CPU result (the reference's CTC)
    res = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        xi = x32.to(dt).clone().requires_grad_(True)
        lp = F.log_softmax(xi, -1) if logits else xi
        loss = F.ctc_loss(lp, torch.cat([tgts[b, : tl[b]] for b in range(B)]), il, tl, blank, reduction, zero_infinity)
        (loss.sum() if reduction == "none" else loss).backward()
        res[name] = (loss.detach().double(), xi.grad.double())
    if permuted:   # the (T, B, C) view of a (B, T, C) tensor
        xd = x32.permute(1, 0, 2).contiguous().to(dev).requires_grad_(True)
        xv = xd.permute(1, 0, 2)
    else:
        xd = x32.to(dev).requires_grad_(True)
        xv = xd
    out = ctc_loss(xv, t_in.to(dev), il, tl, blank=blank, reduction=reduction, zero_infinity=zero_infinity, logits=logits)
    (out.sum() if reduction == "none" else out).backward()
    got_l, got_g = out.detach().double().cpu(), xd.grad.double().cpu()
    if permuted:
        got_g = got_g.permute(1, 0, 2)
    ref_l, ref_g = res["f64"]
    t32_l, t32_g = res["f32"]
    fin = torch.isfinite(ref_l)
    assert torch.equal(torch.isfinite(got_l), fin), (label, got_l, ref_l)
    assert torch.equal(torch.isnan(got_g), torch.isnan(ref_g)), label
    ok = ~torch.isnan(ref_g)
    for what, got, ref, t32 in (("loss", got_l[fin], ref_l[fin], t32_l[fin]), ("grad", got_g[ok], ref_g[ok], t32_g[ok])):
        if got.numel() == 0:
            continue
        scale = max(float(ref.abs().max()), 1e-30)
        err, err32 = float((got - ref).abs().max()), float((t32 - ref).abs().max())
        bound = 2 * err32 + 1e-6 * scale
        WORST[f"ctc {label} {what} / torch fp32"] = err / max(err32, 1e-30)
        assert err <= bound, f"{label} {what}: max err {err:.3e} > 2 x torch fp32's {err32:.3e} + 1e-6 * {scale:.3e}"
    return out, xd.grad


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("zero_infinity", [False, True])
@pytest.mark.parametrize("logits", [False, True])
def test_ctc_matches_torch_fp64(reduction, zero_infinity, logits, dev):
    x, tgts, il, tl = _ctc_case(6, 40, 12, 9, seed=1, repeats=True, zero_len=True)
    il[1] = 3   # an impossible alignment (target longer than the input)
    tl[1] = 7
    tgts[1, :7] = torch.arange(1, 8)
    _check_ctc(x, tgts, il, tl, dev, reduction, zero_infinity, logits, label=f"{reduction}/{zero_infinity}/{logits}")


@pytest.mark.parametrize("one_d,permuted", [(True, False), (False, True), (True, True)])
def test_ctc_target_forms_and_permuted_view(one_d, permuted, dev):
    x, tgts, il, tl = _ctc_case(5, 33, 9, 6, seed=2, repeats=True)
    _check_ctc(x, tgts, il, tl, dev, "mean", True, True, one_d=one_d, permuted=permuted, label=f"forms {one_d}/{permuted}")
    _check_ctc(x, tgts, il, tl, dev, "sum", False, False, one_d=one_d, permuted=permuted, label=f"forms lp {one_d}/{permuted}")


def test_ctc_thesis_batch_and_determinism(dev):
    from artspeech_amd.phoneme_recognition.ctc import ctc_loss
    x, tgts, il, tl = _ctc_case(32, 200, 45, 60, seed=3)
    _check_ctc(x, tgts, il, tl, dev, "mean", True, True, permuted=True, label="B32 T200")
    outs = []
    for _ in range(2):
        xd = x.to(dev).requires_grad_(True)
        loss = ctc_loss(xd, tgts.to(dev), il, tl, zero_infinity=True, logits=True)
        loss.backward()
        outs.append((loss.detach().cpu(), xd.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_ctc_long_targets_multi_wave_path(dev):
    x, tgts, il, tl = _ctc_case(2, 2100, 20, 1000, seed=4, min_in=2050)
    _check_ctc(x, tgts, il, tl, dev, "sum", True, True, label="L1000 T2100")


def test_ctc_past_the_limit_raises(dev):
    from artspeech_amd.phoneme_recognition.ctc import ctc_loss
    x = torch.randn(4200, 1, 5, device=dev)
    with pytest.raises(ValueError, match="exceeds"):
        ctc_loss(x, torch.ones(1, 2048, dtype=torch.long), [4200], [2048])


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("C", [2, 63, 64, 65, 130])
def test_ctc_class_widths_around_the_wave(C, logits, dev):
    """ctc_row_lse_kernel and ctc_grad_kernel stride the classes over 64 lanes: one partial pass, one whole, a second pass of one
    class, two whole passes and a third; C = 2 leaves one label, so every neighbouring pair is a repeat."""
    x, tgts, il, tl = _ctc_case(3, 12, C, 4, seed=10 + C)
    _check_ctc(x, tgts, il, tl, dev, "mean", False, logits, label=f"C={C} logits={logits}")


@pytest.mark.parametrize("one_d", [False, True])
@pytest.mark.parametrize("blank", [4, 2])
def test_ctc_blank_is_not_class_zero(blank, one_d, dev):
    x, tgts, il, tl = _ctc_case(4, 20, 5, 6, seed=20 + blank, repeats=True, blank=blank)
    tgts[-1, 2] = 0   # (the last utterance has all 6 labels)
    assert (tgts == 0).any() and not (tgts == blank).any()
    for logits in (False, True):
        _check_ctc(x, tgts, il, tl, dev, "sum", False, logits, one_d=one_d, label=f"blank={blank} 1-D={one_d} logits={logits}", blank=blank)


@pytest.mark.parametrize("repeats", [True, "across"])
@pytest.mark.parametrize("L", [127, 128])
def test_ctc_state_count_boundary_of_the_two_exchange_paths(L, repeats, dev):
    """S = 2 L + 1 = 255 states run in one wave of 4 states per thread (cross-lane shifts), 257 in 256 threads of 16 (LDS exchange).
    A repeat inside a label pair (2k, 2k+1) forbids a skip between two states of one thread; a repeat across pairs (2k-1, 2k) forbids
    the skip into a thread's first label state, whose r - 2 neighbour is the previous thread's."""
    x, tgts, il, tl = _ctc_case(4, 280, 20, L, seed=30 + L, repeats=repeats, lengths=[L, 0, 1, L])
    for b in (0, 3):   # the frames allow the alignment: il >= L + repeats
        n_rep = int((tgts[b, 1:L] == tgts[b, :L - 1]).sum())
        assert n_rep >= L // 2 - 1 and int(il[b]) >= L + n_rep
    _check_ctc(x, tgts, il, tl, dev, "mean", True, True, label=f"L={L} repeats={repeats}")
    if L == 128:
        _check_ctc(x, tgts, il, tl, dev, "sum", False, False, one_d=True, label=f"L={L} repeats={repeats} 1-D")


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_ctc_single_frame_and_no_frames(reduction, dev):
    g = torch.Generator().manual_seed(40)
    # one frame: the empty target and a single label
    x = torch.randn(1, 2, 6, generator=g) * 2
    tgts, il, tl = torch.tensor([[-1], [3]]), torch.tensor([1, 1]), torch.tensor([0, 1])
    # no frames: loss 0 for the empty target, +inf for a label, an all-zero gradient either way (torch's own result)
    x0 = torch.randn(5, 3, 6, generator=g) * 2
    tgts0, il0, tl0 = torch.tensor([[2, 4], [-1, -1], [5, -1]]), torch.tensor([5, 0, 0]), torch.tensor([2, 0, 1])
    for zero_infinity in (False, True):
        for logits in (False, True):
            label = f"{reduction}/{zero_infinity}/{logits}"
            _check_ctc(x, tgts, il, tl, dev, reduction, zero_infinity, logits, label="T=1 " + label)
            _, grad = _check_ctc(x0, tgts0, il0, tl0, dev, reduction, zero_infinity, logits, label="no frames " + label)
            assert not bool(grad[:, 1:].any())
    out, _ = _check_ctc(x0, tgts0, il0, tl0, dev, "none", False, False, one_d=True, label="no frames 1-D")
    assert out[1].item() == 0.0 and out[2].item() == float("inf")


@pytest.mark.parametrize("zero_infinity", [False, True])
def test_ctc_forbidden_label(zero_infinity, dev):
    """A label of utterance 1 has log-probability -inf on every frame: its loss is +inf and its in-length gradient rows are NaN
    (torch's), or 0 and exact zeros with zero_infinity; the other utterances are unaffected.  Log-probability input only: with
    -inf among raw scores torch's log-softmax backward spreads the NaN over the whole row and the fused kernel does not, so no
    pattern is asserted in logits mode."""
    x, tgts, il, tl = _ctc_case(3, 15, 7, 4, seed=50)
    tl[1], il[1] = 3, 11
    tgts[1] = torch.tensor([2, 5, 3, -1])
    x[:, 1, 5] = float("-inf")
    out, grad = _check_ctc(x, tgts, il, tl, dev, "none", zero_infinity, False, label=f"forbidden label zi={zero_infinity}")
    if zero_infinity:
        assert out[1].item() == 0.0 and not bool(grad[:, 1].any())
    else:
        assert out[1].item() == float("inf") and bool(torch.isnan(grad[:11, 1]).all()) and not bool(grad[11:, 1].any())
    assert bool(torch.isfinite(out[[0, 2]]).all()) and bool(torch.isfinite(grad[:, [0, 2]]).all())


@pytest.mark.parametrize("L_max", [9, 140])   # both recursion kernels
def test_ctc_loss_without_gradient_is_the_same_loss(L_max, dev):
    """x.requires_grad = False runs the alpha recursion alone (with_beta = 0): bit-equal to the differentiable call's loss."""
    from artspeech_amd.phoneme_recognition.ctc import ctc_loss
    x, tgts, il, tl = _ctc_case(4, 300, 12, L_max, seed=60, repeats=True, zero_len=True)
    for logits in (False, True):
        xd = x.to(dev)
        plain = ctc_loss(xd, tgts.to(dev), il, tl, reduction="none", logits=logits)
        diff = ctc_loss(xd.clone().requires_grad_(True), tgts.to(dev), il, tl, reduction="none", logits=logits)
        assert not plain.requires_grad and diff.requires_grad
        assert torch.equal(plain, diff.detach()), (plain, diff)


# ------------------------------------------------------------------------------------- convolution / LN parameter gradients
def _slab(dev):
    from artspeech_amd.phoneme_recognition.deepspeech2 import _slab
    return _slab(dev)


@pytest.mark.parametrize("B,T,D", [(1, 1, 3), (2, 5, 7), (3, 17, 13), (32, 200, 80)])
def test_conv3x3_c32_wgrad_matches_fp64(B, T, D, dev):
    L, lib = _lib(), _lib().lib()
    g = torch.Generator().manual_seed(B * 100 + T + D)
    x, dy = torch.randn(B, T, D, 32, generator=g), torch.randn(B, T, D, 32, generator=g)
    dw, db = torch.empty(9, 32, 32, device=dev), torch.empty(32, device=dev)
    slab = _slab(dev)
    xd, dyd = x.to(dev), dy.to(dev)
    runs = []
    for _ in range(2):
        L.check(lib.as_conv3x3_c32_wgrad(L.ptr(xd), L.ptr(dyd), L.ptr(dw), L.ptr(db), B, T, D, L.ptr(slab), slab.numel(), L.stream_ptr()))
        runs.append((dw.cpu().clone(), db.cpu().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # fp64 truth on the reference layout (B, C, D, T); bound: 1e-6 * sum |x dy| over each element's terms
    xr, dyr = x.double().permute(0, 3, 2, 1), dy.double().permute(0, 3, 2, 1)
    w = torch.zeros(32, 32, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w, padding=1).mul(dyr).sum().backward()
    wa = torch.zeros(32, 32, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr.abs(), wa, padding=1).mul(dyr.abs()).sum().backward()
    got = runs[0][0].double().view(3, 3, 32, 32).permute(2, 3, 0, 1)
    assert ((got - w.grad).abs() <= 1e-6 * wa.grad + 1e-30).all(), float(((got - w.grad).abs() / wa.grad).max())
    ref_b = dyr.sum(dim=(0, 2, 3))
    assert ((runs[0][1].double() - ref_b).abs() <= 1e-6 * dyr.abs().sum(dim=(0, 2, 3))).all()


@pytest.mark.parametrize("Cin", [1, 2, 3, 4])
@pytest.mark.parametrize("B,T,D", [(1, 1, 5), (3, 11, 9), (32, 200, 80)])
def test_conv3x3_stem_wgrad_with_strided_planes(Cin, B, T, D, dev):
    L, lib = _lib(), _lib().lib()
    g = torch.Generator().manual_seed(Cin * 7 + B + T + D)
    big = torch.randn(B, Cin, T, D + 3, generator=g)   # (B, C, T, D) rows of a wider buffer: strides (C T (D+3), T (D+3), 1, D+3)
    x = big[..., :D]
    dy = torch.randn(B, T, D, 32, generator=g)
    xd = big.to(dev)
    strides = (Cin * T * (D + 3), T * (D + 3), 1, D + 3)
    dw, db = torch.empty(9, 32, Cin, device=dev), torch.empty(32, device=dev)
    slab = _slab(dev)
    dyd = dy.to(dev)
    L.check(lib.as_conv3x3_stem_wgrad(L.ptr(xd), *strides, L.ptr(dyd), L.ptr(dw), L.ptr(db), B, T, D, Cin, L.ptr(slab),
                                      slab.numel(), L.stream_ptr()))
    xr, dyr = x.double().transpose(2, 3), dy.double().permute(0, 3, 2, 1)   # (B, Cin, D, T), (B, 32, D, T)
    w = torch.zeros(32, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w, padding=1).mul(dyr).sum().backward()
    wa = torch.zeros(32, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr.abs(), wa, padding=1).mul(dyr.abs()).sum().backward()
    got = dw.cpu().double().view(3, 3, 32, Cin).permute(2, 3, 0, 1)
    assert ((got - w.grad).abs() <= 1e-6 * wa.grad + 1e-30).all()
    assert ((db.cpu().double() - dyr.sum(dim=(0, 2, 3))).abs() <= 1e-6 * dyr.abs().sum(dim=(0, 2, 3))).all()


@pytest.mark.parametrize("D", [5, 80, 200])
def test_ln_param_grads_match_fp64(D, dev):
    L, lib = _lib(), _lib().lib()
    g = torch.Generator().manual_seed(D)
    rows = 300
    x, dy = torch.randn(rows, D, 32, generator=g), torch.randn(rows, D, 32, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    dg, dbt = torch.empty(D, device=dev), torch.empty(D, device=dev)
    slab = _slab(dev)
    xd, gd, bd, dyd = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)   # (held: bare pointers below)
    L.check(lib.as_ln_feat_gelu_param_grad(L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(dyd), rows, D, 32, L.ptr(dg), L.ptr(dbt), L.ptr(slab),
                                           slab.numel(), L.stream_ptr()))
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.gelu(F.layer_norm(x.double().transpose(1, 2), (D,), g64, b64, 1e-5)).transpose(1, 2)
    (y * dy.double()).sum().backward()
    assert_grad_close(dg.cpu(), g64.grad, f"ln_feat dgamma D={D}", rtol=1e-4, atol_frac=1e-5)
    assert_grad_close(dbt.cpu(), b64.grad, f"ln_feat dbeta D={D}", rtol=1e-4, atol_frac=1e-5)
    # row LayerNorm from a saved xhat
    xh, dz = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    dzd, xhd = dz.to(dev), xh.to(dev)
    L.check(lib.as_layernorm_param_grad(L.ptr(dzd), L.ptr(xhd), rows, D, L.ptr(dg), L.ptr(dbt), L.ptr(slab), slab.numel(), L.stream_ptr()))
    assert_grad_close(dg.cpu(), (dz.double() * xh.double()).sum(0), f"row LN dgamma D={D}")
    assert_grad_close(dbt.cpu(), dz.double().sum(0), f"row LN dbeta D={D}")


# ------------------------------------------------------------------------------------------------------------- the model
CFG_SMALL = dict(in_channels=2, num_residual_layers=2, num_rnn_layers=2, rnn_hidden_size=16, num_classes=9, num_features=12,
                 adapter_out_features=10)
CFG_THESIS = dict(in_channels=2, num_residual_layers=4, num_rnn_layers=2, rnn_hidden_size=64, num_classes=45, num_features=500,
                  adapter_out_features=80)


def _models(cfg, seed, dropout, dev):
    from artspeech_amd.phoneme_recognition import TrainableDeepSpeech2
    torch.manual_seed(seed)
    m = TrainableDeepSpeech2(dropout=dropout, **cfg)
    with torch.no_grad():   # non-trivial LayerNorm affines
        for n, p in m.named_parameters():
            if "layer_norm" in n or "adapter.adapter.0" in n or "adapter.adapter.2" in n:
                p.add_(0.1 * torch.randn(p.shape))
    ref = DeepSpeech2F64(dropout=dropout, **cfg)
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    return m.to(dev), ref


def _batch(cfg, B, T, seed, voiced=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg["in_channels"], cfg["num_features"], T, generator=g)
    v = (torch.rand(B, T, generator=g) > 0.5).float() if voiced else None
    C = cfg["num_classes"]
    tl = torch.randint(1, max(2, T // 3), (B,), generator=g)
    tg = torch.randint(1, C, (B, int(tl.max())), generator=g)
    for b in range(B):
        tg[b, tl[b]:] = -1
    il = torch.randint(max(1, T - 3), T + 1, (B,), generator=g)
    il[0] = T
    return x, v, tg, il, tl


def _engine_step(m, x, v, tg, il, tl, dev, x_grad=False):
    from artspeech_amd.phoneme_recognition import CTCLoss
    xd = x.to(dev).requires_grad_(x_grad)
    m.zero_grad(set_to_none=True)
    logits = m(xd, v.to(dev) if v is not None else None)
    loss = CTCLoss(zero_infinity=True)(F.log_softmax(logits, -1).permute(1, 0, 2), tg.to(dev), il, tl)
    loss.backward()
    grads = {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}
    return logits.detach().cpu().double(), loss.item(), grads, (xd.grad.cpu() if x_grad else None)


def _ref_step(ref, x, v, tg, il, tl, masks=None):
    ref.zero_grad(set_to_none=True)
    logits, _ = ref(x.double(), v.double() if v is not None else None, masks)
    loss = F.ctc_loss(F.log_softmax(logits, -1).permute(1, 0, 2), tg, il, tl, zero_infinity=True)
    loss.backward()
    return logits.detach(), loss.item(), {n: p.grad for n, p in ref.named_parameters()}


def _compare(got, ref, label):
    lg, ll, gg = got[:3]
    lr, lref, gr = ref[:3]
    assert_grad_close(lg, lr, f"{label} logits", rtol=1e-4, atol_frac=1e-5)
    assert abs(ll - lref) <= 1e-4 * abs(lref) + 1e-6, (label, ll, lref)
    assert set(gg) == set(gr)
    # absolute floor: 1e-6 of the largest gradient of the model.  The biases of every cnn1 have an exactly zero gradient in exact
    # arithmetic (the feature-axis LayerNorm behind them removes a per-channel constant), so fp32 rounding is all they get
    floor = 1e-6 * max(float(v.abs().max()) for v in gr.values())
    for n in gr:
        assert_grad_close(gg[n], gr[n], f"{label} {n}", rtol=1e-3, atol_frac=1e-4, atol_abs=floor)


@pytest.mark.parametrize("seed,B,T,voiced", [(0, 3, 11, True), (1, 2, 7, False), (2, 4, 16, True)])
def test_trainable_model_gradients_match_fp64(seed, B, T, voiced, dev):
    m, ref = _models(CFG_SMALL, seed, 0.0, dev)
    m.train()
    batch = _batch(CFG_SMALL, B, T, seed, voiced)
    _compare(_engine_step(m, *batch, dev), _ref_step(ref, *batch), f"small seed {seed}")


def test_trainable_model_without_adapter_matches_fp64(dev):
    cfg = dict(CFG_SMALL, adapter_out_features=None, in_channels=1)
    m, ref = _models(cfg, 5, 0.0, dev)
    m.train()
    batch = _batch(cfg, 2, 9, 5)
    _compare(_engine_step(m, *batch, dev), _ref_step(ref, *batch), "no adapter")


def test_trainable_model_thesis_size_matches_fp64(dev):
    m, ref = _models(CFG_THESIS, 7, 0.0, dev)
    m.train()
    batch = _batch(CFG_THESIS, 2, 40, 7)
    _compare(_engine_step(m, *batch, dev), _ref_step(ref, *batch), "thesis")


def test_dropout_masks_follow_the_seed_rule(dev):
    m, ref = _models(CFG_SMALL, 11, 0.1, dev)
    m.train()
    x, v, tg, il, tl = _batch(CFG_SMALL, 3, 13, 11)
    got = _engine_step(m, x, v, tg, il, tl, dev)
    masks = engine_masks(m, m.last_dropout_seed, 3, 13, dev)
    _compare(got, _ref_step(ref, x, v, tg, il, tl, masks), "dropout")
    kept = torch.cat([(mk != 0).double().flatten() for mk in masks.values()])
    big = _lib().lib()
    ones = torch.ones(1 << 20, device=dev)
    from artspeech_amd.phoneme_recognition.deepspeech2 import _dropout
    frac = float((_dropout(ones, (0.1, 12345), 0, torch.empty_like(ones)) != 0).float().mean())
    assert abs(frac - 0.9) < 0.003 and abs(float(kept.mean()) - 0.9) < 0.05, (frac, float(kept.mean()))
    # under no_grad, train mode still drops (as nn.Dropout does); eval does not
    with torch.no_grad():
        a = m(x.to(dev), v.to(dev))
        m.eval()
        b1, b2 = m(x.to(dev), v.to(dev)), m(x.to(dev), v.to(dev))
    assert not torch.equal(a, b1) and torch.equal(b1, b2)


def test_consistency_with_the_frozen_scorer(dev):
    from artspeech_amd.phoneme_recognition import DeepSpeech2
    m, _ = _models(CFG_THESIS, 3, 0.0, dev)
    frozen = DeepSpeech2(**CFG_THESIS).to(dev)
    frozen.load_state_dict(m.state_dict())
    frozen.eval()
    for p in frozen.parameters():
        p.requires_grad_(False)
    x, v, tg, il, tl = _batch(CFG_THESIS, 2, 30, 3)
    xd, vd = x.to(dev), v.to(dev)
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(xd, vd), frozen(xd, vd))
    # grad path forward values and dx: bitwise the frozen scorer's input gradient (dropout off)
    gl = torch.randn(2, 30, 45, device=dev)
    m.train()
    x1 = xd.clone().requires_grad_(True)
    out1 = m(x1, vd)
    (out1 * gl).sum().backward()
    x2 = xd.clone().requires_grad_(True)
    out2 = frozen(x2, vd)
    (out2 * gl).sum().backward()
    assert torch.equal(out1, out2) and torch.equal(x1.grad, x2.grad)
    # gradients are the same under both matrix arithmetics, and repeat bit for bit
    lib = _lib().lib()
    grads = []
    try:
        for arith in (0, 1, 0):
            lib.as_set_matrix_arith(arith)
            m.zero_grad(set_to_none=True)
            (m(xd, vd) * gl).sum().backward()
            grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    finally:
        lib.as_set_matrix_arith(0)
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]) and torch.equal(grads[0][n], grads[2][n]), n


def test_trainable_model_matches_reference_fixture(dev):
    from artspeech_amd.phoneme_recognition import TrainableDeepSpeech2
    from artspeech_amd.phoneme_recognition.ctc import CTCLoss
    fx = load_golden("recognizer_training")
    cfg = json.loads(str(fx["config"]))
    m = TrainableDeepSpeech2(**cfg)
    sd = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    m.load_state_dict(sd)
    m.to(dev).train()
    x, v = torch.from_numpy(fx["x"]).to(dev), torch.from_numpy(fx["voicing"]).to(dev)
    tg, il, tl = torch.from_numpy(fx["targets"]), torch.from_numpy(fx["input_lengths"]), torch.from_numpy(fx["target_lengths"])
    logits = m(x, v)
    loss = CTCLoss(zero_infinity=True)(F.log_softmax(logits, -1).permute(1, 0, 2), tg.to(dev), il, tl)
    loss.backward()
    assert_grad_close(logits.detach().cpu(), fx["logits"], "fixture logits", rtol=1e-4, atol_frac=1e-5)
    assert abs(loss.item() - float(fx["loss"])) <= 1e-5 * abs(float(fx["loss"])), (loss.item(), float(fx["loss"]))
    floor = 1e-6 * max(float(np.abs(fx["grad/" + n]).max()) for n, _ in m.named_parameters())   # see _compare
    for n, p in m.named_parameters():
        assert_grad_close(p.grad.cpu(), fx["grad/" + n], f"fixture grad {n}", rtol=1e-3, atol_frac=1e-4, atol_abs=floor)
    # three steps of Adam(weight_decay) + CyclicLR.  Adam divides each gradient by its own running magnitude, so an element whose
    # gradient lies within fp32 noise of zero (below the gradient check's own bound: 1e-4 of its tensor's largest plus the floor
    # above) moves by up to ~lr per step in a direction the noise picks: those may differ by 3 lr after three steps.  Every other
    # element must agree to 1 % of one step
    lr = float(fx["lr"])
    m.load_state_dict(sd)
    opt = torch.optim.Adam(m.parameters(), lr=lr, weight_decay=float(fx["weight_decay"]))
    sched = torch.optim.lr_scheduler.CyclicLR(opt, base_lr=lr / 25, max_lr=lr, cycle_momentum=False)
    for _ in range(3):
        opt.zero_grad()
        logits = m(x, v)
        CTCLoss(zero_infinity=True)(F.log_softmax(logits, -1).permute(1, 0, 2), tg.to(dev), il, tl).backward()
        opt.step()
        sched.step()
    for n, p in m.named_parameters():
        d = (p.detach().cpu().double() - torch.from_numpy(fx["after/" + n]).double()).abs()
        g = torch.from_numpy(fx["grad/" + n]).double().abs()
        noise = g <= 1e-4 * float(g.max()) + floor
        assert float(d.max()) <= 3 * lr, (n, float(d.max()))
        worst = float(torch.cat([d[~noise], d.new_zeros(1)]).max())
        assert worst <= 0.01 * lr, (n, worst)


# ------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_learns_resumes_and_feeds_the_pc_trainer(dev, tmp_path):
    import train_phoneme_recognition as T
    from artspeech_amd.phoneme_recognition import DeepSpeech2, TrainableDeepSpeech2
    with open(os.path.join(ROOT, "configs", "train_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    # 40 epochs of 64 batches of 4; CyclicLR climbs from lr / 25 over its 2000-step half cycle, hence the large nominal lr
    cfg.update(num_epochs=40, train_seq_dict={"num_sentences": 256}, valid_seq_dict={"num_sentences": 16},
               test_seq_dict={"num_sentences": 8}, num_workers=0, results_dir=str(tmp_path), learning_rate=0.01, patience=40,
               synthetic={"min_len": 20, "max_len": 40})
    torch.manual_seed(0)
    out = T.main(**cfg)
    for f in ("best_model.pt", "last_model.pt", "checkpoint.pt", "info_test.json"):
        assert os.path.exists(tmp_path / f), f
    h = out["history"]
    first, last = h[0]["train"]["loss"], h[-1]["train"]["loss"]
    print("train loss by epoch", [round(e["train"]["loss"], 4) for e in h], "valid edit distance",
          [round(e["valid"]["edit_distance"], 4) for e in h])
    assert last < 0.5 * first, ("the training CTC loss should halve over 40 epochs", first, last)
    # the untrained model's validation edit distance, same data
    torch.manual_seed(0)
    untrained = TrainableDeepSpeech2(num_classes=45, **cfg["model_params"])
    best = TrainableDeepSpeech2(num_classes=45, **cfg["model_params"])
    best.load_state_dict(torch.load(tmp_path / "best_model.pt"))
    from artspeech_amd.phoneme_recognition.datasets import SyntheticPhonemeRecognitionDataset, collate_fn
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder
    from artspeech_amd.phoneme_recognition.metrics import EditDistance
    from artspeech_amd.phoneme_recognition import Feature, Target, run_test
    vocab = T.build_vocabulary(None, T.Criterion.CTC)
    ds = SyntheticPhonemeRecognitionDataset(8, vocab, seed=1, min_len=20, max_len=40)
    dl = torch.utils.data.DataLoader(ds, batch_size=4, collate_fn=lambda b: collate_fn(b, [Feature.VOCAL_TRACT]))
    metric = {"edit_distance": EditDistance(GreedyCTCDecoder(list(vocab), blank_token="<blank>"))}
    ed = [run_test(mm.to(dev), dl, metric, Target.CTC, feature=Feature.VOCAL_TRACT, device=dev)["edit_distance"]
          for mm in (untrained, best)]
    assert ed[1] < ed[0], ed
    # resume continues the epoch count
    cfg2 = dict(cfg, num_epochs=41)
    out2 = T.main(**cfg2, checkpoint_filepath=str(tmp_path / "checkpoint.pt"))
    assert [e["epoch"] for e in out2["history"]] == [41]
    # best_model.pt loads strictly into the frozen scorer the PC trainer builds from recognizer_filepath
    with open(os.path.join(ROOT, "configs", "train_pc_based_recognizer_synthetic.yaml")) as f:
        pc = yaml.safe_load(f)
    frozen = DeepSpeech2(num_classes=45, **pc["recognizer_params"])
    frozen.load_state_dict(torch.load(tmp_path / "best_model.pt", map_location="cpu"), strict=True)
