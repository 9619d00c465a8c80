"""Op-level checks of the fused attention kernels (csrc/attention.hip) and of the triangular GEMMs of their backward
against float64: masked and causal forwards at every key count the kernel rounds to a compiled key-block count, the two
dS kernels and the three backward routes, the causal detection of ops._key_major_mask, and model-level forwards whose
lengths fall in those key-block ranges.  Every batch has B >= 3 utterances with masks of their own, so that a mask read
at the wrong per-utterance offset shows in an interior utterance and in the last one."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import transformer_oracle as TO

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEG = float("-inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ops():
    from artspeech_amd.phoneme_to_articulation.transformer import ops
    return ops


def _L():
    from artspeech_amd import _lib
    return _lib, _lib.lib()


def _qkv(G, B, T, Tk, d, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randn(G, B * n, d, device=dev, generator=g) for n in (T, Tk, Tk))


def _general_mask(B, T, Tk, dev, seed):
    """(B, T, Tk): finite additive values with -inf entries, drawn per utterance; key 0 stays visible in every row"""
    g = torch.Generator(device=dev).manual_seed(seed)
    am = 0.25 * torch.randn(B, T, Tk, device=dev, generator=g).clamp(-2, 2)
    am.masked_fill_(torch.rand(B, T, Tk, device=dev, generator=g) < 0.3, NEG)
    am[:, :, 0] = 0.5 * torch.rand(B, T, device=dev, generator=g)
    return am


def _causal_mask(B, T, Tk, dev, seed):
    """(B, T, Tk): -inf for key > q, finite additive values (per utterance) on and below the diagonal"""
    g = torch.Generator(device=dev).manual_seed(seed)
    am = 0.25 * torch.randn(B, T, Tk, device=dev, generator=g).clamp(-2, 2)
    return am.masked_fill(torch.triu(torch.ones(T, Tk, dtype=torch.bool, device=dev), diagonal=1), NEG)


def _ragged_kpm(B, Tk, dev):
    """(B, Tk) key padding: utterance b keeps its first max(1, Tk - b Tk / (B + 1)) keys (key 0 is never padded)"""
    kpm = torch.zeros(B, Tk, device=dev)
    for b in range(B):
        kpm[b, max(1, Tk - b * Tk // (B + 1)):] = NEG
    return kpm


def _ref(Q, K, V, mask, kpm, B, h):
    """float64: ctx [G, B*T, d], P [Z, T, Tk], logsumexp [Z, T] (z = (g B + b) heads + head, the kernels' order)"""
    G, R, d = Q.shape
    T, Tk, dh = R // B, K.shape[1] // B, d // h
    q = Q.double().view(G, B, T, h, dh).permute(0, 1, 3, 2, 4)
    k = K.double().view(G, B, Tk, h, dh).permute(0, 1, 3, 2, 4)
    v = V.double().view(G, B, Tk, h, dh).permute(0, 1, 3, 2, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if mask is not None:
        s = s + mask.double()[None, :, None]
    if kpm is not None:
        s = s + kpm.double()[None, :, None, None]
    p = torch.softmax(s, -1)
    ctx = (p @ v).permute(0, 1, 3, 2, 4).reshape(G, B * T, d)
    Z = G * B * h
    return ctx, p.reshape(Z, T, Tk), torch.logsumexp(s, -1).reshape(Z, T)


def _key_major(mask, Tk, T, pad=3.0):
    """the C contract of as_attention_fwd: [B][Tk rounded up to 32][T], key-major, finite padding (here not 0, so that a
    padding row read in place of a real key shows)"""
    mt = torch.full((mask.shape[0], (Tk + 31) // 32 * 32, T), pad, device=mask.device)
    mt[:, :Tk] = mask.transpose(1, 2)
    return mt


def _fwd(Q, K, V, mt, kpm, B, h, causal=False):
    """as_attention_fwd(_causal) through the C entry point: (ctx, probs_t [Z][Tk][Tp], lse [Z][T]), outputs NaN-prefilled"""
    _lib, L = _L()
    G, R, d = Q.shape
    T, Tk = R // B, K.shape[1] // B
    Z, Tp = G * B * h, (T + 31) // 32 * 32
    out = torch.full_like(Q, NAN)
    pt = torch.full((Z, Tk, Tp), NAN, device=Q.device)
    lse = torch.full((Z, T), NAN, device=Q.device)
    fn = L.as_attention_fwd_causal if causal else L.as_attention_fwd
    _lib.check(fn(_lib.ptr(Q), _lib.ptr(K), _lib.ptr(V), _lib.ptr(mt), _lib.ptr(kpm), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(pt), G, B, h,
                  T, Tk, d, 1.0 / math.sqrt(d // h), _lib.stream_ptr()), "as_attention_fwd")
    torch.cuda.synchronize()
    return out, pt, lse


def _same(a, b):
    """bit-for-bit up to the NaN payload: NaN at the same places, equal values elsewhere"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, 0.0), torch.nan_to_num(b, 0.0))


def _close(got, ref, tol, what, scale=None):
    scale = ref.abs().max().item() if scale is None else scale
    err = (got.double() - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: max|err| {err:.3e} > {tol} x {scale:.3e}"


def _check_fwd(out, pt, lse, ref, T, Tk, what):
    ctx64, p64, lse64 = ref
    _close(out, ctx64, 1e-5, f"{what}: ctx")
    _close(pt[:, :Tk, :T], p64.transpose(1, 2), 1e-5, f"{what}: probs_t")
    if lse is not None:
        _close(lse, lse64, 1e-5, f"{what}: lse")
    assert torch.isnan(pt[:, :, T:]).all(), f"{what}: probs_t columns beyond T written"


# --- a. masked forward at every key-block count --------------------------------------------------------------------------
# attn_with_shape (attention.hip) rounds nb = ceil(Tk / 32) up to a compiled NB in {1, 2, 4, 6, 7, 8}: these Tk give nb = NB for every NB and
# nb < NB for the two rounded ones (nb = 3 -> 4: Tk 65-96, nb = 5 -> 6: Tk 129-160), at every head width
_TKS = [1, 31, 32, 33, 64, 65, 80, 96, 97, 128, 129, 150, 160, 161, 192, 193, 224, 225, 255, 256]
_DHS = (16, 32, 64)
_MASKED = ([(Tk, Tk, dh) for Tk in _TKS for dh in _DHS]
           + [(Tk * 5 // 7 + 3, Tk, _DHS[i % 3]) for i, Tk in enumerate(_TKS)]
           + [(Tk * 5 // 7 + 3, Tk, dh) for i, Tk in enumerate(_TKS) if Tk in (80, 150) for dh in _DHS if dh != _DHS[i % 3]])


@pytest.mark.parametrize("T,Tk,dh", _MASKED)
def test_masked_forward_every_key_count(dev, T, Tk, dh):
    """as_attention_fwd with {general additive mask, none} x {ragged key padding, none}: ctx, the key-major probabilities and
    the log-sum-exp against float64; ops.attention_forward (its own key-major copy of the mask) gives the same bits."""
    ops = _ops()
    G, B, h = 2, 3, 2
    d = dh * h
    Q, K, V = _qkv(G, B, T, Tk, d, dev, seed=1000 * Tk + T + dh)
    am = _general_mask(B, T, Tk, dev, seed=Tk + 7 * T)
    kp = _ragged_kpm(B, Tk, dev)
    for mask, kpm in ((am, kp), (am, None), (None, kp), (None, None)):
        what = f"T={T} Tk={Tk} dh={dh} mask={mask is not None} kpm={kpm is not None}"
        out, pt, lse = _fwd(Q, K, V, _key_major(mask, Tk, T) if mask is not None else None, kpm, B, h)
        _check_fwd(out, pt, lse, _ref(Q, K, V, mask, kpm, B, h), T, Tk, what)
        o2, saved, _, causal = ops.attention_forward(Q, K, V, mask, kpm, B, h, True)
        assert len(saved) == 5 and not causal, what
        assert _same(o2, out) and _same(saved[3][:, :, :T], pt[:, :, :T]), f"{what}: ops.attention_forward"


# --- b. causal forward ---------------------------------------------------------------------------------------------------
_CAUSAL = ([(T, T, dh) for T in (1, 2, 31, 33, 64, 65, 80, 100, 128, 150, 161, 200, 224, 256) for dh in _DHS]
           + [(300, 256, 64), (257, 200, 16), (40, 256, 32), (5, 70, 64), (100, 33, 16)])


@pytest.mark.parametrize("T,Tk,dh", _CAUSAL)
def test_causal_forward(dev, T, Tk, dh):
    """as_attention_fwd_causal (key blocks beyond a strip's own skipped, strips dealt over the waves; at T > 256 the plain
    strip loop) under a triu(1) mask with finite values below the diagonal and ragged key padding: against float64, exact
    zeros above the diagonal, bit-identical to as_attention_fwd, and what ops.attention_forward detects and runs."""
    ops = _ops()
    G, B, h = 1, 3, 2
    d = dh * h
    Q, K, V = _qkv(G, B, T, Tk, d, dev, seed=31 * T + Tk + dh)
    am = _causal_mask(B, T, Tk, dev, seed=T + Tk)
    kpm = _ragged_kpm(B, Tk, dev)
    mt = _key_major(am, Tk, T)
    what = f"T={T} Tk={Tk} dh={dh}"
    out, pt, lse = _fwd(Q, K, V, mt, kpm, B, h, causal=True)
    _check_fwd(out, pt, lse, _ref(Q, K, V, am, kpm, B, h), T, Tk, what)
    above = torch.triu(torch.ones(T, Tk, dtype=torch.bool, device=dev), diagonal=1).t()   # [key][q]: q < key
    assert (pt[:, :Tk, :T][:, above] == 0).all(), f"{what}: probs_t above the diagonal"
    o_g, pt_g, lse_g = _fwd(Q, K, V, mt, kpm, B, h, causal=False)
    assert torch.equal(out, o_g) and _same(pt, pt_g) and torch.equal(lse, lse_g), f"{what}: causal != general"
    if T > 1:
        o2, saved, _, causal = ops.attention_forward(Q, K, V, am, kpm, B, h, True)
        assert causal and torch.equal(o2, out) and torch.equal(saved[3][:, :, :T], pt[:, :, :T]), f"{what}: ops.attention_forward"


@pytest.mark.parametrize("T,dh", [(80, 32), (150, 64), (33, 16)])
def test_causal_forward_fully_masked_query(dev, T, dh):
    """key padding that hides key 0 of utterance 1 under a causal mask: exactly that utterance's query 0 has no visible key
    -- NaN in both entry points (PyTorch semantics), in every head and channel group, and nowhere else."""
    G, B, h = 2, 3, 2
    d = dh * h
    Q, K, V = _qkv(G, B, T, T, d, dev, seed=T + dh)
    am = _causal_mask(B, T, T, dev, seed=T)
    kpm = _ragged_kpm(B, T, dev)
    kpm[1, 0] = NEG
    mt = _key_major(am, T, T)
    expect = torch.zeros(G, B, T, d, dtype=torch.bool, device=dev)
    expect[:, 1, 0] = True
    for causal in (True, False):
        out, _, _ = _fwd(Q, K, V, mt, kpm, B, h, causal=causal)
        assert torch.equal(torch.isnan(out.view(G, B, T, d)), expect), f"causal={causal}"


# --- c. backward ---------------------------------------------------------------------------------------------------------
def _ds_ref(Q, K, V, mask, kpm, B, h, dctx):
    """float64 dS^T [Z][Tk][T] = (P o (dctx V^T - D) * scale)^T, D[q] = sum_c dctx[q][c] ctx[q][c] over the head's columns"""
    G, R, d = Q.shape
    T, Tk, dh = R // B, K.shape[1] // B, d // h
    ctx, p, _ = _ref(Q, K, V, mask, kpm, B, h)
    go = dctx.double().view(G, B, T, h, dh).permute(0, 1, 3, 2, 4).reshape(-1, T, dh)
    v = V.double().view(G, B, Tk, h, dh).permute(0, 1, 3, 2, 4).reshape(-1, Tk, dh)
    D = (go * ctx.view(G, B, T, h, dh).permute(0, 1, 3, 2, 4).reshape(-1, T, dh)).sum(-1)
    return (p * (go @ v.transpose(1, 2) - D[..., None]) / math.sqrt(dh)).transpose(1, 2)


@pytest.mark.parametrize("T,Tk,dh,causal", [(33, 33, 16, True), (80, 80, 32, True), (150, 150, 64, True), (200, 200, 64, True),
                                            (256, 256, 32, True), (40, 256, 16, True), (100, 33, 64, True), (300, 256, 32, True),
                                            (70, 150, 32, False), (96, 80, 64, False), (129, 129, 16, False)])
def test_ds_kernels(dev, T, Tk, dh, causal):
    """as_attention_bwd_ds(_causal) on the probabilities the forward left: against float64 P o (dctx V^T - D) scale, every
    element of [:Tk, :T] written, exact zeros for q < key under a causal mask (the causal kernel's empty pairs are zero-
    filled; the general kernel multiplies by P == 0).  At T > 256 the causal entry point falls back to the general kernel."""
    _lib, L = _L()
    G, B, h = 1, 3, 2
    d = dh * h
    Q, K, V = _qkv(G, B, T, Tk, d, dev, seed=T * 3 + Tk + dh)
    am = (_causal_mask if causal else _general_mask)(B, T, Tk, dev, seed=T + 5 * Tk)
    kpm = _ragged_kpm(B, Tk, dev)
    out, pt, _ = _fwd(Q, K, V, _key_major(am, Tk, T), kpm, B, h, causal=causal)
    dctx = torch.randn_like(Q)
    ref = _ds_ref(Q, K, V, am, kpm, B, h, dctx)
    above = torch.triu(torch.ones(T, Tk, dtype=torch.bool, device=dev), diagonal=1).t()
    for fn in ((L.as_attention_bwd_ds_causal, L.as_attention_bwd_ds) if causal else (L.as_attention_bwd_ds,)):
        ds = torch.full_like(pt, NAN)
        _lib.check(fn(_lib.ptr(V), _lib.ptr(dctx), _lib.ptr(out), _lib.ptr(pt), _lib.ptr(ds), G, B, h, T, Tk, d, 1.0 / math.sqrt(dh),
                      _lib.stream_ptr()), "as_attention_bwd_ds")
        torch.cuda.synchronize()
        got = ds[:, :Tk, :T]
        assert not torch.isnan(got).any(), fn.__name__
        _close(got, ref, 2e-5, f"{fn.__name__} T={T} Tk={Tk} dh={dh}")
        if causal:
            assert (got[:, above] == 0).all(), f"{fn.__name__}: dS^T above the diagonal"


_ROUTES = (("fused", True), ("unfused", False))


@pytest.mark.parametrize("T,Tk,dh,causal", [(80, 80, 32, True), (150, 150, 16, True), (200, 200, 64, True), (33, 33, 64, True),
                                            (300, 256, 32, True), (300, 300, 16, True), (70, 150, 64, False), (96, 80, 16, False),
                                            (129, 129, 32, False), (300, 513, 16, False), (64, 1024, 32, False), (257, 257, 64, True),
                                            (40, 700, 24, False)])
def test_attention_gradients_both_routes(dev, T, Tk, dh, causal):
    """(dQ, dK, dV) of ops.Attention against float64 autograd by the fused forward with the fused dS kernel and by the unfused
    forward and backward.  Where as_attention_supported says no -- Tk > 256 (every utterance longer than 256 frames:
    as_attn_softmax at NW = 8 and 16) or a head width outside {16, 32, 64} (dh = 24) -- both settings take the unfused route,
    the only one there is."""
    ops = _ops()
    _lib, L = _L()
    G, B, h = 1, 3, 2
    d = dh * h
    Q, K, V = _qkv(G, B, T, Tk, d, dev, seed=T + 11 * Tk + dh)
    am = (_causal_mask if causal else _general_mask)(B, T, Tk, dev, seed=2 * T + Tk)
    kpm = _ragged_kpm(B, Tk, dev)
    go = torch.randn_like(Q)
    Qd, Kd, Vd = (t.double().requires_grad_() for t in (Q, K, V))
    gref = torch.autograd.grad(_ref(Qd, Kd, Vd, am, kpm, B, h)[0], (Qd, Kd, Vd), go.double())
    fusable = bool(L.as_attention_supported(T, Tk, d, h))
    assert fusable == (Tk <= 256 and dh in (16, 32, 64))
    for route, fused_att in _ROUTES:
        ops.FUSED_ATTENTION = fused_att
        try:
            q, k, v = (t.clone().requires_grad_() for t in (Q, K, V))
            out = ops.Attention.apply(q, k, v, am, kpm, B, h)
            assert len(out.grad_fn.saved_tensors) == (5 if fused_att and fusable else 4), route
            assert out.grad_fn.causal == (causal and fused_att and fusable), route
            got = torch.autograd.grad(out, (q, k, v), go)
        finally:
            ops.FUSED_ATTENTION = True
        for name, a_, r_ in zip("QKV", got, gref):
            _close(a_, r_, 2e-5, f"{route} T={T} Tk={Tk} dh={dh}: d{name}")


def test_attention_forward_refuses_more_than_1024_keys(dev):
    """Tk = 1025 is beyond the unfused softmax's widest instantiation (16 values per lane): ops.attention_forward raises the
    library's error, which names the limit, instead of returning whatever the score buffer held"""
    ops = _ops()
    G, B, h, T, Tk, d = 1, 2, 2, 8, 1025, 32
    Q, K, V = _qkv(G, B, T, Tk, d, dev, seed=1)
    with pytest.raises(RuntimeError, match=r"as_attn_softmax.*1025 > 1024"):
        ops.attention_forward(Q, K, V, None, None, B, h, True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,Tk,dh,causal,fused", [(80, 80, 32, True, True), (70, 150, 64, False, True), (160, 160, 16, True, False)])
def test_attention_backward_into_nan_buffer_slices(dev, T, Tk, dh, causal, fused):
    """attention_backward with dQ / dK / dV handed in as slices of one NaN-filled buffer (what ChannelBlocks does) gives
    the same bits as with buffers of its own: every element is written, none read."""
    ops = _ops()
    G, B, h = 2, 3, 2
    d = dh * h
    Q, K, V = _qkv(G, B, T, Tk, d, dev, seed=T + Tk)
    am = (_causal_mask if causal else _general_mask)(B, T, Tk, dev, seed=T)
    kpm = _ragged_kpm(B, Tk, dev)
    dctx = torch.randn_like(Q)
    ops.FUSED_ATTENTION = fused
    try:
        _, saved, scale, c = ops.attention_forward(Q, K, V, am, kpm, B, h, True)
        fresh = ops.attention_backward(saved, B, h, scale, dctx, causal=c)
        nq, nk = Q.numel(), K.numel()
        buf = torch.full((nq + 2 * nk,), NAN, device=dev)
        into = ops.attention_backward(saved, B, h, scale, dctx, dQ=buf[:nq].view_as(Q), dK=buf[nq:nq + nk].view_as(K),
                                      dV=buf[nq + nk:].view_as(V), causal=c)
    finally:
        ops.FUSED_ATTENTION = True
    assert c == (causal and fused)
    for a_, b_ in zip(fresh, into):
        assert torch.equal(a_, b_)
    assert not torch.isnan(buf).any()


# --- d. triangular GEMMs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Tk,dh,Z", [(40, 256, 64, 7), (100, 160, 32, 5), (64, 200, 16, 3), (200, 200, 64, 2048)])
def test_gemm_triangular_rectangular_and_wrapping(dev, T, Tk, dh, Z):
    """as_gemm.k_tri on key-major operands P^T [Z][Tk][Tp] (zero for q < key, NaN in the row padding T..Tp that nobody
    writes) as the attention backward runs them: key tiles wholly beyond T (k_tri = 1: an empty reduction range, rows of
    exact zeros), and a batch whose work list wraps the persistent grid (the M-tile rotation).  Bit-identical to k_tri = 0,
    and against float64."""
    _lib, L = _L()
    g = torch.Generator(device=dev).manual_seed(T + Tk + Z)
    Tp = (T + 31) // 32 * 32
    pt = torch.rand(Z, Tk, Tp, device=dev, generator=g)
    pt[:, :, :T] *= torch.triu(torch.ones(Tk, T, device=dev))          # [key][q]: zero for q < key
    pt[:, :, T:] = NAN
    xq = torch.randn(Z, T, dh, device=dev, generator=g)
    xk = torch.randn(Z, Tk, dh, device=dev, generator=g)

    def run(k_tri, M, K, x, **kw):
        out = torch.full((Z, M, dh), NAN, device=dev)
        gm = _lib.Gemm()
        gm.A, gm.B, gm.C = pt.data_ptr(), x.data_ptr(), out.data_ptr()
        gm.M, gm.N, gm.K, gm.batch = M, dh, K, Z
        gm.b_j, gm.b_k, gm.ldc = 1, dh, dh
        gm.a_batch, gm.b_batch, gm.c_batch = Tk * Tp, K * dh, M * dh
        gm.k_tri = k_tri
        for key, val in kw.items():
            setattr(gm, key, val)
        _lib.check(L.as_gemm_f32(C.byref(gm), _lib.stream_ptr()), "as_gemm_f32")
        torch.cuda.synchronize()
        return out

    p64 = pt[:, :, :T].double()
    # rows = keys, reduction over q (dV = P^T dctx, dK = dS^T Q)
    full, tri = run(0, Tk, T, xq, a_i=Tp, a_k=1), run(1, Tk, T, xq, a_i=Tp, a_k=1)
    assert torch.equal(full, tri)
    assert (tri[:, T:] == 0).all()
    _close(tri, p64 @ xq.double(), 2e-5, "P^T x")
    # rows = queries, reduction over keys, A read through its transpose (dQ = dS K)
    full, tri = run(0, T, Tk, xk, a_i=1, a_k=Tp), run(2, T, Tk, xk, a_i=1, a_k=Tp)
    assert torch.equal(full, tri)
    _close(tri, p64.transpose(1, 2) @ xk.double(), 2e-5, "P x")


# --- e. causal detection -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,dh", [(80, 32), (150, 64), (256, 16)])
def test_near_causal_mask_takes_the_general_path(dev, T, dh):
    """-inf above the diagonal everywhere except ONE finite entry, in the last key block of one utterance: not causal (the
    skipping kernels would drop that key), and the forward and gradients match float64."""
    ops = _ops()
    G, B, h = 1, 3, 2
    d = dh * h
    Q, K, V = _qkv(G, B, T, T, d, dev, seed=T * 5 + dh)
    am = _causal_mask(B, T, T, dev, seed=T)
    am[2, 3, T - 1] = 1.5
    assert not ops._key_major_mask(am, T, T).causal
    q, k, v = (t.clone().requires_grad_() for t in (Q, K, V))
    out = ops.Attention.apply(q, k, v, am, None, B, h)
    assert not out.grad_fn.causal
    go = torch.randn_like(Q)
    got = torch.autograd.grad(out, (q, k, v), go)
    Qd, Kd, Vd = (t.double().requires_grad_() for t in (Q, K, V))
    ref = _ref(Qd, Kd, Vd, am, None, B, h)[0]
    _close(out.detach(), ref.detach(), 1e-5, "ctx")
    for name, a_, r_ in zip("QKV", got, torch.autograd.grad(ref, (Qd, Kd, Vd), go.double())):
        _close(a_, r_, 2e-5, f"d{name}")


def test_mask_edited_in_place_is_not_served_from_the_cache(dev):
    """The key-major copy and the causal flag are cached per mask tensor and version: an in-place edit after the first use
    (finite values changed below the diagonal; a key opened above it; then closed again) is seen by the next call."""
    ops = _ops()
    G, B, h, T, dh = 1, 3, 2, 80, 32
    d = dh * h
    Q, K, V = _qkv(G, B, T, T, d, dev, seed=80)
    am = _causal_mask(B, T, T, dev, seed=81)
    kpm = _ragged_kpm(B, T, dev)

    def check(expect_causal, what):
        with torch.no_grad():
            out, _, _, causal = ops.attention_forward(Q, K, V, am, kpm, B, h, False)
        assert causal == expect_causal, what
        _close(out, _ref(Q, K, V, am, kpm, B, h)[0], 1e-5, what)

    check(True, "causal")
    am[1] += 0.75 * torch.isfinite(am[1])           # values below the diagonal move
    check(True, "edited below the diagonal")
    am[2, 10, T - 5] = 0.0                          # a key above the diagonal opens
    check(False, "a key opened above the diagonal")
    am[2, 10, T - 5] = NEG                          # and closes again
    check(True, "closed again")


@pytest.mark.parametrize("Tk,causal", [(1, False), (70, True), (200, False)])
def test_single_query(dev, Tk, causal):
    """T = 1: one 32-query strip with a single live lane; with Tk = 1 there is nothing above the diagonal (not causal), with a
    triu(1) mask every key but key 0 is hidden.  Forward and gradients through ops.Attention against float64."""
    ops = _ops()
    G, B, h, T, dh = 2, 3, 2, 1, 32
    d = dh * h
    Q, K, V = _qkv(G, B, T, Tk, d, dev, seed=Tk)
    am = (_causal_mask if causal else _general_mask)(B, T, Tk, dev, seed=Tk + 1)
    kpm = _ragged_kpm(B, Tk, dev)
    q, k, v = (t.clone().requires_grad_() for t in (Q, K, V))
    out = ops.Attention.apply(q, k, v, am, kpm, B, h)
    assert out.grad_fn.causal == causal
    go = torch.randn_like(Q)
    got = torch.autograd.grad(out, (q, k, v), go)
    Qd, Kd, Vd = (t.double().requires_grad_() for t in (Q, K, V))
    ref = _ref(Qd, Kd, Vd, am, kpm, B, h)[0]
    _close(out.detach(), ref.detach(), 1e-5, "ctx")
    gref = torch.autograd.grad(ref, (Qd, Kd, Vd), go.double())
    # with a single visible key (Tk = 1, or the triu(1) mask) P == 1 and dQ, dK are exactly zero: what fp32 leaves there is the
    # rounding of dP - D, measured against the scale of the incoming gradient (that of dV = P^T dctx)
    floor = gref[2].abs().max().item()
    for name, a_, r_ in zip("QKV", got, gref):
        _close(a_, r_, 2e-5, f"d{name}", scale=r_.abs().max().item() or floor)


# --- f. model level ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,h,lens", [(64, 2, [80, 51, 13]), (64, 1, [80, 51, 13]), (64, 2, [150, 70]), (64, 1, [150, 70])])
def test_model_forward_in_rounded_key_block_ranges(dev, d, h, lens):
    """A small transformer (head widths 32 and 64) on ragged batches whose padded length (80: nb = 3, 150: nb = 5) is rounded
    up to a larger compiled key-block count: the collate function's causal masks through Attention and ChannelBlocks,
    against the fp64 oracle in both encoder modes."""
    from artspeech_amd.phoneme_to_articulation.transformer.models import ArtSpeechTransformer
    from artspeech_amd.phoneme_to_articulation.encoder_decoder.dataset import pad_sequence_transformer_collate_fn
    torch.manual_seed(d + h + len(lens))
    V, A, L, nf = 17, 3, 2, 20
    model = ArtSpeechTransformer(V, A, embed_dim=d, num_heads=h, num_layers=L, num_feat=nf)
    with torch.no_grad():  # non-trivial LayerNorm affines
        for k, v in model.named_views().items():
            if k.endswith("bias") and v.dim() == 1:
                v.uniform_(-0.2, 0.2)
    sd = {k: v.numpy().copy() for k, v in model.state_dict().items()}
    model = model.to(dev).eval()
    batch = [(f"s{i}", torch.randint(1, V, (l,)), torch.rand(l, A, 2, nf // 2), ["p"] * l, torch.rand(l, 1, 2, nf // 2),
              torch.tensor([], dtype=torch.int), list(range(l)), torch.zeros(l)) for i, l in enumerate(lens)]
    c = pad_sequence_transformer_collate_fn(batch)
    tokens, targets = c[1], c[2]
    B, T = tokens.shape
    shifted = torch.cat([torch.zeros(B, 1, A, nf), targets[:, 1:].reshape(B, T - 1, A, nf)], dim=1)
    for grad_mode in (False, True):
        model.set_encoder_grad_mode(grad_mode)
        out = model(tokens.to(dev), shifted.to(dev), src_key_padding_mask=c[8].to(dev), tgt_key_padding_mask=c[9].to(dev),
                    src_attn_mask=c[10].to(dev), tgt_attn_mask=c[11].to(dev))
        ref = TO.forward(sd, (V, A, d, h, L, nf), tokens.numpy(), shifted.numpy(), c[10].numpy(), c[11].numpy(), c[8].numpy(),
                         c[9].numpy(), grad_mode=grad_mode)
        err = np.abs(out.detach().cpu().numpy() - ref)
        assert (err <= 1e-4 * np.abs(ref) + 1e-6).all(), (grad_mode, err.max())
    model.set_encoder_grad_mode(None)
