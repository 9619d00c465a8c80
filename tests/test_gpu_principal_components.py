"""GPU parity of the RNNType switch (LSTM / GRU cells) and the principal-components recurrent model: outputs and every
parameter gradient against fixtures produced by the reference itself, larger cases against the numpy oracle, and the
backward at full size against a directional finite difference."""
import os

import numpy as np
import pytest
import torch

from conftest import assert_grad_close, load_golden, split_wg
from oracle import principal_components_oracle as PO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(V, comps, E, H, lstm, w, dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import PrincipalComponentsArtSpeech
    m = PrincipalComponentsArtSpeech(V, comps, embed_dim=E, hidden_size=H, rnn="lstm" if lstm else "gru")
    if w is not None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in w.items()}, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("name", ["pc_lstm_small", "pc_gru_small"])
def test_matches_reference_fixture_forward_and_gradients(name, dev):
    g = load_golden(name)
    w, grads = split_wg(g)
    V, E, H, latent, lstm = (int(v) for v in g["cfg"])
    comps = {f"a{i}": int(c) for i, c in enumerate(g["comps"])}
    m = _model(V, comps, E, H, lstm, w, dev)
    tokens = torch.from_numpy(g["tokens"]).to(dev)
    out = m(tokens, torch.from_numpy(g["lengths"]))
    assert out.shape == g["out"].shape
    assert np.abs(out.detach().cpu().numpy() - g["out"]).max() < 1e-5
    (out * torch.from_numpy(g["dout"]).to(dev)).sum().backward()
    for k, p in m.named_parameters():
        assert_grad_close(p.grad.cpu().numpy(), grads[k], f"{name}: {k}")
    with torch.no_grad():  # inference path (no saved gates) gives the same numbers
        assert torch.equal(m(tokens, g["lengths"].tolist()), out.detach())


@pytest.mark.parametrize("lstm,H,B,T", [(True, 128, 6, 37), (False, 128, 3, 20), (True, 64, 2, 5)])
def test_matches_oracle(lstm, H, B, T, dev):
    torch.manual_seed(H + T)
    comps = {"tongue": 6, "lower-lip": 4, "pharynx": 2}
    m = _model(29, comps, 64, H, lstm, None, dev)
    w = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    lengths = sorted(np.random.default_rng(T).integers(1, T + 1, B).tolist(), reverse=True)
    lengths[0] = T
    tokens = torch.randint(1, 29, (B, T))
    want = PO.forward(w, tokens.numpy(), lengths, lstm)
    with torch.no_grad():
        got = m(tokens.to(dev), lengths).cpu().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() < 2e-5


@pytest.mark.parametrize("seed", sorted(set(range(int(os.environ.get("AS_FUZZ_SEEDS", "10")))) | {93}))   # 93: ONE component (a one-row weight gradient)
def test_random_configurations_vs_oracle(seed, dev):
    """Seeded random principal-components models (LSTM or GRU cells, hidden 32 / 64 / 128, embedding widths 8-100, 1-4
    articulators with 1-12 components each, 1-7 utterances of 1-60 frames, ragged) against the numpy oracle
    (principal_components/models/rnn.py:58-109)."""
    r = np.random.RandomState(700 + seed)
    lstm, H, E, V = bool(r.randint(0, 2)), int(r.choice([32, 64, 128])), int(r.choice([8, 20, 64, 100])), int(r.randint(2, 60))
    _check_configuration(r, seed, lstm, H, E, V, dev)


@pytest.mark.parametrize("lstm", [True, False], ids=["lstm", "gru"])
@pytest.mark.parametrize("H", [20, 100, 260])
def test_any_hidden_size_vs_oracle(lstm, H, dev):
    """Hidden sizes outside {32, 64, 128} (nn.LSTM / nn.GRU take any): the plain recurrence kernels (`lstm_*_generic_kernel`
    in lstm.hip, `gru_*_generic_kernel` in gru.hip, their shared backward mat-vec in rnn_plain.h), forward and backward, against
    the same oracle and the same bounds."""
    r = np.random.RandomState(900 + H + int(lstm))
    _check_configuration(r, H, lstm, H, int(r.choice([8, 64])), int(r.randint(2, 60)), dev)


def _check_configuration(r, seed, lstm, H, E, V, dev):
    names = ["tongue", "lower-lip", "pharynx", "upper-lip"][:int(r.randint(1, 5))]
    comps = {n: int(r.randint(1, 13)) for n in names}
    B, T = int(r.randint(1, 8)), int(r.randint(1, 61))
    torch.manual_seed(seed)
    m = _model(V, comps, E, H, lstm, None, dev)
    w = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    lengths = sorted(r.randint(1, T + 1, B).tolist(), reverse=True)
    lengths[0] = T
    tokens = torch.from_numpy(r.randint(1, V, (B, T)) if V > 1 else np.zeros((B, T), np.int64))
    want = PO.forward(w, tokens.numpy(), lengths, lstm)
    out = m(tokens.to(dev), lengths)
    got = out.detach().cpu().numpy()
    what = (lstm, H, E, V, comps, B, T, lengths)
    assert got.shape == want.shape and np.abs(got - want).max() < 2e-5, what
    # backward (hand-written LSTM / GRU recurrences, trunk, predictor): <gradient, direction> against central differences of the
    # fp64 oracle along a random direction in parameter space (three step sizes, the nearest counts: a ReLU kink inside the step bends the quotient)
    wgt = torch.randn_like(out)
    (out * wgt).sum().backward()
    w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
    direction = {k: r.randn(*v.shape) * (np.abs(v).mean() + 1e-3) for k, v in w64.items()}
    analytic = sum(float((p.grad.cpu().numpy().astype(np.float64) * direction[k]).sum()) for k, p in m.named_parameters() if p.grad is not None)
    wg = wgt.cpu().numpy().astype(np.float64)

    def numeric_at(eps):
        f = lambda s: float((PO.forward({k: v + s * eps * direction[k] for k, v in w64.items()}, tokens.numpy(), lengths, lstm) * wg).sum())  # noqa: E731
        return (f(+1) - f(-1)) / (2 * eps)

    numeric = min((numeric_at(e) for e in (1e-6, 1e-7, 1e-8)), key=lambda v: abs(v - analytic))
    assert abs(analytic - numeric) <= 1e-3 * max(abs(numeric), 1.0), (what, analytic, numeric)


def _raw_inputs(cell, B, T, H, dev, seed):
    """Seeded inputs of the raw recurrence entry points: input projections gi [B*T][2][G H], W_hh [2][G H][H], b_hh [2][G H]."""
    G = 4 if cell == "lstm" else 3
    g = torch.Generator().manual_seed(seed)
    gi = torch.randn(B * T, 2, G * H, generator=g).to(dev)
    w_hh = (torch.randn(2, G * H, H, generator=g) * 0.2).to(dev)
    b_hh = (torch.randn(2, G * H, generator=g) * 0.1).to(dev)
    return G, gi, w_hh, b_hh


def _raw_fwd(cell, gi, tokens, w_hh, b_hh, lengths, B, T, H, gates):
    from artspeech_amd import _lib
    y = torch.empty(B, T, 2 * H, device=gi.device)
    _lib.call(f"as_{cell}_bidir_fwd", gi, tokens, T if tokens is not None else 0, w_hh, b_hh, lengths, B, T, H, y, gates)
    return y


def _raw_bwd(cell, dy, y, gates, w_hh, lengths, B, T, H):
    """The gate gradients [B][T][2][G H]: (dgi, dgh) of the GRU, (dg,) of the LSTM."""
    from artspeech_amd import _lib
    G = 4 if cell == "lstm" else 3
    out = [torch.empty(B, T, 2, G * H, device=dy.device) for _ in range(1 if cell == "lstm" else 2)]
    if cell == "lstm":
        _lib.call("as_lstm_bidir_bwd", dy, gates, w_hh, lengths, B, T, H, out[0])
    else:
        _lib.call("as_gru_bidir_bwd", dy, y, gates, w_hh, lengths, B, T, H, out[0], out[1])
    return out


@pytest.mark.parametrize("H", [4, 20, 32, 260])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_raw_kernels_ragged_and_padded(cell, H, dev):
    """as_{gru,lstm}_bidir_fwd/bwd on their own, register-resident (H = 32) and plain (H = 4: one chunk per row; 20: the clamped
    tail; 260: the second pass of every loop): zeros at padded frames (outputs and gate gradients), batch independence, the
    token-table form and the forward without saved gates.  Every comparison is exact."""
    from artspeech_amd.phoneme_to_articulation.rnn_ops import BiRNNLayer
    torch.manual_seed(3)
    B, T, I = 4, 11, 20
    lens = [11, 8, 3, 1]
    lengths = torch.tensor(lens, dtype=torch.int32, device=dev)
    G = 4 if cell == "lstm" else 3
    x = torch.randn(B, T, I, device=dev, requires_grad=True)
    w_ih, w_hh = torch.randn(2, G * H, I, device=dev) * 0.2, torch.randn(2, G * H, H, device=dev) * 0.2
    b_ih, b_hh = torch.randn(2, G * H, device=dev) * 0.1, torch.randn(2, G * H, device=dev) * 0.1
    y = BiRNNLayer.apply(x, w_ih, w_hh, b_ih, b_hh, lengths, cell)
    for b, l in enumerate(lens):
        assert torch.all(y[b, l:] == 0)
    y.sum().backward()
    for b, l in enumerate(lens):
        assert torch.all(x.grad[b, l:] == 0)
    # utterance 1 alone gives the same rows (workgroups are independent)
    y1 = BiRNNLayer.apply(x[1:2].detach(), w_ih, w_hh, b_ih, b_hh, lengths[1:2].contiguous(), cell)
    assert torch.equal(y1[0], y[1].detach())
    # the entry points themselves: token-table form of the input projection (embedding folded into W_ih: same rows gathered
    # inside the kernel), forward with and without saved gates, gate gradients
    V = 7
    table = torch.randn(V, 2, G * H, device=dev)
    tokens = torch.randint(0, V, (B, T), device=dev)
    gi = table[tokens].reshape(B * T, 2, G * H).contiguous()
    gates = torch.zeros(B, T, 2, G + 1, H, device=dev)
    y_ref = _raw_fwd(cell, gi, None, w_hh, b_hh, lengths, B, T, H, gates)
    assert torch.equal(_raw_fwd(cell, table, tokens, w_hh, b_hh, lengths, B, T, H, None), y_ref)
    assert torch.equal(_raw_fwd(cell, gi, None, w_hh, b_hh, lengths, B, T, H, None), y_ref)
    assert torch.equal(_raw_fwd(cell, table, tokens, w_hh, b_hh, lengths, B, T, H, torch.empty_like(gates)), y_ref)
    assert torch.equal(_raw_fwd(cell, gi[T:2 * T].contiguous(), None, w_hh, b_hh, lengths[1:2].contiguous(), 1, T, H, None)[0], y_ref[1])
    grads = _raw_bwd(cell, torch.randn(B, T, 2 * H, device=dev), y_ref, gates, w_hh, lengths, B, T, H)
    for b, l in enumerate(lens):
        assert torch.all(y_ref[b, l:] == 0)
        for dg in grads:
            assert torch.all(dg[b, l:] == 0) and torch.any(dg[b, :l] != 0)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_raw_kernels_hidden_size_4_vs_oracle(cell, dev):
    """H = 4 (one 16-byte chunk per row: three lanes of every quad have none), which the model-level oracle tests do not
    reach: y against the oracle's float64 cell recurrence fed the input projections directly (W_ih = identity, b_ih = 0), to
    the 2e-5 of test_matches_oracle; the gate gradients against central differences of that recurrence along every input
    projection (smooth in float64: step 1e-5, error ~1e-10), to assert_grad_close.  The GRU's hidden-side gradients are its
    input-side ones with the n plane times r (artspeech_oracle.gru_dir_bwd)."""
    B, T, H = 3, 6, 4
    lens = np.array([6, 4, 1])
    G, gi, w_hh, b_hh = _raw_inputs(cell, B, T, H, dev, 40)
    lengths = torch.tensor(lens, dtype=torch.int32, device=dev)
    dy = torch.randn(B, T, 2 * H, generator=torch.Generator().manual_seed(41)).to(dev)
    gates = torch.zeros(B, T, 2, G + 1, H, device=dev)
    y = _raw_fwd(cell, gi, None, w_hh, b_hh, lengths, B, T, H, gates)
    got = [g.cpu().numpy() for g in _raw_bwd(cell, dy, y, gates, w_hh, lengths, B, T, H)]

    gi64, w64, b64 = (a.cpu().numpy().astype(np.float64) for a in (gi.view(B, T, 2, G * H), w_hh, b_hh))
    dy64 = dy.cpu().numpy().astype(np.float64).reshape(B, T, 2, H)
    eye, zero = np.eye(G * H), np.zeros(G * H)
    want_y, want = np.zeros((B, T, 2, H)), [np.zeros((B, T, 2, G * H)) for _ in got]
    for d in range(2):
        def fwd(g):
            if cell == "lstm":
                return PO.lstm_dir_fwd(g, lens, eye, w64[d], zero, b64[d], bool(d)), None
            return PO.gru_dir_fwd(g, lens, eye, w64[d], zero, b64[d], bool(d))
        want_y[:, :, d], cache = fwd(gi64[:, :, d])
        eps = 1e-5
        for b in range(B):
            for t in range(lens[b]):
                for c in range(G * H):
                    g = gi64[:, :, d].copy()
                    g[b, t, c] += eps
                    up = (fwd(g)[0] * dy64[:, :, d]).sum()
                    g[b, t, c] -= 2 * eps
                    want[0][b, t, d, c] = (up - (fwd(g)[0] * dy64[:, :, d]).sum()) / (2 * eps)
        if cell == "gru":
            want[1][:, :, d] = want[0][:, :, d]
            want[1][:, :, d, 2 * H:] *= cache[0]
    err = np.abs(y.cpu().numpy().reshape(B, T, 2, H) - want_y).max()
    print(f"{cell} H=4: max|y - oracle| = {err:.2e}")
    assert err < 2e-5
    for name, a, w in zip(("dgi", "dgh") if cell == "gru" else ("dg",), got, want):
        print(f"{cell} H=4: {name} max rel err {assert_grad_close(a, w, f'{cell} H=4 {name}'):.2e}")


# (entry point, gate rows, directions, largest hidden size whose state fits the plain kernel's 64 KB of LDS)
_LIMITS = [("as_gru_bidir_fwd", 3, 2, 8192), ("as_gru_unidir_fwd_gates", 3, 1, 8192), ("as_gru_bidir_bwd", 3, 2, 1820),
           ("as_gru_unidir_bwd", 3, 1, 1820), ("as_lstm_bidir_fwd", 4, 2, 5460), ("as_lstm_bidir_bwd", 4, 2, 1636)]


@pytest.mark.parametrize("entry,G,nd,limit", _LIMITS, ids=[e[0] for e in _LIMITS])
def test_plain_kernels_refuse_beyond_their_lds_limit(entry, G, nd, limit, dev):
    """Every recurrence entry point refuses the first multiple of 4 beyond its limit with AS_ERR_UNSUPPORTED and a message that
    names the limit, and accepts the limit itself: the launch at B = T = 1 goes through and completes (all-zero inputs, so
    the outputs stay zero; this is an acceptance check, not a numeric one).  The buffers are sized for the refused width."""
    from artspeech_amd import _lib
    B = T = 1
    Hb = limit + 4
    z = lambda *shape: torch.zeros(*shape, device=dev)   # noqa: E731
    w_hh, b_hh, gi = z(nd, G * Hb, Hb), z(nd, G * Hb), z(B * T, nd, G * Hb)
    y, gates, dy = z(B, T, nd * Hb), z(B, T, nd, G + 1, Hb), z(B, T, nd * Hb)
    dg, dg2 = z(B, T, nd, G * Hb), z(B, T, nd, G * Hb)
    lengths = torch.ones(B, dtype=torch.int32, device=dev)

    def run(H):
        if entry.endswith("bidir_fwd"):
            _lib.call(entry, gi, None, 0, w_hh, b_hh, lengths, B, T, H, y, gates)
        elif entry == "as_gru_unidir_fwd_gates":
            _lib.call(entry, gi, w_hh, b_hh, lengths, B, T, H, y, gates)
        elif entry == "as_lstm_bidir_bwd":
            _lib.call(entry, dy, gates, w_hh, lengths, B, T, H, dg)
        else:
            _lib.call(entry, dy, y, gates, w_hh, lengths, B, T, H, dg, dg2)

    with pytest.raises(RuntimeError, match=rf"\(code -2\).*hidden size {Hb} \(a multiple of 4 up to {limit}\)"):
        run(Hb)
    run(limit)
    torch.cuda.synchronize()
    assert not y.any() and not dg.any() and not dg2.any()


@pytest.mark.parametrize("lstm", [True, False])
def test_full_size_backward_matches_finite_difference(lstm, dev):
    """B=32, T=200, H=128: directional derivative of sum(out * dout) along a random parameter direction."""
    torch.manual_seed(7)
    m = _model(45, {"a": 6, "b": 6}, 64, 128, lstm, None, dev)
    B, T = 32, 200
    lengths = torch.linspace(200, 60, B).int().tolist()
    tokens = torch.randint(1, 45, (B, T), device=dev)
    dout = torch.rand(B, T, m.latent_size, device=dev) / (B * T)
    loss = (m(tokens, lengths) * dout).sum()
    loss.backward()
    params = [p for p in m.parameters()]
    dirs = [torch.randn_like(p) for p in params]
    norm = float(sum((d.double() ** 2).sum() for d in dirs)) ** 0.5
    dirs = [d / norm for d in dirs]  # unit-norm direction over all parameters
    analytic = sum(float((p.grad.double() * d.double()).sum()) for p, d in zip(params, dirs))
    eps = 1e-2
    vals = []
    with torch.no_grad():
        for sgn in (1.0, -1.0):
            for p, d in zip(params, dirs):
                p.add_(sgn * eps * d)
            vals.append(float((m(tokens, lengths).double() * dout.double()).sum()))
            for p, d in zip(params, dirs):
                p.sub_(sgn * eps * d)
    numeric = (vals[0] - vals[1]) / (2 * eps)
    assert abs(numeric - analytic) < 1e-2 * max(abs(analytic), 1e-3) + 2e-5, (numeric, analytic)


def test_autoencoder_matches_reference_fixture_forward_and_gradients(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    g = load_golden("pc_autoencoder")
    w, grads = split_wg(g)
    comps = dict(zip(["tongue", "lower-lip", "upper-lip"], (int(c) for c in g["comps"])))
    m = MultiArticulatorAutoencoder(in_features=20, indices_dict=comps, hidden_features=16)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.to(dev)
    out, latent = m(torch.from_numpy(g["x"]).to(dev))
    assert np.abs(out.detach().cpu().numpy() - g["out"]).max() < 2e-6
    assert np.abs(latent.detach().cpu().numpy() - g["latent"]).max() < 2e-6
    ((out * torch.from_numpy(g["dout"]).to(dev)).sum() + (latent * torch.from_numpy(g["dlat"]).to(dev)).sum()).backward()
    for k, p in m.named_parameters():
        assert np.abs(p.grad.cpu().numpy() - grads[k]).max() < 1e-5 * max(1.0, np.abs(grads[k]).max()), k


def test_critical_loss_matches_reference_fixture_and_oracle(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import CriticalLoss
    c = load_golden("pc_critical_loss")
    arts = ["lower-lip", "tongue", "upper-lip"]
    crit = CriticalLoss(["TTCD", "LA"], list(arts))
    shapes = torch.from_numpy(c["shapes"]).to(dev).requires_grad_(True)
    loss = crit(shapes, torch.from_numpy(c["targets"]).to(dev), torch.from_numpy(c["ref"]).to(dev), torch.from_numpy(c["mask"]).to(dev))
    assert abs(float(loss.detach()) - float(c["loss"])) < 1e-7
    loss.backward()
    assert np.abs(shapes.grad.cpu().numpy() - c["dshapes"]).max() < 1e-6
    assert float(CriticalLoss([], arts)(shapes, shapes, None, None)) == 0.0
    # 50-point contours, four variables, against the oracle (the reference's cdist would use its matmul expansion here)
    rng = np.random.default_rng(5)
    arts = ["lower-lip", "pharynx", "soft-palate", "tongue", "upper-incisor", "upper-lip"]
    big = rng.random((3, 7, 6, 2, 50), dtype=np.float32)
    mask = (rng.random((3, 4, 7)) > 0.3).astype(np.float32)
    got = CriticalLoss(["LA", "TTCD", "TBCD", "VEL"], arts)(torch.from_numpy(big).to(dev), torch.from_numpy(big).to(dev), None,
                                                             torch.from_numpy(mask).to(dev))
    want = PO.critical_loss(big, None, mask, ["LA", "TTCD", "TBCD", "VEL"], arts)
    assert abs(float(got) - want) < 1e-6


def test_wrapper_decodes_components_to_shapes(dev):
    """PrincipalComponentsArtSpeechWrapper: rnn -> MultiDecoder -> per-articulator denormalisation."""
    from artspeech_amd.phoneme_to_articulation.principal_components.models import (MultiDecoder, PrincipalComponentsArtSpeech,
                                                                                    PrincipalComponentsArtSpeechWrapper)
    torch.manual_seed(9)
    comps = {"tongue": 4, "lower-lip": 3}
    rnn = PrincipalComponentsArtSpeech(13, comps, embed_dim=16, hidden_size=32, rnn="lstm").to(dev)
    dec = MultiDecoder(comps, in_features=20, hidden_features=16).to(dev)
    denorm = {"tongue": lambda a: a * 2.0 + 0.5, "lower-lip": lambda a: a - 1.0}
    model = PrincipalComponentsArtSpeechWrapper(rnn, dec, denorm).eval()
    tokens, lengths = torch.randint(1, 13, (3, 6), device=dev), [6, 4, 2]
    with torch.no_grad():
        out = model(tokens, lengths)
        z = rnn(tokens, lengths)
    assert out.shape == (3, 6, 2, 2, 10)
    w = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in dec.state_dict().items()}
    zz = z.cpu().numpy().astype(np.float64)
    for i, (name, idx, f) in enumerate((("lower-lip", [4, 5, 6], lambda a: a - 1.0), ("tongue", [0, 1, 2, 3], lambda a: a * 2.0 + 0.5))):
        want = f(PO._mlp(zz[..., idx], w, f"decoders.{name}.decoder.").reshape(3, 6, 2, 10))
        assert np.abs(out[:, :, i].cpu().numpy() - want).max() < 1e-5
