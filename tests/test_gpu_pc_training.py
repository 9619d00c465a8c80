"""GPU tests of the principal-components method's training path: the fused multi-articulator MLP kernel (as_multi_mlp_fwd /
as_multi_mlp_bwd) and the fused masked MSE (as_masked_mse_fwd_bwd) through the modules that use them, against an fp64 torch
restatement of the reference's modules written here, and the fused path against the per-articulator GEMM path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARTS = ["lower-lip", "pharynx", "soft-palate", "tongue", "upper-lip"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ fp64 restatement
def _seq_params(seq):
    return [(seq[i].weight.detach().cpu().double().requires_grad_(True), seq[i].bias.detach().cpu().double().requires_grad_(True))
            for i in (0, 2, 4)]


def _mlp64(params, x):
    h = x
    for i, (W, b) in enumerate(params):
        h = h @ W.T + b
        if i < len(params) - 1:
            h = torch.relu(h)
    return h


def _enc_params(enc):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import PCAEncoder
    out = {}
    for a in enc.sorted_articulators:
        m = enc.encoders[a]
        if isinstance(m, PCAEncoder):
            out[a] = [(m.eigenvectors.detach().cpu().double().requires_grad_(True), None), m.eigenvalues.detach().cpu().double(), m.whiten]
        else:
            out[a] = _seq_params(m.encoder)
    return out


def _dec_params(dec):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import PCADecoder
    out = {}
    for a in dec.sorted_articulators:
        m = dec.decoders[a]
        if isinstance(m, PCADecoder):
            out[a] = [(m.eigenvectors.detach().cpu().double().requires_grad_(True), None)]
        else:
            out[a] = _seq_params(m.decoder)
    return out


def encoder64(enc, params, x, tanh):
    """MultiEncoder.forward of the reference (autoencoder.py:153-173) in fp64: -inf spaces, index_put, stack, max."""
    lead = x.shape[:-2]
    spaces = []
    for i, a in enumerate(enc.sorted_articulators):
        p = params[a]
        if isinstance(p[-1], bool):   # PCA: [(eigenvectors, None), eigenvalues, whiten]
            (E, _), ev, whiten = p
            z = x[..., i, :] @ E.T
            if whiten:
                z = z / torch.sqrt(ev)
        else:
            z = _mlp64(p, x[..., i, :])
        space = torch.full((*lead, enc.latent_size), -torch.inf, dtype=torch.float64)
        space[..., enc.indices_dict[a]] = z
        spaces.append(space)
    lat = torch.stack(spaces, dim=-2).max(dim=-2).values
    return torch.tanh(lat) if tanh else lat


def decoder64(dec, params, x, scale=1.0):
    x = scale * x
    outs = []
    for a in dec.sorted_articulators:
        p = params[a]
        xi = x[..., dec.indices_dict[a]]
        outs.append((xi @ p[0][0] if len(p) == 1 else _mlp64(p, xi)).unsqueeze(-2))
    return torch.cat(outs, dim=-2)


def _all64(params):
    out = []
    for p in params.values():
        for item in p:
            if isinstance(item, tuple):
                out += [t for t in item if t is not None]
    return out


def _sorted_params(container):
    """(name, parameter) of a MultiEncoder / MultiDecoder in sorted-articulator order (the order of the fp64 lists)."""
    mods = container.encoders if hasattr(container, "encoders") else container.decoders
    return [(f"{a}.{n}", p) for a in container.sorted_articulators for n, p in mods[a].named_parameters()]


def _close(got, want, frac, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin]), what
    scale = max(np.abs(want[fin]).max() if fin.any() else 0.0, 1e-30)
    err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
    assert err <= frac * scale, f"{what}: max|err| / max|ref| = {err / scale:.2e} > {frac:g}"


# ------------------------------------------------------------------------------------------------ 1. kernel vs fp64
INDEX_CASES = {
    "disjoint": {"tongue": 12, "lower-lip": 4, "upper-lip": 3, "pharynx": 2, "soft-palate": 1},
    "overlapping": {"tongue": [0, 1, 2, 3, 4], "lower-lip": [3, 4, 5], "upper-lip": [0, 5, 6]},
    "gapped": {"tongue": [0, 1, 4], "lower-lip": [6, 7], "upper-lip": [2, 9]},
}


@pytest.mark.parametrize("rows", [1, 63, 2407])
@pytest.mark.parametrize("case", sorted(INDEX_CASES))
@pytest.mark.parametrize("widths", [(100, 50), (3, 10), (20, 16)], ids=["thesis", "odd", "small"])
def test_multi_mlp_matches_fp64(case, widths, rows, dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder, MultiEncoder
    in_features, hidden = widths
    torch.manual_seed(rows + in_features)
    idx = INDEX_CASES[case]
    enc = MultiEncoder(idx, in_features, hidden).to(dev)
    dec = MultiDecoder(idx, in_features, hidden).to(dev)
    assert enc._plan.supported and dec._plan.supported
    A = len(enc.sorted_articulators)
    x = torch.randn(rows, A, in_features)
    dlat = torch.randn(rows, enc.latent_size)
    dout = torch.randn(rows, A, in_features)

    def run():
        xd = x.to(dev).requires_grad_(True)
        enc.zero_grad(set_to_none=True)
        dec.zero_grad(set_to_none=True)
        lat = enc._forward(xd, tanh=True)
        z = lat.detach().clone().requires_grad_(True)
        out = dec(z, scale=1.5)
        (lat * dlat.to(dev)).sum().backward()
        (out * dout.to(dev)).sum().backward()
        grads = [p.grad.clone() for _, p in _sorted_params(enc) + _sorted_params(dec)]
        return lat.detach(), out.detach(), xd.grad.clone(), z.grad.clone(), grads

    lat, out, dx, dz, grads = run()
    lat2, out2, dx2, dz2, grads2 = run()
    assert torch.equal(lat, lat2) and torch.equal(out, out2) and torch.equal(dx, dx2) and torch.equal(dz, dz2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2)), "two runs differ"

    pe, pd = _enc_params(enc), _dec_params(dec)
    x64 = x.double().requires_grad_(True)
    lat64 = encoder64(enc, pe, x64, tanh=True)
    (lat64 * dlat.double()).sum().backward()
    z64 = lat.cpu().double().requires_grad_(True)
    out64 = decoder64(dec, pd, z64, scale=1.5)
    (out64 * dout.double()).sum().backward()
    _close(lat.cpu(), lat64.detach(), 1e-5, "latent")
    _close(out.cpu(), out64.detach(), 1e-5, "decoder output")
    _close(dx.cpu(), x64.grad, 5e-5, "encoder dx")
    _close(dz.cpu(), z64.grad, 5e-5, "decoder dx")
    names = [n for n, _ in _sorted_params(enc) + _sorted_params(dec)]
    assert len(names) == len(_all64(pe) + _all64(pd))
    for got, want, name in zip(grads, _all64(pe) + _all64(pd), names):
        _close(got.cpu(), want.grad, 5e-5, name)
    if case == "gapped":
        unowned = [j for j in range(enc.latent_size) if all(j not in v for v in idx.values())]
        assert torch.all(lat[:, unowned] == -1) and torch.all(dx.abs().sum() > 0)
        assert torch.all(dz[:, unowned] == 0)


def test_encoder_without_activation_keeps_minus_inf_and_ties_go_to_the_first_group(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiEncoder
    torch.manual_seed(5)
    idx = {"tongue": [0, 1], "lower-lip": [1, 3]}   # index 2 unowned; index 1 owned twice
    enc = MultiEncoder(idx, 6, 8).to(dev)
    with torch.no_grad():   # make both owners of index 1 produce the same value: identical last layers
        for a in idx:
            enc.encoders[a].encoder[4].weight.zero_()
            enc.encoders[a].encoder[4].bias.fill_(0.25)
    x = torch.randn(9, 2, 6, device=dev, requires_grad=True)
    lat = enc(x)
    assert torch.all(lat[:, 2] == -torch.inf) and torch.all(lat[:, 1] == 0.25)
    lat[:, [0, 1, 3]].sum().backward()
    # the tie goes to the first sorted articulator ("lower-lip"): its last bias receives the gradient of index 1
    assert float(enc.encoders["lower-lip"].encoder[4].bias.grad[0]) == 9.0
    assert float(enc.encoders["tongue"].encoder[4].bias.grad[1]) == 0.0


def test_single_layer_pca_projection(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import (MultiDecoder, MultiEncoder, PCADecoder,
                                                                                   PCAEncoder)
    torch.manual_seed(11)
    idx = {"tongue": 5, "lower-lip": 3, "upper-lip": 2}
    enc = MultiEncoder(idx, 20, 8, encoder_cls="PCA").to(dev)
    dec = MultiDecoder(idx, 20, 8, decoder_cls=PCADecoder).to(dev)
    assert enc._plan.layers == 1 and dec._plan.layers == 1
    for m in enc.encoders.values():
        m.whiten = True
    x = torch.randn(37, 3, 20, device=dev, requires_grad=True)
    lat = enc(x)
    pe = _enc_params(enc)
    x64 = x.detach().cpu().double().requires_grad_(True)
    lat64 = encoder64(enc, pe, x64, tanh=False)
    _close(lat.detach().cpu(), lat64.detach(), 1e-5, "PCA latent")
    lat.sum().backward()
    lat64.sum().backward()
    _close(x.grad.cpu(), x64.grad, 5e-5, "PCA dx")
    for a in enc.sorted_articulators:   # whitening folded into the projection: gradients reach both parameters
        assert enc.encoders[a].eigenvalues.grad is not None and enc.encoders[a].eigenvectors.grad is not None
    z = torch.randn(2, 4, enc.latent_size, device=dev)
    out = dec(z)
    out64 = decoder64(dec, _dec_params(dec), z.cpu().double())
    _close(out.detach().cpu(), out64.detach(), 1e-5, "PCA decoder")
    # a PCAEncoder / PCADecoder on its own (one group, layers = 1)
    e = PCAEncoder(20, 4).to(dev)
    _close(e(x.detach()[:, 0]).detach().cpu(), x.detach()[:, 0].cpu().double() @ e.eigenvectors.detach().cpu().double().T, 1e-5, "PCAEncoder")


def test_pca_widths_beyond_the_lds_budget_take_the_grouped_path(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder, MultiEncoder, PCAEncoder
    torch.manual_seed(12)
    enc = MultiEncoder({"tongue": 3, "lower-lip": 2}, 300, 8, encoder_cls="PCA").to(dev)
    dec = MultiDecoder({"tongue": 3, "lower-lip": 2}, 300, 8, decoder_cls="PCA").to(dev)
    assert not enc._plan.supported and not dec._plan.supported
    x = torch.randn(7, 2, 300, device=dev)
    lat = enc(x)
    _close(lat.detach().cpu(), encoder64(enc, _enc_params(enc), x.cpu().double(), tanh=False).detach(), 1e-5, "PCA fallback latent")
    z = torch.randn(2, 3, enc.latent_size, device=dev)
    _close(dec(z).detach().cpu(), decoder64(dec, _dec_params(dec), z.cpu().double()).detach(), 1e-5, "PCA fallback decoder")
    e = PCAEncoder(300, 4).to(dev)   # on its own, too
    _close(e(x[:, 0]).detach().cpu(), x[:, 0].cpu().double() @ e.eigenvectors.detach().cpu().double().T, 1e-5, "PCAEncoder fallback")


def test_widths_beyond_the_lds_budget_take_the_grouped_path(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    torch.manual_seed(2)
    m = MultiArticulatorAutoencoder(300, {"tongue": 3, "lower-lip": 2}, hidden_features=64).to(dev)
    assert not m.encoders._plan.supported and not m.decoders._plan.supported
    x = torch.randn(10, 2, 300, device=dev)
    out, lat = m(x)
    lat64 = encoder64(m.encoders, _enc_params(m.encoders), x.cpu().double(), tanh=True)
    _close(lat.detach().cpu(), lat64.detach(), 1e-5, "fallback latent")


# ------------------------------------------------------------------------------------------------ 3. fused vs grouped
def test_autoencoder_fused_matches_grouped(dev, monkeypatch):
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder, autoencoder
    torch.manual_seed(4)
    comps = {a: c for a, c in zip(ARTS, (3, 2, 4, 12, 3))}
    m = MultiArticulatorAutoencoder(100, comps, hidden_features=50).to(dev)
    crit = RegularizedLatentsMSELoss2(0.1, m.indices_dict)
    x = torch.randn(700, len(comps), 100, device=dev)
    w = torch.rand(700, device=dev)
    results = {}
    for mode in ("fused", "grouped"):
        monkeypatch.setattr(autoencoder, "FUSED_MLP", mode == "fused")
        m.zero_grad(set_to_none=True)
        out, lat = m(x)
        loss = crit(out, lat, x, w)
        loss.backward()
        results[mode] = (out.detach().cpu(), lat.detach().cpu(), float(loss), {k: p.grad.cpu() for k, p in m.named_parameters()})
    (of, lf, sf, gf), (og, lg, sg, gg) = results["fused"], results["grouped"]
    _close(of, og, 1e-5, "outputs")
    _close(lf, lg, 1e-5, "latents")
    assert abs(sf - sg) <= 1e-5 * abs(sg)
    for k in gf:
        _close(gf[k], gg[k], 3e-4, k)


# ------------------------------------------------------------------------------------------------ losses vs fp64
def test_regularized_latents_loss_matches_fp64(dev):
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    torch.manual_seed(8)
    comps = {"tongue": 4, "lower-lip": 2, "upper-lip": 1}
    m = MultiArticulatorAutoencoder(20, comps, hidden_features=10).to(dev)
    crit = RegularizedLatentsMSELoss2(0.7, m.indices_dict)
    x = torch.randn(64, 3, 20, device=dev)
    w = torch.rand(64, device=dev)
    out, lat = m(x)
    loss = crit(out, lat, x, w)
    loss.backward()
    pe, pd = _enc_params(m.encoders), _dec_params(m.decoders)
    x64, w64 = x.cpu().double(), w.cpu().double()
    lat64 = encoder64(m.encoders, pe, x64, tanh=True)
    out64 = decoder64(m.decoders, pd, lat64)
    mse64 = ((out64 - x64) ** 2 * w64[:, None, None]).mean()
    cov64 = sum(torch.cov(lat64.T[i]).square().sum() - torch.cov(lat64.T[i]).diag().square().sum()
                for i in m.indices_dict.values() if len(i) > 1)
    want = float(mse64 + 0.7 * cov64)
    assert abs(float(loss) - want) <= 1e-5 * abs(want), (float(loss), want)
    mse64.backward()   # the covariance term is detached (the reference's torch.tensor([...])): gradients from the MSE alone
    got = [p.grad for _, p in _sorted_params(m.encoders) + _sorted_params(m.decoders)]
    for g, r in zip(got, _all64(pe) + _all64(pd)):
        _close(g.cpu(), r.grad, 3e-4, "RegularizedLatentsMSELoss2 gradient")


def _denorm(arts, N):
    from artspeech_amd.phoneme_to_articulation.transforms import Normalize
    g = torch.Generator().manual_seed(3)
    return {a: Normalize(torch.rand(2, N, generator=g) * 0.2, 0.5 + torch.rand(2, N, generator=g)).inverse for a in arts}


def _critical64(TVs, arts, denorm, out_shapes, ref, mask):
    """CriticalLoss (losses.py:23-99) in fp64 with cdist + min."""
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import CriticalLoss
    tv_map = CriticalLoss.TV_TO_ARTICULATOR_MAP
    arts_all = sorted(arts + ["upper-incisor"])
    ri = arts_all.index("upper-incisor")
    shapes = torch.cat([out_shapes[:, :, :ri], ref, out_shapes[:, :, ri:]], dim=2)
    dists = []
    for tv in sorted(TVs):
        sets = []
        for a in tv_map[tv]:
            arr = shapes[..., arts_all.index(a), :, :]
            if a != "upper-incisor":
                arr = denorm[a](arr)
            sets.append(arr.transpose(2, 3))
        dists.append(torch.cdist(sets[0], sets[1]).flatten(-2).min(dim=-1).values)   # (B, T)
    crit = torch.stack(dists, dim=1)   # (B, n_TV, T)
    return crit[mask == 1].mean()


@pytest.mark.parametrize("kind,rescale", [("AE", 1.0), ("AE", 12.0), ("PCA", 1.0)])
def test_autoencoder_loss2_thesis_size_matches_fp64(kind, rescale, dev, tmp_path):
    """AutoencoderLoss2 at B=12, T=200, 10 articulators, in 100 / hidden 50, 35 components, TVs LA / TTCD / TBCD (upper
    incisor injected), ragged lengths down to 1, a denormalize_fn: value and d(output_pcs) against fp64 autograd."""
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder, MultiEncoder
    arts = ["arytenoid-cartilage", "epiglottis", "lower-incisor", "lower-lip", "pharynx", "soft-palate", "thyroid-cartilage",
            "tongue", "upper-lip", "vocal-folds"]
    comps = dict(zip(arts, (2, 3, 2, 4, 3, 4, 2, 8, 4, 3)))
    assert sum(comps.values()) == 35
    torch.manual_seed(21)
    enc, dec = MultiEncoder(comps, 100, 50, encoder_cls=kind), MultiDecoder(comps, 100, 50, decoder_cls=kind)
    if kind == "PCA":   # an SVD-built projection, like the scikit-learn PCA of the reference
        data = torch.randn(500, 100, dtype=torch.float64)
        _, S, Vh = torch.linalg.svd(data - data.mean(0), full_matrices=False)
        with torch.no_grad():
            for a, n in comps.items():
                enc.encoders[a].eigenvectors.copy_(Vh[:n].float())
                enc.encoders[a].eigenvalues.copy_((S[:n] ** 2 / 499).float())
                dec.decoders[a].eigenvectors.copy_(Vh[:n].float())
    torch.save(enc.state_dict(), tmp_path / "enc.pt")
    torch.save(dec.state_dict(), tmp_path / "dec.pt")
    TVs = ["LA", "TTCD", "TBCD"]
    denorm = _denorm(arts, 50)
    crit = AutoencoderLoss2(comps, TVs, 100, 50, tmp_path / "enc.pt", tmp_path / "dec.pt", dev, encoder_cls=kind, decoder_cls=kind,
                            denormalize_fn=denorm, beta1=0.5, beta2=1.0, beta3=0.3, rescale_factor=rescale)
    B, T = 12, 200
    lengths = torch.tensor([200, 199, 180, 150, 120, 100, 77, 50, 31, 10, 2, 1])
    g = torch.Generator().manual_seed(5)
    targets = torch.rand(B, T, 10, 2, 50, generator=g) * 0.5
    ref = torch.rand(B, T, 1, 2, 50, generator=g)
    mask = (torch.rand(B, 3, T, generator=g) > 0.5).long()
    for b, l in enumerate(lengths.tolist()):
        mask[b, :, l:] = 0
    pcs = (torch.rand(B, T, 35, generator=g) * 2 - 1) / rescale
    out_pcs = pcs.to(dev).requires_grad_(True)
    loss = crit(out_pcs, targets.to(dev), ref.to(dev), lengths, mask.to(dev))
    loss.backward()

    pe, pd = _enc_params(crit.encode.transform), _dec_params(crit.decode.transform)
    pcs64 = pcs.double().requires_grad_(True)
    t64 = targets.double()
    tgt_pcs = encoder64(crit.encode.transform, pe, t64.reshape(B * T, 10, 100), tanh=True).reshape(B, T, 35).detach()
    shapes64 = decoder64(crit.decode.transform, pd, pcs64, scale=rescale).reshape(B, T, 10, 2, 50)
    valid = torch.arange(T)[None] < lengths[:, None]
    lat_loss = ((pcs64 - tgt_pcs) ** 2)[valid].mean()
    rec_loss = ((shapes64 - t64) ** 2)[valid].mean()
    crit_loss = _critical64(TVs, arts, denorm, shapes64, ref.double(), mask)
    want = 0.5 * lat_loss + rec_loss + 0.3 * crit_loss
    want.backward()
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    _close(out_pcs.grad.cpu(), pcs64.grad, 3e-4, "d output_pcs")
    assert all(not p.requires_grad for p in crit.parameters())


def test_run_autoencoder_epoch_trains_with_adam(dev):
    """reference __init__.py:8-66 on captured batches: three Adam steps move the parameters, the eval pass leaves them."""
    from artspeech_amd.phoneme_to_articulation.principal_components import run_autoencoder_epoch
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    torch.manual_seed(9)
    m = MultiArticulatorAutoencoder(20, {"tongue": 3, "lower-lip": 2}, hidden_features=10).to(dev)
    crit = RegularizedLatentsMSELoss2(0.1, m.indices_dict)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    batches = [(["f"] * 16, torch.rand(16, 2, 20), torch.rand(16), ["a"] * 16) for _ in range(3)]
    before = [p.detach().clone() for p in m.parameters()]
    info = run_autoencoder_epoch("train", 0, m, batches, opt, crit, device=dev)
    assert np.isfinite(info["loss"])
    assert all(not torch.equal(a, p) for a, p in zip(before, m.parameters()))
    after = [p.detach().clone() for p in m.parameters()]
    info = run_autoencoder_epoch("validation", 0, m, batches, opt, crit, device=dev)
    assert np.isfinite(info["loss"]) and all(torch.equal(a, p) for a, p in zip(after, m.parameters()))


# ------------------------------------------------------------------------------------------------ 2. reference fixtures
def _fixture():
    from conftest import load_golden
    return load_golden("pc_training")


FIX_ARTS = ["lower-lip", "tongue", "upper-lip"]
FIX_COMPS = {"tongue": 4, "lower-lip": 3, "upper-lip": 2}


def _sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}


def _norms(g, prefix):
    from artspeech_amd.phoneme_to_articulation.transforms import Normalize
    return {a: Normalize(torch.from_numpy(g[f"{prefix}norm_mean.{a}"]), torch.from_numpy(g[f"{prefix}norm_std.{a}"])) for a in FIX_ARTS}


def _rel(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-30)


@pytest.mark.parametrize("case", ["ae_r1", "ae_r12", "pca"])
def test_autoencoder_loss2_matches_reference_fixture(case, dev, tmp_path):
    """Reference AutoencoderLoss2 (AE and SVD-built PCA types, rescale_factor 1 / 12, hidden 10 -> 5, LA + TTCD with the
    upper incisor injected, a denormalize_fn, lengths down to 1): loss <= 1e-5 relative, d(output_pcs) <= 3e-4 of its max."""
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    g = _fixture()
    p = f"ael2_{case}."
    kind = "PCA" if case == "pca" else "AE"
    torch.save(_sd(g, p + "enc."), tmp_path / "enc.pt")
    torch.save(_sd(g, p + "dec."), tmp_path / "dec.pt")
    b1, b2, b3 = (float(v) for v in g[p + "betas"])
    crit = AutoencoderLoss2(FIX_COMPS, ["LA", "TTCD"], 20, 10, tmp_path / "enc.pt", tmp_path / "dec.pt", dev, encoder_cls=kind,
                            decoder_cls=kind, denormalize_fn={a: n.inverse for a, n in _norms(g, p).items()}, beta1=b1, beta2=b2,
                            beta3=b3, rescale_factor=float(g[p + "rescale"]))
    pcs = torch.from_numpy(g[p + "pcs"]).to(dev).requires_grad_(True)
    loss = crit(pcs, torch.from_numpy(g[p + "targets"]).to(dev), torch.from_numpy(g[p + "ref"]).to(dev),
                torch.from_numpy(g[p + "lengths"]), torch.from_numpy(g[p + "mask"]).to(dev))
    assert _rel(loss, g[p + "loss"]) <= 1e-5, (float(loss), float(g[p + "loss"]))
    loss.backward()
    _close(pcs.grad.cpu(), g[p + "dpcs"], 3e-4, f"{case}: d output_pcs")


def test_regularized_latents_loss_matches_reference_fixture(dev):
    """Reference RegularizedLatentsMSELoss2 on a MultiArticulatorAutoencoder with sample weights: the loss (with the detached
    covariance term) and every parameter gradient."""
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    g = _fixture()
    m = MultiArticulatorAutoencoder(in_features=20, indices_dict=FIX_COMPS, hidden_features=10)
    m.load_state_dict(_sd(g, "rl.w."), strict=True)
    m.to(dev)
    crit = RegularizedLatentsMSELoss2(float(g["rl.alpha"]), m.indices_dict)
    x = torch.from_numpy(g["rl.x"]).to(dev)
    out, lat = m(x)
    loss = crit(out, lat, x, torch.from_numpy(g["rl.weights"]).to(dev))
    assert _rel(loss, g["rl.loss"]) <= 1e-5, (float(loss), float(g["rl.loss"]))
    loss.backward()
    for k, prm in m.named_parameters():
        _close(prm.grad.cpu(), g["rl.g." + k], 3e-4, k)


def test_decoder_p2cp_matches_reference_fixture_and_denormalises_targets_in_place(dev, tmp_path):
    from artspeech_amd.phoneme_to_articulation.principal_components.metrics import DecoderMeanP2CPDistance2
    from artspeech_amd.settings import DATASET_CONFIG
    g = _fixture()
    torch.save(_sd(g, "p2cp.dec."), tmp_path / "dec.pt")
    metric = DecoderMeanP2CPDistance2(DATASET_CONFIG["artspeech2"], tmp_path / "dec.pt", FIX_COMPS,
                                      {"in_features": 20, "hidden_features": 10}, {a: n.inverse for a, n in _norms(g, "p2cp.").items()},
                                      dev)
    targets = torch.from_numpy(g["p2cp.targets_in"]).to(dev)
    value = metric(torch.from_numpy(g["p2cp.outputs"]).to(dev), targets, torch.from_numpy(g["p2cp.lengths"]))
    assert _rel(value, g["p2cp.value"]) <= 1e-5, (float(value), float(g["p2cp.value"]))
    _close(targets.cpu(), g["p2cp.targets_after"], 1e-6, "targets denormalised in place")


def test_run_autoencoder_epoch_matches_reference_adam_steps(dev):
    """Three Adam steps of the reference's run_autoencoder_epoch on captured batches: per-step losses and final parameters."""
    from artspeech_amd.phoneme_to_articulation.principal_components import run_autoencoder_epoch
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import RegularizedLatentsMSELoss2
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiArticulatorAutoencoder
    g = _fixture()
    m = MultiArticulatorAutoencoder(in_features=20, indices_dict=FIX_COMPS, hidden_features=10)
    m.load_state_dict(_sd(g, "loop.w0."), strict=True)
    m.to(dev)
    crit = RegularizedLatentsMSELoss2(0.1, m.indices_dict)
    losses = []

    def criterion(*args):
        value = crit(*args)
        losses.append(float(value))
        return value

    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-6)
    batches = [(["f"] * 16, torch.from_numpy(g[f"loop.x{i}"]), torch.from_numpy(g[f"loop.weights{i}"]), ["a"] * 16) for i in range(3)]
    info = run_autoencoder_epoch("train", 1, m, batches, opt, criterion, device=dev)
    for got, want in zip(losses, g["loop.losses"]):
        assert _rel(got, want) <= 1e-5, (losses, g["loop.losses"])
    assert _rel(info["loss"], g["loop.info_loss"]) <= 1e-5
    want = _sd(g, "loop.w3.")
    for k, v in m.state_dict().items():
        _close(v.cpu(), want[k], 3e-4, k)


# ------------------------------------------------------------------------------------------------ 5. chained trainers
def test_chained_trainers_and_resume(dev, tmp_path):
    """The autoencoder trainer (2 epochs, synthetic config) feeds the method trainer: 2 epochs with GRU, 1 with LSTM, 1 with
    PCA types (an SVD-built PCA state dict), and a resume from checkpoint.pt that continues at the next epoch."""
    import os
    import sys

    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import train_phoneme_to_principal_components as TP
    import train_principal_components_autoencoder as TA
    from artspeech_amd.phoneme_to_articulation.principal_components.models import MultiDecoder, MultiEncoder

    cfg = yaml.safe_load(open(os.path.join(root, "configs", "train_pc_autoencoder_synthetic.yaml")))
    cfg.update(results_dir=str(tmp_path / "ae"), train_seq_dict={"num_frames": 512}, valid_seq_dict={"num_frames": 128},
               test_seq_dict={"num_frames": 128})
    res = TA.main(**cfg)
    assert [h["epoch"] for h in res["history"]] == [1, 2]
    assert all(np.isfinite(h["train"]["loss"]) and np.isfinite(h["valid"]["p2cp_mm"]) for h in res["history"])
    assert np.isfinite(res["test"]["loss"]) and np.isfinite(res["test"]["p2cp_mm"])
    for f in ("best_encoders.pt", "best_decoders.pt", "last_encoders.pt", "last_decoders.pt", "checkpoint.pt"):
        assert os.path.exists(tmp_path / "ae" / f), f

    pcfg = yaml.safe_load(open(os.path.join(root, "configs", "train_pc_based_synthetic.yaml")))
    pcfg.update(encoder_state_dict_filepath=str(tmp_path / "ae" / "best_encoders.pt"),
                decoder_state_dict_filepath=str(tmp_path / "ae" / "best_decoders.pt"),
                train_seq_dict={"num_sentences": 16}, valid_seq_dict={"num_sentences": 8}, test_seq_dict={"num_sentences": 8})

    def run(name, **kw):
        c = dict(pcfg, results_dir=str(tmp_path / name), **kw)
        out = TP.main(**c)
        assert all(np.isfinite(h["train"]["loss"]) and np.isfinite(h["valid"]["p2cp_mean"]) for h in out["history"]), name
        assert np.isfinite(out["test"]["loss"]) and np.isfinite(out["test"]["p2cp_mean"]), name
        for f in ("best_model.pt", "last_model.pt", "checkpoint.pt"):
            assert os.path.exists(tmp_path / name / f), (name, f)
        return out, c

    gru, gru_cfg = run("gru")
    assert [h["epoch"] for h in gru["history"]] == [1, 2]
    run("lstm", rnn_type="LSTM", num_epochs=1)
    # PCA types: an SVD-built projection of the same widths
    comps, ae_kw = pcfg["indices_dict"], pcfg["autoencoder_kwargs"]
    enc = MultiEncoder(comps, ae_kw["in_features"], ae_kw["hidden_features"], encoder_cls="PCA")
    dec = MultiDecoder(comps, ae_kw["in_features"], ae_kw["hidden_features"], decoder_cls="PCA")
    data = torch.rand(400, ae_kw["in_features"], dtype=torch.float64)
    _, S, Vh = torch.linalg.svd(data - data.mean(0), full_matrices=False)
    with torch.no_grad():
        for a, n in comps.items():
            enc.encoders[a].eigenvectors.copy_(Vh[:n].float())
            enc.encoders[a].eigenvalues.copy_((S[:n] ** 2 / 399).float())
            dec.decoders[a].eigenvectors.copy_(Vh[:n].float())
    torch.save(enc.state_dict(), tmp_path / "pca_enc.pt")
    torch.save(dec.state_dict(), tmp_path / "pca_dec.pt")
    run("pca", num_epochs=1, encoder_type="PCA", decoder_type="PCA", encoder_state_dict_filepath=str(tmp_path / "pca_enc.pt"),
        decoder_state_dict_filepath=str(tmp_path / "pca_dec.pt"))
    # resume: the GRU run's checkpoint (epoch 2) continues at epoch 3
    resumed = TP.main(**dict(gru_cfg, num_epochs=3, checkpoint_filepath=str(tmp_path / "gru" / "checkpoint.pt")))
    assert [h["epoch"] for h in resumed["history"]] == [3]
    assert torch.load(tmp_path / "gru" / "checkpoint.pt")["epoch"] == 3
