"""Input gradient of the frozen DeepSpeech2 scorer (phoneme_recognition/deepspeech2.py) and AutoencoderLoss2's recognition
term (principal_components/losses.py:226-243): against fixtures produced by the reference's own code
(tests/golden/make_golden_scorer_grad.py), against an fp64 torch-autograd restatement of the scorer written below, and the
new kernels one by one."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel_max(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _scorer(cfg, sd, dev):
    from artspeech_amd.phoneme_recognition import DeepSpeech2
    c = [int(v) for v in cfg]
    m = DeepSpeech2(c[0], c[1], c[2], c[3], num_classes=c[4], num_features=c[5], adapter_out_features=c[6] or None)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in sd.items()}, strict=True)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(dev).eval()


def _random_state(cfg, seed):
    from artspeech_amd.phoneme_recognition import DeepSpeech2
    torch.manual_seed(seed)
    c = cfg
    m = DeepSpeech2(c[0], c[1], c[2], c[3], num_classes=c[4], num_features=c[5], adapter_out_features=c[6] or None)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.uniform_(0.7, 1.3)
                mod.bias.uniform_(-0.2, 0.2)
    return {k: v.clone() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------------ fp64 restatement
def ref_scorer(sd, x, voicing):
    """deepspeech2.py:159-195 in float64 torch (eval mode): (logits, features), differentiable in x."""
    w = {k: v.double() for k, v in sd.items()}
    if "adapter.adapter.0.weight" in w:
        a = x.transpose(2, 3)
        a = F.layer_norm(a, a.shape[-1:], w["adapter.adapter.0.weight"], w["adapter.adapter.0.bias"])
        a = F.linear(a, w["adapter.adapter.1.weight"], w["adapter.adapter.1.bias"])
        a = F.layer_norm(a, a.shape[-1:], w["adapter.adapter.2.weight"], w["adapter.adapter.2.bias"])
        a = F.linear(a, w["adapter.adapter.3.weight"], w["adapter.adapter.3.bias"])
        x = a.transpose(2, 3)
    out = F.conv2d(x, w["cnn.weight"], w["cnn.bias"], padding=1)
    if voicing is not None:
        out = out + voicing.double()[:, None, None, :]
    D = out.shape[2]

    def ln_feat(t, p):
        return F.layer_norm(t.transpose(2, 3), (D,), w[p + ".weight"], w[p + ".bias"]).transpose(2, 3)

    i = 0
    while f"residual_layers.{i}.cnn1.weight" in w:
        p = f"residual_layers.{i}."
        h = F.gelu(ln_feat(out, p + "layer_norm1"))
        h = F.conv2d(h, w[p + "cnn1.weight"], w[p + "cnn1.bias"], padding=1)
        h = F.gelu(ln_feat(h, p + "layer_norm2"))
        out = F.conv2d(h, w[p + "cnn2.weight"], w[p + "cnn2.bias"], padding=1) + out
        i += 1
    B, C, D, T = out.shape
    h = F.linear(out.reshape(B, C * D, T).permute(0, 2, 1), w["linear.weight"], w["linear.bias"])   # (B, T, H)
    i = 0
    while f"recurrent_layers.{i}.rnn.weight_ih_l0" in w:
        p = f"recurrent_layers.{i}."
        a = F.gelu(F.layer_norm(h, h.shape[-1:], w[p + "layer_norm.weight"], w[p + "layer_norm.bias"]))
        H = h.shape[-1]
        gru = torch.nn.GRU(H, H, batch_first=True).double()
        gru.weight_ih_l0.data, gru.weight_hh_l0.data = w[p + "rnn.weight_ih_l0"], w[p + "rnn.weight_hh_l0"]
        gru.bias_ih_l0.data, gru.bias_hh_l0.data = w[p + "rnn.bias_ih_l0"], w[p + "rnn.bias_hh_l0"]
        for q in gru.parameters():
            q.requires_grad_(False)
        h, _ = gru(a)
        i += 1
    features = F.gelu(F.linear(h, w["feature_extractor.0.weight"], w["feature_extractor.0.bias"]))
    return F.linear(features, w["classifier.weight"], w["classifier.bias"]), features


def _ref_dx(sd, x, voicing, gl, gf):
    xr = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    v = torch.from_numpy(np.asarray(voicing)) if voicing is not None else None
    logits, features = ref_scorer(sd, xr, v)
    outs, grads = [], []
    if gl is not None:
        outs.append(logits), grads.append(torch.from_numpy(np.asarray(gl, np.float64)))
    if gf is not None:
        outs.append(features), grads.append(torch.from_numpy(np.asarray(gf, np.float64)))
    torch.autograd.backward(outs, grads)
    return xr.grad.numpy()


def _dev_dx(m, x, voicing, gl, gf, dev):
    xd = x.clone().requires_grad_(True) if torch.is_tensor(x) else torch.from_numpy(x).to(dev).requires_grad_(True)
    v = None if voicing is None else (voicing if torch.is_tensor(voicing) else torch.from_numpy(voicing).to(dev))
    logits, features = m(xd, v, return_features=True)
    outs, grads = [], []
    if gl is not None:
        outs.append(logits), grads.append(torch.as_tensor(gl).to(dev))
    if gf is not None:
        outs.append(features), grads.append(torch.as_tensor(gf).to(dev))
    torch.autograd.backward(outs, grads)
    return xd.grad


# ------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize("name", ["deepspeech2_small", "deepspeech2_plain"])
@pytest.mark.parametrize("kind", ["feat", "logits", "both"])
def test_input_grad_matches_reference_fixture(name, kind, dev):
    """dx of the reference's own scorer (eval mode, fp32 CPU) for an upstream gradient on the features, the logits or both:
    within 1e-4 of the tensor's max, like the forward's fixtures."""
    g, fx = load_golden(name), load_golden("scorer_grad")
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    m = _scorer(g["cfg"], sd, dev)
    gl = fx[f"{name}.gl"] if kind in ("logits", "both") else None
    gf = fx[f"{name}.gf"] if kind in ("feat", "both") else None
    dx = _dev_dx(m, g["x"], g.get("voicing"), gl, gf, dev)
    assert _rel_max(dx.cpu().numpy(), fx[f"{name}.dx_{kind}"]) < 1e-4
    # the fp64 restatement agrees with the reference's fixture (the restatement itself is what the cases below trust)
    want = _ref_dx({k: torch.from_numpy(v) for k, v in sd.items()}, g["x"], g.get("voicing"), gl, gf)
    assert _rel_max(fx[f"{name}.dx_{kind}"], want) < 1e-5


# ------------------------------------------------------------------------------------------------ fp64 restatement
@pytest.mark.parametrize("cfg,B,T,voiced", [
    ((2, 2, 2, 64, 44, 550, 80), 2, 37, True),    # the thesis structure (adapter 550 -> 80, H = 64), voicing
    ((2, 2, 3, 128, 31, 80, 0), 3, 70, False),    # LibriSpeech-style widths (H = 128, no adapter)
    ((3, 1, 1, 32, 5, 200, 0), 2, 7, True),       # D > 175: the convolution's fallback kernel, the looped LN backward
    ((1, 1, 1, 48, 5, 24, 0), 2, 11, False),      # one plane; a GRU width without a register-resident kernel
    ((4, 1, 2, 32, 5, 24, 16), 2, 9, True),       # four planes through the adapter
    ((3, 1, 1, 32, 7, 100, 0), 1, 1, False),      # B = 1, T = 1, D between the register-resident LN widths
])
def test_input_grad_matches_fp64(cfg, B, T, voiced, dev):
    sd = _random_state(cfg, seed=sum(cfg) + T)
    m = _scorer(cfg, sd, dev)
    rng = np.random.default_rng(T + B)
    x = rng.random((B, cfg[0], cfg[5], T), dtype=np.float32)
    v = (rng.random((B, T)) > 0.5).astype(np.float32) if voiced else None
    gl = rng.standard_normal((B, T, cfg[4])).astype(np.float32)
    gf = rng.standard_normal((B, T, cfg[3])).astype(np.float32)
    got = _dev_dx(m, x, v, gl, gf, dev).cpu().numpy()
    want = _ref_dx(sd, x, v, gl, gf)
    assert _rel_max(got, want) < 1e-4, (cfg, B, T)


def test_input_grad_thesis_size_matches_fp64(dev):
    """The thesis scorer at B = 32, T = 200 (2 planes x 500 features -> 80, 4 residual blocks, 2 GRU layers of 64)."""
    cfg = (2, 4, 2, 64, 45, 500, 80)
    sd = _random_state(cfg, seed=7)
    m = _scorer(cfg, sd, dev)
    rng = np.random.default_rng(7)
    x = rng.random((32, 2, 500, 200), dtype=np.float32)
    gf = rng.standard_normal((32, 200, 64)).astype(np.float32)
    got = _dev_dx(m, x, None, None, gf, dev).cpu().numpy()
    want = _ref_dx(sd, x, None, None, gf)
    assert _rel_max(got, want) < 1e-4


def test_input_grad_of_a_permuted_view(dev):
    """A permuted, non-contiguous input view gets the same gradient (in its own layout) as its dense copy."""
    cfg = (2, 1, 1, 32, 9, 24, 16)
    m = _scorer(cfg, _random_state(cfg, 3), dev)
    base = torch.rand(9, 2, 24, 3, device=dev)
    gf = torch.randn(3, 9, 32, device=dev)
    xv = base.clone().requires_grad_(True)
    m(xv.permute(3, 1, 2, 0), None, return_features=True)[1].backward(gf)
    xd = base.permute(3, 1, 2, 0).contiguous().requires_grad_(True)
    m(xd, None, return_features=True)[1].backward(gf)
    assert torch.equal(xv.grad.permute(3, 1, 2, 0), xd.grad)


# ------------------------------------------------------------------------------------------------ behaviour
def test_grad_path_values_are_bitwise_the_no_grad_forward_and_deterministic(dev):
    cfg = (2, 2, 2, 64, 11, 60, 24)
    m = _scorer(cfg, _random_state(cfg, 5), dev)
    x = torch.rand(3, 2, 60, 33, device=dev)
    v = (torch.rand(3, 33, device=dev) > 0.5).float()
    with torch.no_grad():
        l0, f0 = m(x, v, return_features=True)
    xg = x.clone().requires_grad_(True)
    l1, f1 = m(xg, v, return_features=True)
    assert l1.grad_fn is not None and f1.grad_fn is not None
    assert torch.equal(l0, l1) and torch.equal(f0, f1)
    gl, gf = torch.randn_like(l1), torch.randn_like(f1)
    d1 = torch.autograd.grad([l1, f1], [xg], [gl, gf])[0]
    l2, f2 = m(xg, v, return_features=True)
    d2 = torch.autograd.grad([l2, f2], [xg], [gl, gf])[0]
    assert torch.equal(d1, d2)
    # without requires_grad (or under no_grad) nothing is connected
    assert m(x, v).grad_fn is None
    with torch.no_grad():
        assert m(xg, v).grad_fn is None


def test_grad_path_refuses_trainable_parameters_and_training_mode(dev):
    cfg = (2, 1, 1, 32, 5, 12, 0)
    m = _scorer(cfg, _random_state(cfg, 1), dev)
    x = torch.rand(1, 2, 12, 3, device=dev, requires_grad=True)
    m.classifier.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="freeze"):
        m(x)
    m.classifier.weight.requires_grad_(False)
    m.train()
    with pytest.raises(RuntimeError):
        m(x)


# ------------------------------------------------------------------------------------------------ raw kernels
def _gru_ref(gi, w_hh, b_hh, lengths):
    """h_t = GRU step with the input projections gi (B, T, 3H) given (fp64), zeros past each length."""
    B, T, H3 = gi.shape
    H = H3 // 3
    ys = []
    for b in range(B):
        h = torch.zeros(H, dtype=torch.float64)
        row = []
        for t in range(T):
            if t >= lengths[b]:
                row.append(torch.zeros(H, dtype=torch.float64))
                continue
            gh = w_hh @ h + b_hh
            r = torch.sigmoid(gi[b, t, :H] + gh[:H])
            z = torch.sigmoid(gi[b, t, H:2 * H] + gh[H:2 * H])
            n = torch.tanh(gi[b, t, 2 * H:] + r * gh[2 * H:])
            h = (1 - z) * n + z * h
            row.append(h)
        ys.append(torch.stack(row))
    return torch.stack(ys)


@pytest.mark.parametrize("H", [32, 64, 128, 48])
def test_gru_unidir_bwd_matches_fp64(H, dev):
    from artspeech_amd import _lib
    L, st = _lib.lib(), _lib.stream_ptr()
    B, T = 3, 23
    lengths = [23, 11, 1]
    g = torch.Generator().manual_seed(H)
    gi = torch.randn(B, T, 3 * H, generator=g) * 0.5
    w_hh = torch.randn(3 * H, H, generator=g) / H ** 0.5
    b_hh = torch.randn(3 * H, generator=g) * 0.1
    dy = torch.randn(B, T, H, generator=g)
    gi_d, w_d, b_d, dy_d = gi.to(dev), w_hh.to(dev), b_hh.to(dev), dy.to(dev)
    len_d = torch.tensor(lengths, dtype=torch.int32, device=dev)
    y = torch.empty(B, T, H, device=dev)
    y0 = torch.empty_like(y)
    gates = torch.empty(B, T, 4 * H, device=dev)
    _lib.check(L.as_gru_unidir_fwd_gates(_lib.ptr(gi_d), _lib.ptr(w_d), _lib.ptr(b_d), _lib.ptr(len_d), B, T, H, _lib.ptr(y),
                                         _lib.ptr(gates), st))
    _lib.check(L.as_gru_unidir_fwd(_lib.ptr(gi_d), _lib.ptr(w_d), _lib.ptr(b_d), _lib.ptr(len_d), B, T, H, _lib.ptr(y0), st))
    assert torch.equal(y, y0)   # the gate-saving forward computes exactly as_gru_unidir_fwd's outputs
    dgi = torch.full((B * T, 3 * H), float("nan"), device=dev)
    dgh = torch.full_like(dgi, float("nan"))
    _lib.check(L.as_gru_unidir_bwd(_lib.ptr(dy_d), _lib.ptr(y), _lib.ptr(gates), _lib.ptr(w_d), _lib.ptr(len_d), B, T, H,
                                   _lib.ptr(dgi), _lib.ptr(dgh), st))
    gi64 = gi.double().requires_grad_(True)
    w64 = w_hh.double().requires_grad_(True)
    b64 = b_hh.double().requires_grad_(True)
    y_ref = _gru_ref(gi64, w64, b64, lengths)
    assert _rel_max(y.cpu(), y_ref.detach()) < 1e-5
    y_ref.backward(dy.double())
    assert _rel_max(dgi.cpu().view(B, T, 3 * H), gi64.grad) < 1e-4
    # dgh is the gradient of W_hh h + b_hh: its sum over frames is d b_hh, its outer products with h_{t-1} give d W_hh
    assert _rel_max(dgh.cpu().sum(0), b64.grad) < 1e-4
    hprev = torch.cat([torch.zeros(B, 1, H, dtype=torch.float64), y_ref.detach()[:, :-1]], 1).reshape(B * T, H)
    assert _rel_max(dgh.cpu().double().t() @ hprev, w64.grad) < 1e-4
    for b, l in enumerate(lengths):   # padded frames are exact zeros
        assert (dgi.view(B, T, -1)[b, l:] == 0).all() and (dgh.view(B, T, -1)[b, l:] == 0).all()


@pytest.mark.parametrize("D", [80, 37, 200])
@pytest.mark.parametrize("with_res", [False, True])
def test_ln_feat_gelu_bwd_matches_fp64(D, with_res, dev):
    from artspeech_amd import _lib
    rows, C = 13, 32
    g = torch.Generator().manual_seed(D)
    x = torch.randn(rows, D, C, generator=g) * 2 + 0.3
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g) * 0.2
    dy = torch.randn(rows, D, C, generator=g)
    res = torch.randn(rows, D, C, generator=g) if with_res else None
    dx = torch.empty(rows, D, C, device=dev)
    xd, gd, bd, dyd = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    resd = res.to(dev) if with_res else None
    _lib.check(_lib.lib().as_ln_feat_gelu_bwd(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(dyd), _lib.ptr(resd), _lib.ptr(dx),
                                              rows, D, C, _lib.stream_ptr()))
    x64 = x.double().requires_grad_(True)
    y = F.gelu(F.layer_norm(x64.transpose(1, 2), (D,), gamma.double(), beta.double())).transpose(1, 2)
    y.backward(dy.double())
    want = x64.grad + (res.double() if with_res else 0)
    assert _rel_max(dx.cpu(), want) < 1e-5


def test_conv3x3_stem_bwd_with_strided_planes(dev):
    """dx of the stem written through the forward's planar strides: (B, C, T, D) rows (the adapter's layout) and a padded
    plane pitch; every element of the planes is written, nothing between them."""
    from artspeech_amd import _lib
    for Cin in (1, 2, 3, 4):
        B, T, D = 2, 9, 13
        g = torch.Generator().manual_seed(Cin)
        w = torch.randn(32, Cin, 3, 3, generator=g)
        dy = torch.randn(B, 32, D, T, generator=g)
        taps = w.permute(2, 3, 0, 1).contiguous().to(dev)
        dy_cl = dy.permute(0, 3, 2, 1).contiguous().to(dev)   # [B][T][D][32]
        pitch = T * D + 5                                      # planes [B][Cin][pitch], (T, D) rows inside
        buf = torch.full((B, Cin, pitch), 7.0, device=dev)
        _lib.check(_lib.lib().as_conv3x3_stem_bwd(_lib.ptr(dy_cl), _lib.ptr(taps), _lib.ptr(buf), Cin * pitch, pitch, 1, D, B, T, D,
                                                  Cin, _lib.stream_ptr()))
        x64 = torch.zeros(B, Cin, D, T, dtype=torch.float64, requires_grad=True)
        F.conv2d(x64, w.double(), padding=1).backward(dy.double())
        got = buf[:, :, :T * D].view(B, Cin, T, D).transpose(2, 3)
        assert _rel_max(got.cpu(), x64.grad) < 1e-5, Cin
        assert (buf[:, :, T * D:] == 7.0).all()


# ------------------------------------------------------------------------------------------------ AutoencoderLoss2
FIX_COMPS = {"tongue": 4, "lower-lip": 3, "upper-lip": 2}
FIX_ARTS = ["lower-lip", "tongue", "upper-lip"]


def _loss_case(fx, p, dev, tmp_path, beta4=None, recognizer=True):
    from artspeech_amd.phoneme_recognition import DeepSpeech2
    from artspeech_amd.phoneme_to_articulation.principal_components.losses import AutoencoderLoss2
    from artspeech_amd.phoneme_to_articulation.transforms import Normalize
    sd = lambda pre: {k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)}
    torch.save(sd(p + "enc."), tmp_path / "enc.pt")
    torch.save(sd(p + "dec."), tmp_path / "dec.pt")
    rec = None
    if recognizer:
        rec = DeepSpeech2(**json.loads(str(fx["rec_cfg"])))
        rec.load_state_dict(sd("rec_model."))
        rec.to(dev)
        for q in rec.parameters():
            q.requires_grad = False
    norms = {a: Normalize(torch.from_numpy(fx[f"{p}norm_mean.{a}"]), torch.from_numpy(fx[f"{p}norm_std.{a}"])) for a in FIX_ARTS}
    b1, b2, b3, b4 = (float(v) for v in fx[p + "betas"])
    crit = AutoencoderLoss2(FIX_COMPS, ["LA", "TTCD"], 20, 10, tmp_path / "enc.pt", tmp_path / "dec.pt", dev, encoder_cls="AE",
                            decoder_cls="AE", denormalize_fn={a: n.inverse for a, n in norms.items()}, beta1=b1, beta2=b2, beta3=b3,
                            beta4=b4 if beta4 is None else beta4, rescale_factor=float(fx[p + "rescale"]), recognizer=rec)
    pcs = torch.from_numpy(fx[p + "pcs"]).to(dev).requires_grad_(True)
    loss = crit(pcs, torch.from_numpy(fx[p + "targets"]).to(dev), torch.from_numpy(fx[p + "ref"]).to(dev),
                torch.from_numpy(fx[p + "lengths"]), torch.from_numpy(fx[p + "mask"]).to(dev),
                torch.from_numpy(fx[p + "voicing"]).to(dev))
    loss.backward()
    return loss.detach(), pcs.grad


@pytest.mark.parametrize("case", ["b05_r1", "b1_r1", "b05_r12", "b1_r12"])
def test_autoencoder_loss2_with_recognizer_matches_reference_fixture(case, dev, tmp_path):
    fx = load_golden("scorer_grad")
    p = f"rec_{case}."
    loss, dpcs = _loss_case(fx, p, dev, tmp_path)
    assert abs(float(loss) - float(fx[p + "loss"])) <= 1e-5 * abs(float(fx[p + "loss"])), (float(loss), float(fx[p + "loss"]))
    assert _rel_max(dpcs.cpu(), fx[p + "dpcs"]) < 3e-4
    # the term counts: without the recognizer the loss is a different number
    loss0, _ = _loss_case(fx, p, dev, tmp_path, recognizer=False)
    assert abs(float(loss0) - float(loss)) > 1e-4 * abs(float(loss))


def test_autoencoder_loss2_beta4_zero_equals_no_recognizer(dev, tmp_path):
    fx = load_golden("scorer_grad")
    p = "rec_b1_r12."
    l_rec, g_rec = _loss_case(fx, p, dev, tmp_path, beta4=0.0)
    l_none, g_none = _loss_case(fx, p, dev, tmp_path, beta4=0.0, recognizer=False)
    assert torch.equal(l_rec, l_none) and torch.equal(g_rec, g_none)


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_with_recognizer_and_resume(dev, tmp_path):
    """train_principal_components_autoencoder.py feeds train_phoneme_to_principal_components.py with the recognizer config
    (a seeded thesis-scorer checkpoint): 2 epochs, finite losses that differ from the beta4 = 0 run, a resume."""
    import os
    import sys

    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import train_phoneme_to_principal_components as TP
    import train_principal_components_autoencoder as TA
    from artspeech_amd.phoneme_recognition import DeepSpeech2

    cfg = yaml.safe_load(open(os.path.join(root, "configs", "train_pc_autoencoder_synthetic.yaml")))
    cfg.update(results_dir=str(tmp_path / "ae"), train_seq_dict={"num_frames": 256},
               valid_seq_dict={"num_frames": 64}, test_seq_dict={"num_frames": 64})
    TA.main(**cfg)
    pcfg = yaml.safe_load(open(os.path.join(root, "configs", "train_pc_based_recognizer_synthetic.yaml")))
    torch.manual_seed(0)
    torch.save(DeepSpeech2(num_classes=45, **pcfg["recognizer_params"]).state_dict(), tmp_path / "recognizer.pt")
    pcfg.update(encoder_state_dict_filepath=str(tmp_path / "ae" / "best_encoders.pt"),
                decoder_state_dict_filepath=str(tmp_path / "ae" / "best_decoders.pt"), recognizer_filepath=str(tmp_path / "recognizer.pt"),
                train_seq_dict={"num_sentences": 16}, valid_seq_dict={"num_sentences": 8}, test_seq_dict={"num_sentences": 8})
    assert pcfg["beta4"] > 0
    rec = TP.main(**dict(pcfg, results_dir=str(tmp_path / "rec")))
    base = TP.main(**dict(pcfg, results_dir=str(tmp_path / "base"), beta4=0.0))
    assert [h["epoch"] for h in rec["history"]] == [1, 2]
    for h in rec["history"]:
        assert np.isfinite(h["train"]["loss"]) and np.isfinite(h["valid"]["loss"]) and np.isfinite(h["valid"]["p2cp_mean"])
    assert np.isfinite(rec["test"]["loss"])
    assert rec["history"][0]["train"]["loss"] != base["history"][0]["train"]["loss"]
    for f in ("best_model.pt", "last_model.pt", "checkpoint.pt"):
        assert os.path.exists(tmp_path / "rec" / f), f
    resumed = TP.main(**dict(pcfg, results_dir=str(tmp_path / "rec"), num_epochs=3,
                             checkpoint_filepath=str(tmp_path / "rec" / "checkpoint.pt")))
    assert [h["epoch"] for h in resumed["history"]] == [3]
    assert np.isfinite(resumed["history"][0]["train"]["loss"])
