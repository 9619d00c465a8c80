"""DeepSpeech2-style articulatory scorer, inference on the C ABI (reference ``phoneme_recognition/deepspeech2.py``).

Same constructor, ``state_dict`` keys and seed-for-seed initialisation as the reference ``DeepSpeech2`` (:90-157): the
sub-modules below are PARAMETER CONTAINERS created in the reference's order; none of their ``forward`` methods is ever
called.  ``DeepSpeech2.forward`` runs (deepspeech2.py:159-195)

    [Adapter: LN -> Linear -> LN -> Linear over the feature axis]                 as_layernorm_fwd + as_gemm_f32
    Conv2d(Cin, 32, 3x3) (+ voicing)                                              as_conv3x3_stem
    ResidualCNN x N: (LN over features -> GELU -> Conv2d(32, 32, 3x3)) x 2 + skip as_ln_feat_gelu + as_conv3x3_c32 (MFMA)
    Linear(32*D -> H)                                                             as_gemm_f32
    RecurrentBlock x M: LN -> GELU -> uni-GRU                                     as_layernorm_fwd + as_gelu + as_gemm_f32
                                                                                  + as_gru_unidir_fwd
    Linear -> GELU (features), Linear (logits)                                    as_gemm_f32 (GELU epilogue)

on channels-last feature maps ``[B][T][D][32]``: a frame's 32*D features are one contiguous row, so the reference's
``view(B, C*D, T).permute(2, 0, 1)`` (:183-185) costs nothing -- the Linear weight's columns are permuted once instead.
Inference only (``eval()`` mode, the way ``phoneme_recognition/__init__.py:213-236`` scores); there is no CPU path.

Input gradients (a FROZEN scorer inside a loss, principal_components/losses.py:228-243): when grad mode is on and ``x``
requires grad, ``forward`` runs through ``_ScorerInputGrad``, which keeps the activations its backward needs (block inputs
and pre-LN2 maps, GRU outputs and gates, row-LayerNorm ``xhat`` / ``rstd``) and returns the same values, bit for bit.  Its
backward walks the layers in reverse on the HIP library: as_gemm_f32 for every dX = dY . W, as_gelu_bwd /
as_layernorm_bwd, as_gru_unidir_bwd, as_conv3x3_c32 over flipped taps, as_ln_feat_gelu_bwd and as_conv3x3_stem_bwd.  The
scorer's own parameters get no gradient: if any of them requires grad, that path raises instead.
"""
import torch
import torch.nn as nn

from .. import _lib

OUT_CHANNELS = 32  # deepspeech2.py:104


class _Params(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: the scorer runs in DeepSpeech2.forward on the HIP library")


class ResidualCNN(_Params):
    """Parameters of deepspeech2.py:15-27 (kernel 3, stride 1)."""

    def __init__(self, channels, num_features):
        super().__init__()
        self.cnn1 = nn.Conv2d(channels, channels, 3, 1, padding=1)
        self.layer_norm1 = nn.LayerNorm(num_features)
        self.cnn2 = nn.Conv2d(channels, channels, 3, 1, padding=1)
        self.layer_norm2 = nn.LayerNorm(num_features)


class RecurrentBlock(_Params):
    """Parameters of deepspeech2.py:50-62."""

    def __init__(self, size):
        super().__init__()
        self.rnn = nn.GRU(input_size=size, hidden_size=size, num_layers=1, bidirectional=False, batch_first=False)
        self.layer_norm = nn.LayerNorm(size)


class Adapter(_Params):
    """Parameters of deepspeech2.py:73-81."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.adapter = nn.Sequential(nn.LayerNorm(in_features), nn.Linear(in_features, out_features),
                                     nn.LayerNorm(out_features), nn.Linear(out_features, out_features))


def _slab(dev):
    return _lib.slab(dev, 4 << 20)  # split-K partial tiles (16 MB); as_gemm_f32 derives its split-K factor from the size


def _gemm(A, W, bias, out, act=0, split_k=False):
    """out[M][N] = act(A[M][K] . W[N][K]^T + bias) (bias None: none).  split_k (act == 0 only): few output tiles under a long reduction --
    the bias is laid down first and the GEMM accumulates onto it, its K range split over workgroups (deterministic slabs)."""
    assert A.is_contiguous() and W.is_contiguous() and out.is_contiguous(), "bare pointers below: dense row-major operands"
    N, K = W.shape
    if split_k and act == 0:
        out.copy_(bias.expand_as(out))
        slab = _slab(out.device)
        how = dict(accumulate=1, splitk_ws=slab, splitk_ws_floats=slab.numel())
    else:
        how = dict(bias=bias)
    _lib.gemm(A=A, B=W, C=out, M=A.shape[0], N=N, K=K, a_i=K, a_k=1, b_j=K, b_k=1, ldc=N, act=act, **how)
    return out


def _ln(x, ln, out, keep=None):
    """out = LayerNorm(x) (affine); keep: a list that receives the normalised rows xhat and their rstd (for the backward)."""
    rows, D = x.shape
    assert x.is_contiguous() and out.is_contiguous(), "bare pointers below: dense row-major operands"
    xhat = rstd = None
    if keep is not None:
        xhat, rstd = torch.empty_like(x), torch.empty(rows, device=x.device, dtype=torch.float32)
        keep += [xhat, rstd]
    _lib.call("as_layernorm_fwd", x, None, ln.weight, ln.bias, out, xhat, rstd, rows, D, 0)
    return out


def _ln_bwd(dxhat, xhat, rstd, out):
    rows, D = xhat.shape
    _lib.call("as_layernorm_bwd", dxhat, xhat, rstd, None, out, rows, D)
    return out


def _gelu_bwd(dy, x, scale, out):
    _lib.call("as_gelu_bwd", dy, x, scale, out, dy.numel(), scale.numel() if scale is not None else 0)
    return out


class _ScorerInputGrad(torch.autograd.Function):
    """(x, voicing) -> (logits, features) of a frozen DeepSpeech2 in eval mode, differentiable with respect to x only."""

    @staticmethod
    def forward(ctx, x, voicing, model):
        saved = {}
        logits, features = model._run(x, voicing, saved)
        ctx.model, ctx.saved, ctx.x_dtype = model, saved, x.dtype
        ctx.set_materialize_grads(False)
        return logits, features

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits, dfeatures):
        if dlogits is None and dfeatures is None:
            return None, None, None
        dx = ctx.model._backward(ctx.saved, dlogits, dfeatures)
        return dx.to(ctx.x_dtype), None, None


def _site_seed(seed, k):
    """Seed of dropout site k (0, 1: the two GELUs of residual block 0, ..., 2N + j: recurrent block j, 2N + M: the classifier's
    input) under a forward's seed: seed + k modulo 2^64."""
    return (seed + k) % (1 << 64)


def _dropout(t, drop, k, out=None):
    """out (default: t, in place) = t * keep / (1 - p) with site k's mask; the backward applies the same call to the gradient."""
    p, seed = drop
    out = t if out is None else out
    _lib.call("as_dropout_fwd", t, out, t.numel(), p, _site_seed(seed, k))
    return out


def top1_phonemes(logits):
    """``torch.topk(outputs, k=1, dim=-1).indices`` (phoneme_recognition/__init__.py:236, decoders.py:36)."""
    return torch.topk(logits, k=1, dim=-1).indices


class DeepSpeech2(nn.Module):
    def __init__(self, in_channels, num_residual_layers, num_rnn_layers, rnn_hidden_size, num_classes=31, num_features=80,
                 dropout=0.1, adapter_out_features=None):
        super().__init__()
        if adapter_out_features is not None:
            self.adapter = Adapter(num_features, adapter_out_features)
            num_features = adapter_out_features
        else:
            self.adapter = None
        self.cnn = nn.Conv2d(in_channels, OUT_CHANNELS, 3, stride=1, padding=1)
        self.residual_layers = nn.ModuleList([ResidualCNN(OUT_CHANNELS, num_features) for _ in range(num_residual_layers)])
        self.linear = nn.Linear(num_features * OUT_CHANNELS, rnn_hidden_size)
        self.recurrent_layers = nn.ModuleList([RecurrentBlock(rnn_hidden_size) for _ in range(num_rnn_layers)])
        self.feature_extractor = nn.Sequential(nn.Linear(rnn_hidden_size, rnn_hidden_size), nn.GELU())
        self.classifier = nn.Linear(rnn_hidden_size, num_classes)
        self.dropout_p = dropout  # nn.Dropout holds no state; eval-mode forward never applies it
        self.num_features, self.hidden, self.num_classes, self.in_channels = num_features, rnn_hidden_size, num_classes, in_channels
        self._prepared = None
        self._prepared_bwd = None

    @property
    def total_parameters(self):
        return sum(p.numel() for p in self.parameters())

    @staticmethod
    def get_noise_logits(x, factor):
        return x + factor * torch.randn_like(x)

    @staticmethod
    def get_normalized_outputs(x, use_log_prob=False):
        return (torch.log_softmax if use_log_prob else torch.softmax)(x, dim=-1)

    # ------------------------------------------------------------------ weights in kernel order (cached per version)
    def _prepare(self):
        # (address, version) of every parameter; the entry also holds the parameters' storages, so none of those
        # addresses can be freed and handed to a different tensor while the entry is alive
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._prepared is not None and self._prepared[0] == key:
            return self._prepared[1]
        keep = [p.untyped_storage() for p in self.parameters()]
        with torch.no_grad():
            taps = lambda conv: conv.weight.permute(2, 3, 0, 1).contiguous()  # [kd][kt][co][ci]
            D = self.num_features
            w = dict(stem=taps(self.cnn),
                     res=[(taps(r.cnn1), taps(r.cnn2)) for r in self.residual_layers],
                     # column c*D + d of the reference's (B, C*D, T) view -> column d*32 + c of a channels-last frame row
                     linear=self.linear.weight.view(self.hidden, OUT_CHANNELS, D).permute(0, 2, 1).reshape(self.hidden, -1).contiguous())
        self._prepared = (key, w, keep)
        self._prepared_bwd = None
        return w

    def _prepare_bwd(self):
        """Operands of the input gradient, cached like _prepare: every dX = dY . W as out = dY . W'^T with W' = W^T dense;
        the gammas of the adapter's LayerNorms folded into the Linear behind them (its dX is then d xhat); the 32 -> 32
        convolutions' taps flipped and transposed, w'[kd][kt][ci][co] = w[2 - kd][2 - kt][co][ci] (their data gradient is the
        same convolution); a zero bias for as_conv3x3_c32, which requires one."""
        w = self._prepare()
        if self._prepared_bwd is not None:
            return self._prepared_bwd
        with torch.no_grad():
            tr = lambda m: m.t().contiguous()
            flip = lambda conv: conv.weight.flip(2, 3).transpose(0, 1).permute(2, 3, 0, 1).contiguous()
            wb = dict(classifier=tr(self.classifier.weight), fe=tr(self.feature_extractor[0].weight),
                      w_ih=[tr(blk.rnn.weight_ih_l0) for blk in self.recurrent_layers], linear=tr(w["linear"]),
                      res=[(flip(r.cnn1), flip(r.cnn2)) for r in self.residual_layers],
                      zero_bias=torch.zeros(OUT_CHANNELS, device=self.cnn.weight.device, dtype=torch.float32))
            if self.adapter is not None:
                ad = self.adapter.adapter
                wb["adapter"] = (tr(ad[1].weight * ad[0].weight[None, :]), tr(ad[3].weight * ad[2].weight[None, :]))
        self._prepared_bwd = wb
        return wb

    def forward(self, x, voicing=None, return_features=False):
        """x (B, C, D, T) float32 on the GPU, voicing (B, T) or None -> logits (B, T, classes) [, features (B, T, H)].
        Differentiable with respect to x (only) when grad mode is on and x requires grad."""
        if self.training:
            raise RuntimeError("DeepSpeech2 (HIP): inference only -- call .eval() (the reference scores in eval mode)")
        _lib.require_gpu(x, "x")
        if torch.is_grad_enabled() and x.requires_grad:
            if any(p.requires_grad for p in self.parameters()):
                raise NotImplementedError(
                    "DeepSpeech2 (HIP): gradients reach the scorer's input only, not its parameters -- freeze the recognizer "
                    "(`for p in recognizer.parameters(): p.requires_grad = False`, as the reference trainer does)")
            logits, features = _ScorerInputGrad.apply(x, voicing, self)
        else:
            logits, features = self._run(x, voicing)
        return (logits, features) if return_features else logits

    def _run(self, x, voicing, keep=None, drop=None):
        """The forward on the HIP library; keep (a dict) receives what _backward needs -- and, when it holds a "train" entry,
        what its parameter gradients need (without one those slots of the per-layer records are None).  drop: None, or (p, seed):
        training-mode dropout at the reference's sites, site k's mask being as_dropout_fwd's at _site_seed(seed, k)
        (TrainableDeepSpeech2)."""
        train = keep is not None and "train" in keep
        B, Cin, Din, T = x.shape
        assert Cin == self.in_channels
        x = x.float()
        dev, f32 = x.device, torch.float32
        w = self._prepare()
        D, H = self.num_features, self.hidden
        kad = None
        with torch.no_grad():
            if self.adapter is not None:
                ad = self.adapter.adapter
                # the reference's own transpose (:84); glue copy of the input.  (.contiguous(): with B = C = 1 the reshape of the
                # transposed view is itself a VIEW with strides (1, T) -- the kernels below take bare pointers)
                rows = x.transpose(2, 3).reshape(B * Cin * T, Din).contiguous()
                kad = [] if keep is not None else None
                a0 = _ln(rows, ad[0], torch.empty_like(rows), kad)
                a = _gemm(a0, ad[1].weight, ad[1].bias, torch.empty(rows.shape[0], D, device=dev, dtype=f32))
                a = _ln(a, ad[2], torch.empty_like(a), kad)
                planes = _gemm(a, ad[3].weight, ad[3].bias, torch.empty_like(a))  # (B, C, T, D)
                if train:
                    keep.update(adapter_in=(a0, a))
                strides = (Cin * T * D, T * D, 1, D)
            else:
                assert Din == D
                planes = x.contiguous()  # (B, C, D, T)
                strides = (Cin * D * T, D * T, T, 1)
            if voicing is not None:
                voicing = voicing.to(device=dev, dtype=f32).contiguous()
            fmap = torch.empty(B, T, D, OUT_CHANNELS, device=dev, dtype=f32)
            sb, sc, sd, st = strides
            _lib.call("as_conv3x3_stem", planes, sb, sc, sd, st, w["stem"], self.cnn.bias, voicing, fmap, B, T, D, Cin)
            act, mid = torch.empty_like(fmap), torch.empty_like(fmap)
            kres = []
            act2 = act
            for i, (r, (w1, w2)) in enumerate(zip(self.residual_layers, w["res"])):
                if keep is not None:   # the block's input and its pre-LN2 map (training: also both convolutions' inputs)
                    mid = torch.empty_like(fmap)
                    if train:
                        act, act2 = torch.empty_like(fmap), torch.empty_like(fmap)
                    kres.append((fmap, mid, act, act2) if train else (fmap, mid, None, None))
                _lib.call("as_ln_feat_gelu", fmap, r.layer_norm1.weight, r.layer_norm1.bias, act, B * T, D, OUT_CHANNELS)
                if drop:
                    _dropout(act, drop, 2 * i)
                _lib.call("as_conv3x3_c32", act, w1, r.cnn1.bias, None, mid, B, T, D)
                _lib.call("as_ln_feat_gelu", mid, r.layer_norm2.weight, r.layer_norm2.bias, act2, B * T, D, OUT_CHANNELS)
                if drop:
                    _dropout(act2, drop, 2 * i + 1)
                nxt = torch.empty_like(fmap)
                _lib.call("as_conv3x3_c32", act2, w2, r.cnn2.bias, fmap, nxt, B, T, D)
                fmap = nxt
            if train:
                keep.update(planes_t=planes, lin_in=fmap)
            h = _gemm(fmap.view(B * T, D * OUT_CHANNELS), w["linear"], self.linear.bias, torch.empty(B * T, H, device=dev, dtype=f32),
                      split_k=True)  # K = 32 * D (2560) against N = H (64) columns
            lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
            gi = torch.empty(B * T, 3 * H, device=dev, dtype=f32)
            krnn = []
            nres = len(self.residual_layers)
            for j, blk in enumerate(self.recurrent_layers):
                # keep: the same values, keeping the LayerNorm's xhat / rstd, the GELU's input and the GRU's gates
                kln = [] if keep is not None else None
                a = _ln(h, blk.layer_norm, torch.empty_like(h), kln)
                ag = torch.empty_like(a) if keep is not None else a
                _lib.call("as_gelu", a, ag, a.numel())
                _gemm(ag, blk.rnn.weight_ih_l0, blk.rnn.bias_ih_l0, gi)
                h = torch.empty_like(h)
                if keep is None:
                    _lib.call("as_gru_unidir_fwd", gi, blk.rnn.weight_hh_l0, blk.rnn.bias_hh_l0, lengths, B, T, H, h)
                    if drop:
                        _dropout(h, drop, 2 * nres + j)
                else:
                    gates = torch.empty(B * T, 4 * H, device=dev, dtype=f32)
                    _lib.call("as_gru_unidir_fwd_gates", gi, blk.rnn.weight_hh_l0, blk.rnn.bias_hh_l0, lengths, B, T, H, h, gates)
                    krnn.append((kln[0], kln[1], a, h, gates, ag if train else None))
                    if drop:   # the GRU's own output stays in krnn (its backward and dW_hh read it); the next block reads the copy
                        h = _dropout(h, drop, 2 * nres + j, torch.empty_like(h))
            fe = self.feature_extractor[0]
            features = _gemm(h, fe.weight, fe.bias, torch.empty_like(h), act=3)
            cls_in = _dropout(features, drop, 2 * nres + len(self.recurrent_layers), torch.empty_like(features)) if drop else features
            logits = _gemm(cls_in, self.classifier.weight, self.classifier.bias,
                           torch.empty(B * T, self.num_classes, device=dev, dtype=f32))
            if train:
                keep.update(fe_in=h, cls_in=cls_in)
            if keep is not None:
                keep.update(shape=(B, Cin, Din, T), planes=(tuple(planes.shape), strides), adapter=kad, res=kres, rnn=krnn,
                            lengths=lengths, fe_pre=_gemm(h, fe.weight, fe.bias, torch.empty_like(h)))
        return logits.view(B, T, -1), features.view(B, T, H)

    def _backward(self, saved, dlogits, dfeatures, drop=None, grads=None, need_dx=True):
        """d(logits, features) -> dx (B, C, D, T): the layers of _run in reverse.  drop: the forward's (p, seed) or None (its masks
        are regenerated).  grads: None (a frozen scorer: no parameter gradients), or a dict that receives every parameter's gradient
        by name -- as_gemm_f32 for the Linear / GRU weights and biases (dW_hh over h_{t-1}), as_conv3x3_c32_wgrad /
        as_conv3x3_stem_wgrad for the convolutions, as_ln_feat_gelu_param_grad / as_layernorm_param_grad for the LayerNorms; it
        needs the "train" entries of saved.  The launches that lead to dx are the same either way, so dx is too, bit for bit.
        need_dx false (with grads only): the walk stops behind the first layer's parameter gradients and returns None."""
        wb = self._prepare_bwd()
        w = self._prepare()
        B, Cin, Din, T = saved["shape"]
        D, H, M = self.num_features, self.hidden, B * T
        dev, f32 = saved["lengths"].device, torch.float32
        nres, nrnn = len(self.residual_layers), len(self.recurrent_layers)
        g, train = grads, grads is not None
        empty = lambda *s: torch.empty(*s, device=dev, dtype=f32)
        with torch.no_grad():
            # logits = dropout(features) W_cls^T + b_cls; features = gelu(h W_fe^T + b_fe)
            if dlogits is not None:
                dl = dlogits.reshape(M, -1).float().contiguous()
                if train:
                    g["classifier.weight"] = _wgrad(dl, saved["cls_in"], empty(self.num_classes, H),
                                                    g.setdefault("classifier.bias", empty(self.num_classes)))
                df = _gemm(dl, wb["classifier"], None, empty(M, H))
                if drop:
                    _dropout(df, drop, 2 * nres + nrnn)
                if dfeatures is not None:
                    dfc = dfeatures.reshape(M, H).float().contiguous()
                    _lib.call("as_add", df, dfc, df, df.numel())
            else:
                df = dfeatures.reshape(M, H).float().contiguous().clone()
            _gelu_bwd(df, saved["fe_pre"], None, df)
            if train:
                g["feature_extractor.0.weight"] = _wgrad(df, saved["fe_in"], empty(H, H), g.setdefault("feature_extractor.0.bias", empty(H)))
            dh = _gemm(df, wb["fe"], None, empty(M, H))
            # recurrent blocks: h_out = dropout(GRU(gelu(LN(h_in))))
            dgi = empty(M, 3 * H)
            dgh = torch.empty_like(dgi)
            da = empty(M, H)
            for j in reversed(range(nrnn)):
                blk, w_ih_t = self.recurrent_layers[j], wb["w_ih"][j]
                xhat, rstd, a, h_out, gates, ag = saved["rnn"][j]
                pre = f"recurrent_layers.{j}."
                if drop:
                    _dropout(dh, drop, 2 * nres + j)
                _lib.call("as_gru_unidir_bwd", dh, h_out, gates, blk.rnn.weight_hh_l0, saved["lengths"], B, T, H, dgi, dgh)
                if train:
                    g[pre + "rnn.weight_ih_l0"] = _wgrad(dgi, ag, empty(3 * H, H), g.setdefault(pre + "rnn.bias_ih_l0", empty(3 * H)))
                    g[pre + "rnn.weight_hh_l0"] = _wgrad(dgh, h_out, empty(3 * H, H), g.setdefault(pre + "rnn.bias_hh_l0", empty(3 * H)),
                                                         shift=T)
                _gemm(dgi, w_ih_t, None, da)
                if train:
                    _ln_param_grad(_gelu_bwd(da, a, None, empty(M, H)), xhat, blk.layer_norm, g, pre + "layer_norm")
                _gelu_bwd(da, a, blk.layer_norm.weight, da)     # d xhat = d gelu-out * gelu'(a) * gamma
                dh = _ln_bwd(da, xhat, rstd, torch.empty_like(da))
            # Linear(32 D -> H) over the channels-last frame rows; its weight gradient back in the reference's column order c*D + d
            if train:
                dwl = _wgrad(dh, saved["lin_in"].view(M, D * OUT_CHANNELS), empty(H, D * OUT_CHANNELS), g.setdefault("linear.bias", empty(H)))
                g["linear.weight"] = dwl.view(H, D, OUT_CHANNELS).permute(0, 2, 1).reshape(H, OUT_CHANNELS * D)
            dmap = _gemm(dh, wb["linear"], None, empty(M, D * OUT_CHANNELS))
            # residual blocks: out = conv2(drop(lngelu2(conv1(drop(lngelu1(in)))))) + in
            dact, dmid = torch.empty_like(dmap), torch.empty_like(dmap)
            zb = wb["zero_bias"]
            slab = _slab(dev) if train else None
            taps_grad = lambda dwk, cin: dwk.view(3, 3, OUT_CHANNELS, cin).permute(2, 3, 0, 1).contiguous()   # [kd][kt][co][ci] -> torch

            def c32_wgrad(x, dy, name):
                dwk, dbk = empty(9, OUT_CHANNELS, OUT_CHANNELS), empty(OUT_CHANNELS)
                _lib.call("as_conv3x3_c32_wgrad", x, dy, dwk, dbk, B, T, D, slab, slab.numel())
                g[name + ".weight"], g[name + ".bias"] = taps_grad(dwk, OUT_CHANNELS), dbk

            for i in reversed(range(nres)):
                r, (f1, f2), (fin, mid, act1, act2) = self.residual_layers[i], wb["res"][i], saved["res"][i]
                pre = f"residual_layers.{i}."
                if train:
                    c32_wgrad(act2, dmap, pre + "cnn2")
                _lib.call("as_conv3x3_c32", dmap, f2, zb, None, dact, B, T, D)
                if drop:
                    _dropout(dact, drop, 2 * i + 1)
                if train:
                    _ln_feat_param_grad(mid, r.layer_norm2, dact, g, pre + "layer_norm2")
                _lib.call("as_ln_feat_gelu_bwd", mid, r.layer_norm2.weight, r.layer_norm2.bias, dact, None, dmid, M, D, OUT_CHANNELS)
                if train:
                    c32_wgrad(act1, dmid, pre + "cnn1")
                _lib.call("as_conv3x3_c32", dmid, f1, zb, None, dact, B, T, D)
                if drop:
                    _dropout(dact, drop, 2 * i)
                if train:
                    _ln_feat_param_grad(fin, r.layer_norm1, dact, g, pre + "layer_norm1")
                nxt = torch.empty_like(dmap)
                _lib.call("as_ln_feat_gelu_bwd", fin, r.layer_norm1.weight, r.layer_norm1.bias, dact, dmap, nxt, M, D, OUT_CHANNELS)
                dmap = nxt
            # stem: into the planes the forward read (voicing gets no gradient)
            pshape, (sb, sc, sd, st) = saved["planes"]
            if train:
                dwk, dbk = empty(9, OUT_CHANNELS, Cin), empty(OUT_CHANNELS)
                _lib.call("as_conv3x3_stem_wgrad", saved["planes_t"], sb, sc, sd, st, dmap, dwk, dbk, B, T, D, Cin, slab, slab.numel())
                g["cnn.weight"], g["cnn.bias"] = taps_grad(dwk, Cin), dbk
                if self.adapter is None and not need_dx:
                    return None
            dplanes = empty(*pshape)
            _lib.call("as_conv3x3_stem_bwd", dmap, w["stem"], dplanes, sb, sc, sd, st, B, T, D, Cin)
            if self.adapter is None:
                return dplanes
            # adapter: LN0 -> Linear1 -> LN2 -> Linear3 over (B, C, T, D) rows; for dx the gammas sit in the folded weights
            ad = self.adapter.adapter
            xhat0, rstd0, xhat2, rstd2 = saved["adapter"]
            w1g_t, w3g_t = wb["adapter"]
            if train:
                a0, a2 = saved["adapter_in"]
                g["adapter.adapter.3.weight"] = _wgrad(dplanes, a2, empty(D, D), g.setdefault("adapter.adapter.3.bias", empty(D)))
                dz2 = _gemm(dplanes, ad[3].weight.t().contiguous(), None, empty(dplanes.shape[0], D))
                _ln_param_grad(dz2, xhat2, ad[2], g, "adapter.adapter.2")
            dxhat2 = _gemm(dplanes, w3g_t, None, torch.empty_like(dplanes))
            dl1 = _ln_bwd(dxhat2, xhat2, rstd2, dxhat2)
            if train:
                g["adapter.adapter.1.weight"] = _wgrad(dl1, a0, empty(D, Din), g.setdefault("adapter.adapter.1.bias", empty(D)))
                dz0 = _gemm(dl1, ad[1].weight.t().contiguous(), None, empty(dl1.shape[0], Din))
                _ln_param_grad(dz0, xhat0, ad[0], g, "adapter.adapter.0")
                if not need_dx:
                    return None
            dxhat0 = _gemm(dl1, w1g_t, None, empty(dl1.shape[0], Din))
            drows = _ln_bwd(dxhat0, xhat0, rstd0, dxhat0)
            return drows.view(B, Cin, T, Din).transpose(2, 3)


def _wgrad(dy, x, dw, db=None, shift=None):
    """dw[n][k] = sum_m dy[m][n] x[m][k] (db[n] = sum_m dy[m][n]) on the exact fp32 instruction, deterministic split-K;
    shift = T: x is read one frame back within each utterance (h_{t-1} of dW_hh, zero at t = 0)."""
    R, N, K = dy.shape[0], dy.shape[1], x.shape[1]
    slab = _slab(dy.device)
    back = dict(b_kshift=-1, b_kT=shift) if shift is not None else {}
    _lib.gemm(A=dy, B=x, C=dw, M=N, N=K, K=R, a_i=1, a_k=N, b_j=1, b_k=K, ldc=K, precision=0, colsum=db, splitk_ws=slab,
              splitk_ws_floats=slab.numel(), **back)
    return dw


def _ln_param_grad(dz, xhat, ln, grads, name):
    rows, D = xhat.shape
    dg, db = torch.empty(D, device=dz.device, dtype=torch.float32), torch.empty(D, device=dz.device, dtype=torch.float32)
    slab = _slab(dz.device)
    _lib.call("as_layernorm_param_grad", dz, xhat, rows, D, dg, db, slab, slab.numel())
    grads[name + ".weight"], grads[name + ".bias"] = dg, db


def _ln_feat_param_grad(x, ln, dy, grads, name):
    D = ln.weight.numel()
    dg, db = torch.empty(D, device=x.device, dtype=torch.float32), torch.empty(D, device=x.device, dtype=torch.float32)
    slab = _slab(x.device)
    _lib.call("as_ln_feat_gelu_param_grad", x, ln.weight, ln.bias, dy, x.numel() // (D * OUT_CHANNELS), D, OUT_CHANNELS, dg, db, slab,
              slab.numel())
    grads[name + ".weight"], grads[name + ".bias"] = dg, db


class _ScorerTrain(torch.autograd.Function):
    """(x, voicing, *parameters) -> (logits, features) of TrainableDeepSpeech2, differentiable with respect to x and every
    parameter; drop: None or the forward's (p, seed)."""

    @staticmethod
    def forward(ctx, x, voicing, model, drop, *params):
        saved = {"train": True}
        logits, features = model._run(x, voicing, saved, drop)
        ctx.model, ctx.saved, ctx.drop, ctx.x_dtype = model, saved, drop, x.dtype
        ctx.set_materialize_grads(False)
        return logits, features

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits, dfeatures):
        names = [n for n, _ in ctx.model.named_parameters()]
        if dlogits is None and dfeatures is None:
            return (None, None, None, None) + (None,) * len(names)
        grads = {}
        dx = ctx.model._backward(ctx.saved, dlogits, dfeatures, ctx.drop, grads, ctx.needs_input_grad[0])
        dx = dx.to(ctx.x_dtype) if dx is not None else None
        return (dx, None, None, None) + tuple(grads.get(n) for n in names)


class TrainableDeepSpeech2(DeepSpeech2):
    """DeepSpeech2 that trains (train_phoneme_recognition.py): the same constructor, state_dict keys and seed-for-seed
    initialisation, so checkpoints load into either class.  ``forward(x, voicing=None, return_features=False)``:

    * with grad enabled and any parameter or x requiring grad it runs ``_ScorerTrain``, whose backward fills every parameter's
      ``.grad`` (and x's): ``DeepSpeech2._backward``, the frozen scorer's walk, with the parameter gradients added at every
      layer; otherwise ``_run``;
    * in ``train()`` mode -- with or without grad, as nn.Dropout -- the reference's dropout (deepspeech2.py:35, 43, 69, 190):
      after both GELUs of every ResidualCNN, after every RecurrentBlock's GRU, before the classifier (the returned features are
      not dropped).  Each forward draws one seed from torch's CPU generator (``int(torch.randint(0, 2**62, (1,)))``); site k
      uses ``_site_seed(seed, k)`` with as_dropout_fwd, so ``as_dropout_fwd`` on a tensor of ones rebuilds any mask, and the
      backward regenerates the masks instead of storing them.  The last forward's seed is kept in ``last_dropout_seed``.
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.last_dropout_seed = None

    def forward(self, x, voicing=None, return_features=False):
        _lib.require_gpu(x, "x")
        drop = None
        if self.training and self.dropout_p > 0.0:
            drop = (float(self.dropout_p), int(torch.randint(0, 2 ** 62, (1,))))
            self.last_dropout_seed = drop[1]
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            logits, features = _ScorerTrain.apply(x, voicing, self, drop, *params)
        else:
            logits, features = self._run(x, voicing, None, drop)
        return (logits, features) if return_features else logits
