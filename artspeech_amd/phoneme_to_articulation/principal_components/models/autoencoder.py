"""Per-articulator autoencoders of the principal-components method (reference principal_components/models/autoencoder.py):
the closed-form ``PCAEncoder`` / ``PCADecoder`` (:10-80), the MLP ``Encoder`` / ``Decoder`` (:83-111), their multi-articulator
containers (:124-213) and ``MultiArticulatorAutoencoder`` (:216-255), with the reference's constructors, ``state_dict`` keys
and seed-for-seed initial weights.

A ``MultiEncoder`` / ``MultiDecoder`` runs all its articulators in ONE launch per direction (``as_multi_mlp_fwd`` /
``as_multi_mlp_bwd``, artspeech_amd/csrc/multi_mlp.hip): the encoder reads its slices of the (rows, A, in_features) input and
takes the maximum over the articulators that own each latent index inside the kernel (tanh fused when the autoencoder applies
it), the decoder gathers its latent indices and stacks its outputs.  Widths beyond the kernel's LDS budget, or every width
while ``FUSED_MLP`` is set to False (A/B runs), take the per-articulator path: every Linear a ``GroupedLinear`` GEMM, the
slicing / max over articulators torch glue.
"""
from enum import Enum

import torch
import torch.nn as nn

from .... import _lib
from ....helpers import make_indices_dict
from ...transformer.ops import GroupedLinear


FUSED_MLP = True  # False: the per-articulator GEMM path at every width (A/B hook of the tests and tools/bench_pc_training.py)


def _linear(x, W, b, relu):
    """rows x [R, K] -> [R, N] on the GEMM path (the per-articulator fallback)."""
    if b is None:
        b = torch.zeros(W.shape[0], dtype=torch.float32, device=x.device)
    return GroupedLinear.apply(x[None], W[None], b[None], (0,), relu)[0]


def _mlp(seq, x):
    """nn.Sequential(Linear, ReLU, Linear, ReLU, Linear) of parameter containers on rows x [R, in] -> [R, out]."""
    _lib.require_gpu(x, "x")
    h = x.reshape(-1, x.shape[-1]).float()
    for idx, relu in ((0, True), (2, True), (4, False)):
        lin = seq[idx]
        h = _linear(h, lin.weight, lin.bias, relu)
    return h.reshape(*x.shape[:-1], h.shape[-1])


def _nonzero_mean(mean):
    return mean is not None and bool((mean != 0).any())


def _cached_projection(module, build):
    """module.projection(): rebuilt whenever a gradient has to flow through it, else reused while the parameters keep their
    storage and version (frozen projections, AutoencoderLoss2 / DecoderMeanP2CPDistance2: one fold per weight update, and
    the kernel's pointer table stays cached)."""
    params = (module.eigenvalues, module.eigenvectors)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return build()
    key = (module.whiten, module.mean.data_ptr(), module.mean._version) + tuple((p.data_ptr(), p._version) for p in params)
    cache = getattr(module, "_projection_cache", None)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            cache = (key, build())
        module._projection_cache = cache
    return cache[1]


class PCAEncoder(nn.Module):
    """z = (x - mean) eigenvectors^T, / sqrt(eigenvalues) if whiten (reference :10-39); parameters in the reference's shapes
    and torch.rand order.  The whitening is folded into the projection: one Linear (layers = 1) of the fused kernel."""

    def __init__(self, in_features, num_components, mean=None, whiten=False, **kwargs):
        super().__init__()
        self.eigenvalues = nn.Parameter(torch.rand(size=(num_components,)))
        self.eigenvectors = nn.Parameter(torch.rand(size=(num_components, in_features)))
        self.mean = mean or torch.zeros(size=(in_features,))
        self.whiten = whiten

    def projection(self):
        """(W [num_components][in_features], b [num_components] or None): z = x W^T + b."""
        return _cached_projection(self, self._build_projection)

    def _build_projection(self):
        W = self.eigenvectors
        if self.whiten:
            W = W / torch.sqrt(self.eigenvalues)[:, None]
        b = -(W @ self.mean.to(W.device)) if _nonzero_mean(self.mean) else None
        return W.contiguous(), b

    def forward(self, x):
        _lib.require_gpu(x, "x")
        W, b = self.projection()
        return _single(x, W, b)


class PCADecoder(nn.Module):
    """out = z eigenvectors + mean (reference :42-80), z (bs, length, num_components).  ``whiten=True`` is refused: the
    reference's expression there, ``torch.mm(z, sqrt(eigenvalues)) * eigenvectors``, only broadcasts for special shapes, and
    MultiDecoder never sets it."""

    def __init__(self, out_features, num_components, mean=None, whiten=False, **kwargs):
        super().__init__()
        if whiten:
            raise NotImplementedError("PCADecoder(whiten=True): the reference's whitened reconstruction is not a well-formed "
                                      "product for general shapes; MultiDecoder never uses it")
        self.eigenvalues = nn.Parameter(torch.rand(size=(num_components, 1)))
        self.eigenvectors = nn.Parameter(torch.rand(size=(num_components, out_features)))
        self.mean = mean or torch.zeros(size=(out_features,))
        self.whiten = whiten

    def projection(self):
        """(W [out_features][num_components], b [out_features] or None): out = z W^T + b."""
        return _cached_projection(self, self._build_projection)

    def _build_projection(self):
        b = self.mean.to(self.eigenvectors.device) if _nonzero_mean(self.mean) else None
        return self.eigenvectors.t().contiguous(), b

    def forward(self, z):
        _lib.require_gpu(z, "z")
        bs, length, _ = z.shape
        W, b = self.projection()
        return _single(z, W, b).reshape(bs, length, W.shape[0])


class Encoder(nn.Module):
    def __init__(self, in_features, num_components, hidden_features):
        super().__init__()
        self.encoder = nn.Sequential(nn.Linear(in_features, hidden_features), nn.ReLU(),
                                     nn.Linear(hidden_features, hidden_features // 2), nn.ReLU(),
                                     nn.Linear(hidden_features // 2, num_components))

    def forward(self, x):
        return _mlp(self.encoder, x)


class Decoder(nn.Module):
    def __init__(self, num_components, out_features, hidden_features):
        super().__init__()
        self.decoder = nn.Sequential(nn.Linear(num_components, hidden_features // 2), nn.ReLU(),
                                     nn.Linear(hidden_features // 2, hidden_features), nn.ReLU(),
                                     nn.Linear(hidden_features, out_features))

    def forward(self, x):
        return _mlp(self.decoder, x)


class EncoderType(Enum):
    AE = Encoder
    PCA = PCAEncoder


class DecoderType(Enum):
    AE = Decoder
    PCA = PCADecoder


def _resolve(indices_dict):
    if isinstance(list(indices_dict.values())[0], int):
        indices_dict = make_indices_dict(indices_dict)
    latent_size = max(i for indices in indices_dict.values() for i in indices) + 1
    return indices_dict, latent_size, sorted(indices_dict.keys())


def _resolve_cls(cls, enum):
    if isinstance(cls, str):
        cls = enum[cls].value
    if cls not in {member.value for member in enum}:
        raise NotImplementedError(f"{cls!r}: only {[m.name for m in enum]} are built on the C ABI")
    return cls


def _group_params(module):
    """[W1, b1, W2, b2, W3, b3] of an Encoder / Decoder, [W, b] of a PCA projection (b may be None)."""
    if isinstance(module, (PCAEncoder, PCADecoder)):
        return list(module.projection())
    seq = module.encoder if isinstance(module, Encoder) else module.decoder
    return [t for idx in (0, 2, 4) for t in (seq[idx].weight, seq[idx].bias)]


# ------------------------------------------------------------------------------------------------ the fused kernel
class _Plan:
    """Geometry and index tables of one MultiEncoder (slice -> max-scatter) or MultiDecoder (gather -> stack)."""

    def __init__(self, encoder, indices_dict, sorted_articulators, latent_size, features, layers, hidden):
        self.encoder, self.layers, self.latent = encoder, layers, latent_size
        self.h1, self.h2 = (hidden, hidden // 2) if encoder else (hidden // 2, hidden)
        if layers == 1:
            self.h1 = self.h2 = 0
        idx = [list(indices_dict[a]) for a in sorted_articulators]
        self.G = len(idx)
        widths = [len(i) for i in idx]
        self.dims = [(features, w) if encoder else (w, features) for w in widths]
        self.k_max, self.n_max = max(d[0] for d in self.dims), max(d[1] for d in self.dims)
        width = self.n_max if encoder else self.k_max
        self.idx = [i + [-1] * (width - len(i)) for i in idx]
        own_ptr, own = [0], []
        for j in range(latent_size):
            own += [g * width + p for g, i in enumerate(idx) for p, v in enumerate(i) if v == j]
            own_ptr.append(len(own))
        self.own_ptr, self.own = own_ptr, own or [0]
        self.supported = bool(_lib.call("as_multi_mlp_supported", layers, self.k_max, self.h1, self.h2, self.n_max))
        self.P = int(_lib.call("as_multi_mlp_param_floats", layers, self.k_max, self.h1, self.h2, self.n_max))
        self._dev, self._ptr_tables = {}, {}

    def tables(self, dev):
        if dev not in self._dev:
            t32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
            self._dev[dev] = (t32(self.dims), t32(self.idx), t32(self.own_ptr), t32(self.own))
        return self._dev[dev]

    def ptr_table(self, dev, params):
        key = (dev, tuple(0 if p is None else p.data_ptr() for p in params))
        table = self._ptr_tables.get(key)
        if table is None:
            if len(self._ptr_tables) >= 16:
                self._ptr_tables.clear()
            per = 2 * self.layers
            flat = []
            for g in range(self.G):
                ps = [0 if p is None else p.data_ptr() for p in params[g * per:(g + 1) * per]]
                flat += ps + [0] * (6 - per)
            table = self._ptr_tables[key] = torch.tensor(flat, dtype=torch.int64, device=dev)
        return table

    def geometry(self, g, l):
        """(wout, win, slot offset of W, offset of b) of layer l of group g in the packed gradient slot."""
        K, N = self.dims[g]
        wins, wouts = ([self.k_max], [self.n_max]) if self.layers == 1 else ([self.k_max, self.h1, self.h2], [self.h1, self.h2, self.n_max])
        ins, outs = ([K], [N]) if self.layers == 1 else ([K, self.h1, self.h2], [self.h1, self.h2, N])
        off = sum(wouts[i] * wins[i] + wouts[i] for i in range(l))
        return outs[l], ins[l], off, off + wouts[l] * wins[l]


def _descriptor(plan, x, scale, act, table, ptrs):
    dims, idx, own_ptr, own = table
    d = _lib.MultiMlp()
    d.groups, d.layers, d.h1, d.h2, d.k_max, d.n_max, d.latent = plan.G, plan.layers, plan.h1, plan.h2, plan.k_max, plan.n_max, plan.latent
    d.dims, d.params, d.own_ptr, d.own = dims.data_ptr(), ptrs.data_ptr(), own_ptr.data_ptr(), own.data_ptr()
    d.x, d.in_scale, d.act = x.data_ptr(), float(scale), int(act)
    if plan.encoder:
        if x.dim() < 2 or x.shape[-2] < plan.G or x.shape[-1] != plan.k_max:
            raise ValueError(f"encoder input {tuple(x.shape)}: expected (..., >= {plan.G}, {plan.k_max})")
        d.in_mode, d.out_mode, d.out_idx = 0, 1, idx.data_ptr()
        d.rows, d.x_r, d.x_g = x.numel() // (x.shape[-2] * x.shape[-1]), x.shape[-2] * x.shape[-1], x.shape[-1]
    else:
        if x.shape[-1] < plan.latent:
            raise ValueError(f"decoder input {tuple(x.shape)}: expected (..., >= {plan.latent})")
        d.in_mode, d.out_mode, d.in_idx = 1, 0, idx.data_ptr()
        d.rows, d.x_r, d.x_g = x.numel() // x.shape[-1], x.shape[-1], 0
    return d


class _MultiMlpFn(torch.autograd.Function):
    """encoder: x (..., A, K) -> latent (..., L) [act(max over owners)];  decoder: x (..., >= L) -> (..., G, N)."""

    @staticmethod
    def forward(ctx, plan, scale, act, x, *params):
        _lib.require_gpu(x, "x")
        x = x.contiguous().float()
        params = [None if p is None else p.contiguous() for p in params]
        dev = x.device
        table, ptrs = plan.tables(dev), plan.ptr_table(dev, params)
        d = _descriptor(plan, x, scale, act, table, ptrs)
        lead = x.shape[:-2] if plan.encoder else x.shape[:-1]
        win = None
        if plan.encoder:
            y = torch.empty((d.rows, plan.latent), dtype=torch.float32, device=dev)
            win = torch.empty((d.rows, plan.latent), dtype=torch.int32, device=dev)
            d.y, d.y_r, d.win = y.data_ptr(), plan.latent, win.data_ptr()
        else:
            y = torch.empty((d.rows, plan.G, plan.n_max), dtype=torch.float32, device=dev)
            d.y, d.y_r, d.y_g = y.data_ptr(), plan.G * plan.n_max, plan.n_max
        n = _lib.call("as_multi_mlp_workspace_floats", d, 0)
        ws = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        d.ws, d.ws_floats = ws.data_ptr(), n
        _lib.call("as_multi_mlp_fwd", d)
        ctx.plan, ctx.scale, ctx.act = plan, scale, act
        ctx.save_for_backward(x, y, win, ptrs, *params)
        return y.reshape(*lead, plan.latent) if plan.encoder else y.reshape(*lead, plan.G, plan.n_max)

    @staticmethod
    def backward(ctx, dy):
        plan = ctx.plan
        x, y, win, ptrs, *params = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[3]
        need_dp = any(ctx.needs_input_grad[4:])
        if not (need_dx or need_dp):
            return (None,) * (4 + len(params))
        dev = x.device
        d = _descriptor(plan, x, ctx.scale, ctx.act, plan.tables(dev), ptrs)
        dy = dy.contiguous().float()
        d.dy = dy.data_ptr()
        if plan.encoder:
            d.y, d.y_r, d.win = y.data_ptr(), plan.latent, win.data_ptr()
        else:
            d.y, d.y_r, d.y_g = y.data_ptr(), plan.G * plan.n_max, plan.n_max
        dx = dparams = None
        if need_dx:
            covered = (x.shape[-2] == plan.G) if plan.encoder else (x.shape[-1] == plan.latent)
            dx = torch.empty_like(x) if covered else torch.zeros_like(x)
            d.dx = dx.data_ptr()
        if need_dp:
            dparams = torch.empty((plan.G, plan.P), dtype=torch.float32, device=dev)
            d.dparams = dparams.data_ptr()
        n = _lib.call("as_multi_mlp_workspace_floats", d, 1)
        ws = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        d.ws, d.ws_floats = ws.data_ptr(), n
        _lib.call("as_multi_mlp_bwd", d)
        grads = [None] * len(params)
        if need_dp:
            per = 2 * plan.layers
            for g in range(plan.G):
                for l in range(plan.layers):
                    wout, win_, w_off, b_off = plan.geometry(g, l)
                    i = g * per + 2 * l
                    if ctx.needs_input_grad[4 + i]:
                        grads[i] = dparams[g, w_off:w_off + wout * win_].view(wout, win_)
                    if ctx.needs_input_grad[5 + i]:
                        grads[i + 1] = dparams[g, b_off:b_off + wout]
        return (None, None, None, dx, *grads)


def _single(x, W, b):
    """One projection x [..., K] -> [..., N] (a PCAEncoder / PCADecoder on its own): the fused kernel with one group."""
    if not FUSED_MLP:
        return _linear(x.reshape(-1, x.shape[-1]).float(), W, b, False).reshape(*x.shape[:-1], W.shape[0])
    N, K = W.shape
    plan = _single_plan(K, N)
    if not plan.supported:   # beyond the kernel's LDS budget: the GEMM path, like the containers
        return _linear(x.reshape(-1, x.shape[-1]).float(), W, b, False).reshape(*x.shape[:-1], N)
    out = _MultiMlpFn.apply(plan, 1.0, 0, x.reshape(-1, 1, K), W, b)
    return out.reshape(*x.shape[:-1], N)


_SINGLE_PLANS = {}


def _single_plan(K, N):
    """a one-group 'decoder' plan whose gather reads every input column in order (in_idx = 0..K-1)"""
    if (K, N) not in _SINGLE_PLANS:
        _SINGLE_PLANS[(K, N)] = _Plan(False, {"x": list(range(K))}, ["x"], K, N, 1, 0)
    return _SINGLE_PLANS[(K, N)]


def _fused_params(modules):
    return [t for m in modules for t in _group_params(m)]


class MultiEncoder(nn.Module):
    """One encoder per articulator; every latent index takes the maximum over the articulators that own it (:124-173)."""

    def __init__(self, indices_dict, in_features, hidden_features, encoder_cls=Encoder):
        super().__init__()
        self.indices_dict, self.latent_size, self.sorted_articulators = _resolve(indices_dict)
        encoder_cls = _resolve_cls(encoder_cls, EncoderType)
        self.encoders = nn.ModuleDict({articulator: encoder_cls(in_features=in_features, num_components=len(indices),
                                                                hidden_features=hidden_features)
                                       for articulator, indices in self.indices_dict.items()})
        layers = 1 if encoder_cls is PCAEncoder else 3
        self._plan = _Plan(True, self.indices_dict, self.sorted_articulators, self.latent_size, in_features, layers, hidden_features)

    def forward(self, x):
        """x (bs, n_articulators, in_features), channels in sorted-articulator order -> (bs, latent_size)."""
        return self._forward(x, tanh=False)

    def _forward(self, x, tanh):
        _lib.require_gpu(x, "x")
        if FUSED_MLP and self._plan.supported:
            modules = [self.encoders[a] for a in self.sorted_articulators]
            return _MultiMlpFn.apply(self._plan, 1.0, int(tanh), x, *_fused_params(modules))
        lead = x.shape[:-2]
        spaces = []
        for i, articulator in enumerate(self.sorted_articulators):
            space = torch.full((*lead, self.latent_size), -torch.inf, dtype=torch.float32, device=x.device)
            space[..., self.indices_dict[articulator]] = self.encoders[articulator](x[..., i, :])
            spaces.append(space)
        latent = torch.stack(spaces, dim=-2).max(dim=-2).values
        return torch.tanh(latent) if tanh else latent


class MultiDecoder(nn.Module):
    """One decoder per articulator on its own slice of the latent vector, outputs stacked on dim -2 (:176-213)."""

    def __init__(self, indices_dict, in_features, hidden_features, decoder_cls=Decoder):
        super().__init__()
        self.indices_dict, self.latent_size, self.sorted_articulators = _resolve(indices_dict)
        decoder_cls = _resolve_cls(decoder_cls, DecoderType)
        self.decoders = nn.ModuleDict({articulator: decoder_cls(num_components=len(indices), out_features=in_features,
                                                                hidden_features=hidden_features)
                                       for articulator, indices in self.indices_dict.items()})
        layers = 1 if decoder_cls is PCADecoder else 3
        self._plan = _Plan(False, self.indices_dict, self.sorted_articulators, self.latent_size, in_features, layers,
                           hidden_features)

    def forward(self, x, scale=1.0):
        """x (..., latent_size) -> (..., n_articulators, in_features); ``scale`` multiplies the input inside the kernel
        (AutoencoderLoss2's rescale_factor)."""
        _lib.require_gpu(x, "x")
        if FUSED_MLP and self._plan.supported:
            modules = [self.decoders[a] for a in self.sorted_articulators]
            return _MultiMlpFn.apply(self._plan, float(scale), 0, x, *_fused_params(modules))
        if scale != 1.0:
            x = scale * x
        outs = [self.decoders[articulator](x[..., self.indices_dict[articulator]].contiguous()).unsqueeze(-2)
                for articulator in self.sorted_articulators]
        return torch.cat(outs, dim=-2)


class MultiArticulatorAutoencoder(nn.Module):
    def __init__(self, in_features, indices_dict, hidden_features=64):
        super().__init__()
        self.indices_dict, self.latent_size, self.sorted_articulators = _resolve(indices_dict)
        self.encoders = MultiEncoder(indices_dict=indices_dict, in_features=in_features, hidden_features=hidden_features)
        self.decoders = MultiDecoder(indices_dict=indices_dict, in_features=in_features, hidden_features=hidden_features)

    @property
    def total_parameters(self):
        return sum(p.numel() for p in self.parameters())

    def forward(self, x):
        """x (bs, n_articulators, in_features) -> (outputs (bs, n_articulators, in_features), latent (bs, latent_size))."""
        latent_space = self.encoders._forward(x, tanh=True)
        return self.decoders(latent_space), latent_space
