"""Float64 yardstick of the point-to-closest-point loss (torch, CPU), written from the definition: the distance matrix by direct
differences sqrt(dx^2 + dy^2), the closest point as the LOWEST index among equals (torch.min), nothing from a pair at zero
distance (cdist's backward), gradients by torch autograd.  The same function in float32 is "stock torch's fp32 direct formula",
whose error against the float64 result is the unit of the tests' bound.  Independent of the library (no import of
artspeech_amd); used by tests/golden/make_golden_p2cp_grad.py and tests/test_gpu_p2cp_loss.py."""
import torch


def distances(u, v):
    """u (*, N, 2), v (*, M, 2) -> (*, N, M), direct differences; a zero distance is a constant 0 (no gradient, no NaN)."""
    dx = u[..., :, None, 0] - v[..., None, :, 0]
    dy = u[..., :, None, 1] - v[..., None, :, 1]
    s = dx * dx + dy * dy
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def _first_min(d, dim):
    """min over dim, taken at the first index that attains it (argmax returns the first maximal value)."""
    idx = (d == d.min(dim=dim, keepdim=True).values).to(torch.int8).argmax(dim=dim, keepdim=True)
    return d.gather(dim, idx).squeeze(dim)


def p2cp(u, v):
    """MeanP2CPDistance, reduction "none": (*, N, 2), (*, M, 2) -> (*), in the dtype of the inputs."""
    d = distances(u, v)
    return (_first_min(d, -1).sum(-1) / u.shape[-2] + _first_min(d, -2).sum(-1) / v.shape[-2]) / 2


def value_and_grads(u, v, dout, dtype=torch.float64):
    """u, v float32 CPU tensors, dout (*) -> (value, du, dv) as float64 tensors, computed in `dtype` by autograd."""
    a = u.detach().cpu().to(dtype).clone().requires_grad_(True)
    b = v.detach().cpu().to(dtype).clone().requires_grad_(True)
    val = p2cp(a, b)
    (val * dout.detach().cpu().to(dtype)).sum().backward()
    return val.detach().double(), a.grad.double(), b.grad.double()


def decided(u, v, margin=1e-6):
    """(*) bool: in float64 every row and column minimum beats its runner-up by more than margin x the tile's largest
    distance, and no distance is 0 -- the tiles on which the closest points do not hang on the last bits of a distance."""
    d = distances(u.detach().cpu().double(), v.detach().cpu().double())
    big = d.amax(dim=(-1, -2))
    ok = (d > 0).all(-1).all(-1)
    for dim in (-1, -2):
        if d.shape[dim] > 1:
            two = d.topk(2, dim=dim, largest=False).values
            gap = two.select(dim, 1) - two.select(dim, 0)
            ok &= (gap > margin * big[..., None]).all(-1)
    return ok


def masked_loss(outputs, targets, lengths, n_valid=None, dtype=torch.float64):
    """outputs (B, T, A, 2, N), targets (B, >= T, A, 2, N) float32, lengths (B,) -> (loss, dloss/doutputs (B, T, A, 2, N)) in
    float64: the mean over valid frames and articulators of the P2CP; padded frames are never touched (their gradient is 0)."""
    B, T, A = outputs.shape[:3]
    lengths = [int(l) for l in lengths]
    n_valid = sum(lengths) if n_valid is None else n_valid
    o = outputs.detach().cpu().to(dtype)
    t = targets.detach().cpu().to(dtype)
    grad = torch.zeros(o.shape, dtype=torch.float64)
    total = torch.zeros((), dtype=torch.float64)
    for b, l in enumerate(lengths):
        if l == 0:
            continue
        ob = o[b, :l].clone().requires_grad_(True)
        val = p2cp(ob.transpose(-1, -2), t[b, :l].transpose(-1, -2)).sum() / (n_valid * A)
        val.backward()
        total += val.detach().double()
        grad[b, :l] = ob.grad.double()
    return total, grad
