"""Fixture of the point-to-closest-point loss, produced by the reference's own MeanP2CPDistance
(phoneme_to_articulation/metrics.py:27-46) and torch autograd on the CPU.  Run from the repository root with the reference
checkout at make_golden.REF:

    python tests/golden/make_golden_p2cp_grad.py

Writes tests/golden/p2cp_grad.npz (data only): 12 tiles of N = 20 by M = 25 points, float32, with the upstream gradient dout,
the reference's values and its gradients du, dv.  At these sizes torch.cdist evaluates direct differences (its matrix-product
expansion starts above 25 points), so the reference agrees with the float64 restatement tests/p2cp_fp64.py to rounding --
asserted here, the measured figure is stored -- and the fixture pins the two conventions:
  tile COINCIDENT  u_4 == v_7: that pair contributes exactly nothing (cdist's backward), no NaN
  tile TIE         u_3 = (100, 100) has v_5 = (101, 100) and v_9 = (99, 100) at distance exactly 1, all coordinates multiples
                   of 1/8, far from the other points: the lowest index takes the gradient.  `tie_lowest` records whether the
                   reference's CPU result does that; where it does not, the tile is left out of the comparison."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import p2cp_fp64 as Y  # noqa: E402
from make_golden import _load, save  # noqa: E402

TILES, N, M = 12, 20, 25
COINCIDENT, TIE = 5, 8
SEED = 211


def main():
    ref = _load("ref_p2a_metrics", "phoneme_to_articulation/metrics.py")
    g = torch.Generator().manual_seed(SEED)
    u = torch.rand(TILES, N, 2, generator=g)
    v = torch.rand(TILES, M, 2, generator=g)
    dout = torch.randn(TILES, generator=g)
    dout[2] = 0.0
    v[COINCIDENT, 7] = u[COINCIDENT, 4]
    u[TIE] = torch.randint(0, 400, (N, 2), generator=g) / 8.0
    v[TIE] = torch.randint(0, 400, (M, 2), generator=g) / 8.0
    u[TIE, 3] = torch.tensor([100.0, 100.0])
    v[TIE, 5] = torch.tensor([101.0, 100.0])
    v[TIE, 9] = torch.tensor([99.0, 100.0])

    a, b = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
    val = ref.MeanP2CPDistance(reduction="none")(a, b)
    (val * dout).sum().backward()
    du, dv = a.grad, b.grad
    assert torch.isfinite(du).all() and torch.isfinite(dv).all()

    t_val, t_du, t_dv = Y.value_and_grads(u, v, dout)
    tie_lowest = bool((du[TIE].double() - t_du[TIE]).abs().max() < 1e-6 and (dv[TIE].double() - t_dv[TIE]).abs().max() < 1e-6)
    keep = torch.ones(TILES, dtype=torch.bool)
    keep[TIE] = tie_lowest
    scale = max(float(t_du.abs().max()), float(t_dv.abs().max()))
    err = max(float((du.double() - t_du)[keep].abs().max()), float((dv.double() - t_dv)[keep].abs().max())) / scale
    assert err < 1e-6, err
    assert float((val.detach().double() - t_val).abs().max()) < 1e-6
    print(f"reference against fp64 direct: {err:.2e} of max|g|; tie tile takes the lowest index: {tie_lowest}")
    save("p2cp_grad", u=u.numpy(), v=v.numpy(), dout=dout.numpy(), value=val.detach().numpy(), du=du.numpy(), dv=dv.numpy(),
         coincident=np.int32(COINCIDENT), tie=np.int32(TIE), tie_lowest=np.bool_(tie_lowest), err_vs_fp64=np.float64(err))


if __name__ == "__main__":
    main()
