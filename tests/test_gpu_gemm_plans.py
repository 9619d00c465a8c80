"""Every kernel the GEMM planner (csrc/gemm_plan.cpp) can name, run on the device at the smallest shape that reaches it, against
float64 (tests/gemm_fp64.py): the gemm_plans[...] rows of tests/golden/gemm_plan_rows.json, whose plans tests/test_gemm_plan_host.py
pins and proves to cover every (kernel, reduce kernel) pair of its sweep.  Each row runs in both matrix arithmetics.

Per row and mode: C, colsum and relu_bits against the reference; no NaN in a result (every operand element outside the descriptor's
extent is NaN, and so is the split-K workspace); every word outside [M][N] -- the ldc gap, rows past M, the bands around C,
colsum and relu_bits -- bit-identical afterwards; under accumulate the prior contents enter once (they are of the operands'
magnitude: a miss or a double count is ~1e5 bounds); three launches of a row with a workspace give torch.equal results; a k_tri row
equals the same product without the hint, bit for bit.

Bounds: max |error| <= 2e-6 max|ref| sqrt(K) (test_gemm_split_k_paths and the weight-gradient tests of test_gpu_parity.py; it holds
for precision = 3 too); rows with act >= 2 take test_gemm_nt's rtol 2e-5, atol 2e-5 sqrt(K).
Run with ``pytest -m gpu`` on an MI355X.

Measured on an MI355X when the rows were added (largest error over C and colsum as a fraction of the bound, per planned kernel and
reduce kernel, with the rows that run the pair; `counters/X`: summed in the kernel by arrival counters, X behind it on a stream
without a counter block -- test_split_k_without_a_counter_block runs that form, 0.004 of the bound):
  gemm_f32_kernel<128, 128, false, false, false, false>    -                                  0.020  t128_tn_slow
  gemm_f32_kernel<128, 128, false, false, false, false>    splitk_reduce_kernel               0.010  t128_splitk_tn
  gemm_f32_kernel<128, 128, false, false, true, false>     -                                  0.023  t128_tn
  gemm_f32_kernel<128, 128, false, false, true, true>      -                                  0.023  tri2_128
  gemm_f32_kernel<128, 128, false, true, true, false>      -                                  0.022  t128_otkc
  gemm_f32_kernel<128, 128, true, false, false, false>     -                                  0.021  t128_nn_slow
  gemm_f32_kernel<128, 128, true, false, false, false>     splitk_reduce_kernel               0.009  t128_splitk_nn_slow
  gemm_f32_kernel<128, 128, true, false, true, false>      -                                  0.023  t128_nn
  gemm_f32_kernel<128, 128, true, false, true, false>      splitk_reduce_kernel               0.009  t128_splitk_nn
  gemm_f32_kernel<128, 128, true, false, true, true>       -                                  0.021  tri1_128
  gemm_f32_kernel<128, 128, true, true, false, false>      -                                  0.018  t128_nt_slow
  gemm_f32_kernel<128, 128, true, true, false, false>      splitk_reduce_kernel               0.009  t128_splitk_nt_slow
  gemm_f32_kernel<128, 128, true, true, true, false>       -                                  0.030  panels, t128_nt_fast
  gemm_f32_kernel<128, 128, true, true, true, false>       splitk_reduce_kernel               0.010  t128_splitk
  gemm_f32_kernel<128, 128, true, true, true, true>        -                                  0.022  ext128_ragged
  gemm_f32_kernel<64, 64, false, false, false, false>      counters/splitk_reduce4_kernel     0.003  sk_tn_slow_c4
  gemm_f32_kernel<64, 64, false, false, false, false>      counters/splitk_reduce_kernel      0.004  sk_counters
  gemm_f32_kernel<64, 64, false, false, false, false>      splitk_reduce4_kernel              0.002  sk_tn_slow_r4
  gemm_f32_kernel<64, 64, false, false, true, false>       -                                  0.027  s6_anc, s6_anc_novec
  gemm_f32_kernel<64, 64, false, false, true, false>       counters/splitk_reduce_kernel      0.004  sk_shift
  gemm_f32_kernel<64, 64, false, false, true, false>       splitk_reduce4_kernel              0.002  sk_r4
  gemm_f32_kernel<64, 64, false, false, true, true>        -                                  0.015  ext64_tri2
  gemm_f32_kernel<64, 64, false, true, false, false>       -                                  0.015  otkc_slow
  gemm_f32_kernel<64, 64, false, true, true, false>        -                                  0.021  otkc_colsum, otkc_fast
  gemm_f32_kernel<64, 64, true, false, false, false>       counters/splitk_reduce4_kernel     0.002  sk_nn_slow_c4
  gemm_f32_kernel<64, 64, true, false, false, false>       counters/splitk_reduce_kernel      0.005  sk_nn_slow_c
  gemm_f32_kernel<64, 64, true, false, false, false>       splitk_reduce4_kernel              0.001  sk_nn_slow_r4
  gemm_f32_kernel<64, 64, true, false, true, false>        -                                  0.016  s6_bnc
  gemm_f32_kernel<64, 64, true, false, true, false>        counters/splitk_reduce_kernel      0.003  sk_counters_dx
  gemm_f32_kernel<64, 64, true, false, true, true>         -                                  0.014  ext64_dx_mask
  gemm_f32_kernel<64, 64, true, true, false, false>        counters/splitk_reduce4_kernel     0.002  sk_nt_slow_c4
  gemm_f32_kernel<64, 64, true, true, false, false>        counters/splitk_reduce_kernel      0.004  sk_nt_slow_c
  gemm_f32_kernel<64, 64, true, true, false, false>        splitk_reduce4_kernel              0.002  sk_nt_slow_r4
  gemm_f32_kernel<64, 64, true, true, true, false>         counters/splitk_reduce4_kernel     0.003  sk_nt_c4
  gemm_f32_kernel<64, 64, true, true, true, false>         counters/splitk_reduce_kernel      0.004  sk_nt_c
  gemm_f32_kernel<64, 64, true, true, true, false>         splitk_reduce4_kernel              0.002  sk_nt_r4
  gemm_s6_kernel<false, true, false>                       -                                  0.017  s6_bnc
  gemm_s6_kernel<true, true, false>                        -                                  0.021  s6_anc, s6_anc_novec
  wgrad_f32_kernel<128, false, false>                      -                                  0.022  wg_whole
  wgrad_f32_kernel<128, false, false>                      wgrad_reduce_kernel                0.007  wg_split128
  wgrad_f32_kernel<128, false, true>                       -                                  0.020  wg_whole
  wgrad_f32_kernel<128, false, true>                       wgrad_reduce_kernel                0.005  wg_split128
  wgrad_f32_kernel<128, true, false>                       wgrad_reduce_sk_kernel<128>        0.019  wg128_sk
  wgrad_f32_kernel<128, true, true>                        wgrad_reduce_sk_kernel<128>        0.015  wg128_sk
  wgrad_f32_kernel<256, false, false>                      -                                  0.019  wg_shift_nows
  wgrad_f32_kernel<256, false, false>                      wgrad_reduce_kernel                0.007  wg_shift, wg_split
  wgrad_f32_kernel<256, false, true>                       -                                  0.023  wg_shift_nows
  wgrad_f32_kernel<256, false, true>                       wgrad_reduce_kernel                0.006  wg_shift, wg_split
  wgrad_f32_kernel<256, true, false>                       wgrad_reduce_sk_kernel<256>        0.015  wg256_sk
  wgrad_f32_kernel<256, true, true>                        wgrad_reduce_sk_kernel<256>        0.014  wg256_sk
No row failed against the kernels as they stood: no kernel source changed with these tests."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_fp64
from artspeech_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "gemm_plan_rows.json")) as f:
    ROWS = {r["name"][len("gemm_plans["):-1]: r for r in json.load(f) if r["name"].startswith("gemm_plans[")}
TABLES = ("a_off", "b_off", "c_off", "bias_off", "res_off", "a_seg_off", "b_seg_off")
OUTPUTS = ("C", "colsum", "relu_bits")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def matrix_arith():
    """tests that switch the library's matrix arithmetic restore the default (1 = split) afterwards"""
    L = _lib.lib()
    keep = L.as_get_matrix_arith()
    yield L.as_set_matrix_arith
    L.as_set_matrix_arith(keep)


def device_product(dev):
    """a b^T in float64 on the device (rocBLAS: no code under test), for the rows whose reference is tens of GFLOP"""
    return lambda a, b: (torch.from_numpy(a).to(dev) @ torch.from_numpy(b).to(dev).T).cpu().numpy()


_posed = {}


def posed(name, dev):
    """(operands, reference) of a row: posed and computed once, shared by both modes, never written (one row is kept at a time)"""
    if name not in _posed:
        _posed.clear()
        row = ROWS[name]
        ops = gemm_fp64.pose(row, np.random.RandomState(len(name) + row["M"] + row["K"]))
        big = 2.0 * row["M"] * row["N"] * row["K"] * row["batch"] > 4e9
        _posed[name] = (ops, gemm_fp64.reference(row, ops, device_product(dev) if big else None))
    return _posed[name]


class Launch:
    """A row's operands on the device and its descriptor; run() restores the outputs' prior contents, launches on the current
    stream and returns the outputs' whole allocations (bands and gaps included) as they are afterwards."""

    def __init__(self, row, ops, dev, **override):
        self.row, self.ops = row, ops
        self.t = {k: torch.from_numpy(v.data.view(np.int32) if v.data.dtype == np.uint32 else v.data).to(dev)
                  for k, v in ops.items() if isinstance(v, gemm_fp64.Operand)}
        self.tables = {k: torch.from_numpy(v).to(dev) for k, v in ops.items() if k in TABLES}
        self.prior = {k: self.t[k].clone() for k in OUTPUTS if k in self.t}
        fields = {k: v for k, v in row.items() if k not in gemm_fp64.POINTERS and k != "name"}
        fields.update(override)
        for k, t in self.t.items():
            fields[k] = t.data_ptr() + 4 * ops[k].start
            assert fields[k] % 16 == row[k] % 16, k   # the recorded misalignment
        fields.update(self.tables)
        if row["splitk_ws"]:   # NaN: a slab element that is summed without having been written shows
            self.ws = fields["splitk_ws"] = torch.full((row["splitk_ws_floats"],), float("nan"), device=dev)
        self.desc = _lib.gemm_desc(**fields)

    def run(self):
        for k, p in self.prior.items():
            self.t[k].copy_(p)
        rc = _lib.lib().as_gemm_f32(C.byref(self.desc), _lib.stream_ptr())
        assert rc == 0, _lib.lib().as_last_error()
        return {k: self.t[k].clone() for k in self.prior}


def check(row, ops, ref, out, what):
    """the outputs of one launch (host arrays of the whole allocations) against the reference; returns error / bound per output"""
    K = row["K"]
    worst = {}
    for k in out:
        o, raw = ops[k], out[k].view(np.uint32)
        stray = np.flatnonzero((raw != gemm_fp64.SENTINEL) & ~o.addressed)
        assert stray.size == 0, f"{what}: {k}: {stray.size} words outside the descriptor's extent were written, first at element " \
                                f"{stray[0] - o.start} from the pointer"
    got = ops["C"].gather(out["C"]).astype(np.float64)
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} NaN in C"
    err = np.abs(got - ref["C"])
    if row["act"] >= 2:
        worst["C"] = float((err / (2e-5 * np.sqrt(K) + 2e-5 * np.abs(ref["C"]))).max())
    else:
        worst["C"] = float(err.max() / (2e-6 * np.abs(ref["C"]).max() * np.sqrt(K)))
    if "colsum" in out:
        cs = ops["colsum"].gather(out["colsum"]).astype(np.float64)
        assert not np.isnan(cs).any(), f"{what}: NaN in colsum"
        worst["colsum"] = float(np.abs(cs - ref["colsum"]).max() / (2e-6 * np.abs(ref["colsum"]).max() * np.sqrt(K)))
    print(f"{what}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f"{what}: {k}: {v:.3f} x the bound"
    if "relu_bits" in out:
        # the bit image of THIS result, and nothing beyond N.  (With C inside its bound that is the reference's image wherever the
        # reference is further from zero than the bound; the count of the others is printed.)
        bits = ops["relu_bits"].gather(out["relu_bits"].view(np.uint32))
        assert np.array_equal(bits, gemm_fp64.pack_bits(got > 0)), f"{what}: relu_bits is not (result > 0) with the bits beyond N clear"
        print(f"{what}: relu_bits words that differ from the reference's: {int((bits != ref['relu_bits']).sum())} of {bits.size}")
    return worst


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name,mode", [(n, m) for n in ROWS for m in (0, 1)], ids=lambda v: str(v))
def test_planned_kernel_against_fp64(dev, matrix_arith, name, mode):
    row = ROWS[name]
    ops, ref = posed(name, dev)
    matrix_arith(mode)
    launch = Launch(row, ops, dev)
    first = launch.run()
    torch.cuda.synchronize()
    check(row, ops, ref, host(first), f"{name} arith {mode}")
    if row["splitk_ws"]:   # slabs and pieces are summed in a fixed order: run to run the same bits
        for again in (launch.run(), launch.run()):
            assert all(torch.equal(first[k], again[k]) for k in first), f"{name}: two launches differ"
    if row["k_tri"]:       # the hint skips exact zeros only
        # Without the hint a weight-gradient-shaped product (both operands reduction-strided) is planned for wgrad_f32.hip, which
        # in arithmetic 1 multiplies on the bf16 instruction: no bit-for-bit yardstick.  The full product is then taken in
        # arithmetic 0, where either kernel adds the same k-ordered fp32 chain; the general kernel is the same in both modes.
        if mode == 1 and row["a_i"] == 1 and row["b_j"] == 1:
            matrix_arith(0)
        full = Launch(row, ops, dev, k_tri=0).run()
        assert torch.equal(first["C"], full["C"]), f"{name}: k_tri = {row['k_tri']} differs from the full product"


def test_split_k_without_a_counter_block():
    """counters_for (gemm_f32.hip) serves 64 (device, stream) slots for the life of the process; a launch on any further stream sums
    its slabs with the planned fallback reduce kernel instead of in the kernel.  A fresh process (tests/_gemm_slot_worker.py) runs
    the counter rows on 70 streams: all results equal bit for bit -- the in-kernel sum has the reduce kernel's order -- and the
    first is fp64-close."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_gemm_slot_worker.py")], capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    for name in ("sk_counters", "sk_counters_dx", "sk_shift", "sk_r4"):
        assert f"{name}: ok" in r.stdout, r.stdout[-3000:]
