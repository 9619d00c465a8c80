"""A restatement of as_gemm_f32 (include/artspeech_hip.h, `struct as_gemm`) in float64 for ANY descriptor, and host operands to go
with a row of tests/golden/gemm_plan_rows.json (an as_gemm with its pointers recorded as 0 = absent, or 16 + the address's low
four bits):

* ``pose(row, rng)``: one host allocation per operand, laid out as the row's strides, batch strides (which may be smaller than an
  operand's extent: the batch members are then overlapping windows of one array), offset and segment tables and recorded
  misalignment say.  Every element of an input that the descriptor does not address -- stride gaps, the slack behind a buffer
  -- is NaN, so a kernel that lets one into a product shows it.  C, colsum and relu_bits are NaN / all-ones where the
  descriptor addresses them (seeded values under ``accumulate``) and carry the word SENTINEL everywhere else: in a band before
  and behind them and in every gap (ldc > N, batch strides), so a kernel that stores outside [M][N] shows it too.
* ``reference(row, operands)``: the product with everything the header documents -- both orientations of either operand,
  b_kshift / b_kT / b_kshift_batch, k_seg with its tables, res (+ res_off), mask_bits, bias (+ bias_off), act 0 to 3, relu_bits,
  colsum, accumulate, c_off / ldc.

Plain numpy (the error function of the GELU comes from torch on the CPU, in float64)."""
import numpy as np
import torch

SENTINEL = np.uint32(0xDEADBEEF)      # a finite float32 (-6.26e18): never the result of a product of the operands posed here
BAND = 64                             # words in front of and behind every operand's addressed range (a multiple of 4)
POINTERS = ("A", "B", "C", "bias", "splitk_ws", "colsum", "a_off", "b_off", "c_off", "bias_off", "res", "res_off", "mask_bits",
            "relu_bits", "a_seg_off", "b_seg_off")


class Operand:
    """One allocation.  data: all of it, 1-D; start: the element the descriptor's pointer names; bases[g] + idx: the elements
    (relative to start) of batch member g, idx shaped as the operand reads ([M][K], [N][K], [M][N], [M], [N], [M][words]);
    valid: None, or per member the mask of idx that the descriptor reads at all (a shifted B); addressed: mask over data."""

    def __init__(self, dtype, bits, bases, idx, valid=None):
        self.bases, self.idx, self.valid = [np.asarray(b, np.int64) for b in bases], idx, valid
        hi = max(int(b.max()) for b in self.bases) + int(idx.max()) + 1
        self.start = BAND + (bits & 15) // 4
        self.data = np.empty(self.start + hi + BAND, dtype)
        self.addressed = np.zeros(self.data.size, bool)
        for g, base in enumerate(self.bases):
            for b in base.reshape(-1):
                at = self.start + b + (idx if valid is None else idx[valid[g]])
                self.addressed[at] = True

    def gather(self, data=None):
        """[batch][*idx.shape] (segments side by side along the last axis) of data (default: the posed contents)"""
        data = self.data if data is None else data
        return np.stack([np.concatenate([data[self.start + b + self.idx] for b in base.reshape(-1)], axis=-1) for base in self.bases])


def _up4(n):
    return (n + 3) // 4 * 4


def pose(row, rng):
    """row -> {operand name: Operand, table name: int64 array}.  rng: a numpy RandomState."""
    r = row
    M, N, K, batch = r["M"], r["N"], r["K"], r["batch"]
    nseg = K // r["k_seg"] if r["k_seg"] else 1
    kspan = r["k_seg"] or K
    ops = {}

    def bases(ext, stride, off, count=batch):
        """first elements of the batch members: a table (posed here, shuffled, multiples of 4) or the linear stride"""
        if off is not None:
            ops[off] = (rng.permutation(count) * (_up4(ext) + 4)).astype(np.int64)
            return ops[off]
        return np.arange(count, dtype=np.int64) * stride

    def values(o, poison):
        o.data[:] = poison
        o.data[o.addressed] = rng.standard_normal(int(o.addressed.sum())).astype(np.float32)
        return o

    idx_a = np.arange(M, dtype=np.int64)[:, None] * r["a_i"] + np.arange(kspan, dtype=np.int64)[None, :] * r["a_k"]
    idx_b = np.arange(N, dtype=np.int64)[:, None] * r["b_j"] + np.arange(kspan, dtype=np.int64)[None, :] * r["b_k"]
    if r["k_seg"]:
        a_bases = bases(int(idx_a.max()) + 1, 0, "a_seg_off", batch * nseg).reshape(batch, nseg)
        b_bases = bases(int(idx_b.max()) + 1, 0, "b_seg_off", batch * nseg).reshape(batch, nseg)
    else:
        a_bases = bases(int(idx_a.max()) + 1, r["a_batch"], "a_off" if r["a_off"] else None)[:, None]
        b_bases = bases(int(idx_b.max()) + 1, r["b_batch"], "b_off" if r["b_off"] else None)[:, None]
    a = ops["A"] = values(Operand(np.float32, r["A"], a_bases, idx_a), np.nan)
    if r["k_tri"]:   # the hint's promise: exact zeros below (1) or above (2) the diagonal
        i, k = np.arange(M)[:, None], np.arange(K)[None, :]
        zero = (k < i) if r["k_tri"] == 1 else (k > i)
        for base in a.bases:
            a.data[a.start + base[0] + idx_a[zero]] = 0.0
    b_valid = None
    if r["b_kT"] > 0:   # reduction index k reads k + shift, and nothing where its frame k % b_kT + shift leaves the sequence
        k = np.arange(K)
        b_valid, b_base_g = [], []
        for g in range(batch):
            s = r["b_kshift"] + g * r["b_kshift_batch"]
            ok = (k % r["b_kT"] + s >= 0) & (k % r["b_kT"] + s < r["b_kT"])
            b_valid.append(np.broadcast_to(ok[None, :], idx_b.shape))
            b_base_g.append(b_bases[g] + s * r["b_k"])
        b_bases = np.stack(b_base_g)
    ops["B"] = values(Operand(np.float32, r["B"], b_bases, idx_b, b_valid), np.nan)

    cols = np.arange(N, dtype=np.int64)[None, :]
    rows_ = np.arange(M, dtype=np.int64)[:, None]
    ncb = (N + 31) // 32
    if r["bias"]:
        ops["bias"] = values(Operand(np.float32, r["bias"], bases(N, r["bias_batch"], "bias_off" if r["bias_off"] else None)[:, None],
                                     cols[0]), np.nan)
    if r["res"]:
        ops["res"] = values(Operand(np.float32, r["res"], bases((M - 1) * r["res_ld"] + N, r["res_batch"],
                                                                "res_off" if r["res_off"] else None)[:, None],
                                    rows_ * r["res_ld"] + cols), np.nan)
    words = rows_ * ncb + np.arange(ncb, dtype=np.int64)[None, :]
    if r["mask_bits"]:
        m = ops["mask_bits"] = Operand(np.uint32, r["mask_bits"], bases(M * ncb, r["mask_batch"], None)[:, None], words)
        m.data[:] = rng.randint(0, 2 ** 32, m.data.size, dtype=np.uint64).astype(np.uint32)   # bits beyond N: whatever

    def output(name, dtype, o):
        o.data[:] = SENTINEL if dtype == np.uint32 else np.array(SENTINEL).view(np.float32)
        o.data[o.addressed] = 0xFFFFFFFF if dtype == np.uint32 else np.nan
        ops[name] = o
        return o

    c = output("C", np.float32, Operand(np.float32, r["C"], bases((M - 1) * r["ldc"] + N, r["c_batch"], "c_off" if r["c_off"] else None)[:, None],
                                        rows_ * r["ldc"] + cols))
    if r["accumulate"]:
        c.data[c.addressed] = rng.standard_normal(int(c.addressed.sum())).astype(np.float32)
    if r["colsum"]:
        output("colsum", np.float32, Operand(np.float32, r["colsum"], bases(M, r["colsum_batch"], None)[:, None], rows_[:, 0]))
    if r["relu_bits"]:
        output("relu_bits", np.uint32, Operand(np.uint32, r["relu_bits"], bases(M * ncb, r["relu_bits_batch"], None)[:, None], words))
    return ops


def _erf(x):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def activation(x, act):
    if act == 1:
        return np.maximum(x, 0.0)
    if act == 2:
        return 1.0 / (1.0 + np.exp(-x))
    if act == 3:
        return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))
    return x


def pack_bits(flags):
    """[..., N] bool -> [..., ceil(N / 32)] uint32, bit n % 32 of word n / 32; bits beyond N clear"""
    n = flags.shape[-1]
    pad = np.zeros(flags.shape[:-1] + (_up32(n) - n,), bool)
    f = np.concatenate([flags, pad], axis=-1).reshape(flags.shape[:-1] + (-1, 32)).astype(np.uint64)
    return (f << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(words, n):
    """[..., W] uint32 -> [..., n] bool"""
    bits = (words[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(words.shape[:-1] + (-1,))[..., :n].astype(bool)


def _up32(n):
    return (n + 31) // 32 * 32


def reference(row, ops, product=None):
    """float64 results of the descriptor over the posed operands: {"C": [batch][M][N], "colsum": [batch][M] or None, "relu_bits":
    [batch][M][ceil(N / 32)] uint32 or None}.  product(a [M][K], b [N][K]) -> a b^T may replace numpy's (a float64 product
    elsewhere, for the largest rows)."""
    r = row
    product = product or (lambda a, b: a @ b.T)
    a_op, b_op = ops["A"], ops["B"]
    out = np.empty((r["batch"], r["M"], r["N"]))
    colsum = np.empty((r["batch"], r["M"])) if "colsum" in ops else None
    for g in range(r["batch"]):
        a = np.concatenate([a_op.data[a_op.start + s + a_op.idx] for s in a_op.bases[g].reshape(-1)], axis=-1).astype(np.float64)
        if colsum is not None:
            colsum[g] = a.sum(-1)
        if b_op.valid is None:
            b = np.concatenate([b_op.data[b_op.start + s + b_op.idx] for s in b_op.bases[g].reshape(-1)], axis=-1).astype(np.float64)
        else:   # frames outside their sequence are zeros and are never read
            at = np.where(b_op.valid[g], b_op.start + b_op.bases[g].reshape(-1)[0] + b_op.idx, b_op.start)
            b = np.where(b_op.valid[g], b_op.data[at].astype(np.float64), 0.0)
        out[g] = product(a, b)
    if "res" in ops:
        out = ops["res"].gather().astype(np.float64) + out
    if "bias" in ops:
        out = out + ops["bias"].gather().astype(np.float64)[:, None, :]
    out = activation(out, r["act"])
    bits = pack_bits(out > 0) if "relu_bits" in ops else None
    if "mask_bits" in ops:
        out = np.where(unpack_bits(ops["mask_bits"].gather(), r["N"]), out, 0.0)
    if r["accumulate"]:
        out = out + ops["C"].gather().astype(np.float64)
    return {"C": out, "colsum": colsum, "relu_bits": bits}
