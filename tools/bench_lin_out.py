"""The heads' output layer with its fused criterion (lin_out_s6_kernel; lin_out_kernel with --exact), at the benchmark's size
(32 utterances x 200 frames = 6400 frames, 11 heads, N = 2 x 50 outputs): the `head.gemm3` phase of whole
TrainStep.forward_backward passes from the library's own HIP-event table, with as_set_lin_out_row_epilogue alternating
off / on in ONE process, so that box-to-box speed and clocks cannot enter the comparison.
usage: python tools/bench_lin_out.py [rounds >= 6] [steps per reading] [--exact]"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from artspeech_amd import _lib  # noqa: E402
from artspeech_amd.engine import TrainStep  # noqa: E402
from artspeech_amd.phoneme_to_articulation.encoder_decoder.models import ArtSpeech  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
rounds = max(6, int(args[0])) if args else 6
steps = int(args[1]) if len(args) > 1 else 20
V, A, E, H, N, B, T = 45, 11, 64, 128, 50, 32, 200
PHASE = "head.gemm3"

L = _lib.lib()
if "--exact" in sys.argv:
    L.as_set_matrix_arith(0)
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = ArtSpeech(V, A, embed_dim=E, hidden_size=H, n_samples=N).to(dev)
g = torch.Generator().manual_seed(1)
tokens = torch.randint(1, V, (B, T), generator=g).to(dev)
targets = torch.rand(B, T, A, 2, N, generator=g).to(dev)
lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
scale = 1.0 / (B * T * A * N)
step = TrainStep(model, B, T, optimizer=False)


def reading(on):
    """Microseconds per launch of the phase over `steps` passes with the switch at `on`."""
    L.as_set_lin_out_row_epilogue(on)
    for _ in range(3):
        step.forward_backward(tokens, lengths, targets, scale)
    torch.cuda.synchronize()
    L.as_profile_reset()
    L.as_profile_enable(1)
    for _ in range(steps):
        step.forward_backward(tokens, lengths, targets, scale)
    torch.cuda.synchronize()
    L.as_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    L.as_profile_report(buf, len(buf))
    L.as_profile_reset()
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        if name == PHASE:
            return 1e3 * float(ms) / int(cnt)
    raise SystemExit(f"no phase {PHASE} in the profile table")


off, on = [], []
for r in range(rounds):
    off.append(reading(0))
    loss_off = float(step.loss)
    on.append(reading(1))
    loss_on = float(step.loss)
    print(f"round {r}: {PHASE} off {off[-1]:7.2f} us   on {on[-1]:7.2f} us   loss off {loss_off!r} on {loss_on!r}", flush=True)
L.as_set_lin_out_row_epilogue(1)
m_off, m_on, spread = sum(off) / rounds, sum(on) / rounds, max(off) - min(off)
print(f"mean off {m_off:.2f} us (spread {spread:.2f}, min {min(off):.2f}, max {max(off):.2f})   mean on {m_on:.2f} us "
      f"(min {min(on):.2f}, max {max(on):.2f})")
print(f"gain {m_off - m_on:.2f} us = {(m_off - m_on) / spread if spread > 0 else float('inf'):.1f} x the spread of the off rounds "
      f"(asked: more than 3 x)")
