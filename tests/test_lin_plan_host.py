"""csrc/lin_plan.cpp on the host: the kernel every known head-layer descriptor gets, and what must hold for any descriptor.

tests/lin_plan_check.cpp and the planner are compiled with g++ and the address and undefined-behaviour sanitizers and run as a
child process (nothing is preloaded).  Its first part plans the rows of tests/golden/lin_plan_rows.json: every as_lin / as_lin_out
that csrc/artspeech.hip poses for the HEAD_CASES and WIDE_HEAD_CASES of tools/head_stack_cases.py (3 and 11 heads), for the
benchmark's shape (6400 rows, 11 heads, H = 128, N = 50) alone and inside a training step with the fused criterion, and the
as_linear_fwd shapes of test_gpu_parity.py's test_split_matrix_arithmetic_error_vs_fp64 (the Linear shapes the transformer and
principal-components modules ship) -- each in both matrix arithmetics and with as_set_head_short_k / as_set_lin_out_row_epilogue
off in turn (env = arithmetic, short_k, row_epi).  EXPECTED below is what the code BEFORE the planner existed launched for those
descriptors on an MI355X, logged by one fprintf in front of its launches (kernel, grid, workgroup size, dynamic LDS, and what a
grid does not show: the split into 64- and 32-row tiles, head groups, k-chunk, the criterion's epilogue, who sums the loss); the
kernel trace of the same build agrees with the logged kernels and grids line for line (profiles/lin_plan_equivalence.log).  One
difference in how a row is posed: the heads' dx1 (as_lin_plain_s6 with waves_per_simd = 2) was called with the number of chunks
artspeech.hip had worked out; it is now called with ksplit = 0 (AS_LIN_KSPLIT_AUTO) and the planner works it out -- the rows carry
0 and EXPECTED the launch that resulted.  The second part is a seeded sweep of 20 000 random descriptors of each kind."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: {environments "arith short_k row_epi": the launch}
EXPECTED = {
    "lin_try[512-256-128-3-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=48x1 block=512 lds=81920 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=3 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[512-256-256-3-e1]": {
        "111 110 101":
            "kernel=lin_s6_kernel<1> grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[512-100-256-3-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=24x1 block=256 lds=0 planes=1 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=24",
        "011 010 001":
            "kernel=lin_out_kernel grid=24x1 block=512 lds=0 planes=0 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=24",
    },
    "lin_try[512-256-128-3-e2]": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[512-256-256-3-e2]": {
        "111 110 101":
            "kernel=lin_s6_kernel<2> grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[512-128-768-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=16x8 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=96 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_try[37-256-128-3-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=6x1 block=512 lds=81920 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=3 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[37-256-256-3-e1]": {
        "111 110 101":
            "kernel=lin_s6_kernel<1> grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[37-100-256-3-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=6x1 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=6",
        "011 010 001":
            "kernel=lin_out_kernel grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=6",
    },
    "lin_try[37-256-128-3-e2]": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[37-256-256-3-e2]": {
        "111 110 101":
            "kernel=lin_s6_kernel<2> grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[37-128-768-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=2x8 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=96 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_out[37-128-256-3-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=6x1 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=6",
        "011 010 001":
            "kernel=lin_out_kernel grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=6",
    },
    "lin_try[37-256-128-3-e2]#1": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[37-140-256-3-plain]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[37-140-256-3-e0]": {
        "111 110 101 011 010 001":
            "kernel=lin_f32_kernel<64, true, 0> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[37-256-160-3-e2]": {
        "111 110 101":
            "kernel=lin_s6_kernel<2> grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[512-66-256-3-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=24x1 block=256 lds=0 planes=1 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=24",
        "011 010 001":
            "kernel=lin_out_kernel grid=24x1 block=512 lds=0 planes=0 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=24",
    },
    "lin_try[512-256-96-3-e2]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_out[512-2-256-3-plain]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[512-2-256-3-e0]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[512-256-32-3-e2]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_out[37-6-256-3-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=6x1 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=6",
        "011 010 001":
            "kernel=lin_out_kernel grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=6",
    },
    "lin_try[37-256-32-3-e2]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[512-256-64-3-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=48x1 block=512 lds=57344 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=3 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[512-64-768-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=16x8 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=96 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_try[37-256-64-3-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=6x1 block=512 lds=57344 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=3 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=6x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=6x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[37-2-256-3-plain]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[37-2-256-3-e0]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[37-256-32-3-e2]#1": {
        "111 110 101 011 010 001":
            "declined",
    },
    "plain[37-64-768-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=2x8 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=96 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_try[37-256-50-3-e1]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[512-256-50-3-e1]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_out[512-128-256-3-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=24x1 block=256 lds=0 planes=1 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=24",
        "011 010 001":
            "kernel=lin_out_kernel grid=24x1 block=512 lds=0 planes=0 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=24",
    },
    "lin_try[512-256-128-3-e2]#1": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[37-256-7-3-e1]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[512-256-7-3-e1]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_out[512-140-256-3-plain]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[512-140-256-3-e0]": {
        "111 110 101 011 010 001":
            "kernel=lin_f32_kernel<64, true, 0> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[512-256-160-3-e2]": {
        "111 110 101":
            "kernel=lin_s6_kernel<2> grid=48x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=48x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=16 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[512-256-300-3-e1]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[37-256-300-3-e1]": {
        "111 110 101 011 010 001":
            "declined",
    },
    "lin_try[3021-256-128-11-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=480x1 block=512 lds=81920 planes=1 n_big=470 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=10 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=539x1 block=512 lds=0 planes=0 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[3021-256-256-11-e1]": {
        "111 110 101":
            "kernel=lin_s6_kernel<1> grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=539x1 block=512 lds=0 planes=0 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[3021-100-256-11-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=528x1 block=256 lds=0 planes=1 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=528",
        "011 010 001":
            "kernel=lin_out_kernel grid=528x1 block=512 lds=0 planes=0 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=528",
    },
    "lin_try[3021-256-128-11-e2]": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=539x1 block=512 lds=0 planes=0 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[3021-256-256-11-e2]": {
        "111 110 101":
            "kernel=lin_s6_kernel<2> grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=539x1 block=512 lds=0 planes=0 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[3021-128-2816-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=48x8 block=256 lds=0 planes=1 n_big=47 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=352 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_try[3021-256-96-11-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=480x1 block=512 lds=69632 planes=1 n_big=470 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=10 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=539x1 block=512 lds=0 planes=0 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[3021-80-256-11-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=528x1 block=256 lds=0 planes=1 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=528",
        "011 010 001":
            "kernel=lin_out_kernel grid=528x1 block=512 lds=0 planes=0 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=528",
    },
    "lin_try[3021-256-96-11-e2]": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=539x1 block=512 lds=0 planes=1 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=539x1 block=512 lds=0 planes=0 n_big=506 big_per_batch=46 big_per_batch_rows=2944 small_per_batch=3 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[3021-96-2816-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=48x8 block=256 lds=0 planes=1 n_big=47 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=352 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_try[6400-256-128-11-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=500x1 block=512 lds=81920 planes=1 n_big=500 big_per_batch=100 big_per_batch_rows=6400 small_per_batch=1 groups=5 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=1177x1 block=512 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=1177x1 block=512 lds=0 planes=0 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[6400-256-256-11-e1]": {
        "111 110 101":
            "kernel=lin_s6_kernel<1> grid=1177x1 block=512 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=1177x1 block=512 lds=0 planes=0 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[6400-100-256-11-plain]": {
        "111 110 101":
            "kernel=lin_out_s6_kernel grid=1177x1 block=256 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=1177",
        "011 010 001":
            "kernel=lin_out_kernel grid=1177x1 block=512 lds=0 planes=0 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=1177",
    },
    "lin_try[6400-256-128-11-e2]": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=1177x1 block=512 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=1177x1 block=512 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=1177x1 block=512 lds=0 planes=0 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[6400-256-256-11-e2]": {
        "111 110 101":
            "kernel=lin_s6_kernel<2> grid=1177x1 block=512 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=1177x1 block=512 lds=0 planes=0 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[6400-128-2816-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=100x5 block=256 lds=0 planes=1 n_big=100 big_per_batch=100 big_per_batch_rows=6400 small_per_batch=1 groups=0 kchunk=576 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_out[512-100-256-3-tgt]": {
        "111 101":
            "kernel=lin_out_s6_kernel grid=24x1 block=256 lds=0 planes=1 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "110":
            "kernel=lin_out_s6_kernel grid=24x1 block=256 lds=0 planes=1 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
        "011 001":
            "kernel=lin_out_kernel grid=24x1 block=512 lds=0 planes=0 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "010":
            "kernel=lin_out_kernel grid=24x1 block=512 lds=0 planes=0 n_big=24 big_per_batch=8 big_per_batch_rows=512 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
    },
    "lin_try[808-256-128-3-e1]": {
        "111 110":
            "kernel=lin_s6_lnf_shared_kernel grid=78x1 block=512 lds=81920 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=3 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<1> grid=78x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=78x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[808-256-256-3-e1]": {
        "111 110 101":
            "kernel=lin_s6_kernel<1> grid=78x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, true, 1> grid=78x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[808-128-256-3-tgt]": {
        "111 101":
            "kernel=lin_out_s6_kernel grid=42x1 block=256 lds=0 planes=1 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "110":
            "kernel=lin_out_s6_kernel grid=42x1 block=256 lds=0 planes=1 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
        "011 001":
            "kernel=lin_out_kernel grid=42x1 block=512 lds=0 planes=0 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "010":
            "kernel=lin_out_kernel grid=42x1 block=512 lds=0 planes=0 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
    },
    "lin_try[808-256-128-3-e2]": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=78x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=78x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=78x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_try[808-256-256-3-e2]": {
        "111 110 101":
            "kernel=lin_s6_kernel<2> grid=78x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=78x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[808-128-768-1-k0-w2]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 2> grid=26x8 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=96 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "declined",
    },
    "lin_out[808-4-256-3-tgt]": {
        "111 101":
            "kernel=lin_out_s6_kernel grid=42x1 block=256 lds=0 planes=1 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "110":
            "kernel=lin_out_s6_kernel grid=42x1 block=256 lds=0 planes=1 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
        "011 001":
            "kernel=lin_out_kernel grid=42x1 block=512 lds=0 planes=0 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "010":
            "kernel=lin_out_kernel grid=42x1 block=512 lds=0 planes=0 n_big=36 big_per_batch=12 big_per_batch_rows=768 small_per_batch=2 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
    },
    "lin_try[808-256-32-3-e2]": {
        "111 110":
            "kernel=lin_s6_lnb_short_kernel grid=78x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "101":
            "kernel=lin_s6_kernel<2> grid=78x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
        "011 010 001":
            "kernel=lin_f32_kernel<64, false, 2> grid=78x1 block=512 lds=0 planes=0 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=26 groups=0 kchunk=0 row_epi=0 sums_loss=0 partials=0",
    },
    "lin_out[6400-100-256-11-tgt]": {
        "111 101":
            "kernel=lin_out_s6_kernel grid=1177x1 block=256 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "110":
            "kernel=lin_out_s6_kernel grid=1177x1 block=256 lds=0 planes=1 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
        "011 001":
            "kernel=lin_out_kernel grid=1177x1 block=512 lds=0 planes=0 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "010":
            "kernel=lin_out_kernel grid=1177x1 block=512 lds=0 planes=0 n_big=1023 big_per_batch=93 big_per_batch_rows=5952 small_per_batch=14 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
    },
    "lin_out[3021-80-256-11-tgt]": {
        "111 101":
            "kernel=lin_out_s6_kernel grid=528x1 block=256 lds=0 planes=1 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "110":
            "kernel=lin_out_s6_kernel grid=528x1 block=256 lds=0 planes=1 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
        "011 001":
            "kernel=lin_out_kernel grid=528x1 block=512 lds=0 planes=0 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=1 sums_loss=1 partials=0",
        "010":
            "kernel=lin_out_kernel grid=528x1 block=512 lds=0 planes=0 n_big=517 big_per_batch=47 big_per_batch_rows=3008 small_per_batch=1 groups=0 kchunk=0 row_epi=0 sums_loss=1 partials=0",
    },
    "plain[6400-256-256-1-k1-w4]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<8, 4> grid=200x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=200 groups=0 kchunk=256 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[6400-256-128-1-k1-w4]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<8, 4> grid=200x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=200 groups=0 kchunk=128 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[6400-256-256-3-k1-w4]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<8, 4> grid=600x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=200 groups=0 kchunk=256 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[6400-128-512-1-k1-w4]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 4> grid=200x1 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=200 groups=0 kchunk=512 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[6400-100-256-1-k1-w4]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<4, 4> grid=200x1 block=256 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=200 groups=0 kchunk=256 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[1000-256-2816-1-k1-w4]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<8, 4> grid=32x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=32 groups=0 kchunk=2816 row_epi=0 sums_loss=0 partials=0",
    },
    "plain[37-130-64-1-k1-w4]": {
        "111 110 101":
            "kernel=lin_s6_plain_kernel<8, 4> grid=2x1 block=512 lds=0 planes=1 n_big=0 big_per_batch=1 big_per_batch_rows=0 small_per_batch=2 groups=0 kchunk=64 row_epi=0 sums_loss=0 partials=0",
    },
}


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """(rows by name, {(name, env): launch}, the sweep's summary line)"""
    tmp = tmp_path_factory.mktemp("lin_plan")
    with open(os.path.join(ROOT, "tests", "golden", "lin_plan_rows.json")) as f:
        rows = json.load(f)
    listing = tmp / "rows.txt"
    listing.write_text("".join(r["name"] + " " + " ".join(f"{k}={v}" for k, v in r.items() if k not in ("name", "first_case")) + "\n" for r in rows))
    exe = str(tmp / "lin_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan",   # the runtime inside the program: whatever else a machine loads into its processes
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "artspeech_amd", "csrc", "lin_plan.cpp"), os.path.join(ROOT, "tests", "lin_plan_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe, str(listing)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    got = {}
    for line in lines[:-1]:
        name, env, launch = line.split(" ", 2)
        got[(name, env[4:])] = launch
    assert len(got) == 6 * len(rows)
    return {r["name"]: r for r in rows}, got, lines[-1]


def test_planner_decision_table_and_sweep(planned):
    rows, got, summary = planned
    assert re.fullmatch(r"sweep: 120000 plans; families( \d+){8}; .*", summary), summary
    assert sorted(rows) == sorted(EXPECTED)
    wrong = [(name, env, want, got[(name, env)]) for name, by_env in EXPECTED.items() for envs, want in by_env.items() for env in envs.split()
             if got[(name, env)] != want]
    assert not wrong, wrong[:10]
    # every row was launched or declined by the old code in the split arithmetic with both switches on, and most in all six environments
    assert all(any("111" in envs.split() for envs in by_env) for by_env in EXPECTED.values())
    assert sum(len(env.split()) for by_env in EXPECTED.values() for env in by_env) >= 5 * len(EXPECTED)


def field(launch, key):
    return int(re.search(rf"\b{key}=(-?\d+)", launch).group(1))


def grid(launch):
    return re.search(r" (grid=\d+x\d+) ", launch).group(1)


def test_documented_figures(planned):
    """The tile lists, chunks and groups the kernels' comments, DESIGN.md and tools/head_stack_cases.py state."""
    rows, got, _ = planned

    def launches(pattern, kernel):
        hit = [l for (name, env), l in got.items() if env == "111" and re.fullmatch(pattern, name) and l.startswith("kernel=" + kernel)]
        assert hit, (pattern, kernel)
        return hit

    # 3021 rows x 11 heads.  Head layers: 46 tiles of 64 rows per head, then 3 of 32
    for l in launches(r"lin_try\[3021-256-256-11-e[12]\](#\d+)?", "lin_s6_kernel"):
        assert (field(l, "n_big"), field(l, "big_per_batch"), field(l, "small_per_batch"), grid(l)) == (46 * 11, 46, 3, "grid=539x1"), l
    # output layer and dx1: 47 + 1; dx1: 8 chunks of 352
    for l in launches(r"lin_out\[3021-\d+-256-11-\w+\](#\d+)?", "lin_out_s6_kernel"):
        assert (field(l, "n_big"), field(l, "big_per_batch"), field(l, "small_per_batch"), grid(l)) == (47 * 11, 47, 1, "grid=528x1"), l
    for l in launches(r"plain\[3021-128-2816-1-k0-w2\]", "lin_s6_plain_kernel<4, 2>"):
        assert (field(l, "n_big"), field(l, "small_per_batch"), grid(l), field(l, "kchunk")) == (47, 1, "grid=48x8", 352), l
    # 6400 x 11.  Linear 1: 500 workgroups, groups of 2, 2, 2, 2, 3 heads, 80 KB
    for l in launches(r"lin_try\[6400-256-128-11-e1\](#\d+)?", "lin_s6_lnf_shared_kernel"):
        g = field(l, "groups")
        assert (grid(l), g, field(l, "lds")) == ("grid=500x1", 5, 80 * 1024), l
        assert [(t + 1) * 11 // g - t * 11 // g for t in range(g)] == [2, 2, 2, 2, 3]
    # head layers and output layer: 1023 + 154 tiles
    for l in launches(r"lin_try\[6400-256-256-11-e[12]\](#\d+)?", "lin_s6_kernel") + launches(r"lin_out\[6400-100-256-11-\w+\](#\d+)?", "lin_out_s6_kernel"):
        assert (field(l, "n_big"), grid(l)) == (1023, "grid=1177x1"), l
