"""csrc/gemm_plan.cpp on the host: the kernel every known descriptor gets, and what must hold for any descriptor.

tests/gemm_plan_check.cpp and the planner are compiled with g++ and the address and undefined-behaviour sanitizers and run as a
child process (nothing is preloaded).  Its first part plans the rows of tests/golden/gemm_plan_rows.json -- the shapes of the GEMM
tests in test_gpu_parity.py and the descriptors the Python call sites pose at the benchmark's sizes (tools/gemm_plan_cases.py runs
the same rows on the GPU) -- in both matrix arithmetics; EXPECTED below is what the kernel trace of those rows showed on an
MI355X (256 CUs; 768 resident workgroups of the 128 x 128 kernel; 8192 arrival counters) BEFORE the planner existed
(profiles/gemm_plan_equivalence.log): kernel name, reduce kernel, grid in workgroups, and where the grid shows it the split-K
factor with the chunk length that follows from it (every row has both: see the note above the table).  Its second part is a seeded
sweep of 30 000 random descriptors, which also lists every (kernel, reduce kernel) pair it planned: each must be the plan of a row
that a device test runs (the gemm_plans[...] rows of test_gpu_gemm_plans.py and the rows named after tests of test_gpu_parity.py)."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (both arithmetics,) or (fp32 arithmetic, split arithmetic); "kernel  reduce kernel  grid  splitk  kchunk".
# A row without a workspace cannot split: splitk 1, kchunk K, whatever its grid.  Four rows with a workspace have grids that do not
# show the split (gemm_split_k_paths[6400-256-768-1]/*: a grid clamped to the resident slots, slabs summed by arrival counters;
# ops.py:226#1, #3: a weight-gradient grid rounded up to whole XCD rounds); theirs was printed by the code before the planner, built
# with one fprintf in front of those launches (profiles/gemm_plan_equivalence.log).  The gemm_plans[...] entries at the end of the table
# are of another kind: the planner's own output, recorded when the rows were added (see the note above them).
EXPECTED = {
    "gemm_nt[64-64-32]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 1 1 32",),
    "gemm_nt[200-100-128]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 8 1 128",),
    "gemm_nt[1-1-1]": ("gemm_f32_kernel<64, 64, true, true, false, false> - 1 1 1",),
    "gemm_nt[257-130-70]": ("gemm_f32_kernel<64, 64, true, true, false, false> - 15 1 70",),
    "gemm_nt[6400-256-128]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 128",),
    "gemm_nt[45-768-64]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 12 1 64",),
    "gemm_nt[33-17-5]": ("gemm_f32_kernel<64, 64, true, true, false, false> - 1 1 5",),
    "gemm_nt[300-2816-128]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 220 1 128",),
    "gemm_nn_tn[128-128-64]/nn": ("gemm_f32_kernel<64, 64, true, false, true, false> - 4 1 64",),
    "gemm_nn_tn[128-128-64]/tn": ("gemm_f32_kernel<64, 64, false, false, true, false> - 4 1 64",),
    "gemm_nn_tn[128-128-64]/tn+acc": ("gemm_f32_kernel<64, 64, false, false, true, false> - 4 1 64",),
    "gemm_nn_tn[100-256-100]/nn": ("gemm_f32_kernel<64, 64, true, false, true, false> - 8 1 100",),
    "gemm_nn_tn[100-256-100]/tn": ("gemm_f32_kernel<64, 64, false, false, true, false> - 8 1 100",),
    "gemm_nn_tn[100-256-100]/tn+acc": ("gemm_f32_kernel<64, 64, false, false, true, false> - 8 1 100",),
    "gemm_nn_tn[6400-128-2816]/nn": ("gemm_f32_kernel<64, 64, true, false, true, false> - 200 1 2816",),
    "gemm_nn_tn[6400-128-2816]/tn": ("wgrad_f32_kernel<128, false, false> - 56 1 2816",
        "wgrad_f32_kernel<128, false, true> - 56 1 2816"),
    "gemm_nn_tn[6400-128-2816]/tn+acc": ("wgrad_f32_kernel<128, false, false> - 56 1 2816",
        "wgrad_f32_kernel<128, false, true> - 56 1 2816"),
    "gemm_nn_tn[7-3-9]/nn": ("gemm_f32_kernel<64, 64, true, false, false, false> - 1 1 9",),
    "gemm_nn_tn[7-3-9]/tn": ("gemm_f32_kernel<64, 64, false, false, false, false> - 1 1 9",),
    "gemm_nn_tn[7-3-9]/tn+acc": ("gemm_f32_kernel<64, 64, false, false, false, false> - 1 1 9",),
    "gemm_nn_tn[70-200-333]/nn": ("gemm_f32_kernel<64, 64, true, false, false, false> - 8 1 333",),
    "gemm_nn_tn[70-200-333]/tn": ("gemm_f32_kernel<64, 64, false, false, false, false> - 8 1 333",),
    "gemm_nn_tn[70-200-333]/tn+acc": ("gemm_f32_kernel<64, 64, false, false, false, false> - 8 1 333",),
    "gemm_split_precision[500-200-264]/p2": ("refused",),
    "gemm_split_precision[500-200-264]/p1": ("refused",),
    "split_general_forward_odd[37-130-64-1]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 3 1 64",
        "gemm_s6_kernel<false, false, false> - 16 1 64"),
    "split_general_forward_odd[37-130-64-1]/bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 3 1 64",
        "gemm_s6_kernel<false, false, false> - 16 1 64"),
    "split_general_forward_odd[200-45-32-2]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 4 1 32",
        "gemm_s6_kernel<false, false, false> - 2 1 32"),
    "split_general_forward_odd[129-258-48-0]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 15 1 48",
        "gemm_s6_kernel<false, false, false> - 24 1 48"),
    "split_general_forward_odd[300-128-256-1]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 10 1 256",
        "gemm_s6_kernel<false, false, false> - 3 1 256"),
    "split_general_forward_odd[300-128-256-1]/bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 10 1 256",
        "gemm_s6_kernel<false, false, false> - 3 1 256"),
    "gemm_batched_strided": ("gemm_f32_kernel<64, 64, true, true, true, false> - 9 1 64",),
    "gemm_shift": ("gemm_f32_kernel<64, 64, false, false, true, false> - 1 1 36",),
    "gemm_shift_batched": ("gemm_f32_kernel<64, 64, false, false, true, false> - 2 1 36",),
    "gemm_residual_mask_seg[200-64-6-p0]/out+res": ("gemm_f32_kernel<64, 64, true, true, true, true> - 24 1 64",),
    "gemm_residual_mask_seg[200-64-6-p0]/out": ("gemm_f32_kernel<64, 64, true, true, true, false> - 24 1 64",),
    "gemm_residual_mask_seg[200-64-6-p0]/relu_bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 24 1 64",),
    "gemm_residual_mask_seg[200-64-6-p0]/dx+res+mask": ("gemm_f32_kernel<64, 64, true, false, true, true> - 24 1 64",),
    "gemm_residual_mask_seg[200-64-6-p0]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 12 1 128",),
    "gemm_residual_mask_seg[200-64-6-p0]/wgrad+res": ("refused",),
    "gemm_residual_mask_seg[1500-256-12-p0]/out+res": ("gemm_f32_kernel<64, 64, true, true, true, true> - 1152 1 256",),
    "gemm_residual_mask_seg[1500-256-12-p0]/out": ("gemm_f32_kernel<64, 64, true, true, true, false> - 1024 1 256",),
    "gemm_residual_mask_seg[1500-256-12-p0]/relu_bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 1152 1 256",),
    "gemm_residual_mask_seg[1500-256-12-p0]/dx+res+mask": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1152 1 256",),
    "gemm_residual_mask_seg[1500-256-12-p0]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 288 1 1024",),
    "gemm_residual_mask_seg[1500-256-12-p0]/wgrad+res": ("refused",),
    "gemm_residual_mask_seg[77-32-3-p0]/out+res": ("gemm_f32_kernel<64, 64, true, true, true, true> - 6 1 32",),
    "gemm_residual_mask_seg[77-32-3-p0]/out": ("gemm_f32_kernel<64, 64, true, true, true, false> - 6 1 32",),
    "gemm_residual_mask_seg[77-32-3-p0]/relu_bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 6 1 32",),
    "gemm_residual_mask_seg[77-32-3-p0]/dx+res+mask": ("gemm_f32_kernel<64, 64, true, false, true, true> - 6 1 32",),
    "gemm_residual_mask_seg[77-32-3-p0]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 6 1 32",),
    "gemm_residual_mask_seg[77-32-3-p0]/wgrad+res": ("refused",),
    "gemm_residual_mask_seg[6400-256-6-p0]/out+res": ("gemm_f32_kernel<128, 128, true, true, true, true> - 600 1 256",),
    "gemm_residual_mask_seg[6400-256-6-p0]/out": ("gemm_f32_kernel<128, 128, true, true, true, false> - 600 1 256",),
    "gemm_residual_mask_seg[6400-256-6-p0]/relu_bits": ("gemm_f32_kernel<128, 128, true, true, true, true> - 600 1 256",),
    "gemm_residual_mask_seg[6400-256-6-p0]/dx+res+mask": ("gemm_f32_kernel<128, 128, true, false, true, true> - 600 1 256",),
    "gemm_residual_mask_seg[6400-256-6-p0]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1200 1 512",),
    "gemm_residual_mask_seg[6400-256-6-p0]/wgrad+res": ("refused",),
    "gemm_residual_mask_seg[200-64-6-p3]/out+res": ("gemm_f32_kernel<64, 64, true, true, true, true> - 24 1 64",
        "gemm_s6_kernel<false, false, true> - 12 1 64"),
    "gemm_residual_mask_seg[200-64-6-p3]/out": ("gemm_f32_kernel<64, 64, true, true, true, false> - 24 1 64",
        "gemm_s6_kernel<false, false, false> - 12 1 64"),
    "gemm_residual_mask_seg[200-64-6-p3]/relu_bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 24 1 64",
        "gemm_s6_kernel<false, false, false> - 12 1 64"),
    "gemm_residual_mask_seg[200-64-6-p3]/dx+res+mask": ("gemm_f32_kernel<64, 64, true, false, true, true> - 24 1 64",
        "gemm_s6_kernel<false, true, true> - 12 1 64"),
    "gemm_residual_mask_seg[200-64-6-p3]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 12 1 128",
        "gemm_s6_kernel<false, true, true> - 6 1 128"),
    "gemm_residual_mask_seg[200-64-6-p3]/wgrad+res": ("refused",),
    "gemm_residual_mask_seg[1500-256-12-p3]/out+res": ("gemm_f32_kernel<64, 64, true, true, true, true> - 1152 1 256",
        "gemm_s6_kernel<false, false, true> - 288 1 256"),
    "gemm_residual_mask_seg[1500-256-12-p3]/out": ("gemm_f32_kernel<64, 64, true, true, true, false> - 1024 1 256",
        "gemm_s6_kernel<false, false, false> - 288 1 256"),
    "gemm_residual_mask_seg[1500-256-12-p3]/relu_bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 1152 1 256",
        "gemm_s6_kernel<false, false, false> - 288 1 256"),
    "gemm_residual_mask_seg[1500-256-12-p3]/dx+res+mask": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1152 1 256",
        "gemm_s6_kernel<false, true, true> - 288 1 256"),
    "gemm_residual_mask_seg[1500-256-12-p3]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 288 1 1024",
        "gemm_s6_kernel<false, true, true> - 80 1 1024"),
    "gemm_residual_mask_seg[1500-256-12-p3]/wgrad+res": ("refused",),
    "gemm_residual_mask_seg[77-32-3-p3]/out+res": ("gemm_f32_kernel<64, 64, true, true, true, true> - 6 1 32",
        "gemm_s6_kernel<false, false, true> - 3 1 32"),
    "gemm_residual_mask_seg[77-32-3-p3]/out": ("gemm_f32_kernel<64, 64, true, true, true, false> - 6 1 32",
        "gemm_s6_kernel<false, false, false> - 3 1 32"),
    "gemm_residual_mask_seg[77-32-3-p3]/relu_bits": ("gemm_f32_kernel<64, 64, true, true, true, true> - 6 1 32",
        "gemm_s6_kernel<false, false, false> - 3 1 32"),
    "gemm_residual_mask_seg[77-32-3-p3]/dx+res+mask": ("gemm_f32_kernel<64, 64, true, false, true, true> - 6 1 32",
        "gemm_s6_kernel<false, true, true> - 3 1 32"),
    "gemm_residual_mask_seg[77-32-3-p3]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 6 1 32",
        "gemm_s6_kernel<false, true, true> - 3 1 32"),
    "gemm_residual_mask_seg[77-32-3-p3]/wgrad+res": ("refused",),
    "gemm_residual_mask_seg[6400-256-6-p3]/out+res": ("gemm_f32_kernel<128, 128, true, true, true, true> - 600 1 256",
        "gemm_s6_kernel<false, false, true> - 608 1 256"),
    "gemm_residual_mask_seg[6400-256-6-p3]/out": ("gemm_f32_kernel<128, 128, true, true, true, false> - 600 1 256",
        "gemm_s6_kernel<false, false, false> - 608 1 256"),
    "gemm_residual_mask_seg[6400-256-6-p3]/relu_bits": ("gemm_f32_kernel<128, 128, true, true, true, true> - 600 1 256",
        "gemm_s6_kernel<false, false, false> - 608 1 256"),
    "gemm_residual_mask_seg[6400-256-6-p3]/dx+res+mask": ("gemm_f32_kernel<128, 128, true, false, true, true> - 600 1 256",
        "gemm_s6_kernel<false, true, true> - 608 1 256"),
    "gemm_residual_mask_seg[6400-256-6-p3]/segmented": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1200 1 512",
        "gemm_s6_kernel<false, true, true> - 304 1 512"),
    "gemm_residual_mask_seg[6400-256-6-p3]/wgrad+res": ("refused",),
    "gemm_triangular[200-64-40]/rows-full": ("gemm_f32_kernel<64, 64, true, false, true, false> - 160 1 200",),
    "gemm_triangular[200-64-40]/rows-tri1": ("gemm_f32_kernel<64, 64, true, false, true, true> - 160 1 200",),
    "gemm_triangular[200-64-40]/cols-full": ("gemm_f32_kernel<64, 64, false, false, true, false> - 160 1 200",),
    "gemm_triangular[200-64-40]/cols-tri2": ("gemm_f32_kernel<64, 64, false, false, true, true> - 160 1 200",),
    "gemm_triangular[77-16-9]/rows-full": ("gemm_f32_kernel<64, 64, true, false, false, false> - 18 1 77",),
    "gemm_triangular[77-16-9]/rows-tri1": ("gemm_f32_kernel<64, 64, true, false, false, false> - 18 1 77",),
    "gemm_triangular[77-16-9]/cols-full": ("gemm_f32_kernel<64, 64, false, false, false, false> - 18 1 77",),
    "gemm_triangular[77-16-9]/cols-tri2": ("gemm_f32_kernel<64, 64, false, false, false, false> - 18 1 77",),
    "gemm_triangular[256-32-5]/rows-full": ("gemm_f32_kernel<64, 64, true, false, true, false> - 20 1 256",),
    "gemm_triangular[256-32-5]/rows-tri1": ("gemm_f32_kernel<64, 64, true, false, true, true> - 20 1 256",),
    "gemm_triangular[256-32-5]/cols-full": ("gemm_f32_kernel<64, 64, false, false, true, false> - 20 1 256",),
    "gemm_triangular[256-32-5]/cols-tri2": ("gemm_f32_kernel<64, 64, false, false, true, true> - 20 1 256",),
    "weight_gradient_stream_k[256-256-1024-70-False]/ws": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 1024",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 1024"),
    "weight_gradient_stream_k[256-256-1024-70-False]/plain": ("wgrad_f32_kernel<256, false, false> - 144 1 1024",
        "wgrad_f32_kernel<256, false, true> - 144 1 1024"),
    "weight_gradient_stream_k[256-256-1024-70-False]/ws+acc": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 1024",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 1024"),
    "weight_gradient_stream_k[200-132-2048-75-True]/ws": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 2048",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 2048"),
    "weight_gradient_stream_k[200-132-2048-75-True]/plain": ("wgrad_f32_kernel<256, false, false> - 152 1 2048",
        "wgrad_f32_kernel<256, false, true> - 152 1 2048"),
    "weight_gradient_stream_k[200-132-2048-75-True]/ws+acc": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 2048",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 2048"),
    "weight_gradient_stream_k[256-256-6400-110-False]/ws": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 6400",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 6400"),
    "weight_gradient_stream_k[256-256-6400-110-False]/plain": ("wgrad_f32_kernel<256, false, false> - 224 1 6400",
        "wgrad_f32_kernel<256, false, true> - 224 1 6400"),
    "weight_gradient_stream_k[256-256-6400-110-False]/ws+acc": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 6400",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 6400"),
    "weight_gradient_stream_k[128-256-800-300-False]/ws": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 800",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 800"),
    "weight_gradient_stream_k[128-256-800-300-False]/plain": ("wgrad_f32_kernel<256, false, false> - 304 1 800",
        "wgrad_f32_kernel<256, false, true> - 304 1 800"),
    "weight_gradient_stream_k[128-256-800-300-False]/ws+acc": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 800",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 256 1 800"),
    "weight_gradient_split_tiles[256-256-6400-110-False]": ("wgrad_f32_kernel<256, false, false> - 224 1 6400",
        "gemm_s6_kernel<true, true, false> - 448 1 6400"),
    "weight_gradient_split_tiles[200-132-2048-7-True]": ("gemm_f32_kernel<64, 64, false, false, true, false> - 84 1 2048",),
    "weight_gradient_split_tiles[128-384-160-3-False]": ("gemm_f32_kernel<64, 64, false, false, true, false> - 36 1 160",),
    "weight_gradient_split_tiles[256-256-6400-110-True]": ("wgrad_f32_kernel<256, false, false> - 224 1 6400",
        "gemm_s6_kernel<true, true, false> - 448 1 6400"),
    "gemm_split_k_paths[384-128-6400-2]/wgrad": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 960 40 160",),
    "gemm_split_k_paths[384-128-6400-2]/dx": ("gemm_f32_kernel<64, 64, true, false, true, false> splitk_reduce4_kernel 600 50 128",),
    "gemm_split_k_paths[256-256-4096-3]/wgrad": ("gemm_f32_kernel<64, 64, false, false, true, false> - 768 16 256",),
    "gemm_split_k_paths[256-256-4096-3]/dx": ("gemm_f32_kernel<64, 64, true, false, true, false> splitk_reduce4_kernel 512 32 128",),
    "gemm_split_k_paths[45-64-768-1]/wgrad": ("gemm_f32_kernel<64, 64, false, false, false, false> - 12 12 64",),
    "gemm_split_k_paths[45-64-768-1]/dx": ("gemm_f32_kernel<64, 64, true, false, true, false> - 12 12 64",),
    "gemm_split_k_paths[6400-256-768-1]/wgrad": ("gemm_f32_kernel<64, 64, false, false, true, false> - 1024 3 256",),
    "gemm_split_k_paths[6400-256-768-1]/dx": ("gemm_f32_kernel<64, 64, true, false, true, false> - 1024 3 256",),
    "gemm_split_k_paths[100-256-2048-5]/wgrad": ("gemm_f32_kernel<64, 64, false, false, true, false> - 640 16 128",),
    "gemm_split_k_paths[100-256-2048-5]/dx": ("gemm_f32_kernel<64, 64, true, false, true, false> - 128 16 128",),
    "ops.py:198": ("gemm_f32_kernel<64, 64, true, true, true, false> - 1024 1 256",),
    "ops.py:198#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 256",),
    "ops.py:198#2": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:198#3": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 2048",),
    "ops.py:198#4": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 100",),
    "ops.py:417": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:428": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:432": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:458": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:417#1": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:428#1": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:432#1": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:458#1": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:198#5": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 2560",),
    "ops.py:198#6": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 256",),
    "ops.py:198#7": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 2816",),
    "ops.py:417#2": ("gemm_f32_kernel<128, 128, true, true, true, true> - 768 1 256",),
    "ops.py:428#2": ("gemm_f32_kernel<128, 128, true, true, true, true> - 768 1 256",),
    "ops.py:417#3": ("gemm_f32_kernel<128, 128, true, true, true, true> - 768 1 256",),
    "ops.py:428#3": ("gemm_f32_kernel<128, 128, true, true, true, true> - 768 1 256",),
    "ops.py:226": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 248 11 608",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 248 11 608"),
    "ops.py:229": ("gemm_f32_kernel<128, 128, true, false, true, false> - 768 1 256",
        "gemm_s6_kernel<false, true, false> - 1232 1 256"),
    "ops.py:226#1": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 128 63 1120",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 128 63 1120"),
    "ops.py:229#1": ("gemm_f32_kernel<128, 128, true, false, true, false> - 768 1 256",
        "gemm_s6_kernel<false, true, false> - 1104 1 256"),
    "ops.py:536": ("gemm_f32_kernel<128, 128, true, false, true, false> - 768 1 256",
        "gemm_s6_kernel<false, true, false> - 1104 1 256"),
    "ops.py:539": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 248 11 608",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 248 11 608"),
    "ops.py:334": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1536 1 200",),
    "ops.py:343": ("gemm_f32_kernel<64, 64, false, false, true, true> - 1536 1 200",),
    "ops.py:344": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1536 1 200",),
    "ops.py:551": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 248 11 608",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 248 11 608"),
    "ops.py:555": ("gemm_f32_kernel<128, 128, true, false, true, true> - 768 1 256",
        "gemm_s6_kernel<false, true, true> - 1104 1 256"),
    "ops.py:557": ("gemm_f32_kernel<128, 128, true, false, true, true> - 768 1 256",
        "gemm_s6_kernel<false, true, true> - 2208 1 256"),
    "ops.py:564": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 248 11 608",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 248 11 608"),
    "ops.py:566": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 224 5 1280",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 224 5 1280"),
    "ops.py:585": ("gemm_f32_kernel<128, 128, true, false, true, false> - 768 1 256",
        "gemm_s6_kernel<false, true, false> - 1104 1 256"),
    "ops.py:594": ("gemm_f32_kernel<64, 64, true, false, true, true> - 400 1 5632",
        "gemm_s6_kernel<false, true, true> - 112 1 5632"),
    "ops.py:226#2": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 6400",
        "gemm_s6_kernel<true, true, false> - 640 1 6400"),
    "ops.py:229#2": ("gemm_f32_kernel<128, 128, true, false, true, false> - 768 1 256",
        "gemm_s6_kernel<false, true, false> - 11040 1 256"),
    "ops.py:536#1": ("gemm_f32_kernel<128, 128, true, false, true, false> - 768 1 256",
        "gemm_s6_kernel<false, true, false> - 11008 1 256"),
    "ops.py:539#1": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 6400",
        "gemm_s6_kernel<true, true, false> - 448 1 6400"),
    "ops.py:334#1": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1536 1 200",),
    "ops.py:343#1": ("gemm_f32_kernel<64, 64, false, false, true, true> - 1536 1 200",),
    "ops.py:344#1": ("gemm_f32_kernel<64, 64, true, false, true, true> - 1536 1 200",),
    "ops.py:551#1": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 6400",
        "gemm_s6_kernel<true, true, false> - 448 1 6400"),
    "ops.py:555#1": ("gemm_f32_kernel<128, 128, true, false, true, true> - 768 1 256",
        "gemm_s6_kernel<false, true, true> - 11008 1 256"),
    "ops.py:557#1": ("gemm_f32_kernel<128, 128, true, false, true, true> - 768 1 256",
        "gemm_s6_kernel<false, true, true> - 22000 1 256"),
    "ops.py:564#1": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 6400",
        "gemm_s6_kernel<true, true, false> - 448 1 6400"),
    "ops.py:566#1": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 256 1 6400",
        "gemm_s6_kernel<true, true, false> - 896 1 6400"),
    "ops.py:594#1": ("gemm_f32_kernel<128, 128, true, false, true, true> - 768 1 2560",
        "gemm_s6_kernel<false, true, true> - 1104 1 2560"),
    "ops.py:594#2": ("gemm_f32_kernel<128, 128, true, false, true, true> - 768 1 5120",
        "gemm_s6_kernel<false, true, true> - 1104 1 5120"),
    "ops.py:594#3": ("gemm_f32_kernel<128, 128, true, false, true, true> - 768 1 512",
        "gemm_s6_kernel<false, true, true> - 1104 1 512"),
    "ops.py:226#3": ("wgrad_f32_kernel<128, false, false> wgrad_reduce_kernel 128 63 1120",
        "wgrad_f32_kernel<128, false, true> wgrad_reduce_kernel 128 63 1120"),
    "ops.py:226#4": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 256 16 416",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 256 16 416"),
    "ops.py:229#3": ("gemm_f32_kernel<128, 128, true, false, true, false> - 768 1 256",
        "gemm_s6_kernel<false, true, false> - 896 1 256"),
    "ops.py:226#5": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 256 16 416",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 256 16 416"),
    "ops.py:229#4": ("gemm_f32_kernel<64, 64, true, false, true, false> - 400 1 2048",
        "gemm_s6_kernel<false, true, false> - 112 1 2048"),
    "ops.py:226#6": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 640 40 160",),
    "ops.py:229#5": ("gemm_f32_kernel<64, 64, true, false, true, false> - 400 1 256",
        "gemm_s6_kernel<false, true, false> - 112 1 256"),
    "ops.py:334#2": ("gemm_f32_kernel<64, 64, true, false, true, false> - 512 1 200",),
    "ops.py:343#2": ("gemm_f32_kernel<64, 64, false, false, true, false> - 512 1 200",),
    "ops.py:344#2": ("gemm_f32_kernel<64, 64, true, false, true, false> - 512 1 200",),
    "ops.py:226#7": ("gemm_f32_kernel<64, 64, false, false, true, false> - 48 1 6400",),
    "ops.py:229#6": ("gemm_f32_kernel<64, 64, true, false, true, false> - 1024 1 256",
        "gemm_s6_kernel<false, true, false> - 304 1 256"),
    "deepspeech2.py:258": ("gemm_f32_kernel<64, 64, true, true, true, false> - 50 1 500",),
    "deepspeech2.py:260": ("gemm_f32_kernel<64, 64, true, true, true, false> - 50 1 80",),
    "deepspeech2.py:294": ("gemm_f32_kernel<64, 64, true, true, true, false> splitk_reduce4_kernel 260 20 128",),
    "deepspeech2.py:306": ("gemm_f32_kernel<64, 64, true, true, true, false> - 39 1 64",),
    "deepspeech2.py:319": ("gemm_f32_kernel<64, 64, true, true, true, false> - 13 1 64",),
    "deepspeech2.py:321": ("gemm_f32_kernel<64, 64, true, true, true, false> - 13 1 64",),
    "deepspeech2.py:327": ("gemm_f32_kernel<64, 64, true, true, true, false> - 13 1 64",),
    "deepspeech2.py:461": ("gemm_f32_kernel<64, 64, false, false, false, false> - 9 9 96",),
    "deepspeech2.py:352": ("gemm_f32_kernel<64, 64, true, true, false, false> - 13 1 45",),
    "deepspeech2.py:461#1": ("gemm_f32_kernel<64, 64, false, false, true, false> - 9 9 96",),
    "deepspeech2.py:363": ("gemm_f32_kernel<64, 64, true, true, true, false> - 13 1 64",),
    "deepspeech2.py:461#2": ("gemm_f32_kernel<64, 64, false, false, true, false> - 27 9 96",),
    "deepspeech2.py:461#3": ("gemm_f32_kernel<64, 64, false, false, true, false> - 27 9 96",),
    "deepspeech2.py:379": ("gemm_f32_kernel<64, 64, true, true, true, false> - 13 1 192",),
    "deepspeech2.py:461#4": ("gemm_f32_kernel<64, 64, false, false, true, false> - 200 5 160",),
    "deepspeech2.py:388": ("gemm_f32_kernel<64, 64, true, true, true, false> - 520 1 64",),
    "deepspeech2.py:461#5": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 100 25 64",),
    "deepspeech2.py:440": ("gemm_f32_kernel<64, 64, true, true, true, false> - 50 1 80",),
    "deepspeech2.py:442": ("gemm_f32_kernel<64, 64, true, true, true, false> - 50 1 80",),
    "deepspeech2.py:461#6": ("gemm_f32_kernel<64, 64, false, false, true, false> - 128 8 224",),
    "deepspeech2.py:446": ("gemm_f32_kernel<64, 64, true, true, true, false> - 200 1 80",),
    "deepspeech2.py:258#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 500",),
    "deepspeech2.py:260#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 80",),
    "deepspeech2.py:294#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 1000 10 256",),
    "deepspeech2.py:306#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 300 1 64",),
    "deepspeech2.py:319#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 100 1 64",),
    "deepspeech2.py:321#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 100 1 64",),
    "deepspeech2.py:327#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 100 1 64",),
    "deepspeech2.py:461#7": ("gemm_f32_kernel<64, 64, false, false, false, false> splitk_reduce4_kernel 50 50 128",),
    "deepspeech2.py:352#1": ("gemm_f32_kernel<64, 64, true, true, false, false> - 100 1 45",),
    "deepspeech2.py:461#8": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 50 50 128",),
    "deepspeech2.py:363#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 100 1 64",),
    "deepspeech2.py:461#9": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 150 50 128",),
    "deepspeech2.py:461#10": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 150 50 128",),
    "deepspeech2.py:379#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 100 1 192",),
    "deepspeech2.py:461#11": ("gemm_f32_kernel<64, 64, false, false, true, false> - 640 16 416",),
    "deepspeech2.py:388#1": ("gemm_f32_kernel<128, 128, true, true, true, false> - 768 1 64",),
    "deepspeech2.py:461#12": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 232 58 224",),
    "deepspeech2.py:440#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 80",),
    "deepspeech2.py:442#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 400 1 80",),
    "deepspeech2.py:461#13": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 640 40 320",),
    "deepspeech2.py:446#1": ("gemm_f32_kernel<64, 64, true, true, true, false> - 1024 1 80",),
    "rnn_ops.py:47": ("gemm_f32_kernel<64, 64, true, true, true, false> - 1024 1 256",),
    "rnn_ops.py:81": ("gemm_f32_kernel<64, 64, true, false, true, false> - 400 1 768",),
    "rnn_ops.py:84": ("gemm_f32_kernel<64, 64, false, false, true, false> - 768 16 416",),
    "rnn_ops.py:89": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 600 50 128",),
    "rnn_ops.py:89#1": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 600 50 128",),
    # gemm_plans[...]: the rows tests/test_gpu_gemm_plans.py runs on the device, one per (kernel, reduce kernel) pair the planner can
    # name and per path inside one (tile numbering, epilogue, shifted operand).  No trace stands behind these: each entry is what the
    # planner printed for the row in the commit that added the row, so they pin the planner to itself from then on.
    "gemm_plans[otkc_slow]": ("gemm_f32_kernel<64, 64, false, true, false, false> - 2 1 33",),
    "gemm_plans[otkc_fast]": ("gemm_f32_kernel<64, 64, false, true, true, false> - 1 1 64",),
    "gemm_plans[otkc_colsum]": ("gemm_f32_kernel<64, 64, false, true, true, false> - 6 1 64",),
    "gemm_plans[t128_nt_fast]": ("gemm_f32_kernel<128, 128, true, true, true, false> - 512 1 32",),
    "gemm_plans[t128_nt_slow]": ("gemm_f32_kernel<128, 128, true, true, false, false> - 512 1 33",),
    "gemm_plans[t128_nn]": ("gemm_f32_kernel<128, 128, true, false, true, false> - 512 1 40",),
    "gemm_plans[t128_tn]": ("gemm_f32_kernel<128, 128, false, false, true, false> - 512 1 40",),
    "gemm_plans[t128_otkc]": ("gemm_f32_kernel<128, 128, false, true, true, false> - 512 1 40",),
    "gemm_plans[t128_splitk]": ("gemm_f32_kernel<128, 128, true, true, true, false> splitk_reduce_kernel 1536 3 704",),
    "gemm_plans[t128_splitk_tn]": ("gemm_f32_kernel<128, 128, false, false, false, false> splitk_reduce_kernel 1536 3 704",),
    "gemm_plans[panels]": ("gemm_f32_kernel<128, 128, true, true, true, false> - 2058 1 32",),
    "gemm_plans[sk_counters]": ("gemm_f32_kernel<64, 64, false, false, false, false> - 16 8 64",),
    "gemm_plans[sk_counters_dx]": ("gemm_f32_kernel<64, 64, true, false, true, false> - 60 10 64",),
    "gemm_plans[sk_r4]": ("gemm_f32_kernel<64, 64, false, false, true, false> splitk_reduce4_kernel 136 34 64",),
    "gemm_plans[sk_shift]": ("gemm_f32_kernel<64, 64, false, false, true, false> - 12 6 96",),
    "gemm_plans[wg128_sk]": ("wgrad_f32_kernel<128, true, false> wgrad_reduce_sk_kernel<128> 16 1 3328",
        "wgrad_f32_kernel<128, true, true> wgrad_reduce_sk_kernel<128> 16 1 3328"),
    "gemm_plans[wg256_sk]": ("wgrad_f32_kernel<256, true, false> wgrad_reduce_sk_kernel<256> 16 1 3328",
        "wgrad_f32_kernel<256, true, true> wgrad_reduce_sk_kernel<256> 16 1 3328"),
    "gemm_plans[wg_split]": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 64 4 1056",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 64 4 1056"),
    "gemm_plans[wg_split128]": ("wgrad_f32_kernel<128, false, false> wgrad_reduce_kernel 64 4 1056",
        "wgrad_f32_kernel<128, false, true> wgrad_reduce_kernel 64 4 1056"),
    "gemm_plans[wg_whole]": ("wgrad_f32_kernel<128, false, false> - 64 1 1056",
        "wgrad_f32_kernel<128, false, true> - 64 1 1056"),
    "gemm_plans[wg_shift]": ("wgrad_f32_kernel<256, false, false> wgrad_reduce_kernel 64 4 1056",
        "wgrad_f32_kernel<256, false, true> wgrad_reduce_kernel 64 4 1056"),
    "gemm_plans[wg_shift_nows]": ("wgrad_f32_kernel<256, false, false> - 16 1 4160",
        "wgrad_f32_kernel<256, false, true> - 16 1 4160"),
    "gemm_plans[s6_anc]": ("gemm_f32_kernel<64, 64, false, false, true, false> - 768 1 48",
        "gemm_s6_kernel<true, true, false> - 256 1 48"),
    "gemm_plans[s6_anc_novec]": ("gemm_f32_kernel<64, 64, false, false, true, false> - 768 1 48",
        "gemm_s6_kernel<true, true, false> - 256 1 48"),
    "gemm_plans[s6_bnc]": ("gemm_f32_kernel<64, 64, true, false, true, false> - 6 1 48",
        "gemm_s6_kernel<false, true, false> - 3 1 48"),
    "gemm_plans[tri1_128]": ("gemm_f32_kernel<128, 128, true, false, true, true> - 512 1 256",),
    "gemm_plans[tri2_128]": ("gemm_f32_kernel<128, 128, false, false, true, true> - 512 1 256",),
    "gemm_plans[ext128_ragged]": ("gemm_f32_kernel<128, 128, true, true, true, true> - 512 1 64",),
    "gemm_plans[ext64_tri2]": ("gemm_f32_kernel<64, 64, false, false, true, true> - 6 1 72",),
    "gemm_plans[ext64_dx_mask]": ("gemm_f32_kernel<64, 64, true, false, true, true> - 6 1 64",),
    "gemm_plans[t128_tn_slow]": ("gemm_f32_kernel<128, 128, false, false, false, false> - 512 1 40",),
    "gemm_plans[t128_nn_slow]": ("gemm_f32_kernel<128, 128, true, false, false, false> - 512 1 40",),
    "gemm_plans[t128_splitk_nn_slow]": ("gemm_f32_kernel<128, 128, true, false, false, false> splitk_reduce_kernel 1536 3 704",),
    "gemm_plans[t128_splitk_nn]": ("gemm_f32_kernel<128, 128, true, false, true, false> splitk_reduce_kernel 1536 3 704",),
    "gemm_plans[t128_splitk_nt_slow]": ("gemm_f32_kernel<128, 128, true, true, false, false> splitk_reduce_kernel 1536 3 704",),
    "gemm_plans[sk_nn_slow_c]": ("gemm_f32_kernel<64, 64, true, false, false, false> - 16 8 64",),
    "gemm_plans[sk_nt_slow_c]": ("gemm_f32_kernel<64, 64, true, true, false, false> - 16 8 64",),
    "gemm_plans[sk_nt_c]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 32 8 64",),
    "gemm_plans[sk_tn_slow_c4]": ("gemm_f32_kernel<64, 64, false, false, false, false> - 32 16 64",),
    "gemm_plans[sk_nn_slow_c4]": ("gemm_f32_kernel<64, 64, true, false, false, false> - 32 16 64",),
    "gemm_plans[sk_nt_slow_c4]": ("gemm_f32_kernel<64, 64, true, true, false, false> - 32 16 64",),
    "gemm_plans[sk_nt_c4]": ("gemm_f32_kernel<64, 64, true, true, true, false> - 64 16 64",),
    "gemm_plans[sk_tn_slow_r4]": ("gemm_f32_kernel<64, 64, false, false, false, false> splitk_reduce4_kernel 68 34 64",),
    "gemm_plans[sk_nn_slow_r4]": ("gemm_f32_kernel<64, 64, true, false, false, false> splitk_reduce4_kernel 68 34 64",),
    "gemm_plans[sk_nt_slow_r4]": ("gemm_f32_kernel<64, 64, true, true, false, false> splitk_reduce4_kernel 68 34 64",),
    "gemm_plans[sk_nt_r4]": ("gemm_f32_kernel<64, 64, true, true, true, false> splitk_reduce4_kernel 136 34 64",),
}


def _grid(kernel, work, per_xcd):
    """The grid a plan's launcher asks for, unless it clamps to resident slots: the weight-gradient kernels launch whole XCD rounds."""
    return 8 * per_xcd if kernel.startswith("wgrad_f32_kernel") else work


def test_planner_decision_table_and_sweep(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan_rows.json")) as f:
        rows = json.load(f)
    assert sorted(r["name"] for r in rows) == sorted(EXPECTED)
    listing = tmp_path / "rows.txt"
    listing.write_text("".join(r["name"] + " " + " ".join(f"{k}={v}" for k, v in r.items() if k != "name" and v) + "\n" for r in rows))
    exe = str(tmp_path / "gemm_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan",   # the runtime inside the program: whatever else a machine loads into its processes
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "artspeech_amd", "csrc", "gemm_plan.cpp"), os.path.join(ROOT, "tests", "gemm_plan_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe, str(listing)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"sweep: \d+ plans, \d+ refusals; .*", lines[-1]), lines[-1]
    swept = {line[len("pair: "):] for line in lines if line.startswith("pair: ")}
    assert len(swept) >= 40, sorted(swept)
    got = {}
    for line in lines[:-1]:
        if line.startswith("pair: "):
            continue
        name, rest = line.split(" arith=")
        got[(name, int(rest[0]))] = rest[2:]
    assert len(got) == 2 * len(rows)
    wrong = []
    shape = {r["name"]: r for r in rows}
    for name, want in EXPECTED.items():
        for arith in (0, 1):
            w, g = want[arith if len(want) == 2 else 0], got[(name, arith)]
            if w == "refused":
                ok = g.startswith("refused (-1)")
            else:
                m = re.fullmatch(r"(.*) reduce=(\S+) work=(\d+) per_xcd=(\d+) splitk=(\d+) kchunk=(\d+)", g)
                ok = m is not None
                if ok:
                    kernel, reduce = m.group(1), m.group(2)
                    work, per_xcd, splitk, kchunk = (int(x) for x in m.groups()[2:])
                    wk, wr, wgrid, wsplit, wchunk = re.fullmatch(r"(.*>) (\S+) (\d+) (\S+) (\S+)", w).groups()
                    grid = _grid(kernel, work, per_xcd)
                    clamped = kernel.startswith("gemm_f32_kernel") and grid > int(wgrid) >= 512 and int(wgrid) % 256 == 0
                    # (the arrival counters leave no reduce kernel in a trace)
                    tile = re.match(r"gemm_f32_kernel<(\d+), ", kernel)
                    if tile:   # a tile kernel's work items follow from the shape and the split
                        t, r = int(tile.group(1)), shape[name]
                        clamped = clamped and work == -(-r["M"] // t) * -(-r["N"] // t) * r["batch"] * splitk
                    ok = (kernel == wk and (reduce if not reduce.startswith("counters/") else "-") == wr and
                          (grid == int(wgrid) or clamped) and (splitk, kchunk) == (int(wsplit), int(wchunk)))
            if not ok:
                wrong.append((name, arith, w, g))
    assert not wrong, wrong[:10]
    # closure: whatever the planner can name for a legal descriptor runs on the device in a kernel-level test.  The call-site rows
    # (file.py:line) do not count: the suite reaches them only inside whole-model checks.
    tested = set()
    for (name, arith), g in got.items():
        m = re.fullmatch(r"(.*) reduce=(\S+) work=.*", g)
        if m and not re.match(r"\w+\.py:\d+", name):
            tested.add(m.group(1) + " | " + m.group(2))
    assert not swept - tested, sorted(swept - tested)


def test_fp64_reference_against_a_scalar_loop():
    """tests/gemm_fp64.py, the yardstick of test_gpu_gemm_plans.py, against the header's formula written out element by element of C:
    strides, overlapping batch windows, the shifted B operand and its zeros.  Every legal row of modest size poses, and no NaN
    (an element the descriptor does not address) reaches its reference."""
    import numpy as np

    import gemm_fp64 as G
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan_rows.json")) as f:
        rows = {r["name"]: r for r in json.load(f)}
    for name in ("gemm_plans[sk_shift]", "gemm_shift_batched", "gemm_plans[otkc_slow]"):
        r = rows[name]
        ops = G.pose(r, np.random.RandomState(2))
        A, B = ops["A"], ops["B"]
        want = np.zeros((r["batch"], r["M"], r["N"]))
        for g in range(r["batch"]):
            s = r["b_kshift"] + g * r["b_kshift_batch"]
            k = np.arange(r["K"])
            live = (k % r["b_kT"] + s >= 0) & (k % r["b_kT"] + s < r["b_kT"]) if r["b_kT"] > 0 else np.ones(r["K"], bool)
            kb = k[live] + (s if r["b_kT"] > 0 else 0)
            for i in range(r["M"]):
                for j in range(r["N"]):
                    a = A.data[A.start + g * r["a_batch"] + i * r["a_i"] + k[live] * r["a_k"]].astype(np.float64)
                    b = B.data[B.start + g * r["b_batch"] + j * r["b_j"] + kb * r["b_k"]].astype(np.float64)
                    want[g, i, j] = float(np.dot(a, b))
        got = G.reference(r, ops)["C"]
        assert not np.isnan(want).any() and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name
    posed = 0
    for name, want in EXPECTED.items():
        r = rows[name]
        if want[0] == "refused" or 2.0 * r["M"] * r["N"] * r["K"] * r["batch"] > 2e6:
            continue
        ops = G.pose(r, np.random.RandomState(posed))
        ref = G.reference(r, ops)
        assert not np.isnan(ref["C"]).any() and (ref["colsum"] is None or not np.isnan(ref["colsum"]).any()), name
        for k, o in ops.items():
            if isinstance(o, G.Operand):
                assert o.start * 4 % 16 == r[k] % 16 and o.data.size - int(np.flatnonzero(o.addressed)[-1]) > 4, (name, k)
        posed += 1
    assert posed >= 30
