"""Operator edge cases shared by tests/test_emu_ops_edges.py (CPU, through the emulator) and tests/test_gpu_ops_edges.py (device memory).

What the value tests of test_gpu_ops / test_gpu_winograd / test_gpu_fp16 / test_gpu_b3 cannot see:
  * an access outside a tensor.  Every case here runs on a guarded mem (opcheck.GuardedNumpyMem / GuardedTorchMem: NaN bands around the
    inputs, a fixed pattern around the outputs) and ends with mem.verify(); the shapes are the smallest at which each kernel's ragged
    paths exist (Cout = 19 / 130, a last M tile of a few rows, a Winograd tile grid that overhangs the map, a key tile of one key);
  * kernels and launch shapes that otherwise run inside whole frames only, where the 1e-3 logit gate is all that judges them: the three
    classifier kernels, the classifier inside the head conv's output transform, the plane LayerNorm at 2048 channels and at the
    512-strip cap, the attention as two 256-channel slices and at d_v = 2048;
  * the forms of the fp16 mode (tdnet_opts.precision = 1) that only the rim of a frame's fp16 backbone reaches, where the 3e-2 logit gate
    is all that judges them: the max-pool alone in its three storage forms (on data with negative values, so the padding value shows),
    the fp16-MFMA stem writing an fp16 map + the fp16 max-pool, convs with mixed storage (fp32 in / fp16 out, fp16 in + fp16 residual /
    fp32 out, the latter on every LDS-DMA form), the LayerNorm map as fp16, the fp16 attention on the edge shapes.  Their references are
    fp64 on the operands as the kernels round them (opcheck.t16 / gate_f16), or bit equality where the code makes two forms the same.
  * the split kernels of tdnet_opts.precision = 2 / 3 (three bf16 parts per fp32 operand, six bf16-MFMA products per product) on their
    edge shapes -- every epilogue role of the split GEMM, tiles outnumbering workgroups, the narrow direct convs and the packed-row stem,
    the three attention forms at 128 / 512 / 2048 channels, the head conv + classifier behind the split GEMM -- where 1e-4 against fp32
    cannot see a lost product (~2^-18): the products alone against fp64, in max and rms error, relative to the fp32 CPU evaluation's own
    error (x3 / x2) or, on the Winograd route, to the exact-fp32 Winograd kernel's (x1.25 / x1.1): opcheck.split_conv / split_stem /
    split_attention, also on non-negative data and on per-channel power-of-two scales.
  * three launch forms that ran inside whole frames only (sections 8 to 10), through the function a frame calls:
      8. grouped fp16 convs -- run_conv_group / k_conv_igemm_h_group, up to three convs in one grid, each block on a member-local (bid, nblk) --
         against the single launches BIT FOR BIT (opcheck.conv_group; the single launch is held to the rounding-aware fp64 gate by
         opcheck.conv_f16io), with the entry's "grouped" flag asserted; and the fallbacks that must run the members one by one;
      9. the cache sub-sample -- k_subsample2 through encode_frame's launch -- against numpy's [::4, ::4] bit for bit, up to a case that needs
         a second trip of the grid-stride loop;
     10. the 1x1 downsample conv on one row class -- run_ds_rows, a batched GEMM with one weight set, on k_gemm_persistent and k_gemm_b3 --
         against the same rows of the whole-map conv bit for bit, at the route's gate on those rows, the other rows still unwritten
         (opcheck.conv1x1_rows; the guarded mem's unwritten_rows).
    Section 8: all 36 grouped cases (6 member lists x tiles 3 / 4 / 5 x fp16 / fp32 maps) really ran k_conv_igemm_h_group -- the flag is asserted -- and
    the 5 fallback cases ran one launch per member; member block counts covered: 1, 5, 9, 10, 15, 18 and 20 (10 | 18 | 15 beside 5 | 9 | 5 beside
    5 | 9 | 5 on the three-member lists).  Section 10 on the split GEMM (k_gemm_b3, precision 3), written rows only, max / rms error against fp64 as
    multiples of the fp32 CPU evaluation's (gate x3 + 1e-7 / x2 + 1e-9), rows 0 mod 2 | rows 1 mod 2, under the emulator:
        5x9 64->128          x0.69 / x0.68 | x0.52 / x0.67        9x17 128->256        x0.63 / x0.64 | x0.70 / x0.65
        1x9 64->128          x0.61 / x0.65 | no rows              12x70 256->512 g3    x0.65 / x0.63 | x0.54 / x0.63
        4x300 64->132        x0.45 / x0.67 | x0.73 / x0.67        6x150 64->130        x1.00 / x1.00: N % 4 != 0, the plan keeps the fp32 GEMM
    (the device's figures: tests/test_gpu_ops_edges.py).  With one defect seeded at a time, under the emulator: a member called with another member's
    block count, member 0 of the KS0 != KS1 branch with end[1], `<=` in the member pick -- 15, 9 and 18 of the 18 test_conv_groups cases fail;
    k_subsample2 indexing the source with wo -- the three test_cache_subsample cases; its loop without the grid stride --
    test_cache_subsample_second_trip_of_the_grid; run_ds_rows with MP = W, or starting at row 0 for cy = 1 -- 20 and 10 of the 24
    test_row_class_downsample cases (all that have rows to write).

Each function takes (lib, mem) and one entry of its case list; values are checked by the opcheck functions at the tolerance the
route's existing tests use."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import opcheck
from tdnet_amd import _capi

DIRECT = {"winograd": 0}
WINO = {"winograd": 4}
CHAINS = 41 | 4                                                        # tdnet_opts.overlap: row-parity chunks on the wave-per-tile transforms

# ---- 1. guard bands on the routes that already have value tests ---------------------------------------------------------------------
# (H, W, Cin, Cout, KS, stride, dil, act, resid)
DIRECT_CONVS = [(11, 19, 64, 19, 1, 1, 1, 2, False),                   # 19 channels, LeakyReLU
                (5, 7, 32, 1, 1, 1, 1, 0, False),                      # one output channel
                (13, 21, 32, 96, 3, 2, 1, 0, False),                   # stride 2, Cout not a tile multiple
                (5, 7, 64, 130, 3, 1, 2, 1, True),                     # two channels into a second N tile, dilation 2 on a 5 x 7 map, residual
                (7, 9, 96, 64, 1, 1, 1, 1, False)]                     # three K steps, 63 rows
DIRECT_TILES = [0, 1, 2, 3, 4, 5, None]                                # None: the heuristic's
WINO_CONVS = [(13, 21, 64, 128, 3, 1, 2, 1, True), (5, 9, 256, 512, 3, 1, 16, 2, False), (1, 1, 32, 32, 3, 1, 1, 0, False),
              (9, 17, 128, 256, 3, 1, 8, 0, True)]
CHUNKED_CONVS = [(12, 30, 128, 128, 3, 1, 4, 1, False), (9, 17, 128, 256, 3, 1, 8, 0, True)]   # 9 rows: the two parities differ in size
# (conv arguments, tdnet_opts)
SPLIT_CONVS = [((12, 17, 32, 48, 3, 2, 1, 2, True), {"precision": 2}), ((13, 21, 128, 132, 3, 1, 2, 1, False), {"precision": 3})]
STEMS = [(7, 9), (33, 65)]
STEM_OPTS = [{}, {"precision": 2}, {"precision": 1}]                   # precision 1: the fp16-MFMA stem writing fp32, against the rounding-aware reference
# (conv arguments, tiles)
F16_CONVS = [((13, 21, 128, 160, 3, 1, 1, 1, True), (16, 17, 31, 32)), ((13, 21, 64, 64, 3, 1, 1, 1, True), (34,)),
             ((9, 11, 192, 130, 1, 2, 1, 2, True), (16, None))]
PPMS = [(5, 9), (5, 5), (6, 6), (7, 13)]                               # h, w >= 5: the smallest feature map of an accepted frame
UPSAMPLES = [(19, 5, 9, 33, 65), (3, 5, 9, 33, 64), (1, 2, 2, 7, 7), (2, 1, 1, 5, 8)]   # W % 4 == 0: the x4 kernel on a small map
SCHEDULES = [0, 1, 2]
# (Lq, Lk, DV): one row past a 32-row strip, one key past a 128-key tile
ATTENTIONS = [(45, 6, 512), (33, 1, 128), (65, 129, 512)]
ATTENTION_F16 = 16                                                     # tdnet_op_attention's code of the fp16-MFMA kernel (td_attn_h.h), on ATTENTIONS

# ---- 2. the classifier kernels ------------------------------------------------------------------------------------------------------
# (NC, C, HW): k_classifier<19> / <32> on both sides of 19 and 32, the class-tiled kernel with a ragged last tile; C = 512 with 32
# classes is a 96 KiB dynamic-LDS launch
CLASSIFIERS = [(1, 16, 1), (19, 128, 65), (19, 64, 63), (20, 64, 63), (32, 128, 64), (32, 512, 70), (33, 512, 70), (40, 128, 131),
               (150, 128, 131), (256, 16, 5)]

# ---- 3. the head conv with the classifier inside ------------------------------------------------------------------------------------
# (Cout, Cin, (H, W)); 7 x 4: two tiles, not a multiple of the four a workgroup takes
HEADS = [(co, ci, hw) for co in (64, 128) for ci in (128, 512) for hw in ((5, 9), (13, 21), (7, 4))]
HEAD_NCS = [1, 19, 20, 32]
HEAD_ACTS = [0, 1]

# ---- 4. plane LayerNorm -------------------------------------------------------------------------------------------------------------
# (HW, C): C = 2048 is 512 threads with one row per strip pass; 513 and 1025 rows hit the 512-strip cap with 2 and 3 rows per strip, a
# ragged last strip and empty strips
LAYERNORMS = [(2, 4), (1, 128), (45, 2048), (513, 2048), (1025, 512)]
# (HW, C, mean, std)
LAYERNORMS_FLAT = [(45, 128, 5.0, 1e-3), (1000, 512, 50.0, 1e-3), (513, 2048, 5.0, 3e-3)]

# ---- 5. attention routes only frames reach ------------------------------------------------------------------------------------------
# (Lq, Lk, bias, resid, spike) at d_v = 512 as two 256-channel slices (online | 64)
SLICED_ATTENTIONS = [(45, 6, True, True, False), (153, 200, True, True, True), (64, 128, False, False, False)]
WIDE_ATTENTIONS = [(70, 260, 2048), (33, 1, 2048)]                     # four 512-channel launches on a strided V'

# ---- 6. forms of the fp16 mode (tdnet_opts.precision = 1) that otherwise run inside frames only --------------------------------------
# the max-pool alone: (H, W) x C x mode (0: fp32, 1: fp32 in / fp16 out, 2: fp16 in and out); C = 128: behind the deep stem
MAXPOOLS = [(1, 1), (2, 3), (7, 9), (8, 10), (33, 65)]
MAXPOOL_CS = [64, 128]
MAXPOOL_MODES = [0, 1, 2]
STEMS_F16 = [(7, 9), (33, 65), (40, 52)]                               # the fp16-MFMA stem writing an fp16 map + the fp16 max-pool
MIXED_TILES = [3, 4, 5, None]                                          # register-staged tiles for in32 -> out16 and in16 -> out32
DMA_TILES = [16, 17, 18, 19, 31, 32, 34, 35, None]                     # in16 -> out32 with a residual: the head conv's epilogue of every LDS-DMA form

# ---- 7. the split kernels of tdnet_opts.precision = 2 / 3 (three bf16 parts per fp32 operand, six bf16-MFMA products per product) -----
# Each case runs twice on the guarded mem: the full form (bias, residual, activation, LayerNorm statistics) at the route's tolerance, then
# the products alone against fp64 at a gate that sees ONE lost product of the six (opcheck.SPLIT_GATE / SPLIT_WINO_GATE).
SPLIT = {"precision": 3}                                               # the split GEMM at any size
SPLIT_WINO = {"winograd": 4, "precision": 3}
NARROW = {"precision": 2}
# (conv arguments, tdnet_opts, Winograd route): k_gemm_b3<2> (1x1), <0> (1x1 + residual), <1> (the 36 Winograd GEMMs).
# K = 32 is the two-step minimum of gemm_b3_supports, but plan_conv gives a GEMM to the persistent kernels -- k_gemm_b3 among them -- only
# where gemm_supports(K): K % 64 == 0.  So the K = 32 entries run elsewhere: the 1x1 convs on k_conv_adirect_b3<1, 0> (one step), the
# Winograd conv on the exact-fp32 batched conv kernel, bit for bit (SPLIT_STAYS_EXACT); K = 64, four steps, is the least k_gemm_b3 sees.
SPLIT_GEMMS = [((5, 7, 32, 128, 1, 1, 1, 0, False), SPLIT, False),     # K = 32, two 64-column tiles of the split direct kernel
               ((5, 7, 32, 4, 1, 1, 1, 1, True), SPLIT, False),        # K = 32, N = 4 padded to one tile
               ((33, 9, 192, 128, 1, 1, 1, 0, False), SPLIT, False),   # twelve steps, a second M tile of 41 rows
               ((7, 9, 64, 128, 1, 1, 1, 0, True), SPLIT, False),
               ((11, 19, 64, 160, 1, 1, 1, 2, True), SPLIT, False),    # 32 columns into a second N tile, LeakyReLU
               ((35, 37, 64, 256, 1, 1, 1, 1, False), dict(SPLIT, gemm_persistent=3), False),   # 12 tiles (the last rows ragged) walked by three workgroups
               ((1, 1, 32, 32, 3, 1, 1, 0, False), SPLIT_WINO, True),  # K = 32: stays on the exact-fp32 kernel
               ((1, 1, 64, 32, 3, 1, 1, 0, False), SPLIT_WINO, True),  # one tile row per GEMM, four steps, N = 32
               ((5, 9, 256, 512, 3, 1, 16, 2, False), SPLIT_WINO, True),
               ((13, 21, 128, 132, 3, 1, 2, 1, False), SPLIT_WINO, True),
               ((9, 17, 128, 256, 3, 1, 8, 0, True), dict(SPLIT_WINO, overlap=CHAINS), True),   # row-parity chunks of different size
               ((12, 14, 128, 132, 3, 1, 1, 1, True), dict(SPLIT_WINO, gemm_persistent=5), True)]   # 72 tiles in 36 batches walked by five workgroups
SPLIT_STAYS_EXACT = [(1, 1, 32, 32, 3, 1, 1, 0, False)]
# k_conv_adirect_b3<3, 0> / <1, 0>; the packed-row stem <7, 2> runs on STEMS
SPLIT_NARROW = [((13, 21, 64, 64, 3, 1, 1, 1, True), NARROW),          # ResNet layer1
                ((11, 9, 96, 48, 3, 2, 2, 0, False), NARROW),          # 27 steps (odd), stride 2, dilation 2, ragged channels
                ((9, 17, 64, 40, 1, 2, 1, 0, False), NARROW),          # the strided 1x1 form
                ((13, 21, 64, 128, 3, 2, 1, 1, False), dict(NARROW, winograd=0)),   # 65 .. 128 output channels as two 64-column tiles
                ((9, 17, 64, 100, 1, 2, 1, 0, True), NARROW),          # a ragged second column tile, residual
                ((12, 17, 32, 48, 3, 2, 1, 2, True), NARROW),          # one chunk of 32 channels
                ((96, 96, 64, 64, 1, 1, 1, 1, True), NARROW)]          # a stride-1 1x1 on >= 8192 pixels: kept off the GEMM route
# the harder inputs (opcheck.SPLIT_DATA), once per kernel: index into the list above
SPLIT_GEMMS_HARD = [4, 9]
SPLIT_NARROW_HARD = [1, 4]
SPLIT_ONLINES = [17, 18, 19]                                           # 17: the form by size, 18: k_attention_b3w (64 queries), 19: k_attention_b3<1, 4, 4>
# (Lq, Lk, DV, online, spike, ramp)
SPLIT_ATTENTIONS = ([(Lq, Lk, DV, o, False, False) for (Lq, Lk, DV) in ATTENTIONS for o in SPLIT_ONLINES if o == 17 or DV % 512 == 0] +
                    [a + (o, False, False) for a in WIDE_ATTENTIONS for o in SPLIT_ONLINES] +   # four 512-channel launches on ONE pre-split V'
                    [(64, 128, 512, 18, False, False), (97, 130, 512, 18, False, False),        # k_attention_b3w's second query tile: full, one row
                     (130, 193, 128, 17, False, False)] +
                    [(Lq, Lk, DV, o, sp, not sp) for (DV, o) in ((128, 17), (512, 19), (512, 18)) for (Lq, Lk, sp) in ((153, 200, True), (70, 300, False))])
SPLIT_ATTENTIONS_HARD = [(65, 129, 128, 17), (65, 129, 512, 19), (65, 129, 512, 18)]
HEAD_SPLIT = dict(WINO, precision=3)                                   # the head conv's 36 GEMMs on k_gemm_b3: CoutPad = gemm_b3_npad(Cout) in front of k_wino4_out_cls

# Measured under the emulator with the unmodified kernels (the device's figures: tests/test_gpu_ops_edges.py).  Errors against fp64 as
# max / rms; cpu32: the fp32 torch evaluation on the CPU; exact, split: the exact-fp32 and the split kernel as multiples of cpu32 (gate
# of the split kernel: x3 / x2), on the Winograd route the exact kernel's own error and the split kernel as a multiple of it (gate: x1.25
# / x1.1).  p2 / p3: precision, w4 / w0: winograd, g: gemm_persistent.  "scaled" equals "normal" to the digit on the convs: the scales
# are exact, so the kernels form the same products from other exponents.  The largest: x1.50 / x1.21 (11x9 96->48 on abs data).
# With one of the six MFMAs of a product loop removed -- k_gemm_b3 (second- and third-order terms, either column group), k_conv_adirect_b3
# (either k block), the Q K^T and P V' loops of k_attention_b3 and k_attention_b3w -- or with a part used twice, 6 to 24 of the cases below
# miss their gate, in every form of the kernel; a third-order term moves the rms figure to x8.0 .. x29 on the sharpest case (x2.0 on
# the dullest that still fails), a second-order one to x850 and more.
# conv 5x7 32->128 k1 p3                       cpu32 7.72e-07 / 1.01e-07   exact x1.01 / x0.98   split x0.75 / x0.75
# conv 5x7 32->4 k1 p3                         cpu32 4.01e-07 / 8.61e-08   exact x0.79 / x1.00   split x0.60 / x0.68
# conv 33x9 192->128 k1 p3                     cpu32 1.96e-06 / 2.48e-07   exact x0.91 / x0.99   split x0.82 / x0.64
# conv 7x9 64->128 k1 p3                       cpu32 1.02e-06 / 1.46e-07   exact x1.11 / x1.01   split x0.77 / x0.68
# conv 11x19 64->160 k1 p3                     cpu32 1.54e-06 / 1.44e-07   exact x1.00 / x1.01   split x0.68 / x0.68
# conv 35x37 64->256 k1 p3 g3                  cpu32 1.60e-06 / 1.44e-07   exact x0.89 / x1.00   split x0.71 / x0.68
# conv 1x1 32->32 k3 w4 p3                     exact 3.29e-07 / 1.21e-07   split x1.00 / x1.00 of it
# conv 1x1 64->32 k3 w4 p3                     exact 4.14e-07 / 1.23e-07   split x0.42 / x0.67 of it
# conv 5x9 256->512 k3 d16 w4 p3               exact 2.14e-06 / 2.87e-07   split x0.43 / x0.63 of it
# conv 13x21 128->132 k3 d2 w4 p3              exact 3.38e-05 / 1.80e-06   split x0.53 / x0.68 of it
# conv 9x17 128->256 k3 d8 w4 p3 chains        exact 2.66e-06 / 3.76e-07   split x0.81 / x0.67 of it
# conv 12x14 128->132 k3 w4 p3 g5              exact 3.56e-05 / 2.14e-06   split x0.45 / x0.67 of it
# conv 13x21 64->64 k3 p2                      cpu32 1.78e-06 / 2.86e-07   exact x1.67 / x1.40   split x1.20 / x0.88
# conv 11x9 96->48 k3 s2 d2 p2                 cpu32 1.23e-06 / 2.09e-07   exact x2.76 / x1.99   split x0.98 / x1.17
# conv 9x17 64->40 k1 s2 p2                    cpu32 6.60e-07 / 1.42e-07   exact x1.24 / x1.05   split x1.04 / x0.70
# conv 13x21 64->128 k3 s2 p2 w0               cpu32 1.65e-06 / 2.65e-07   exact x1.78 / x1.43   split x1.30 / x0.88
# conv 9x17 64->100 k1 s2 p2                   cpu32 9.69e-07 / 1.42e-07   exact x0.98 / x1.02   split x0.71 / x0.69
# conv 12x17 32->48 k3 s2 p2                   cpu32 1.94e-06 / 2.76e-07   exact x1.08 / x1.05   split x1.07 / x0.63
# conv 96x96 64->64 k1 p2                      cpu32 1.58e-06 / 1.48e-07   exact x1.13 / x1.00   split x0.77 / x0.68
# stem 7x9                                     cpu32 9.96e-07 / 2.03e-07   exact x0.73 / x0.93   split x0.76 / x0.83
# stem 7x9 abs                                 cpu32 8.83e-07 / 1.67e-07   exact x1.00 / x1.03   split x0.85 / x0.99
# stem 7x9 scaled                              cpu32 9.96e-07 / 2.03e-07   exact x0.73 / x0.93   split x0.76 / x0.83
# stem 33x65                                   cpu32 2.19e-06 / 3.31e-07   exact x0.89 / x1.01   split x0.70 / x0.80
# stem 33x65 abs                               cpu32 2.40e-06 / 2.90e-07   exact x1.00 / x1.00   split x0.71 / x0.79
# stem 33x65 scaled                            cpu32 2.19e-06 / 3.31e-07   exact x0.89 / x1.01   split x0.70 / x0.80
# conv 11x19 64->160 k1 p3 abs                 cpu32 1.32e-06 / 1.46e-07   exact x0.97 / x1.00   split x0.69 / x0.67
# conv 13x21 128->132 k3 d2 w4 p3 abs          exact 2.20e-05 / 1.07e-06   split x0.82 / x0.70 of it
# conv 11x9 96->48 k3 s2 d2 p2 abs             cpu32 1.47e-06 / 2.24e-07   exact x1.87 / x1.95   split x1.50 / x1.21
# conv 9x17 64->100 k1 s2 p2 abs               cpu32 1.16e-06 / 1.55e-07   exact x1.03 / x1.02   split x0.64 / x0.66
# conv 11x19 64->160 k1 p3 scaled              cpu32 1.54e-06 / 1.44e-07   exact x1.00 / x1.01   split x0.68 / x0.68
# conv 13x21 128->132 k3 d2 w4 p3 scaled       exact 3.38e-05 / 1.80e-06   split x0.53 / x0.68 of it
# conv 11x9 96->48 k3 s2 d2 p2 scaled          cpu32 1.23e-06 / 2.09e-07   exact x2.76 / x1.99   split x0.98 / x1.17
# conv 9x17 64->100 k1 s2 p2 scaled            cpu32 9.69e-07 / 1.42e-07   exact x0.98 / x1.02   split x0.71 / x0.69
# attention (45, 6, 512) online 17/18/19       cpu32 5.23e-07 / 7.68e-08   exact x1.03 / x0.90   split x0.81 / x0.77
# attention (33, 1, 128) online 17             every error 0
# attention (65, 129, 512) online 17/18/19     cpu32 3.51e-07 / 4.76e-08   exact x1.58 / x0.94   split x0.68 / x0.67
# attention (70, 260, 2048) online 17/18/19    cpu32 8.51e-07 / 4.23e-08   exact x0.76 / x1.00   split x0.43 / x0.66
# attention (33, 1, 2048) online 17/18/19      every error 0
# attention (64, 128, 512) online 18           cpu32 3.36e-07 / 4.84e-08   exact x0.92 / x0.93   split x0.63 / x0.64
# attention (97, 130, 512) online 18           cpu32 5.03e-07 / 4.73e-08   exact x0.84 / x0.95   split x0.65 / x0.66
# attention (130, 193, 128) online 17          cpu32 7.85e-07 / 4.65e-08   exact x0.84 / x1.05   split x0.39 / x0.67
# attention (153, 200, 128) online 17 spike    cpu32 2.38e-06 / 1.38e-07   exact x0.94 / x1.04   split x0.60 / x0.60
# attention (70, 300, 128) online 17 ramp      cpu32 7.92e-06 / 1.60e-06   exact x1.03 / x1.03   split x0.88 / x0.72
# attention (153, 200, 512) online 19 spike    cpu32 2.31e-06 / 1.30e-07   exact x1.06 / x1.00   split x0.58 / x0.54
# attention (70, 300, 512) online 19 ramp      cpu32 9.43e-06 / 1.65e-06   exact x0.99 / x1.03   split x0.72 / x0.72
# attention (153, 200, 512) online 18 spike    cpu32 2.31e-06 / 1.30e-07   exact x1.06 / x1.00   split x0.58 / x0.54
# attention (70, 300, 512) online 18 ramp      cpu32 9.43e-06 / 1.65e-06   exact x0.99 / x1.03   split x0.72 / x0.72
# attention (65, 129, 128) online 17 abs       cpu32 6.56e-07 / 1.48e-07   exact x1.08 / x1.03   split x0.74 / x0.75
# attention (65, 129, 512) online 19/18 abs    cpu32 6.62e-07 / 1.47e-07   exact x1.00 / x1.01   split x0.85 / x0.75
# attention (65, 129, 128) online 17 scaled    cpu32 1.50e-05 / 1.20e-06   exact x0.84 / x0.86   split x0.75 / x0.59
# attention (65, 129, 512) online 19/18 scaled cpu32 1.49e-05 / 1.18e-06   exact x0.97 / x0.87   split x0.74 / x0.53

# ---- 8. grouped fp16 convs: k_conv_igemm_h_group through run_conv_group (tdnet_opts.fusion bit 131072), whole frames' only route to it ----------
# A member: (H, W, Cin, Cout, KS, stride, dil, act, bias, share) -- bias False: a NULL bias; share: the earlier member whose input map it reads.
# 19 x 29 = 551 pixels are 5 M tiles of 128 rows or 9 of 64, the last one ragged (39 rows); 5 x 8 = 40 pixels are one tile.  With Cout 130 /
# 64 / 19 a member is 10 | 18 | 15, 5 | 9 | 5, 5 | 9 | 5 blocks on tiles 3 | 4 | 5: td_xcd_remap(bid, nblk) is not the identity (nblk >= 9,
# nblk % 8 != 0) and every end[] boundary falls inside a round of eight.  Activations 0 / 1 / 2 and the NULL bias sit on different members.
GROUP_TILES = [3, 4, 5]                                                # 128 x 128, 64 x 128, 128 x 64 on the two-stage pipeline
GROUP_STORAGES = [(True, True), (False, False)]                        # (in16, out16): fp16 maps, and the fp32 maps plan_conv leaves on CR_CONV_H
CONV_GROUPS = [
    # the Encoding's first layers: three 1x1 convs on ONE map
    [(19, 29, 64, 130, 1, 1, 1, 1, True, None), (19, 29, 64, 64, 1, 1, 1, 2, False, 0), (19, 29, 64, 19, 1, 1, 1, 0, True, 0)],
    [(19, 29, 128, 130, 1, 1, 1, 0, False, None), (19, 29, 128, 64, 1, 1, 1, 1, True, None), (19, 29, 128, 19, 1, 1, 1, 2, True, None)],   # three maps, two K steps
    # the query / key second layers: the key branch on the 16x smaller grid, one tile
    [(19, 29, 64, 64, 1, 1, 1, 1, True, None), (5, 8, 64, 64, 1, 1, 1, 0, True, None)],
    # a BasicBlock's 3x3 stride-2 conv1 beside its 1x1 stride-2 downsample (the KS0 != KS1 branch: member 0 takes (b, end[0]))
    [(37, 57, 64, 128, 3, 2, 1, 1, True, None), (37, 57, 64, 128, 1, 2, 1, 0, True, 0)],
    # a dilated block: 3x3 stride 1 dilation 2 beside a 1x1 stride-1 downsample
    [(19, 29, 128, 256, 3, 1, 2, 1, False, None), (19, 29, 128, 256, 1, 1, 1, 0, True, 0)],
    # three members with a 3x3 first: the kernel allows it, no frame issues it
    [(19, 29, 64, 64, 3, 1, 1, 1, True, None), (19, 29, 64, 130, 1, 1, 1, 2, False, 0), (5, 8, 128, 19, 1, 1, 1, 0, True, None)],
]
FUSION_CONV_GROUPS = 131072                                            # include/tdnet.h TDNET_FUSION_CONV_GROUPS
# Where run_conv_group must run the members one by one -- and still give the same bits: (members, tile, in16, out16, clear the fusion bit)
CONV_GROUP_FALLBACKS = [
    (CONV_GROUPS[0], 3, True, True, True),                             # the fusion bit cleared
    ([(9, 11, 192, 130, 1, 2, 1, 2, True, None), (9, 11, 192, 130, 1, 2, 1, 0, False, 0)], 16, True, True, False),   # an LDS-DMA tile code: CR_CONV_DMA
    (CONV_GROUPS[2], 3, True, False, False),                           # in16 != out16
    ([(19, 29, 64, 64, 1, 1, 1, 1, True, None), (19, 29, 64, 64, 3, 1, 1, 0, True, 0)], 3, True, True, False),       # a 3x3 as second member
    ([(19, 29, 64, 100, 1, 1, 1, 1, True, None), (19, 29, 64, 64, 1, 1, 1, 0, True, 0)], None, True, True, False),   # the heuristic's tiles differ: 64 x 128 beside 128 x 64
]

# ---- 9. the cache sub-sample: k_subsample2 through encode_frame's launch, q_ and v_ in one grid ---------------------------------------------------
# (h, w): one pixel; 4 x 4 -> 1 x 1; 5 x 9 -> 2 x 3, where the last source row and column are read; 8 x 9, 13 x 21, 6 x 7: neither is
SUBSAMPLES = [(1, 1), (4, 4), (5, 9), (8, 9), (13, 21), (6, 7)]
SUBSAMPLE_C1 = 64
SUBSAMPLE_C2S = [128, 512, 2048]                                       # 2048: the Bottleneck backbones' d_v
# More work than one pass of the grid -- hk x wk x (16 + 512) float4s against td_grid_for's cap of 2048 workgroups x 256 lanes = 524288 -- so that the
# grid-stride loop takes a second trip; (h, w, C1, C2).  SECOND_TRIP: one source row, 1 x 4093 -> 1 x 1024, 540672 float4s from 34 MB of source: the
# smallest map that gets there, run under the emulator and on the device.  GRID_STRIDE: 125 x 125 -> 32 x 32, the same 540672 float4s with rows
# and columns both strided, on 128 MB of source (+ 4 MB of q): DEVICE ONLY.  tests/test_emu_ops_edges.py leaves it out because the CPU suite would
# hold that source three times in host memory (the array, its guarded copy, the reference's gather: ~0.4 GB) in every run; the loop bound it is there
# for is the one SECOND_TRIP already exercises under the emulator.
SUBSAMPLE_SECOND_TRIP = (1, 4093, 64, 2048)
SUBSAMPLE_GRID_STRIDE = (125, 125, 64, 2048)

# ---- 10. the 1x1 downsample conv of one row class: run_ds_rows, a batched GEMM with one weight set (GemmArgs.wshare), batch = image row --------
# (H, W, Cin, Cout), tdnet_opts on top of ROW_OPTS; ny = 2 and both row classes
ROW_NY = 2
ROW_CONVS = [((5, 9, 64, 128), {}),
             ((9, 17, 128, 256), {}),                                  # odd H: the classes differ in row count
             ((1, 9, 64, 128), {}),                                    # cy = 1: no rows, no launch, everything untouched
             ((6, 150, 64, 130), {}),                                  # a batch of 150 pixels is wider than one M tile (64 / 128 rows), N ragged
             ((12, 70, 256, 512), {"gemm_persistent": 3}),             # tiles outnumber workgroups: three walk them all
             ((4, 300, 64, 132), {})]                                  # wider than the split GEMM's 256-row tile too, four channels into a second N tile
ROW_OPTS = [{}, {"precision": 3}]                                      # k_gemm_persistent, k_gemm_b3
ROW_STAYS_EXACT = [(6, 150, 64, 130)]                                  # N % 4 != 0: gemm_b3_supports refuses, precision 3 keeps the fp32 GEMM bit for bit



def conv_id(case):
    (H, W, Cin, Cout, KS, stride, dil, act, resid), opts = case[0], case[1]
    extra = "".join("-%s%d" % (k[0], v) for k, v in sorted(opts.items()) if k not in ("precision", "winograd"))
    return "%dx%d-%dto%d-k%ds%dd%d%s%s" % (H, W, Cin, Cout, KS, stride, dil, "-w4" if opts.get("winograd") == 4 else "-w0" if opts.get("winograd") == 0 else "", extra)


def attention_id(a):
    Lq, Lk, DV, online, spike, ramp = a
    return "%dx%dx%d-%d%s%s" % (Lq, Lk, DV, online, "-spike" if spike else "", "-ramp" if ramp else "")


def dma_tiles_for(a):
    """The LDS-DMA tile codes the conv a can run on: all but the 256 x 256 tile where Cout does not pad to a multiple of 256."""
    Cout = a[3]
    return [t for t in DMA_TILES if t != 19 or ((Cout + 127) // 128 * 128) % 256 == 0]


def direct_conv(lib, mem, a, tile):
    opcheck.conv(lib, mem, *a, tile, opts=DIRECT)
    mem.verify()


def wino_conv(lib, mem, a):
    opcheck.conv(lib, mem, *a, tol=2e-4, opts=WINO)
    mem.verify()


def chunked_conv(lib, mem, a):
    opcheck.conv(lib, mem, *a, tol=2e-4, opts=dict(WINO, overlap=CHAINS))
    mem.verify()


def split_conv(lib, mem, a, opts):
    opcheck.conv(lib, mem, *a, opts=opts)
    mem.verify()


def stem(lib, mem, hw, opts):
    opcheck.stem(lib, mem, *hw, opts=opts)
    mem.verify()


def split_gated_conv(lib, mem, a, opts, wino=False, data="normal"):
    """A SPLIT_GEMMS / SPLIT_NARROW entry: the full form inside the guards at the route's tolerance, then the activation-free, residual-free
    form at the fp64-referenced gate.  data != "normal": the gate alone on one of the harder inputs."""
    H, W, Cin, Cout, KS, stride, dil, _, _ = a
    if data == "normal":
        opcheck.conv(lib, mem, *a, tol=2e-4 if wino else 1e-4, opts=opts)
        mem.verify()
    errs = opcheck.split_conv(lib, mem, H, W, Cin, Cout, KS, stride, dil, opts, wino=wino, data=data, stays_exact=a in SPLIT_STAYS_EXACT)
    mem.verify()
    return errs


def split_gated_stem(lib, mem, hw, data="normal"):
    errs = opcheck.split_stem(lib, mem, *hw, data=data)
    mem.verify()
    return errs


def split_gated_attention(lib, mem, a, data="normal"):
    """A SPLIT_ATTENTIONS entry: bias + residual + the LayerNorm strip statistics inside the guards at 1e-4, then softmax(q k^T / 8) v' alone at
    the fp64-referenced gate."""
    Lq, Lk, DV, online, spike, ramp = a
    if data == "normal":
        opcheck.attention(lib, mem, Lq, Lk, DV, online=online, ln=True, spike=spike, ramp=ramp)
        mem.verify()
    errs = opcheck.split_attention(lib, mem, Lq, Lk, DV, online, spike=spike, ramp=ramp, data=data)
    mem.verify()
    return errs


def f16_conv(lib, mem, a, tile):
    opcheck.conv_f16io(lib, mem, *a, tile)
    mem.verify()


def mixed_conv(lib, mem, a, tile):
    """in32 -> out16 (the deep stem's second conv) and in16 -> out32 (the backbone's last conv: fp16 residual, fp32 output, not in place) on a
    register-staged tile, each against fp64 on the rounded operands; then, on a forced tile, the relations the kernel makes exact
    (td_conv_h.h: IN16 / OUT16 change the staging and the epilogue's last step, not the products or their order):
      * out16 == half(out32) for the same input form;
      * in32(x) == in16(half(x)): the staging convert is k_f2h's rounding (the residual is given in fp16 values, which both forms then add)."""
    fwd = lambda in16, out16: opcheck.conv_f16io(lib, mem, *a, tile, want_out=True, in16=in16, out16=out16, resid16=True)[1]
    h = lambda y: y.astype(np.float16).astype(np.float32)
    o32_16, o16_32 = fwd(False, True), fwd(True, False)
    mem.verify()
    if tile is None:                                                   # the heuristic may send the fp16 map to an LDS-DMA form and the fp32 one not
        return
    o16_16, o32_32 = fwd(True, True), fwd(False, False)
    mem.verify()
    assert np.array_equal(o16_16, h(o16_32)), ("out16 != half(out32), fp16 map in", a, tile)
    assert np.array_equal(o32_16, h(o32_32)), ("out16 != half(out32), fp32 map in", a, tile)
    assert np.array_equal(o32_32, o16_32), ("in32(x) != in16(half(x))", a, tile)


def dma_conv_out32(lib, mem, a, tile):
    """in16 -> out32 with a residual on an LDS-DMA form (the head conv reading the fp16 LayerNorm map: the out16 = false epilogue of
    k_conv_dma_h / _h3 / _h3p / _h3n) against fp64 on the rounded operands; on a forced form also out16 == half(out32): every form ends in
    td_store_acc_h, whose OUT16 only rounds what the fp32 form stores."""
    H, W, Cin, Cout, KS, stride, dil, act, _ = a
    _, wide = opcheck.conv_f16io(lib, mem, H, W, Cin, Cout, KS, stride, dil, act, True, tile, want_out=True, in16=True, out16=False)
    mem.verify()
    if tile is not None:
        _, narrow = opcheck.conv_f16io(lib, mem, H, W, Cin, Cout, KS, stride, dil, act, True, tile, want_out=True)
        mem.verify()
        assert np.array_equal(narrow, wide.astype(np.float16).astype(np.float32)), ("out16 != half(out32) on an LDS-DMA form", a, tile)


def mixed_conv_refusals(lib, mem):
    """An LDS-DMA form needs an fp16 input map; the fp16 stem refuses a tile it has no kernel for: errors, and nothing is launched."""
    (H, W, Cin, Cout, KS, stride, dil, act, _), _ = F16_CONVS[0]
    x, w, b = mem.put(np.zeros((H, W, Cin), np.float32)), np.zeros((Cout, Cin, KS, KS), np.float32), np.zeros(Cout, np.float32)
    out = mem.empty((H, W, Cout))
    with pytest.raises(_capi.TdnetError):
        lib.check(lib.tdnet_op_conv2d_f16mix(mem.ptr(x), H, W, Cin, w.ctypes.data, b.ctypes.data, Cout, KS, stride, dil, None, act, 16, 0, 0, mem.ptr(out), mem.stream))
    mem.verify(untouched=True)
    img, w7, out = mem.put(np.zeros((3, 7, 9), np.float32)), np.zeros((64, 3, 7, 7), np.float32), mem.empty((2, 3, 64))
    for tile in (0, 1, 3, 4):
        with pytest.raises(_capi.TdnetError):
            lib.check(lib.tdnet_op_stem_f16(mem.ptr(img), 7, 9, w7.ctypes.data, None, tile, mem.ptr(out), mem.stream))
    mem.verify(untouched=True)
    x, out = mem.put(np.zeros((2, 3, 6), np.float32)), mem.empty((1, 2, 6))
    for C, mode in ((6, 0), (4, 3)):
        with pytest.raises(_capi.TdnetError):
            lib.check(lib.tdnet_op_maxpool(mem.ptr(x), 2, 3, C, mode, mem.ptr(out), mem.stream))
    mem.verify(untouched=True)


def maxpool(lib, mem, hw, C, mode):
    opcheck.maxpool(lib, mem, *hw, C, mode)
    mem.verify()


def stem_f16(lib, mem, hw):
    opcheck.stem_f16(lib, mem, *hw)
    opcheck.stem_f16(lib, mem, *hw, tile=2)                            # the single-stage form of the same 128 x 64 tile
    mem.verify()


def layernorm_f16(lib, mem, a):
    opcheck.layernorm_f16(lib, mem, *a)
    mem.verify()


def ppm(lib, mem, hw, pid):
    opcheck.ppm(lib, mem, *hw, pid)
    mem.verify()


def upsample(lib, mem, a):
    opcheck.upsample(lib, mem, *a)
    mem.verify()


def attention(lib, mem, a, online):
    opcheck.attention(lib, mem, *a, online=online, ln=True)
    mem.verify()


def sliced_attention(lib, mem, a, online):
    Lq, Lk, bias, resid, spike = a
    opcheck.attention(lib, mem, Lq, Lk, 512, bias, resid, spike=spike, online=online | 64)
    mem.verify()


def _classify(lib, mem, x, wt, b):
    HW, C = x.shape
    out = mem.empty((wt.shape[0], HW))
    lib.check(lib.tdnet_op_classifier(mem.ptr(mem.put(x)), HW, C, mem.ptr(mem.put(wt)), mem.ptr(mem.put(b)), wt.shape[0], mem.ptr(out), mem.stream))
    return mem.get(out).copy()


def classifier(lib, mem, a):
    """tdnet_op_classifier against an fp64 matrix product; NC > 32: the first 32 classes bit for bit the 32-class kernel's."""
    NC, C, HW = a
    g = np.random.default_rng(NC * 1000 + C + HW)
    x = g.standard_normal((HW, C)).astype(np.float32)
    wt = (g.standard_normal((NC, C)) / np.sqrt(C)).astype(np.float32)
    b = g.standard_normal(NC).astype(np.float32)
    out = _classify(lib, mem, x, wt, b)
    ref = wt.astype(np.float64) @ x.astype(np.float64).T + b[:, None]
    err = float(np.abs(out - ref).max())
    assert err <= 1e-5 * max(1.0, float(np.abs(ref).max())), ("classifier", a, err)
    if NC > 32:
        assert np.array_equal(out[:32], _classify(lib, mem, x, wt[:32].copy(), b[:32].copy())), ("classifier: class tile 0 != the 32-class kernel", a)
    mem.verify()


def classifier_refusals(lib, mem):
    """What the kernels cannot run is an error before a launch: 257 classes, C not a multiple of 16, weights beyond a CU's LDS."""
    for NC, C in ((257, 64), (19, 24), (32, 1040), (19, 1904), (33, 528)):
        x, wt, b = mem.put(np.zeros((4, C), np.float32)), mem.put(np.zeros((NC, C), np.float32)), mem.put(np.zeros(NC, np.float32))
        out = mem.empty((NC, 4))
        with pytest.raises(_capi.TdnetError):
            lib.check(lib.tdnet_op_classifier(mem.ptr(x), 4, C, mem.ptr(wt), mem.ptr(b), NC, mem.ptr(out), mem.stream))
        mem.verify(untouched=True)
    # the largest the 32-class kernel holds: exactly 160 KiB
    classifier(lib, mem, (32, 1024, 3))


@functools.lru_cache(maxsize=None)
def _head_case(Cout, Cin, H, W):
    """Inputs and the fp64 hidden map BEFORE the activation, shared by every (NC, act) of one head shape."""
    g = np.random.default_rng(Cout * 7 + Cin + H * 131 + W)
    x = g.standard_normal((H, W, Cin)).astype(np.float32)
    w3 = (g.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    b3 = g.standard_normal(Cout).astype(np.float32)
    hid = F.conv2d(torch.from_numpy(x).double().permute(2, 0, 1)[None], torch.from_numpy(w3).double(), torch.from_numpy(b3).double(), 1, 1)
    return x, w3, b3, hid[0].reshape(Cout, H * W).numpy()


def _head_cls(lib, mem, dx, H, W, Cin, w3, b3, Cout, act, cw, cb, NC, opts, fused):
    out = mem.empty((NC, H * W))
    rc = lib.tdnet_op_head_cls(mem.ptr(dx), H, W, Cin, w3.ctypes.data, b3.ctypes.data, Cout, act, cw.ctypes.data, cb.ctypes.data, NC,
                               ctypes.byref(lib.opts(**opts)), fused, mem.ptr(out), mem.stream)
    return rc, out


def head_cls(lib, mem, a, opts=WINO):
    """tdnet_op_head_cls with the conv planned by opts (WINO: the exact-fp32 GEMMs; HEAD_SPLIT: k_gemm_b3, planned with CoutPad =
    gemm_b3_npad(Cout) instead of conv_cout_pad's value): (a) the classifier inside the Winograd output transform gives the bits of conv + classifier kernel,
    (b) which is within the Winograd operator tolerance (2e-4) of an fp64 conv -> act -> 1x1: the classifier's rows are N(0, 1) /
    sqrt(Cout), a normalised projection that does not amplify the hidden map's error."""
    Cout, Cin, (H, W) = a
    x, w3, b3, hid = _head_case(Cout, Cin, H, W)
    g = np.random.default_rng(Cout + Cin + H + W)
    dx = mem.put(x)
    for NC in HEAD_NCS:
        cw = (g.standard_normal((NC, Cout)) / np.sqrt(Cout)).astype(np.float32)
        cb = g.standard_normal(NC).astype(np.float32)
        for act in HEAD_ACTS:
            ref = cw.astype(np.float64) @ (np.maximum(hid, 0.0) if act == 1 else hid) + cb[:, None]
            outs = []
            for fused in (0, 1):
                rc, out = _head_cls(lib, mem, dx, H, W, Cin, w3, b3, Cout, act, cw, cb, NC, opts, fused)
                lib.check(rc)
                outs.append(mem.get(out).copy())
            err = float(np.abs(outs[0] - ref).max())
            assert err <= 2e-4, ("head_cls vs fp64", a, opts, NC, act, err)
            assert np.array_equal(outs[0], outs[1]), ("head_cls: fused != conv + classifier", a, opts, NC, act, float(np.abs(outs[0] - outs[1]).max()))
    mem.verify()


def head_cls_refusals(lib, mem, wino=WINO):
    """fused = 1 where a frame would not fuse is an error and launches nothing: 33 classes, 96 hidden channels, a direct-conv plan.
    wino: the options of the Winograd plans (WINO or HEAD_SPLIT); the direct plan takes their precision."""
    for Cout, NC, opts in ((128, 33, wino), (96, 19, wino), (128, 19, dict(wino, **DIRECT))):
        x, w3, b3, _ = _head_case(Cout, 128, 5, 9)
        cw, cb = np.zeros((NC, Cout), np.float32), np.zeros(NC, np.float32)
        rc, _ = _head_cls(lib, mem, mem.put(x), 5, 9, 128, w3, b3, Cout, 1, cw, cb, NC, opts, 1)
        with pytest.raises(_capi.TdnetError):
            lib.check(rc)
        mem.verify(untouched=True)
        rc, _ = _head_cls(lib, mem, mem.put(x), 5, 9, 128, w3, b3, Cout, 1, cw, cb, NC, opts, 0)   # the two-kernel form runs all three
        lib.check(rc)
        mem.verify()


def layernorm(lib, mem, a):
    opcheck.layernorm(lib, mem, *a)
    mem.verify()


def layernorm_flat(lib, mem, a):
    ratio = opcheck.layernorm_flat(lib, mem, *a)
    mem.verify()
    return ratio


def wide_attention(lib, mem, a, online):
    opcheck.attention(lib, mem, *a, online=online, ln=True)
    mem.verify()


def group_id(members):
    return "+".join("%dx%d-%dto%d-k%ds%dd%d" % m[:7] for m in members)


def row_conv_id(case):
    (H, W, Cin, Cout), opts = case
    return "%dx%d-%dto%d%s" % (H, W, Cin, Cout, "".join("-%s%d" % (k[0], v) for k, v in sorted(opts.items())))


def conv_group(lib, mem, members, tile):
    """A CONV_GROUPS entry on one tile, in both storages: the grouped kernel must run and give every member the single launch's bits."""
    for in16, out16 in GROUP_STORAGES:
        opcheck.conv_group(lib, mem, members, tile, in16=in16, out16=out16, grouped=True)
        mem.verify()


def conv_group_fallback(lib, mem, case):
    members, tile, in16, out16, clear = case
    fusion = lib.opts().fusion & ~FUSION_CONV_GROUPS if clear else None
    opcheck.conv_group(lib, mem, members, tile, in16=in16, out16=out16, fusion=fusion, grouped=False)
    mem.verify()


def cache_subsample(lib, mem, hw, C2, C1=SUBSAMPLE_C1):
    opcheck.cache_subsample(lib, mem, *hw, C1, C2)
    mem.verify()


def row_conv(lib, mem, case, opts, cy):
    """A ROW_CONVS entry under ROW_OPTS' opts on the row class cy (of ROW_NY): opcheck.conv1x1_rows' three checks inside the guards."""
    shape, extra = case
    o = dict(opts, **extra)
    errs = opcheck.conv1x1_rows(lib, mem, *shape, o, ROW_NY, cy, act=1 + cy, stays_exact=shape in ROW_STAYS_EXACT)
    mem.verify()
    return errs


def row_conv_refusals(lib, mem):
    """Where a frame would refuse (the plan is not the persistent-GEMM route) the entry is an error and launches nothing: the GEMM switched off,
    K = 32 (gemm_supports wants K % 64 == 0), the fp16 mode (CR_CONV_H); and a row class outside 0 .. ny - 1."""
    for (Cin, opts, ny, cy) in ((64, {"gemm_persistent": 0}, 2, 0), (32, {}, 2, 0), (64, {"precision": 1}, 2, 1), (64, {}, 2, 2), (64, {}, 0, 0)):
        x, w = mem.put(np.zeros((4, 9, Cin), np.float32)), np.zeros((128, Cin), np.float32)
        out = mem.empty((4, 9, 128))
        with pytest.raises(_capi.TdnetError):
            lib.check(lib.tdnet_op_conv1x1_rows(mem.ptr(x), 4, 9, Cin, w.ctypes.data, None, 128, 0, ctypes.byref(lib.opts(**opts)), ny, cy, mem.ptr(out), mem.stream))
        mem.verify(untouched=True)
