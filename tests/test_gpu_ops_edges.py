"""tests/ops_edge_cases.py on the device, every tensor inside guard bands (opcheck.GuardedTorchMem): the same lists
tests/test_emu_ops_edges.py proves under the emulator, where buffer-descriptor bounds, LDS-DMA and the MFMA tiles really execute.

layernorm_flat (kernel error / error of F.layer_norm in fp32 on the CPU, both against fp64; the gate is 4), under the emulator and on an
MI355X alike:
    (45, 128, mean 5, std 1e-3)     ratio 0.72
    (1000, 512, mean 50, std 1e-3)  ratio 1.26
    (513, 2048, mean 5, std 3e-3)   ratio 1.12
The 96 KiB (32 x 512) and 160 KiB (32 x 1024) dynamic-LDS classifier launches are accepted there.

The split kernels of tdnet_opts.precision = 2 / 3 (opcheck.split_conv / split_stem / split_attention), measured on an MI355X; two runs gave
every digit twice.  Errors against fp64 as max / rms; cpu32: the fp32 torch evaluation on the host's CPU; exact, split: the exact-fp32 and
the split kernel as multiples of cpu32 (gate of the split kernel: x3 max + 1e-7 / x2 rms + 1e-9); on the Winograd route the exact-fp32
Winograd kernel's own error and the split kernel as a multiple of it (gate: x1.25 / x1.1).  p2 / p3: precision, w4 / w0: winograd, g:
gemm_persistent.  The emulator's figures are in tests/ops_edge_cases.py: there the split kernels are below cpu32 almost everywhere.  The
matrix core adds the 16 products of an instruction in its own order, and on the device the split kernels' sums sit where the exact-fp32
kernels' do: x0.89 .. x0.98 of the exact kernel's rms error on the Winograd route, and below it on the 3x3 direct convs, where BOTH
kernels' single accumulator chain over K = 288 .. 864 is up to x2.1 of the CPU's blocked sum.  The largest rms figure is x1.83 (11x9
96->48 on abs data; the exact kernel x2.08).  The largest max figure, x3.22 at (70, 260, 2048), passes on the floor (1.089e-6 <= 3 *
3.384e-7 + 1e-7).  That element is in query row 48, the one row with a peaked softmax (largest p = 0.29, the next row's 0.12): its
outputs and errors are the largest of every evaluation (row rms: split 1.23e-7, exact 1.02e-7, the median row 3.4e-8; the exact kernel's
max, x1.91, is in the same row), the split kernel's largest error in any other row is 3.08e-7, below cpu32's max -- and cpu32's max is
itself 2.5 times what another host's CPU gives (8.51e-7, the emulator table).  rms is the statistic to read.
    conv 5x7 32->128 k1 p3                       cpu32 7.72e-07 / 1.01e-07   exact x1.01 / x0.98   split x1.08 / x1.03
    conv 5x7 32->4 k1 p3                         cpu32 4.01e-07 / 8.70e-08   exact x0.79 / x0.99   split x0.88 / x1.09
    conv 33x9 192->128 k1 p3                     cpu32 1.96e-06 / 2.48e-07   exact x0.91 / x0.99   split x0.92 / x0.88
    conv 7x9 64->128 k1 p3                       cpu32 1.02e-06 / 1.46e-07   exact x1.11 / x1.01   split x1.04 / x0.94
    conv 11x19 64->160 k1 p3                     cpu32 1.54e-06 / 1.44e-07   exact x1.00 / x1.01   split x0.99 / x0.94
    conv 35x37 64->256 k1 p3 g3                  cpu32 1.60e-06 / 1.44e-07   exact x0.89 / x1.00   split x1.37 / x0.94
    conv 1x1 32->32 k3 w4 p3                     exact 3.29e-07 / 1.21e-07   split x1.00 / x1.00 of it
    conv 1x1 64->32 k3 w4 p3                     exact 4.14e-07 / 1.23e-07   split x0.78 / x0.98 of it
    conv 5x9 256->512 k3 d16 w4 p3               exact 2.14e-06 / 2.87e-07   split x0.72 / x0.89 of it
    conv 13x21 128->132 k3 d2 w4 p3              exact 3.38e-05 / 1.80e-06   split x0.87 / x0.91 of it
    conv 9x17 128->256 k3 d8 w4 p3 chains        exact 2.66e-06 / 3.76e-07   split x0.90 / x0.90 of it
    conv 12x14 128->132 k3 w4 p3 g5              exact 3.56e-05 / 2.14e-06   split x0.83 / x0.91 of it
    conv 13x21 64->64 k3 p2                      cpu32 1.95e-06 / 2.38e-07   exact x1.52 / x1.69   split x1.56 / x1.45
    conv 11x9 96->48 k3 s2 d2 p2                 cpu32 1.46e-06 / 2.01e-07   exact x2.32 / x2.07   split x2.03 / x1.79
    conv 9x17 64->40 k1 s2 p2                    cpu32 6.60e-07 / 1.42e-07   exact x1.24 / x1.05   split x1.42 / x0.99
    conv 13x21 64->128 k3 s2 p2 w0               cpu32 1.41e-06 / 2.22e-07   exact x2.08 / x1.70   split x2.09 / x1.50
    conv 9x17 64->100 k1 s2 p2                   cpu32 9.69e-07 / 1.42e-07   exact x0.98 / x1.02   split x0.97 / x0.96
    conv 12x17 32->48 k3 s2 p2                   cpu32 1.45e-06 / 2.08e-07   exact x1.45 / x1.39   split x1.13 / x1.15
    conv 96x96 64->64 k1 p2                      cpu32 1.58e-06 / 1.48e-07   exact x1.13 / x1.00   split x0.95 / x0.93
    stem 7x9                                     cpu32 9.96e-07 / 2.03e-07   exact x0.73 / x0.93   split x0.93 / x0.97
    stem 7x9 abs                                 cpu32 8.83e-07 / 1.67e-07   exact x1.00 / x1.03   split x0.88 / x1.14
    stem 7x9 scaled                              cpu32 9.96e-07 / 2.03e-07   exact x0.73 / x0.93   split x0.93 / x0.97
    stem 33x65                                   cpu32 2.19e-06 / 3.31e-07   exact x0.89 / x1.01   split x1.14 / x0.96
    stem 33x65 abs                               cpu32 2.40e-06 / 2.90e-07   exact x1.00 / x1.00   split x0.73 / x0.92
    stem 33x65 scaled                            cpu32 2.19e-06 / 3.31e-07   exact x0.89 / x1.01   split x1.14 / x0.96
    conv 11x19 64->160 k1 p3 abs                 cpu32 1.32e-06 / 1.46e-07   exact x0.97 / x1.00   split x0.93 / x0.91
    conv 13x21 128->132 k3 d2 w4 p3 abs          exact 2.20e-05 / 1.07e-06   split x0.77 / x0.92 of it
    conv 11x9 96->48 k3 s2 d2 p2 abs             cpu32 1.20e-06 / 2.10e-07   exact x2.29 / x2.08   split x1.84 / x1.83
    conv 9x17 64->100 k1 s2 p2 abs               cpu32 1.16e-06 / 1.55e-07   exact x1.03 / x1.02   split x0.92 / x0.91
    conv 11x19 64->160 k1 p3 scaled              cpu32 1.54e-06 / 1.44e-07   exact x1.00 / x1.01   split x0.99 / x0.94
    conv 13x21 128->132 k3 d2 w4 p3 scaled       exact 3.38e-05 / 1.80e-06   split x0.87 / x0.91 of it
    conv 11x9 96->48 k3 s2 d2 p2 scaled          cpu32 1.46e-06 / 2.01e-07   exact x2.32 / x2.07   split x2.03 / x1.79
    conv 9x17 64->100 k1 s2 p2 scaled            cpu32 9.69e-07 / 1.42e-07   exact x0.98 / x1.02   split x0.97 / x0.96
    attention (45, 6, 512) online 17/18/19       cpu32 3.33e-07 / 5.21e-08   exact x1.92 / x1.38   split x2.03 / x1.42
    attention (33, 1, 128) online 17             every error 0
    attention (65, 129, 512) online 17/18/19     cpu32 3.51e-07 / 4.76e-08   exact x1.58 / x0.94   split x1.35 / x0.92
    attention (70, 260, 2048) online 17/18/19    cpu32 3.38e-07 / 3.51e-08   exact x1.91 / x1.22   split x3.22 / x1.11
    attention (33, 1, 2048) online 17/18/19      every error 0
    attention (64, 128, 512) online 18           cpu32 3.36e-07 / 4.84e-08   exact x0.92 / x0.92   split x1.13 / x0.87
    attention (97, 130, 512) online 18           cpu32 5.03e-07 / 4.72e-08   exact x0.84 / x0.95   split x1.51 / x0.95
    attention (130, 193, 128) online 17          cpu32 4.44e-07 / 4.09e-08   exact x1.34 / x1.18   split x1.18 / x0.99
    attention (153, 200, 128) online 17 spike    cpu32 2.38e-06 / 1.36e-07   exact x0.94 / x1.05   split x0.73 / x0.82
    attention (70, 300, 128) online 17 ramp      cpu32 7.92e-06 / 1.60e-06   exact x1.03 / x1.03   split x1.17 / x0.99
    attention (153, 200, 512) online 19 spike    cpu32 2.31e-06 / 1.29e-07   exact x1.06 / x1.01   split x0.78 / x0.76
    attention (70, 300, 512) online 19 ramp      cpu32 9.43e-06 / 1.65e-06   exact x0.99 / x1.03   split x1.11 / x0.99
    attention (153, 200, 512) online 18 spike    cpu32 2.31e-06 / 1.29e-07   exact x1.06 / x1.01   split x0.78 / x0.76
    attention (70, 300, 512) online 18 ramp      cpu32 9.43e-06 / 1.65e-06   exact x0.99 / x1.03   split x1.11 / x0.99
    attention (65, 129, 128) online 17 abs       cpu32 6.56e-07 / 1.48e-07   exact x1.08 / x1.03   split x0.87 / x0.97
    attention (65, 129, 512) online 19/18 abs    cpu32 6.62e-07 / 1.47e-07   exact x1.00 / x1.01   split x1.03 / x0.98
    attention (65, 129, 128) online 17 scaled    cpu32 1.50e-05 / 1.20e-06   exact x0.84 / x0.86   split x1.31 / x0.93
    attention (65, 129, 512) online 19/18 scaled cpu32 1.49e-05 / 1.18e-06   exact x0.97 / x0.87   split x1.05 / x0.86

The row-class downsample conv on the split GEMM (opcheck.conv1x1_rows, k_gemm_b3 through run_ds_rows with precision 3), on an MI355X: the written rows
alone, max / rms against fp64 as multiples of cpu32 (the same gate, x3 max + 1e-7 / x2 rms + 1e-9), rows 0 mod 2 | rows 1 mod 2:
    5x9 64->128          x0.71 / x0.92 | x0.88 / x0.90        9x17 128->256        x0.80 / x0.89 | x0.89 / x0.90
    1x9 64->128          x0.71 / x0.89 | no rows              12x70 256->512 g3    x1.09 / x0.87 | x0.81 / x0.87
    4x300 64->132        x0.65 / x0.93 | x0.85 / x0.93        6x150 64->130        x1.00 / x1.00 (N % 4 != 0: the fp32 GEMM, bit for bit)
The written rows equal the whole-map conv's bit for bit on both GEMM kernels, the 36 grouped conv cases equal their single launches bit for bit,
and the 125 x 125 x 2048 cache sub-sample (a second trip of the grid-stride loop) equals [::4, ::4].
"""
import pytest
import torch

import opcheck
import ops_edge_cases as cases
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()                      # the in-tree libtdnet_hip_test.so; raises if it is missing


@pytest.fixture()
def mem():
    return opcheck.GuardedTorchMem()


@pytest.mark.parametrize("tile", cases.DIRECT_TILES)
def test_direct_convs(lib, mem, tile):
    for a in cases.DIRECT_CONVS:
        cases.direct_conv(lib, mem, a, tile)


def test_winograd_convs(lib, mem):
    for a in cases.WINO_CONVS:
        cases.wino_conv(lib, mem, a)
    for a in cases.CHUNKED_CONVS:
        cases.chunked_conv(lib, mem, a)


def test_split_precision_convs_and_stems(lib, mem):
    for a, opts in cases.SPLIT_CONVS:
        cases.split_conv(lib, mem, a, opts)
    for hw in cases.STEMS:
        for opts in cases.STEM_OPTS:
            cases.stem(lib, mem, hw, opts)


def test_fp16_storage_convs(lib, mem):
    for a, tiles in cases.F16_CONVS:
        for tile in tiles:
            cases.f16_conv(lib, mem, a, tile)


@pytest.mark.parametrize("tile", cases.MIXED_TILES)
def test_fp16_mixed_storage_convs(lib, mem, tile):
    for a, _ in cases.F16_CONVS:
        cases.mixed_conv(lib, mem, a, tile)


def test_fp16_lds_dma_convs_writing_fp32(lib, mem):
    for a, _ in cases.F16_CONVS:
        for tile in cases.dma_tiles_for(a):
            cases.dma_conv_out32(lib, mem, a, tile)


def test_fp16_entry_refusals(lib, mem):
    cases.mixed_conv_refusals(lib, mem)


@pytest.mark.parametrize("mode", cases.MAXPOOL_MODES)
def test_maxpool(lib, mem, mode):
    for hw in cases.MAXPOOLS:
        for C in cases.MAXPOOL_CS:
            cases.maxpool(lib, mem, hw, C, mode)


def test_fp16_stem_writing_the_fp16_map(lib, mem):
    for hw in cases.STEMS_F16:
        cases.stem_f16(lib, mem, hw)


def test_ppm_upsample(lib, mem):
    for hw in cases.PPMS:
        for pid in (0, 1):
            cases.ppm(lib, mem, hw, pid)
    for a in cases.UPSAMPLES:
        cases.upsample(lib, mem, a)


@pytest.mark.parametrize("online", cases.SCHEDULES)
def test_attention(lib, mem, online):
    for a in cases.ATTENTIONS:
        cases.attention(lib, mem, a, online)
    for a in cases.SLICED_ATTENTIONS:
        cases.sliced_attention(lib, mem, a, online)
    for a in cases.WIDE_ATTENTIONS:
        cases.wide_attention(lib, mem, a, online)


def test_attention_fp16(lib, mem):
    for a in cases.ATTENTIONS:
        cases.attention(lib, mem, a, cases.ATTENTION_F16)


@pytest.mark.parametrize("a", cases.CLASSIFIERS)
def test_classifier(lib, mem, a):
    cases.classifier(lib, mem, a)


def test_classifier_refusals(lib, mem):
    cases.classifier_refusals(lib, mem)


@pytest.mark.parametrize("a", cases.HEADS)
def test_head_cls(lib, mem, a):
    cases.head_cls(lib, mem, a)


def test_head_cls_refusals(lib, mem):
    cases.head_cls_refusals(lib, mem)


def test_layernorm(lib, mem):
    for a in cases.LAYERNORMS:
        cases.layernorm(lib, mem, a)


def test_layernorm_fp16_map(lib, mem):
    for a in cases.LAYERNORMS:
        cases.layernorm_f16(lib, mem, a)


@pytest.mark.parametrize("a", cases.LAYERNORMS_FLAT)
def test_layernorm_flat(lib, mem, a):
    cases.layernorm_flat(lib, mem, a)


# ---- the split kernels of tdnet_opts.precision = 2 / 3: the full form inside the guards, then the products alone at the fp64-referenced gate ----
@pytest.mark.parametrize("case", cases.SPLIT_GEMMS, ids=cases.conv_id)
def test_split_gemm_gate(lib, mem, case):
    cases.split_gated_conv(lib, mem, *case)


@pytest.mark.parametrize("case", cases.SPLIT_NARROW, ids=cases.conv_id)
def test_split_narrow_conv_gate(lib, mem, case):
    cases.split_gated_conv(lib, mem, *case)


@pytest.mark.parametrize("hw", cases.STEMS)
def test_split_stem_gate(lib, mem, hw):
    for data in opcheck.SPLIT_DATA:
        cases.split_gated_stem(lib, mem, hw, data)


@pytest.mark.parametrize("data", opcheck.SPLIT_DATA[1:])
def test_split_convs_on_harder_inputs(lib, mem, data):
    for i in cases.SPLIT_GEMMS_HARD:
        cases.split_gated_conv(lib, mem, *cases.SPLIT_GEMMS[i], data=data)
    for i in cases.SPLIT_NARROW_HARD:
        cases.split_gated_conv(lib, mem, *cases.SPLIT_NARROW[i], data=data)


@pytest.mark.parametrize("a", cases.SPLIT_ATTENTIONS, ids=cases.attention_id)
def test_split_attention_gate(lib, mem, a):
    cases.split_gated_attention(lib, mem, a)


@pytest.mark.parametrize("data", opcheck.SPLIT_DATA[1:])
def test_split_attention_on_harder_inputs(lib, mem, data):
    for a in cases.SPLIT_ATTENTIONS_HARD:
        cases.split_gated_attention(lib, mem, a + (False, False), data=data)


@pytest.mark.parametrize("a", cases.HEADS)
def test_head_cls_on_the_split_gemm(lib, mem, a):
    cases.head_cls(lib, mem, a, cases.HEAD_SPLIT)


def test_head_cls_refusals_on_the_split_gemm(lib, mem):
    cases.head_cls_refusals(lib, mem, cases.HEAD_SPLIT)


# ---- the launch forms only whole frames reached: grouped fp16 convs, the cache sub-sample, the downsample conv of one row class ----
@pytest.mark.parametrize("tile", cases.GROUP_TILES)
@pytest.mark.parametrize("members", cases.CONV_GROUPS, ids=cases.group_id)
def test_conv_groups(lib, mem, members, tile):
    cases.conv_group(lib, mem, members, tile)


@pytest.mark.parametrize("case", cases.CONV_GROUP_FALLBACKS, ids=["bit-cleared", "lds-dma-tile", "in16-out32", "3x3-second", "tiles-differ"])
def test_conv_group_fallbacks(lib, mem, case):
    cases.conv_group_fallback(lib, mem, case)


@pytest.mark.parametrize("C2", cases.SUBSAMPLE_C2S)
def test_cache_subsample(lib, mem, C2):
    for hw in cases.SUBSAMPLES:
        cases.cache_subsample(lib, mem, hw, C2)


def test_cache_subsample_beyond_one_pass_of_the_grid(lib, mem):
    h, w, C1, C2 = cases.SUBSAMPLE_GRID_STRIDE
    assert ((h - 1) // 4 + 1) * ((w - 1) // 4 + 1) * (C1 + C2) // 4 > 2048 * 256     # td_grid_for's cap: the loop takes a second trip
    cases.cache_subsample(lib, mem, (h, w), C2, C1)


def test_cache_subsample_second_trip_of_the_grid(lib, mem):
    h, w, C1, C2 = cases.SUBSAMPLE_SECOND_TRIP
    assert ((h - 1) // 4 + 1) * ((w - 1) // 4 + 1) * (C1 + C2) // 4 > 2048 * 256     # td_grid_for's cap
    cases.cache_subsample(lib, mem, (h, w), C2, C1)


@pytest.mark.parametrize("cy", [0, 1])
@pytest.mark.parametrize("opts", cases.ROW_OPTS, ids=["fp32", "split"])
@pytest.mark.parametrize("case", cases.ROW_CONVS, ids=cases.row_conv_id)
def test_row_class_downsample(lib, mem, case, opts, cy):
    cases.row_conv(lib, mem, case, opts, cy)


def test_row_class_downsample_refusals(lib, mem):
    cases.row_conv_refusals(lib, mem)
