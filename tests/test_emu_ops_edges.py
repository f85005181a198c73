"""tests/ops_edge_cases.py through the test-only fiber emulator (tests/emu/), numpy arrays with guard bands standing in for HBM: every case is
proven here before tests/test_gpu_ops_edges.py runs it on the device.  Also the guarded mem itself: it catches a store past an interior
and a band value that reaches a result.  CPU only."""
import ctypes

import numpy as np
import pytest

import emu_util
import opcheck
import ops_edge_cases as cases


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


@pytest.fixture()
def mem():
    return opcheck.GuardedNumpyMem()


def test_guarded_mem_catches_what_it_is_for(lib):
    _second_fill_shows_what_a_maximum_swallows(lib)
    mem = opcheck.GuardedNumpyMem()
    x = mem.put(np.arange(6, dtype=np.float32).reshape(2, 3))
    out = mem.empty((2, 3))
    assert mem.ptr(x) % 256 == 0 and mem.ptr(out) % 256 == 0 and opcheck.GuardedNumpyMem.GUARD % 256 == 0 and opcheck.GuardedNumpyMem.GUARD >= 4096
    out[...] = x                                                       # a correct "kernel"
    mem.verify()
    assert mem._live == []                                             # the mem forgets what it verified
    mem.verify()

    def at(t, i):                                                      # the float at element i relative to the interior of t, bands included
        return np.ctypeslib.as_array((ctypes.c_float * 1).from_address(t.ctypes.data + 4 * i))

    for tensor_of, where in ((mem.empty, 6), (mem.empty, -1), (mem.put, 6), (mem.put, -1)):   # one float past / before an interior, outputs and inputs
        t = tensor_of((2, 3)) if tensor_of == mem.empty else tensor_of(np.ones((2, 3), np.float32))
        t[...] = 1.0
        at(t, where)[0] = 1.0
        with pytest.raises(AssertionError, match="guard band"):
            mem.verify()
    x, out = mem.put(np.ones((2, 3), np.float32)), mem.empty((2, 3))
    out[...] = x
    out[1, 2] = at(x, 6)[0]                                       # the result takes in one value from behind the input
    with pytest.raises(AssertionError, match="non-finite"):
        mem.verify()
    out = mem.empty((2, 3))
    out[0] = 1.0                                                       # half of the output never written
    with pytest.raises(AssertionError, match="never written"):
        mem.verify()
    out = mem.empty((2, 3))
    mem.verify(untouched=True)
    out = mem.empty((2, 3))
    out[0, 0] = 1.0
    with pytest.raises(AssertionError, match="launched nothing"):
        mem.verify(untouched=True)


def _second_fill_shows_what_a_maximum_swallows(lib):
    """What the 2^127 fill is for.  tdnet_op_upsample_argmax is told C classes and handed C - 1 planes, so it reads the last plane from the band
    behind them ((C - 1) h w 4 = 1440 bytes in, inside the 4096-byte band: emulator only, no device test reads out of range on purpose).
    With the NaN band `v > best` is false for every value read there: the labels are exactly those of the C - 1 planes, and the out-of-range
    read goes unseen.  With the 2^127 band the out-of-range plane wins and the labels change."""
    C, h, w, H, W = 19, 4, 5, 25, 33
    x = np.random.default_rng(5).standard_normal((C - 1, h, w)).astype(np.float32)
    assert (C - 1) * h * w * 4 + h * w * 4 <= opcheck.GuardedNumpyMem.GUARD

    def labels(planes, classes, poison):
        mem = opcheck.GuardedNumpyMem()
        l32 = np.full((H, W), -1, np.int32)
        lib.check(lib.tdnet_op_upsample_argmax(mem.ptr(mem.put(planes, poison=poison)), classes, h, w, H, W, l32.ctypes.data, None, None))
        mem.verify()                                                   # the bands themselves are intact: only a poisoned RESULT can tell
        return l32

    nan_bits, big_bits = opcheck.GuardedNumpyMem.POISONS
    honest = labels(x, C - 1, nan_bits)
    assert np.array_equal(labels(x, C - 1, big_bits), honest)          # in range, the fill is never seen
    assert np.array_equal(labels(x, C, nan_bits), honest)              # out of range into NaNs: nothing changes, nothing is detected
    lied = labels(x, C, big_bits)
    assert (lied == C - 1).mean() > 0.4 and not np.array_equal(lied, honest)   # out of range into 2^127: the labels give it away
    mem = opcheck.GuardedNumpyMem()
    band = mem.put(np.zeros(3, np.float32), poison=big_bits)
    assert np.ctypeslib.as_array((ctypes.c_float * 1).from_address(band.ctypes.data + 12))[0] == 2.0 ** 127   # finite: 0 * fill is 0, a zero-weight tap stays discarded
    mem.verify()


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


# cases.SUBSAMPLE_GRID_STRIDE (125 x 125 x 2048, device only) is NOT run here: 128 MB of source, held three times by a CPU run (the array, its guarded
# copy, the reference's gather).  The grid-stride loop's second trip runs here on cases.SUBSAMPLE_SECOND_TRIP, one source row of 34 MB.
@pytest.mark.parametrize("C2", cases.SUBSAMPLE_C2S)
def test_cache_subsample(lib, mem, C2):
    for hw in cases.SUBSAMPLES:
        cases.cache_subsample(lib, mem, hw, C2)


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
