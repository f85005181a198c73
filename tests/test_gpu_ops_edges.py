"""tests/ops_edge_cases.py on the device, every tensor inside guard bands (opcheck.GuardedTorchMem): the same lists
tests/test_emu_ops_edges.py proves under the emulator, where buffer-descriptor bounds, LDS-DMA and the MFMA tiles really execute.

layernorm_flat (kernel error / error of F.layer_norm in fp32 on the CPU, both against fp64; the gate is 4), under the emulator:
    (45, 128, mean 5, std 1e-3)     ratio 0.72
    (1000, 512, mean 50, std 1e-3)  ratio 1.26
    (513, 2048, mean 5, std 3e-3)   ratio 1.12
NOT YET MEASURED ON A DEVICE: this module was written without access to an MI355X.  The first device run has to add its ratios here (the
test prints them) and to report whether the 96 KiB (32 x 512) and 160 KiB (32 x 1024) dynamic-LDS classifier launches were accepted."""
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
