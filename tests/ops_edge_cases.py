"""Operator edge cases shared by tests/test_emu_ops_edges.py (CPU, through the emulator) and tests/test_gpu_ops_edges.py (device memory).

Two things the value tests of test_gpu_ops / test_gpu_winograd / test_gpu_fp16 / test_gpu_b3 cannot see:
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


def head_cls(lib, mem, a):
    """tdnet_op_head_cls: (a) the classifier inside the Winograd output transform gives the bits of conv + classifier kernel, (b) which is
    within the Winograd operator tolerance (2e-4) of an fp64 conv -> act -> 1x1: the classifier's rows are N(0, 1) / sqrt(Cout), a
    normalised projection that does not amplify the hidden map's error."""
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
                rc, out = _head_cls(lib, mem, dx, H, W, Cin, w3, b3, Cout, act, cw, cb, NC, WINO, fused)
                lib.check(rc)
                outs.append(mem.get(out).copy())
            err = float(np.abs(outs[0] - ref).max())
            assert err <= 2e-4, ("head_cls vs fp64", a, NC, act, err)
            assert np.array_equal(outs[0], outs[1]), ("head_cls: fused != conv + classifier", a, NC, act, float(np.abs(outs[0] - outs[1]).max()))
    mem.verify()


def head_cls_refusals(lib, mem):
    """fused = 1 where a frame would not fuse is an error and launches nothing: 33 classes, 96 hidden channels, a direct-conv plan."""
    for Cout, NC, opts in ((128, 33, WINO), (96, 19, WINO), (128, 19, DIRECT)):
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
