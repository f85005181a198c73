"""The fused Winograd F(4x4,3x3) kernel of ResNet layer1's 64 -> 64 convs (k_wino4_f64, td_wino_f64.h; tdnet_opts.fusion bit 4194304): the cases
tests/test_emu_wino_f64.py proves under the emulator and tests/test_gpu_wino_f64.py runs on the device.

A frame takes the route only from 32768 output pixels on (td_wino_f64.h TD_WINO_F64_MIN_PIXELS); tdnet_op_conv_wino_f64 runs it at any size, so the
maps here are the smallest at which the kernel's index math can go wrong.  A workgroup owns a block of 8 x 4 tiles of 4 x 4 pixels (32 x 16 pixels)."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import opcheck

WINO_F64 = 4194304                                                     # include/tdnet.h TDNET_FUSION_WINO_F64
MIN_PIXELS = 32768                                                     # td_wino_f64.h TD_WINO_F64_MIN_PIXELS
C = 64

# (H, W): what the map exercises
MAPS = [(1, 1),                                                        # one partly filled tile
        (4, 4),                                                        # exactly one tile
        (5, 9),                                                        # ragged tiles both ways
        (16, 32),                                                      # exactly one block
        (17, 33),                                                      # halo and ragged tiles across block borders in both directions
        (37, 53)]                                                      # several blocks
VARIANTS = [(False, 0), (False, 1), (True, 0), (True, 1)]              # (residual, act)
# what the route does not take: (Cin, Cout, KS, stride, dil, act)
REFUSED = [(128, 64, 3, 1, 1, 1), (64, 128, 3, 1, 1, 1), (64, 64, 1, 1, 1, 1), (64, 64, 3, 2, 1, 1), (64, 64, 3, 1, 2, 1), (64, 64, 3, 1, 1, 2)]

TOL = 1e-4                                                             # opcheck.conv's


def _fused(lib, mem, dx, H, W, w, b, dr, act, Cin=C, Cout=C, KS=3, stride=1, dil=1):
    out = mem.empty((H, W, Cout))
    rc = lib.tdnet_op_conv_wino_f64(mem.ptr(dx), H, W, Cin, w.ctypes.data, b.ctypes.data, Cout, KS, stride, dil, mem.ptr(dr), act, mem.ptr(out), mem.stream)
    return rc, out


def conv(lib, mem, H, W, resid, act, seed=0):
    """opcheck.conv's inputs on the fused kernel, inside guard bands, against an fp64 conv: opcheck's tol = 1e-4; the relation the project holds its Winograd
    kernels to (opcheck.SPLIT_WINO_GATE: max <= 1.25 x, rms <= 1.1 x) over the unfused {"winograd": 4} kernels' own error on the same inputs; two calls
    bit-identical; and the unfused route's values exactly (same transforms, same summation order).  Prints and returns the figures."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((H, W, C)).astype(np.float32)
    w = (g.standard_normal((C, C, 3, 3)) * (1.0 / np.sqrt(C * 9))).astype(np.float32)
    b = g.standard_normal(C).astype(np.float32)
    r = g.standard_normal((H, W, C)).astype(np.float32) if resid else None
    ref = F.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None].double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), 1, 1, 1)
    if resid:
        ref = ref + torch.from_numpy(r).permute(2, 0, 1)[None].double()
    if act == 1:
        ref = F.relu(ref)
    ref = ref[0].permute(1, 2, 0).numpy()
    dx, dr = mem.put(x), (mem.put(r) if resid else None)
    rc, o1 = _fused(lib, mem, dx, H, W, w, b, dr, act)
    lib.check(rc)
    rc, o2 = _fused(lib, mem, dx, H, W, w, b, dr, act)
    lib.check(rc)
    unf = mem.empty((H, W, C))
    o = lib.opts(winograd=4, fusion=lib.opts().fusion & ~WINO_F64)     # the unfused route: input transform, 36 GEMMs, output transform
    lib.check(lib.tdnet_op_conv2d(mem.ptr(dx), H, W, C, w.ctypes.data, b.ctypes.data, C, 3, 1, 1, mem.ptr(dr), act, ctypes.byref(o), -1, mem.ptr(unf), mem.stream))
    got1, got2, gotu = np.array(mem.get(o1)), np.array(mem.get(o2)), np.array(mem.get(unf))
    mem.verify()
    fused, unfused = opcheck.max_rms(got1, ref), opcheck.max_rms(gotu, ref)
    what = ("wino_f64", H, W, resid, act)
    print("wino_f64 %dx%d resid=%d act=%d: fused %.2e / %.2e, unfused %.2e / %.2e (x%.2f / x%.2f)" % (
        H, W, resid, act, *fused, *unfused, fused[0] / max(unfused[0], 1e-30), fused[1] / max(unfused[1], 1e-30)))
    assert np.array_equal(got1.view(np.int32), got2.view(np.int32)), (what, "two calls differ")
    assert fused[0] <= TOL, (what, fused)
    (fm, cm), (fr, cr) = opcheck.SPLIT_WINO_GATE["max"], opcheck.SPLIT_WINO_GATE["rms"]
    assert fused[1] <= fr * unfused[1] + cr, (what, "rms", fused, unfused)
    assert fused[0] <= fm * unfused[0] + cm, (what, "max", fused, unfused)
    # more than the gates ask: the kernel sums over Cin in the persistent GEMMs' order (td_wino_f64.h wino_f64_pack) and shares the transforms' arithmetic
    assert np.array_equal(got1, gotu), (what, "not the values of the unfused route", int((got1 != gotu).sum()))
    return fused, unfused


def refused(lib, mem, shape):
    """A conv the route does not take: the entry fails and writes nothing."""
    Cin, Cout, KS, stride, dil, act = shape
    H, W = 8, 8
    g = np.random.default_rng(1)
    dx = mem.put(g.standard_normal((H, W, Cin)).astype(np.float32))
    w = g.standard_normal((Cout, Cin, KS, KS)).astype(np.float32)
    b = np.zeros(Cout, np.float32)
    pad = dil * (KS // 2)
    Ho, Wo = (H + 2 * pad - dil * (KS - 1) - 1) // stride + 1, (W + 2 * pad - dil * (KS - 1) - 1) // stride + 1
    out = mem.empty((Ho, Wo, Cout))
    rc = lib.tdnet_op_conv_wino_f64(mem.ptr(dx), H, W, Cin, w.ctypes.data, b.ctypes.data, Cout, KS, stride, dil, None, act, mem.ptr(out), mem.stream)
    assert rc < 0 and b"fused Winograd" in lib.tdnet_last_error(), (shape, rc, lib.tdnet_last_error())
    mem.verify(untouched=True)


def refused_size(lib, mem):
    """A map one pixel past the kernel's 32-bit byte offsets (2^31 / 256 pixels): the entry fails on the sizes alone, with a message of its own, and touches
    neither buffer (small stand-ins: nothing may be read or written)."""
    H, W = 4096, 2048                                                  # 8388608 pixels
    dx, out = mem.put(np.zeros((4, 4, C), np.float32)), mem.empty((4, 4, C))
    w, b = np.zeros((C, C, 3, 3), np.float32), np.zeros(C, np.float32)
    rc = lib.tdnet_op_conv_wino_f64(mem.ptr(dx), H, W, C, w.ctypes.data, b.ctypes.data, C, 3, 1, 1, None, 1, mem.ptr(out), mem.stream)
    assert rc < 0 and b"32-bit byte offsets" in lib.tdnet_last_error(), (rc, lib.tdnet_last_error())
    mem.verify(untouched=True)


def plan_keeps_small_maps(lib, mem):
    """Below the size rule tdnet_op_conv2d's plan is the direct kernel with the bit set or clear: the same bits."""
    H, W = 32, 64                                                      # 2048 pixels
    g = np.random.default_rng(2)
    x = g.standard_normal((H, W, C)).astype(np.float32)
    w = (g.standard_normal((C, C, 3, 3)) / 24.0).astype(np.float32)
    b = g.standard_normal(C).astype(np.float32)
    dx, outs = mem.put(x), []
    default = lib.opts().fusion
    for fusion in (default | WINO_F64, default & ~WINO_F64):
        out = mem.empty((H, W, C))
        lib.check(lib.tdnet_op_conv2d(mem.ptr(dx), H, W, C, w.ctypes.data, b.ctypes.data, C, 3, 1, 1, None, 1, ctypes.byref(lib.opts(fusion=fusion)), -1,
                                      mem.ptr(out), mem.stream))
        outs.append(np.array(mem.get(out)))
    mem.verify()
    assert np.array_equal(outs[0], outs[1])
