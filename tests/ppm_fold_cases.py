"""The pyramid folded through the Encoding's first 1x1 convs (tdnet_opts.fusion bit 2097152): the cases tests/test_emu_ppm_fold.py proves under the
emulator and tests/test_gpu_ppm_fold.py runs on the device.  `mem` is an opcheck mem (numpy arrays or torch-ROCm tensors standing in for HBM).

1. enc_first: the three first layers on c4 through tdnet_op_enc_first, by the fold route and by the z route, both against an fp64 evaluation from c4.
   The fold is held to the z route's OWN error on the same inputs: max <= 2 x, rms <= 1.25 x, over the values of v_cur, q1 and k1 together -- the bound
   was set for a population of ~10^4 values (the maximum of that many moves by tens of percent between two equivalent summation orders: a numpy
   restatement of both routes read 0.88 .. 1.25 x; the rms read 0.96 .. 1.00 x), and the key map alone has as few as 128.  The per-output ratios are
   printed.  The basis table's rows sum to 4 (one per level) within 1e-6 and its columns 50 .. 63 are zero.
2. src2_null: a kernel's two-source form with nothing behind the split equals its one-source form bit for bit.
3. frames: whole clips with the bit on and off -- each against the reference's goldens at the suite's tolerances, against each other at the 1e-3 /
   tie-band rule, `z` on request bit-identical, as many launches.
4. shared: two handles on one weight block, fold on, different clips: each equals the same clip on a handle of its own bit for bit (G is per handle).
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

import opcheck
from tdnet_amd import arch, weights
from tdnet_amd.engine import Engine

PPM_FOLD = 2097152
# feature h x w at C = 512: 5x9 -- h < 6: degenerate level-6 bins, M = 45 ragged, a 2 x 3 key grid; 9x17; 1x7 -- sy = 0; 33x40 -- more than one 128-row tile
ENC_SHAPES = [(5, 9), (9, 17), (1, 7), (33, 40)]
ENC_WIDE = (5, 9, 2048, 256)          # (h, w, C, DV): ResNet-50 widths, FS = 256, K = 1088
# the GEMM cases of test_emu_kernels.test_persistent_gemm_multi_tile: (H, W, Cin, Cout, act, resid)
NULL_GEMMS = [(23, 31, 128, 160, 1, True), (40, 40, 64, 64, 0, False)]
NULL_GEMM_ODD = (23, 31, 96, 160, 1, True)        # K = 96: an odd step count, not a persistent GEMM -> no two-source form, the entry refuses
NULL_CAPS = (1, 3, 5, 8, 11)
NULL_TILES = (3, 4, 5)
NULL_DIRECT = (20, 23, 64, 64, 4, 2)             # (H, W, Cin, Cout, stride, act): the stride-4 key conv on k_conv_adirect<1, 0>
FRAME_MODELS = [("td4", "resnet18"), ("td2", "resnet18")]
FRAME_HW = (33, 65)
FRAME_T = 6


def _enc_inputs(h, w, C, DV, seed):
    g = np.random.default_rng(seed)
    c4 = np.abs(g.standard_normal((h, w, C))).astype(np.float32)                        # a backbone output: behind a ReLU
    pw = (g.standard_normal((4, C // 4, C)) * 0.05).astype(np.float32)
    pb = g.standard_normal((4, C // 4)).astype(np.float32)
    ws = [(g.standard_normal((n, C)) / np.sqrt(C)).astype(np.float32) for n in (DV, 64, 64)]
    bs = [g.standard_normal(n).astype(np.float32) for n in (DV, 64, 64)]
    return c4, pw, pb, ws, bs


def _enc_ref64(c4, pw, pb, ws, bs, pid):
    """v_cur, q1, k1 in fp64 from c4: td4_psp18.py:271-284 (pyramid slice), transformer.py:18-26 (first layers; BN folded into ws / bs)."""
    h, w, C = c4.shape
    XS, FS = C // 2, C // 8
    x = torch.from_numpy(c4).double().permute(2, 0, 1)[None]
    parts = [x[:, pid * XS:(pid + 1) * XS]]
    for j, o in enumerate((1, 2, 3, 6)):
        p = F.relu(F.conv2d(F.adaptive_avg_pool2d(x, o), torch.from_numpy(pw[j]).double()[:, :, None, None], torch.from_numpy(pb[j]).double()))
        parts.append(F.interpolate(p, (h, w), mode="bilinear", align_corners=True)[:, pid * FS:(pid + 1) * FS])
    z = torch.cat(parts, 1)
    conv = lambda i, zz: F.conv2d(zz, torch.from_numpy(ws[i]).double()[:, :, None, None], torch.from_numpy(bs[i]).double())[0].permute(1, 2, 0).numpy()
    return conv(0, z), np.asarray(F.leaky_relu(torch.from_numpy(conv(1, z)), 0.01)), np.asarray(F.leaky_relu(torch.from_numpy(conv(2, z[:, :, ::4, ::4])), 0.01))


def enc_first(lib, mem, h, w, pid, C=512, DV=512, seed=0):
    c4, pw, pb, ws, bs = _enc_inputs(h, w, C, DV, seed + 7 * pid)
    ref = _enc_ref64(c4, pw, pb, ws, bs, pid)
    hk, wk = arch.key_size(h), arch.key_size(w)
    got = {}
    for fold in (1, 0):
        dc = mem.put(c4)
        outs = [mem.empty((h * w, DV)), mem.empty((h * w, 64)), mem.empty((hk * wk, 64))]
        basis = mem.empty((h * w, 64)) if fold else None
        lib.check(lib.tdnet_op_enc_first(mem.ptr(dc), h, w, C, pid, pw.ctypes.data, pb.ctypes.data, ws[0].ctypes.data, bs[0].ctypes.data, DV,
                                         ws[1].ctypes.data, bs[1].ctypes.data, ws[2].ctypes.data, bs[2].ctypes.data, fold,
                                         mem.ptr(outs[0]), mem.ptr(outs[1]), mem.ptr(outs[2]), mem.ptr(basis), mem.stream))
        got[fold] = [np.array(mem.get(o), np.float64).reshape(r.shape) for o, r in zip(outs, ref)]
        if fold:
            B = np.array(mem.get(basis), np.float64)
            assert np.abs(B[:, :50].sum(1) - 4.0).max() <= 1e-6, ("basis rows", h, w, float(np.abs(B[:, :50].sum(1) - 4.0).max()))
            assert not B[:, 50:].any() and (B >= 0).all() and (np.count_nonzero(B, 1) <= 16).all()
        if hasattr(mem, "verify"):
            mem.verify()
    errs = {f: [np.abs(a - r).ravel() for a, r in zip(got[f], ref)] for f in (0, 1)}
    stat = lambda e: (float(e.max()), float(np.sqrt((e * e).mean())))
    (fm, fr), (zm, zr) = stat(np.concatenate(errs[1])), stat(np.concatenate(errs[0]))
    per = ["%s x%.2f / x%.2f" % (n, stat(a)[0] / stat(b)[0], stat(a)[1] / stat(b)[1]) for n, a, b in zip(("v", "q1", "k1"), errs[1], errs[0])]
    print("enc_first %dx%d C=%d pid %d: z route %.2e / %.2e, fold %.2e / %.2e = x%.2f max, x%.2f rms (%s)" % (h, w, C, pid, zm, zr, fm, fr, fm / zm, fr / zr, "; ".join(per)))
    assert zm > 0 and zr > 0
    assert fm <= 2.0 * zm, ("fold max error", h, w, C, pid, fm, zm)
    assert fr <= 1.25 * zr, ("fold rms error", h, w, C, pid, fr, zr)
    return fm / zm, fr / zr


def _conv1x1_pair(lib, mem, H, W, Cin, Cout, stride, act, resid, tile, opts, seed=0):
    """(one-source result or None if the two-source entry refused, two-source result or None)"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((H, W, Cin)).astype(np.float32)
    wt = (g.standard_normal((Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)
    b = g.standard_normal(Cout).astype(np.float32)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = g.standard_normal((Ho, Wo, Cout)).astype(np.float32) if resid else None
    o = lib.opts(**(opts or {}))
    res = []
    for two in (False, True):
        dx, dr, out = mem.put(x), (mem.put(r) if resid else None), mem.empty((Ho, Wo, Cout))
        if two:
            rc = lib.tdnet_op_conv1x1_src2_null(mem.ptr(dx), H, W, Cin, wt.ctypes.data, b.ctypes.data, Cout, stride, mem.ptr(dr), act, ctypes.byref(o), tile,
                                                mem.ptr(out), mem.stream)
        else:
            rc = lib.tdnet_op_conv2d(mem.ptr(dx), H, W, Cin, wt.ctypes.data, b.ctypes.data, Cout, 1, stride, 1, mem.ptr(dr), act, ctypes.byref(o), tile,
                                     mem.ptr(out), mem.stream)
        if rc < 0:
            assert two and b"no two-source form" in lib.tdnet_last_error(), lib.tdnet_last_error()
            if hasattr(mem, "verify"):
                mem.verify(untouched=True)
            res.append(None)
            continue
        res.append(np.array(mem.get(out)))
        if hasattr(mem, "verify"):
            mem.verify()
    return res


def src2_null_gemms(lib, mem, cap):
    pers = cap if cap > 1 else 2
    for tile in NULL_TILES:
        for H, W, Cin, Cout, act, resid in NULL_GEMMS:
            one, two = _conv1x1_pair(lib, mem, H, W, Cin, Cout, 1, act, resid, tile, {"gemm_persistent": pers})
            assert two is not None and np.array_equal(one.view(np.int32), two.view(np.int32)), ("gemm", cap, tile, H, W, Cin, Cout)
    H, W, Cin, Cout, act, resid = NULL_GEMM_ODD
    assert _conv1x1_pair(lib, mem, H, W, Cin, Cout, 1, act, resid, NULL_TILES[0], {"gemm_persistent": pers})[1] is None


def src2_null_direct(lib, mem):
    H, W, Cin, Cout, stride, act = NULL_DIRECT
    one, two = _conv1x1_pair(lib, mem, H, W, Cin, Cout, stride, act, False, -1, None)
    assert two is not None and np.array_equal(one.view(np.int32), two.view(np.int32))


def _frame(mem, e, x, pos, H, W):
    dx, out = mem.put(x), mem.empty((1, 19, H, W))
    e.forward(mem.ptr(dx), pos, mem.ptr(out), mem.stream)
    return np.array(mem.get(out))


def frames(lib, mem, golden_dir, name, bb):
    H, W = FRAME_HW
    spec = arch.model_spec(name, 19, bb)
    P = spec.path_num
    h, w = arch.feat_size(H), arch.feat_size(W)
    hk, wk = arch.key_size(h), arch.key_size(w)
    g = np.load(os.path.join(golden_dir, "%s_%s_%dx%d.npz" % (name, bb, H, W)))
    sd = weights.synth_state_dict(spec, h, w, 0)
    default = lib.opts().fusion
    assert default & PPM_FOLD
    eng = {}
    for tag, fusion in (("on", default), ("off", default & ~PPM_FOLD)):
        eng[tag] = Engine(P, int(bb[6:]), 19, H, W, 0, lib=lib, opts={"fusion": fusion})
        eng[tag].load_state_dict(sd)
        assert eng[tag].opts()["fusion"] == fusion
    shapes = {"z": (1, spec.d_model, h, w), "v_cur": (1, spec.d_v, h, w), "q_cur": (1, h * w, 64), "cache_k": (1, hk * wk, 64), "cache_q": (1, hk * wk, 64),
              "cache_v": (1, hk * wk, spec.d_v), "ln": (1, spec.d_v, h, w), "lowres": (1, 19, h, w)}
    worst = 0.0
    for t, x in enumerate(weights.synth_video(H, W, FRAME_T, seed=1)):
        out, z = {}, {}
        for tag, e in eng.items():
            out[tag] = _frame(mem, e, x, t % P, H, W)
            for st, shp in shapes.items():                           # the goldens at the suite's tolerances, both configurations: the fallback route stays alive
                key = "f%d_%s" % (t, st)
                if key in g.files:
                    got = e.stage(st, shp)
                    assert np.abs(got - g[key]).max() <= 1e-4 * max(1.0, np.abs(g[key]).max()), (tag, t, st, float(np.abs(got - g[key]).max()))
                    if st == "z":
                        z[tag] = got
            if "f%d_logits" % t in g.files:                          # (the td2 goldens hold five frames)
                ref = g["f%d_logits" % t]
                assert np.abs(out[tag] - ref).max() <= 1e-3, (tag, t)
                assert (out[tag][0].argmax(0) == ref[0].argmax(0)).all(), (tag, t)
        if t < 2:
            assert np.array_equal(z["on"].view(np.int32), z["off"].view(np.int32)), t
        err = float(np.abs(out["on"] - out["off"]).max())
        worst = max(worst, err)
        assert err <= 1e-3, (t, err)
        bad = out["on"][0].argmax(0) != out["off"][0].argmax(0)
        top2 = np.sort(out["off"][0], 0)[-2:]
        assert ((top2[1] - top2[0])[bad] <= 2 * max(err, 1e-6)).all(), ("label flip outside the top-2 tie band", t)
        assert eng["on"].last_launch_count() == eng["off"].last_launch_count() > 20, t      # k_ppm_fold_g in k_ppm_assemble's place
    print("frames %s-%s: worst |logits(on) - logits(off)| %.2e" % (name, bb, worst))
    for e in eng.values():
        e.close()


def shared(lib, mem):
    name, bb = FRAME_MODELS[0]
    H, W = FRAME_HW
    spec = arch.model_spec(name, 19, bb)
    P = spec.path_num
    sd = weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0)
    owner = Engine(P, int(bb[6:]), 19, H, W, 0, lib=lib)
    assert owner.opts()["fusion"] & PPM_FOLD
    owner.load_state_dict(sd)
    second = owner.share()
    alone = {}
    for tag in ("a", "b"):
        alone[tag] = Engine(P, int(bb[6:]), 19, H, W, 0, lib=lib)
        alone[tag].load_state_dict(sd)
    clips = {"a": weights.synth_video(H, W, 5, seed=1), "b": weights.synth_video(H, W, 5, seed=2)}
    for t in range(5):                                               # the two handles interleaved, each on its own clip
        for tag, e in (("a", owner), ("b", second)):
            together = _frame(mem, e, clips[tag][t], t % P, H, W)
            by_itself = _frame(mem, alone[tag], clips[tag][t], t % P, H, W)
            assert np.array_equal(together.view(np.int32), by_itself.view(np.int32)), (tag, t)
    assert not np.array_equal(_frame(mem, owner, clips["a"][0], 0, H, W), _frame(mem, second, clips["b"][0], 0, H, W))   # the clips do differ
    for e in (owner, second, alone["a"], alone["b"]):
        e.close()
