"""Non-finite values through the kernels that start and end a frame, shared by tests/test_emu_nonfinite.py (CPU, through the emulator) and
tests/test_gpu_nonfinite.py (device memory).  The sources make claims about them -- td_conv.h: td_activate "behaves like the reference's
modules"; td_wino.h: td_w_relu gives "the same bits in every case" through an instruction the host compiler does not have -- which only a
run on the device's own instruction selection can hold.

1. Max-pool: tdnet_op_maxpool in its three storage forms is F.max_pool2d BIT FOR BIT on maps that hold a NaN, a +inf, a channel of -inf
   and a channel of -3.3e38 (below the -3.0e38 the kernels once padded with): a NaN in a window is a NaN, an all -inf window stays -inf,
   nothing is clipped.
2. Conv epilogues: one NaN (or one +inf) input element and a -inf bias through every route of tdnet_op_conv2d, against F.conv2d + F.relu /
   F.leaky_relu.  Direct routes: the reference's NaN mask and its infinities with their signs, everything else finite at the route's
   tolerance.  Winograd routes: reference-non-finite <= kernel-non-finite <= the 6x6 input tiles the element touches (a transform spreads it
   over the tile's outputs).  precision 2 / 3: non-finite exactly where the reference is; the kind is not compared (an infinity split into
   bf16 parts is inf - inf).
   The split kernels carry an infinite activation in the LOW part of the A operand alone (td_gemm_b3.h td_split3a_pair), which the six products
   pair with the weight's high part only: inf x w keeps w's sign and ReLU(-inf) is 0 as in the reference.  (Split as any value, h = inf leaves
   inf - inf in the other parts, and 572 of the 1152 affected outputs of the 3x3 64 -> 128 conv were NaN where the reference has 0.)
3. Labels.  +/-inf logits compare like any value: every label entry equals torch.max(0)[1] of out_ref.up_ref.  NaN logits: the reference
   names the first NaN, the kernels do not -- class 0 starts the running maximum and a NaN never replaces it (td_out.h td_first_max) -- and
   that rule is pinned here as it is, against out_ref.first_max_rule on up_ref's values, for the int32, uint8, score, confidence and matte
   entries.  The logits of these cases are small integers on a geometry with the scale 1 / 8: every interpolated value is exact in fp32,
   so the kernels' values ARE up_ref's and nothing is left to a tolerance."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import opcheck
import out_ref

# ---- 1. max-pool ----------------------------------------------------------------------------------------------------------------------
MAXPOOL_SHAPES = [(6, 8), (7, 9)]
MAXPOOL_MODES = [0, 1, 2]
MAXPOOL_C = 64


def maxpool_input(H, W):
    g = np.random.default_rng(100 * H + W)
    x = g.standard_normal((H, W, MAXPOOL_C)).astype(np.float32)
    x[2, 3, 5] = np.nan
    x[4, 1, 9] = np.inf
    x[:, :, 17] = -np.inf
    x[:, :, 30] = np.float32(-3.3e38)
    return x


def maxpool(lib, mem, hw, mode):
    H, W = hw
    x = maxpool_input(H, W)
    ref = F.max_pool2d(torch.from_numpy(x).permute(2, 0, 1)[None], 3, 2, 1)[0].permute(1, 2, 0).numpy()
    assert np.isnan(ref[..., 5]).sum() >= 1 and np.isposinf(ref[..., 9]).any() and np.isneginf(ref[..., 17]).all() and (ref[..., 30] == np.float32(-3.3e38)).all()
    if mode:
        with np.errstate(over="ignore"):
            ref = ref.astype(np.float16).astype(np.float32)             # -3.3e38 is -inf as fp16
    dx, out = mem.put(x), mem.empty(ref.shape)
    lib.check(lib.tdnet_op_maxpool(mem.ptr(dx), H, W, MAXPOOL_C, mode, mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    bad = got.view(np.int32) != ref.view(np.int32)
    assert not bad.any(), ("maxpool", hw, mode, int(bad.sum()), [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]], got[bad][:4], ref[bad][:4])
    mem.verify(finite=False)


# ---- 2. conv epilogues ----------------------------------------------------------------------------------------------------------------
CONV_H, CONV_W, CONV_CIN = 6, 10, 64
SPOT = (2, 3, 5)                                                       # the non-finite input element
BIAS_CH = 7                                                            # bias[7] = -inf
ACTS = (0, 1, 2)
INPUT_KINDS = ("nan", "inf")
DIRECT, WINO, CHAINS = {"winograd": 0}, {"winograd": 4}, 41 | 4
# (name, KS, Cout, tdnet_opts, tile, Winograd route)
_BASE = ([("direct-t%s" % ("h" if t < 0 else t), 3, 128, DIRECT, t, False) for t in (0, 1, 2, 3, 4, 5, -1)] +
         [("direct-cout48", 3, 48, DIRECT, -1, False),                 # Cout < 64: the direct A operand
          ("gemm-1x1", 1, 128, {}, -1, False),                         # the persistent GEMM
          ("wino", 3, 128, WINO, -1, True), ("wino-overlap2", 3, 128, dict(WINO, overlap=2), -1, True), ("wino-chains", 3, 128, dict(WINO, overlap=CHAINS), -1, True)])
CONV_ROUTES = (_BASE + [(n + "-p%d" % p, ks, co, dict(o, precision=p), t, wino) for p in (2, 3) for (n, ks, co, o, t, wino) in _BASE if t < 0])


def route_id(r):
    return r[0]


def conv_case(kind, KS, Cout):
    g = np.random.default_rng(3 + KS + Cout)
    x = g.standard_normal((CONV_H, CONV_W, CONV_CIN)).astype(np.float32)
    x[SPOT] = np.nan if kind == "nan" else np.inf
    w = (g.standard_normal((Cout, CONV_CIN, KS, KS)) / np.sqrt(CONV_CIN * KS * KS)).astype(np.float32)
    b = g.standard_normal(Cout).astype(np.float32)
    b[BIAS_CH] = -np.inf
    return x, w, b


def act_ref(t, act):
    return F.relu(t) if act == 1 else F.leaky_relu(t, 0.01) if act == 2 else t


def same_non_finite(got, ref, who):
    """the reference's NaN mask and its infinities with their signs"""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), who + ("NaN mask", int((np.isnan(got) != np.isnan(ref)).sum()))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), who + ("infinities",)


def judge(got, ref, reach, rule, tol, who):
    """got against ref, both [H, W, channels]; reach: bool [H, W], the pixels a Winograd tile may spread the element to.
    direct: the reference's NaN mask and infinities; wino: reference-non-finite <= non-finite <= reach, and the reference's outside reach;
    split: the reference's non-finite mask, kinds not compared.  Everything finite in both within tol."""
    bad_ref, bad_got = ~np.isfinite(ref), ~np.isfinite(got)
    if rule == "wino":
        assert not (bad_ref & ~bad_got).any(), who + ("a non-finite value of the reference is finite here", int((bad_ref & ~bad_got).sum()))
        extra = bad_got & ~bad_ref
        assert not extra[~reach].any(), who + ("non-finite outside the touched tiles", int(extra[~reach].sum()))
        same_non_finite(got[~reach], ref[~reach], who)
    elif rule == "split":
        assert np.array_equal(bad_got, bad_ref), who + ("non-finite mask", int((bad_got != bad_ref).sum()), int(bad_got.sum()), int(bad_ref.sum()))
    else:
        assert rule == "direct", rule
        same_non_finite(got, ref, who)
    ok = ~bad_ref & ~bad_got
    err = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    assert err <= tol, who + (err,)


def spot_reach(H, W, y, x, r=5):
    reach = np.zeros((H, W), bool)
    reach[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return reach


def conv(lib, mem, route, kind):
    name, KS, Cout, opts, tile, wino = route
    split = opts.get("precision", 0) >= 2
    x, w, b = conv_case(kind, KS, Cout)
    dx = mem.put(x)
    pre = F.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w), torch.from_numpy(b), 1, KS // 2)
    pre_hwc = pre[0].permute(1, 2, 0).numpy()                          # the case is what it says: the element reaches every channel, the bias a whole plane
    assert not np.isfinite(pre_hwc[SPOT[0], SPOT[1]]).any() and not np.isfinite(pre_hwc[..., BIAS_CH]).any(), (name, kind)
    reach = spot_reach(CONV_H, CONV_W, SPOT[0], SPOT[1])               # the outputs of the 6x6 input tiles that hold the element
    for act in ACTS:
        who = (name, kind, act)
        ref = act_ref(pre, act)[0].permute(1, 2, 0).numpy()
        out = mem.empty(ref.shape)
        lib.check(lib.tdnet_op_conv2d(mem.ptr(dx), CONV_H, CONV_W, CONV_CIN, w.ctypes.data, b.ctypes.data, Cout, KS, 1, 1, None, act,
                                      ctypes.byref(lib.opts(**opts)), tile, mem.ptr(out), mem.stream))
        got = np.array(mem.get(out))
        judge(got, ref, reach, "wino" if wino else "split" if split else "direct", 2e-4 if wino else 1e-4, who)
        if act == 1:                                                   # ReLU(-inf) == 0, exactly
            col = got[..., BIAS_CH][~reach] if wino else got[..., BIAS_CH][np.isfinite(ref[..., BIAS_CH])]
            assert col.size and (col == 0).all(), who
    mem.verify(finite=False)


def wino_f64(lib, mem, kind):
    """tdnet_op_conv_wino_f64 (64 -> 64, act 0 / 1): the fused Winograd kernel's own transforms and epilogue, at the Winograd rule."""
    x, w, b = conv_case(kind, 3, 64)
    dx = mem.put(x)
    pre = F.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w), torch.from_numpy(b), 1, 1)
    reach = spot_reach(CONV_H, CONV_W, SPOT[0], SPOT[1])
    for act in (0, 1):
        who = ("wino_f64", kind, act)
        ref = act_ref(pre, act)[0].permute(1, 2, 0).numpy()
        out = mem.empty(ref.shape)
        lib.check(lib.tdnet_op_conv_wino_f64(mem.ptr(dx), CONV_H, CONV_W, 64, w.ctypes.data, b.ctypes.data, 64, 3, 1, 1, None, act, mem.ptr(out), mem.stream))
        got = np.array(mem.get(out))
        judge(got, ref, reach, "wino", 2e-4, who)
        if act == 1:
            assert (got[..., BIAS_CH][~reach] == 0).all(), who
    mem.verify(finite=False)


HEAD_NC = 19
HEAD_OPTS = [WINO, dict(WINO, precision=2), dict(WINO, precision=3)]


def head_cls(lib, mem, kind, opts):
    """tdnet_op_head_cls, the classifier inside the Winograd output transform (fused) and behind the conv (unfused): 64 -> 128 -> 19 classes.
    Hidden channel 7 is -inf everywhere (act 0: every logit is cw[c, 7] * -inf, an infinity with the sign the reference gives it; act 1:
    ReLU makes it 0 and the logits are finite outside the touched tiles).  A logit mixes every hidden channel, so the Winograd rule holds per
    pixel: reference-non-finite <= non-finite <= the touched tiles; the reference's NaNs and infinities outside them."""
    x, w, b = conv_case(kind, 3, 128)
    g = np.random.default_rng(11)
    cw = (g.standard_normal((HEAD_NC, 128)) / np.sqrt(128)).astype(np.float32)
    cb = g.standard_normal(HEAD_NC).astype(np.float32)
    dx = mem.put(x)
    pre = F.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w), torch.from_numpy(b), 1, 1)
    reach = spot_reach(CONV_H, CONV_W, SPOT[0], SPOT[1])
    for act in (0, 1):
        ref = F.conv2d(act_ref(pre, act), torch.from_numpy(cw)[:, :, None, None], torch.from_numpy(cb))[0].permute(1, 2, 0).numpy()
        assert np.isinf(ref[~reach]).all() if act == 0 else np.isfinite(ref[~reach]).all(), (kind, act)
        outs = []
        for fused in (0, 1):
            out = mem.empty((HEAD_NC, CONV_H * CONV_W))
            lib.check(lib.tdnet_op_head_cls(mem.ptr(dx), CONV_H, CONV_W, CONV_CIN, w.ctypes.data, b.ctypes.data, 128, act, cw.ctypes.data, cb.ctypes.data, HEAD_NC,
                                            ctypes.byref(lib.opts(**opts)), fused, mem.ptr(out), mem.stream))
            got = np.array(mem.get(out)).reshape(HEAD_NC, CONV_H, CONV_W).transpose(1, 2, 0)
            judge(got, ref, reach, "wino", 2e-4, ("head_cls", kind, tuple(sorted(opts.items())), act, fused))
            outs.append(got)
        assert np.array_equal(outs[0], outs[1], equal_nan=True), ("head_cls: fused != conv + classifier", kind, opts, act)
    mem.verify(finite=False)


STEM_HW = (13, 21)                                                     # conv 7 x 11, pool 4 x 6
# (channel, y, x) of the image, a column of either parity: the stride-2 conv reads a pixel beside its window under zero weights (the packed-row
# image of td_conv_ad.h), and only one parity of x ever sits there
STEM_SPOTS = ((1, 6, 9), (1, 6, 8))
STEM_OPTS = [{}, {"precision": 2}, {"precision": 3}]


def stem(lib, mem, kind, opts):
    for spot in STEM_SPOTS:
        _stem(lib, mem, kind, opts, spot)


def _stem(lib, mem, kind, opts, spot):
    """tdnet_op_stem: conv 7x7 -> ReLU -> max-pool, bias[7] = -inf (ReLU: a plane of zeros).  A direct route, so the reference's NaN mask and
    infinities with their signs (precision 2 / 3: its non-finite mask) -- which needs the max-pool to hand a NaN on as F.max_pool2d does."""
    H, W = STEM_HW
    g = np.random.default_rng(17)
    img = g.standard_normal((3, H, W)).astype(np.float32)
    img[spot] = np.nan if kind == "nan" else np.inf
    w = (g.standard_normal((64, 3, 7, 7)) * 0.1).astype(np.float32)
    b = g.standard_normal(64).astype(np.float32)
    b[BIAS_CH] = -np.inf
    ref = F.max_pool2d(F.relu(F.conv2d(torch.from_numpy(img)[None], torch.from_numpy(w), torch.from_numpy(b), 2, 3)), 3, 2, 1)[0].permute(1, 2, 0).numpy()
    plane = ref[..., BIAS_CH]
    assert (~np.isfinite(ref)).any() and (plane[np.isfinite(plane)] == 0).all() and np.isfinite(plane).any(), kind
    di, out = mem.put(img), mem.empty(ref.shape)
    lib.check(lib.tdnet_op_stem(mem.ptr(di), H, W, w.ctypes.data, b.ctypes.data, ctypes.byref(lib.opts(**opts)), mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    who = ("stem", kind, tuple(sorted(opts.items())), spot)
    judge(got, ref, None, "split" if opts.get("precision", 0) >= 2 else "direct", 1e-4, who)
    assert (got[..., BIAS_CH][np.isfinite(plane)] == 0).all(), who
    mem.verify(finite=False)


# ---- 2b. fp16 storage: results beyond the largest fp16 value -------------------------------------------------------------------------------
# 65504 is the largest fp16 value, 65520 the boundary above which rounding to nearest gives inf.  The kernels' fp32 sums are within
# opcheck.t16 (3e-5 relative) of the fp64 reference, so a reference value further than 1 % from 65520 rounds to the same side in both.
F16_MAX, F16_EDGE = 65504.0, 65520.0
F16_TILES = [3, 4, 5, 16, 17, 18, 19, 31, 32, 34, 35, -1]
F16_SHAPE = (6, 10, 128, 256)                                          # Cout pads to a multiple of 256: the 256 x 256 tile runs it too
F16_SCALES = tuple(1.3e4 * 1.01 ** k for k in range(80))               # of the weights: results of about N(0, scale^2), a few beyond 4 sigma; the first that clears the 1 % band


def clears_the_edge(ref):
    a = np.abs(ref)
    return not ((a > 0.99 * F16_EDGE) & (a < 1.01 * F16_EDGE)).any()


def to_half(ref):
    with np.errstate(over="ignore"):
        return np.asarray(ref, np.float64).astype(np.float16).astype(np.float32)


_f16 = {}


def f16_conv_case():
    """(x, w, b, expected fp32 [H, W, Cout]): the first scale of F16_SCALES at which no reference value lies within 1 % of 65520 -- a choice made
    on the reference alone.  Channels 3 and 5 carry a bias of +/-1e6: whole planes of +inf and -inf, decided in the epilogue's rounding."""
    if "conv" not in _f16:
        H, W, Cin, Cout = F16_SHAPE
        g = np.random.default_rng(23)
        x = g.standard_normal((H, W, Cin)).astype(np.float32)
        w0 = g.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)
        b = g.standard_normal(Cout).astype(np.float32)
        b[3], b[5] = 1e6, -1e6
        for s in F16_SCALES:
            w = (w0 * s).astype(np.float32)
            ref = F.conv2d(torch.from_numpy(opcheck.half(x)).permute(2, 0, 1)[None], torch.from_numpy(opcheck.half(w)), torch.from_numpy(b).double(), 1, 1)[0].permute(1, 2, 0).numpy()
            if clears_the_edge(ref) and (np.delete(ref, (3, 5), axis=2) > F16_EDGE).any() and (np.delete(ref, (3, 5), axis=2) < -F16_EDGE).any():
                break
        assert clears_the_edge(ref), "no scale of F16_SCALES clears the 1 % band around 65520"
        exp = to_half(ref)
        assert np.isposinf(exp[..., 3]).all() and np.isneginf(exp[..., 5]).all()
        others = np.delete(exp, (3, 5), axis=2)
        assert np.isposinf(others).any() and np.isneginf(others).any() and np.isfinite(others).mean() > 0.9   # some results exceed 65504, either sign
        _f16["conv"] = (x, w, b, ref, exp)
    return _f16["conv"]


def f16_conv(lib, mem, tile):
    """tdnet_op_conv2d_f16io on one tile code: the +/-inf mask with its signs is the reference's exactly; finite values at opcheck.gate_f16."""
    H, W, Cin, Cout = F16_SHAPE
    x, w, b, ref, exp = f16_conv_case()
    dx, out = mem.put(x), mem.empty((H, W, Cout))
    lib.check(lib.tdnet_op_conv2d_f16io(mem.ptr(dx), H, W, Cin, w.ctypes.data, b.ctypes.data, Cout, 3, 1, 1, None, 0, tile, mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    who = ("f16_conv", tile)
    assert not np.isnan(got).any(), who
    same_non_finite(got, exp, who)
    ok = np.isfinite(exp)
    opcheck.assert_within(got[ok], ref[ok], opcheck.gate_f16(ref[ok]), who)
    mem.verify(finite=False)


def f16_stem(lib, mem):
    """tdnet_op_stem_f16: fp16-MFMA conv 7x7 -> ReLU -> fp16 map -> fp16 max-pool, weights scaled so that some conv results exceed 65504:
    +inf where half() of the fp64 chain is +inf (ReLU leaves no -inf), finite values at opcheck.gate_f16."""
    H, W = 33, 65
    g = np.random.default_rng(29)
    img = g.standard_normal((3, H, W)).astype(np.float32)
    w0 = g.standard_normal((64, 3, 7, 7)) / np.sqrt(147.0)
    b = g.standard_normal(64).astype(np.float32)
    for s in F16_SCALES:
        w = (w0 * s).astype(np.float32)
        pre = F.relu(F.conv2d(torch.from_numpy(opcheck.half(img))[None], torch.from_numpy(opcheck.half(w)), torch.from_numpy(b).double(), 2, 3))
        if clears_the_edge(pre.numpy()) and (pre.numpy() > F16_EDGE).sum() >= 8:
            break
    assert clears_the_edge(pre.numpy()), "no scale of F16_SCALES clears the 1 % band around 65520"
    ref = F.max_pool2d(pre, 3, 2, 1)[0].permute(1, 2, 0).numpy()       # the maximum commutes with the monotone rounding
    exp = to_half(ref)
    assert np.isposinf(exp).any() and np.isfinite(exp).mean() > 0.5
    di, out = mem.put(img), mem.empty(ref.shape)
    lib.check(lib.tdnet_op_stem_f16(mem.ptr(di), H, W, w.ctypes.data, b.ctypes.data, -1, mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    assert not np.isnan(got).any()
    same_non_finite(got, exp, ("f16_stem",))
    ok = np.isfinite(exp)
    opcheck.assert_within(got[ok], ref[ok], opcheck.gate_f16(ref[ok]), ("f16_stem",))
    mem.verify(finite=False)


# ---- 3. labels --------------------------------------------------------------------------------------------------------------------------
LABEL_C, LABEL_LOW, LABEL_HIGH = 19, (5, 9), (33, 65)                  # scales 4 / 32 and 8 / 64: exact


def label_logits(kind):
    """fp32 [19, 5, 9] of small integers.
    inf_pair_0:  +inf in classes 0 and 7 at one pixel.  Where a neighbour reads that pixel with weight exactly 0 both are NaN (0 * inf); the
                 reference names the first NaN, class 0, and so do the kernels (a NaN in class 0 is never replaced).
    inf_pair:    +inf in classes 3 and 11 at source pixel (2, 4), reached with weight 0 from (1..3, 3..5)'s aligned outputs -- where classes
                 3 and 11 are NaN the two rules differ, so this case is compared on first_max_rule like the NaN cases; everywhere else it
                 is torch.max's.
    neg_inf_all: every class -inf at one pixel: ties of -inf (class 0) and, at weight 0, all NaN (class 0 in both rules).
    nan_class0:  one NaN in class 0: never replaced, and the first NaN of the reference too -- the one NaN case on which the two rules agree.
    nan_*:       one NaN in a middle class / in the last class, and two NaNs in one pixel."""
    g = np.random.default_rng(len(kind) * 31 + sum(map(ord, kind)))
    x = g.integers(-8, 9, (LABEL_C,) + LABEL_LOW).astype(np.float32)
    if kind == "inf_pair_0":
        x[0, 2, 4] = x[7, 2, 4] = np.inf
    elif kind == "inf_pair":
        x[3, 2, 4] = x[11, 2, 4] = np.inf
    elif kind == "neg_inf_all":
        x[:, 2, 4] = -np.inf
    elif kind == "nan_class0":
        x[0, 2, 4] = np.nan
    elif kind == "nan_middle":
        x[9, 1, 6] = np.nan
    elif kind == "nan_last":
        x[18, 3, 2] = np.nan
    elif kind == "nan_two":
        x[4, 2, 2] = x[12, 2, 2] = np.nan
    else:
        raise ValueError(kind)
    x.setflags(write=False)
    return x


INF_KINDS = ("inf_pair_0", "neg_inf_all", "nan_class0")                # every label entry == torch.max(0)[1] of up_ref, at every pixel
RULE_KINDS = ("inf_pair", "nan_middle", "nan_last", "nan_two")         # == first_max_rule(up_ref); == torch.max where the pixel holds no NaN
LABEL_KINDS = INF_KINDS + RULE_KINDS


def label_expectation(kind):
    x = label_logits(kind)
    up = out_ref.up_ref(x, *LABEL_HIGH)
    assert np.array_equal(up, up.astype(np.float32).astype(np.float64), equal_nan=True), kind    # exact in fp32: nothing left to a tolerance
    tmax = torch.from_numpy(up).max(0)[1].numpy()
    rule = out_ref.first_max_rule(up)
    has_nan = np.isnan(up).any(axis=0)
    assert np.array_equal(rule[~has_nan], tmax[~has_nan]), kind        # without a NaN the rule is the reference's
    assert not np.isfinite(up).all(), kind
    if kind in INF_KINDS:
        assert np.array_equal(rule, tmax), kind                        # ... and on these cases under the NaNs of 0 * inf too
        return x, up, tmax
    assert (rule != tmax)[has_nan].any(), kind                         # a stated difference, not an accident: the case shows it
    return x, up, rule


def label_forms(lib, mem, x, setenv):
    """{entry: labels [H, W]} of every label entry the operator library has.  mem: put(array) -> (keepalive, address), holder(nbytes, off) ->
    (address, read), stream (tests/out_cases.py's mems)."""
    C, (h, w), (H, W) = LABEL_C, LABEL_LOW, LABEL_HIGH
    n, s = H * W, mem.stream
    keep, px = mem.put(x)
    forms = {}
    p32, read32 = mem.holder(4 * n, 4)
    p8, read8 = mem.holder(n, 1)
    lib.check(lib.tdnet_op_upsample_argmax(px, C, h, w, H, W, p32, p8, s))
    forms["int32"], forms["uint8"] = read32().view(np.int32).reshape(H, W), read8().reshape(H, W)
    gt_keep, gt = mem.put(np.zeros((H, W), np.uint8))
    cm_keep, cm = mem.put(np.zeros((C, C), np.uint64))
    ps, reads = mem.holder(n, 2)
    lib.check(lib.tdnet_op_upsample_argmax_score(px, C, h, w, H, W, gt, None, ps, cm, None, s))
    forms["score"] = reads().reshape(H, W)
    full_keep, pfull = mem.put(np.zeros((C, H, W), np.float32))
    lib.check(lib.tdnet_op_upsample(px, C, h, w, H, W, pfull, s))
    for passes in ("1", "2"):
        setenv("TDNET_CONF_PASSES", passes)
        for name, args in (("conf", (px, h, w, None)), ("conf_full", (None, 0, 0, pfull))):
            pl, readl = mem.holder(n, 3)
            pc, readc = mem.holder(n, 1)
            lib.check(lib.tdnet_op_upsample_argmax_conf(args[0], C, args[1], args[2], H, W, pl, pc, 0, 255, args[3], s))
            forms["%s-%s" % (name, passes)] = readl().reshape(H, W)
            readc()
    ids = np.arange(11, 19, dtype=np.uint8)
    for name, args in (("matte", (px, h, w, None)), ("matte_full", (None, 0, 0, pfull))):
        pl, readl = mem.holder(n, 2)
        pm, readm = mem.holder(n, 3)
        lib.check(lib.tdnet_op_upsample_argmax_matte(args[0], C, args[1], args[2], H, W, pl, pm, ids.ctypes.data, len(ids), args[3], s))
        forms[name] = readl().reshape(H, W)
        readm()
    del keep, gt_keep, cm_keep, full_keep
    return forms


def labels(lib, mem, kind, setenv):
    x, up, want = label_expectation(kind)
    for name, got in label_forms(lib, mem, x, setenv).items():
        bad = got.astype(np.int64) != want
        assert not bad.any(), (kind, name, int(bad.sum()), [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]], got[bad][:4], want[bad][:4])
