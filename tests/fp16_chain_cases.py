"""Teacher-forced stage chain of a tdnet_opts.precision = 1 ("fp16 MFMA") frame, shared by tests/test_emu_fp16_chain.py (emulator) and
tests/test_gpu_fp16_chain.py (device).

Image -> logits in this mode is held to the fp32 reference at 3e-2 only, and cannot be held tighter: on td4-resnet18 at 65x129 the SAME
rounding-aware graph evaluated with fp64 and with fp32 accumulation differs at c4 by 2.0-3.1e-2 (scale 26) and at lowres by 6-9e-3
(scale 4) -- as much as the rounded graph differs from the unrounded one (2.4-3.5e-2, 7-10e-3): one fp16 rounding flipped upstream is a
whole ulp downstream.  Stage by stage it separates.  After every frame the handle's stages are read back (tdnet_get_stage) and each is
checked against oracle/fp16_ops.py applied to THE HANDLE'S OWN previous stage:

  z <- c4, ln <- feat (fp32 kernels)            1e-4 max(1, max|ref|), the goldens' gate; logits <- lowres (the upsample) 1e-5
  v_cur <- z, cache_v <- z (one fp16-MFMA conv)  T16 = 3e-5 max(1, max|ref|) (opcheck.t16)
  q_cur, cache_q, cache_k <- z (two convs),      at most 1 % of the elements (+ the channels of two pixels: share_cap) beyond T16, and every
  lowres <- feat (LayerNorm -> fp16 -> conv ->   element within T16 + 2 F, F = one flipped fp16 rounding of the intermediate map y (2^-10 max|y|)
  classifier)                                    through the second layer's weights (max|w2|; for lowres through the classifier too)
  feat <- q_cur, v_cur, the FIFO                 per element 2^-10 A + 1e-4 (opcheck.attention's gate of the final step) + 4 S, S = what
                                                 rounding P in the chain's earlier steps moves feat by, reference against reference; the 4 is
                                                 the factor opcheck.layernorm_flat and test_gpu_model grant over the CPU's own error
  cache_q / cache_v                              the stride-4 subsample of q_cur / v_cur bit for bit; warm-up: feat is v_cur bit for bit

The FIFO is the test's own: the handle's cache_* stages of the earlier frames.  Image -> c4 is not teacher-forced (no map of the
backbone survives the frame): c4 stays at 3e-2 max|ref| against the fp32 reference, and the backbone's kernels are held by the operator
entries of tests/ops_edge_cases.py.  cache_k's first layer alone is not a stage of the handle; it is held through cache_k.

Every case proves that it discriminates -- the UNROUNDED oracle from the same z misses v_cur's gate by more than 10x in at least one of
its frames (9 .. 13x: T16 is 40x the kernel's error there) -- and that its caps are the reference's own: the fp64- and fp32-accumulated
oracles differ by less than half of each cap."""
import numpy as np
import torch
import torch.nn.functional as F

import opcheck
from oracle import fp16_ops, tdnet_ref
from tdnet_amd import arch, weights
from tdnet_amd.engine import Engine

# (model, layers, backbone, H, W, frames): through warm-up into steady state, every path at least once
CASES = [("td4", 18, "resnet18", 33, 65, 6), ("td4", 18, "resnet18", 65, 129, 6), ("td2", 34, "resnet34", 33, 65, 4)]
# On the device only: a td4-resnet18 frame whose feature map (65 x 65 = 4225 pixels) is past the 4096 up to which conv_dma_pick_rh leaves a
# 512-channel conv on the register-staged kernel (64-row tiles: ceil(M / 64) * 4 <= 256 workgroups, cost 1 / 0.6; from 4097 pixels that is
# two rounds, 3.33, against 2 / 0.85 = 2.35 for 128-row tiles): layer4's convs run as CD_128 -> CD_128_P (loader waves, k_conv_dma_h3p; the
# dilation-8 / 16 ones fall back to k_conv_dma_h3 / k_conv_dma_h where the halo does not fit the image buffer), and the head conv
# (512 -> 128 on <= 16384 pixels) on the narrow tiles CD_128_N (k_conv_dma_h3n) reading the fp16 LayerNorm map.  At the sizes above
# layer4 stays register-staged (k_conv_igemm_h) and the head conv is CD_128_N as well.  Three warm-up frames are only read for their
# cache entries; the fourth, the first steady one, is checked.
DEVICE_CASE = ("td4", 18, "resnet18", 513, 513, 4)


def share_cap(n, half_of_it=False):
    """The share of a two-conv stage's n elements that may lie beyond T16: 1 %, plus the 64 channels of two pixels.  One flipped rounding
    of an intermediate value moves every channel of its pixel, so on a map of a few pixels a single flip is far more than 1 % of the
    stage.  Reference against reference (the fp64- and the fp32-accumulated oracle, no kernel involved): 51 of 960 elements = 5.3 % on
    cache_k at 65x129 (frame 1: one pixel), 88 of 9792 = 0.90 % on q_cur there, 19 of 2880 = 0.66 % on q_cur at 33x65 (frame 2), 0 on most
    other frames.  At 513x513 (270400 elements) the cap is 1.05 %."""
    return (0.005 if half_of_it else 0.01) + (64.0 if half_of_it else 128.0) / n


def _two_conv(tag, got, ref, F1, out):
    """A stage of two convs against fp64 from the stage in front of the first: at most share_cap of the elements beyond T16, every element
    within T16 + 2 F (F: one flipped rounding of the largest intermediate value through the largest weight)."""
    t = opcheck.t16(ref)
    err = np.abs(got.astype(np.float64) - ref)
    share, worst, cap = float((err > t).mean()), float(err.max()), t + 2.0 * F1
    out.append("%s: %.2f %% beyond T16 %.2e (cap %.2f %%), max %.2e, cap %.2e" % (tag, 100.0 * share, t, 100.0 * share_cap(err.size), worst, cap))
    assert share <= share_cap(err.size) and worst <= cap, (tag, share, share_cap(err.size), worst, t, cap)


def _self_check(tag, a64, a32, F1):
    """The caps are the reference's own: fp64 against fp32 accumulation stays under half of each."""
    t = opcheck.t16(a64)
    err = np.abs(a64 - a32)
    assert float((err > t).mean()) <= share_cap(err.size, True) and float(err.max()) <= 0.5 * (t + 2.0 * F1), \
        ("the input is wrong, not the cap: the oracle's own accumulation error", tag, float((err > t).mean()), float(err.max()), t, F1)


def run_case(lib, mem, case, checked=None):
    """Runs the clip; returns the lines it measured (also printed).  checked: the frames whose stages are checked (None: all)."""
    name, layers, bb, H, W, T = case
    P = 4 if name == "td4" else 2
    spec = arch.model_spec(name, 19, bb)
    h, w = arch.feat_size(H), arch.feat_size(W)
    hk, wk = (h - 1) // 4 + 1, (w - 1) // 4 + 1
    Lq, Lk = h * w, hk * wk
    sd = weights.synth_state_dict(spec, h, w, 0)
    e = Engine(P, layers, 19, H, W, 0, lib=lib, opts={"precision": 1})
    e.load_state_dict(sd)
    assert e.opts()["precision"] == 1
    DV = e.cache_dims()[2]
    o64, o32 = fp16_ops.Fp16Stages(spec, sd), fp16_ops.Fp16Stages(spec, sd, acc=torch.float32)
    plain = fp16_ops.Fp16Stages(spec, sd, rounded=False)
    ref = tdnet_ref.TDNetRef(spec, sd)
    ref.trace = {}
    depth = tdnet_ref.REF_FIFO[name]
    fifo, lines, best_miss = [], [], 0.0
    sub = lambda m: m[:, :, ::4, ::4]                                  # [1, C, h, w] -> the key grid
    flat = lambda m: np.ascontiguousarray(np.transpose(m[0], (1, 2, 0))).reshape(-1, m.shape[1])   # -> [positions, C]
    for t, x in enumerate(weights.synth_video(H, W, T, seed=1)):
        pos = t % P
        steady = len(fifo) >= depth
        dx, out = mem.put(x), mem.empty((1, 19, H, W))
        e.forward(mem.ptr(dx), pos, mem.ptr(out), mem.stream)
        logits = np.array(mem.get(out))
        st = {n: e.stage(n, s) for n, s in (("c4", (1, 512, h, w)), ("z", (1, 512, h, w)), ("v_cur", (1, DV, h, w)), ("q_cur", (Lq, 64)),
                                            ("feat", (1, DV, h, w)), ("ln", (1, DV, h, w)), ("lowres", (1, 19, h, w)), ("cache_q", (Lk, 64)),
                                            ("cache_k", (Lk, 64)), ("cache_v", (Lk, DV)))}
        ref.forward(torch.from_numpy(x), pos)
        entry = (st["cache_q"], st["cache_k"], st["cache_v"])
        tag = "%s-%s %dx%d frame %d" % (name, bb, H, W, t)
        # one fp16-MFMA conv: v_cur (every frame: it also measures how far the unrounded oracle is)
        v64, v32, vplain = o64.v_cur(st["z"], pos), o32.v_cur(st["z"], pos), plain.v_cur(st["z"], pos)
        gate = opcheck.t16(v64)
        assert np.abs(v64 - v32).max() <= 0.5 * gate, (tag, "v_cur: the oracle's own accumulation error", float(np.abs(v64 - v32).max()), gate)
        miss = float(np.abs(st["v_cur"] - vplain).max()) / gate
        verr = float(np.abs(st["v_cur"] - v64).max())
        lines.append("%s v_cur: error %.2e, T16 %.2e; the unrounded oracle misses by %.1f gates" % (tag, verr, gate, miss))
        best_miss = max(best_miss, miss)
        assert verr <= gate, (tag, "v_cur", verr, gate)
        if checked is not None and t not in checked:
            fifo = (fifo + [entry])[-depth:]
            continue
        # the backbone: the existing whole-frame gate
        c4r = ref.trace["c4"].numpy()
        assert np.abs(st["c4"] - c4r).max() <= 3e-2 * np.abs(c4r).max(), (tag, "c4")
        # fp32 kernels
        for stage, r in (("z", o64.z_from_c4(st["c4"], pos)), ("ln", o64.ln(st["feat"], pos))):
            err = float(np.abs(st[stage] - r).max())
            assert err <= 1e-4 * max(1.0, float(np.abs(r).max())), (tag, stage, err)
        up = F.interpolate(torch.from_numpy(st["lowres"]).double(), (H, W), mode="bilinear", align_corners=True).numpy()
        assert np.abs(logits - up).max() <= 1e-5, (tag, "logits", float(np.abs(logits - up).max()))
        assert np.array_equal(st["cache_v"], flat(sub(st["v_cur"]))), (tag, "cache_v != subsample(v_cur)")
        assert np.array_equal(st["cache_q"], flat(sub(np.transpose(st["q_cur"].reshape(1, h, w, 64), (0, 3, 1, 2))))), (tag, "cache_q != subsample(q_cur)")
        # two convs: q_cur (and with it cache_q, its subsample), cache_k
        for stage, branch, stride in (("q_cur", "qs", 1), ("cache_k", "ks", 4)):
            (r64, y, w2), (r32, _, _) = o64.qk(st["z"], pos, branch, stride), o32.qk(st["z"], pos, branch, stride)
            F1 = 2.0 ** -10 * float(np.abs(y).max()) * float(w2.max())
            _self_check((tag, stage), r64, r32, F1)
            _two_conv("%s %s" % (tag, stage), st[stage], flat(r64), F1, lines)
        # the head: LayerNorm -> fp16 -> conv -> classifier
        (l64, y, amp), (l32, _, _) = o64.lowres(st["feat"], pos), o32.lowres(st["feat"], pos)
        F1 = 2.0 ** -10 * float(np.abs(y).max()) * amp
        _self_check((tag, "lowres"), l64, l32, F1)
        _two_conv("%s lowres" % tag, st["lowres"], l64, F1, lines)
        # the attention chain
        if not steady:
            assert np.array_equal(st["feat"], st["v_cur"]), (tag, "warm-up: feat != v_cur")
        else:
            q, v = st["q_cur"], flat(st["v_cur"])
            f64, amp = o64.feat(pos, q, v, fifo, round_p=False)
            S = float(np.abs(o64.feat(pos, q, v, fifo, round_p=True)[0] - f64).max())
            gate = 2.0 ** -10 * amp + 1e-4 + 4.0 * S
            ratio = opcheck.assert_within(flat(st["feat"]), f64, gate, (tag, "feat"))
            lines.append("%s feat: S %.2e, worst error / gate %.2f" % (tag, S, ratio))
        fifo = (fifo + [entry])[-depth:]
    e.close()
    print("\n".join(lines))
    assert best_miss > 10.0, (case, "the case does not discriminate: the unrounded oracle stays within 10 gates of v_cur in every frame", best_miss)
    return lines
