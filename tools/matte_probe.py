#!/usr/bin/env python3
"""GPU-box probe for the matte output (csrc/td_matte.h; include/tdnet.h "matte out"): what do the matte and the composite cost, against the
entries they extend -- the label entry, the confidence entry (the same gathers and exponentials, one sum less) and the overlay entry (the same
source read and picture store)?  td4-psp18 fp32 on synthetic weights, frames resident on the device.

  loop     frames/s of six measurements, interleaved in one process (a a' c m o k a a' c m o k ..., one handle per form on one weight block, reset
           and `--warmup` frames before every round):
             (a), (a')  forward_labels_u8, twice     -- the yardstick, and the noise actually seen between two measurements of the same thing
             (c)        forward_labels_conf_u8       -- labels + confidence
             (m)        forward_matte_u8             -- labels + matte of Cityscapes train ids 11..18
             (o)        forward_overlay_u8           -- the overlay at the source's size
             (k)        forward_composite_u8         -- the composite over a background at the source's size
  family   device ms of the frame's "everything else" kernels (tdnet_last_ms(h, 2) with profiling on; the last launch is the only difference
           between the forms): median over 2 P frames, every form.
  kernel   the fused kernels alone through the operator entries on the network's own low-resolution logits: HIP events around the call, which
           include the entry's synchronisation -- `overhead` is the same call on a 1 x 4 image -- tdnet_op_upsample_argmax_conf (one pass)
           and tdnet_op_upsample_argmax_matte in turn, each twice, so that the spread of a kernel's own repeated runs stands beside the difference.

  trace    (--trace: the run to put under the profiler, nothing is timed by the script) 24 frames each of the confidence, matte, overlay and
           composite forms at the first size, the two pictures in two cells: the tight RGB24 frame into the contiguous block, and a BGRA32 source
           view (a crop at an odd origin, padded pitch) into an RGBA32 destination view.  Every form's last kernel is an instantiation of its own,
           so the kernel statistics give the matte kernel beside the confidence kernel and each composite kernel beside the overlay kernel of
           the same source and destination:
               rocprofv3 --kernel-trace --stats -d OUT -o matte -- python tools/matte_probe.py --trace
  baseline (--baseline: uses nothing this feature added, so the same file runs in a checkout of the parent commit) frames/s of forward_labels_u8
           and forward_overlay_u8 alone, `--rounds` rounds in turn.

    timeout 600 python tools/matte_probe.py [--sizes 1024x2048,769x1537] [--src-size 1080x1920] [--frames 48] [--warmup 8] [--rounds 3]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MOVING = tuple(range(11, 19))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x2048,769x1537", help="network sizes HxW, comma separated")
    ap.add_argument("--src-size", default="1080x1920", help="size of the decoded frames HsxWs")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="the frames to put under rocprofv3 --kernel-trace --stats; nothing is timed here")
    ap.add_argument("--baseline", action="store_true", help="frames/s of the label and the overlay entry only (runs in the parent commit's checkout too)")
    a = ap.parse_args()
    if a.trace or a.baseline:
        return side_runs(a)
    import numpy as np
    import torch
    from tdnet_amd import _capi, arch, weights
    from tdnet_amd.model import td4_psp18
    dev = torch.device("cuda", 0)
    tlib = _capi.test_lib()
    Hs, Ws = (int(v) for v in a.src_size.lower().split("x"))
    rng = np.random.default_rng(0)
    NF, P, C = 8, 4, 19
    srcs = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).to(dev) for _ in range(NF)]
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.lower().split("x"))
        spec = arch.model_spec("td4", C, "resnet18")
        sd = weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0)
        owner = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev)
        owner.load_state_dict(sd)
        owner.ensure_engine(H, W, dev)
        forms = ("a", "a'", "c", "m", "o", "k")
        models = {f: td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev).share_weights_with(owner) for f in forms}
        for f in ("m", "k"):
            models[f].set_matte(MOVING)
        last = {}

        def frame(f, t):
            m, img = models[f], srcs[t % NF]
            if f == "c":
                last[f] = m.forward_labels_conf_u8(img, t % P, (H, W))
            elif f == "m":
                last[f] = m.forward_matte_u8(img, t % P, (H, W))
            elif f == "o":
                last[f] = m.forward_overlay_u8(img, t % P, (H, W))
            elif f == "k":
                last[f] = m.forward_composite_u8(img, t % P, (H, W), background=(0, 255, 0))
            else:
                last[f] = m.forward_labels_u8(img, pos_id=t % P, in_size=(H, W))

        def run(f):
            models[f].reset()
            with torch.no_grad():
                for t in range(a.warmup):
                    frame(f, t)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(a.warmup, a.warmup + a.frames):
                    frame(f, t)
                torch.cuda.synchronize()
                return a.frames / (time.perf_counter() - t0)

        fps = {f: [] for f in forms}
        for r in range(a.rounds):
            for f in forms:
                fps[f].append(run(f))
        med = {f: statistics.median(fps[f]) for f in forms}
        print("loop %dx%d from %dx%d bytes, td4-psp18 fp32, %d frames x %d rounds after %d warm-up frames: frames/s  (a) labels_u8 %.1f   (a') the same again %.1f (noise %.2f %%)"
              "   (c) labels + confidence %.1f   (m) labels + matte %.1f (x%.3f of a, x%.3f of c)   (o) overlay %.1f   (k) composite %.1f (x%.3f of a, x%.3f of o)   launches a/c/m/o/k %s"
              % (H, W, Hs, Ws, a.frames, a.rounds, a.warmup, med["a"], med["a'"], 100 * abs(med["a'"] - med["a"]) / med["a"], med["c"], med["m"], med["m"] / med["a"],
                 med["m"] / med["c"], med["o"], med["k"], med["k"] / med["a"], med["k"] / med["o"], "/".join(str(models[f].engine.last_launch_count()) for f in ("a", "c", "m", "o", "k"))))
        for f in forms:
            print("    rounds (%s): %s" % (f, " ".join("%.1f" % v for v in fps[f])))
        la, lm = last["a"][0].cpu().numpy(), last["m"][0][0].cpu().numpy()
        mm = last["m"][1][0].cpu().numpy()
        print("    last frame: labels of (a) and (m) equal: %s; matte bytes %d..%d, mean %.1f" % (bool((la == lm).all()), mm.min(), mm.max(), mm.mean()))
        assert (la == lm).all()

        def family(f):
            m = models[f]
            m.engine.set_profiling(True)
            vals = []
            with torch.no_grad():
                for t in range(a.warmup + a.frames, a.warmup + a.frames + 2 * P):
                    frame(f, t)
                    torch.cuda.synchronize()
                    vals.append(m.engine.last(2)[0])
            m.engine.set_profiling(False)
            return statistics.median(vals)

        fam = {f: family(f) for f in ("a", "c", "m", "o", "k", "a'")}
        print("family %dx%d: device ms of the frame's family-2 kernels (the last launch is the only difference): (a) %.4f   (a') %.4f   (c) %.4f   (m) %.4f   (o) %.4f   (k) %.4f"
              "   m - c %+.1f us   k - o %+.1f us   (a' - a %+.1f us)" % (H, W, fam["a"], fam["a'"], fam["c"], fam["m"], fam["o"], fam["k"], 1e3 * (fam["m"] - fam["c"]),
                                                                         1e3 * (fam["k"] - fam["o"]), 1e3 * (fam["a'"] - fam["a"])))

        # the network's own low-resolution logits (steady state) through the operator entries
        h, w = models["a"].engine.feature_dims()
        torch.cuda.synchronize()
        lowres = torch.from_numpy(models["a"].engine.stage("lowres", (C, h, w))).to(dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        lab = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        out = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        ids = np.array(MOVING, np.uint8)
        os.environ["TDNET_CONF_PASSES"] = "1"

        def op_ms(matte, n, HH=H, WW=W, hh=h, ww=w):
            ms = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if matte:
                    tlib.check(tlib.tdnet_op_upsample_argmax_matte(lowres.data_ptr(), C, hh, ww, HH, WW, lab.data_ptr(), out.data_ptr(), ids.ctypes.data, len(ids), None, s))
                else:
                    tlib.check(tlib.tdnet_op_upsample_argmax_conf(lowres.data_ptr(), C, hh, ww, HH, WW, lab.data_ptr(), out.data_ptr(), 0, 255, None, s))
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms)

        over = op_ms(False, 15, 1, 4, 1, 1)
        res = {False: [], True: []}
        for _ in range(4):
            for k in (False, True):
                res[k].append(op_ms(k, 15))
        print("kernel %dx%d x %d classes: operator entries on the network's own logits, HIP events around the call, median of 15, four times in turn; overhead (1 x 4 image) %.1f us"
              % (H, W, C, 1e3 * over))
        for k, what in ((False, "k_upsample_argmax_conf_u8<true>"), (True, "k_upsample_argmax_matte_u8")):
            print("    %-34s %s us   (minus overhead: min %.1f, spread %.1f)" % (what, " / ".join("%.1f" % (1e3 * v) for v in res[k]), 1e3 * (min(res[k]) - over),
                                                                             1e3 * (max(res[k]) - min(res[k]))))
        os.environ.pop("TDNET_CONF_PASSES", None)
        for m in list(models.values()) + [owner]:
            m.engine.close()


def side_runs(a):
    import numpy as np
    import torch
    from tdnet_amd import arch, weights
    from tdnet_amd.dataloader import PIX_BGRA32, PIX_RGBA32, SourceView, pack_view
    from tdnet_amd.model import td4_psp18
    dev = torch.device("cuda", 0)
    Hs, Ws = (int(v) for v in a.src_size.lower().split("x"))
    H, W = (int(v) for v in a.sizes.split(",")[0].lower().split("x"))
    P, C, NF = 4, 19, 4
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(NF)]
    srcs = [torch.from_numpy(f[None]).to(dev) for f in host]
    sd = weights.synth_state_dict(arch.model_spec("td4", C, "resnet18"), arch.feat_size(H), arch.feat_size(W), 0)
    owner = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev)
    owner.load_state_dict(sd)
    owner.ensure_engine(H, W, dev)

    def shared():
        return td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev).share_weights_with(owner)

    if a.baseline:
        models = {"labels_u8": shared(), "overlay_u8": shared()}
        fps = {f: [] for f in models}
        with torch.no_grad():
            for r in range(a.rounds):
                for f, m in models.items():
                    call = (lambda t: m.forward_labels_u8(srcs[t % NF], pos_id=t % P, in_size=(H, W))) if f == "labels_u8" else \
                           (lambda t: m.forward_overlay_u8(srcs[t % NF], t % P, (H, W)))
                    m.reset()
                    for t in range(a.warmup):
                        call(t)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for t in range(a.warmup, a.warmup + a.frames):
                        call(t)
                    torch.cuda.synchronize()
                    fps[f].append(a.frames / (time.perf_counter() - t0))
        for f in models:
            print("baseline %dx%d from %dx%d bytes, %d frames x %d rounds: %s frames/s %s   median %.1f"
                  % (H, W, Hs, Ws, a.frames, a.rounds, f, " ".join("%.1f" % v for v in fps[f]), statistics.median(fps[f])))
        return
    sview = SourceView(PIX_BGRA32, Hs + 9, Ws + 7, pitch=(Ws + 7) * 4 + 5, crop=(3, 7, Hs, Ws))
    dview = SourceView(PIX_RGBA32, Hs + 9, Ws + 13, pitch=(Ws + 13) * 4 + 5, crop=(3, 5, Hs, Ws))
    big = np.zeros((Hs + 9, Ws + 7, 3), np.uint8)
    big[3:3 + Hs, 7:7 + Ws] = host[0]
    vsrc = torch.from_numpy(pack_view(big, sview, 0)[None]).to(dev)
    forms = {f: shared() for f in ("conf", "matte", "overlay", "composite", "overlay_view", "composite_view")}
    for f in ("matte", "composite", "composite_view"):
        forms[f].set_matte(MOVING)
    with torch.no_grad():
        for t in range(24):
            forms["conf"].forward_labels_conf_u8(srcs[t % NF], t % P, (H, W))
            forms["matte"].forward_matte_u8(srcs[t % NF], t % P, (H, W))
            forms["overlay"].forward_overlay_u8(srcs[t % NF], t % P, (H, W))
            forms["composite"].forward_composite_u8(srcs[t % NF], t % P, (H, W), background=(0, 255, 0))
            forms["overlay_view"].forward_overlay_u8(vsrc, t % P, (H, W), view=sview, out_view=dview)
            forms["composite_view"].forward_composite_u8(vsrc, t % P, (H, W), background=(0, 255, 0), view=sview, out_view=dview)
    torch.cuda.synchronize()
    print("trace: 24 frames of each of %s at %dx%d from %dx%d bytes" % (", ".join(forms), H, W, Hs, Ws))


if __name__ == "__main__":
    main()
