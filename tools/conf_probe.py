#!/usr/bin/env python3
"""GPU-box probe for the confidence output (csrc/td_conf.h; include/tdnet.h "confidence out"): what does asking for the confidence map cost, against
the label entry it extends and against what a caller had to do before -- full-resolution logits and a pass of their own?  td4-psp18 fp32 on
synthetic weights, frames resident on the device.

  loop     frames/s of four measurements, interleaved in one process (a a' b c a a' b c ..., one handle per form on one weight block, reset and
           `--warmup` frames before every round):
             (a), (a')  forward_labels_u8, twice     -- the yardstick, and the noise actually seen between two measurements of the same thing
             (b)        forward_labels_conf_u8       -- the fused form: labels + confidence in the frame's last launch
             (c)        forward_u8 + logits_conf     -- the caller's alternative: 4 nclass bytes of logits per pixel, then the unfused kernel
           and the labels / confidence bytes of (b) and (c) compared on the last frame.
  family   device ms of the frame's "everything else" kernels (tdnet_last_ms(h, 2) with profiling on; the last launch is the only difference
           between (a) and (b)): median over 2 P frames.
  kernel   the fused kernel alone through tdnet_op_upsample_argmax_conf on the network's own low-resolution logits, one-pass against two-pass
           form (TDNET_CONF_PASSES=1 / 2, read by that entry): HIP events around the call, which include the entry's synchronisation --
           `overhead` is the same call on a 1 x 4 image -- next to tdnet_op_upsample_argmax (uint8 labels only) timed the same way.

    timeout 600 python tools/conf_probe.py [--sizes 1024x2048,769x1537] [--src-size 1024x2048] [--frames 48] [--warmup 8] [--rounds 3]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x2048,769x1537", help="network sizes HxW, comma separated")
    ap.add_argument("--src-size", default="1024x2048", help="size of the decoded frames HsxWs")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
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
        forms = ("a", "a'", "b", "c")
        models = {f: td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev).share_weights_with(owner) for f in forms}
        last = {}

        def frame(f, t):
            m, img = models[f], srcs[t % NF]
            if f == "b":
                last[f] = m.forward_labels_conf_u8(img, t % P, (H, W))
            elif f == "c":
                last[f] = m.logits_conf(m.forward_u8(img, pos_id=t % P, in_size=(H, W)))
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
        noise = abs(med["a'"] - med["a"]) / med["a"]
        print("loop %dx%d from %dx%d bytes, td4-psp18 fp32, %d frames x %d rounds after %d warm-up frames: frames/s  (a) labels_u8 %.1f   (a') the same again %.1f (noise %.2f %%)"
              "   (b) labels + confidence fused %.1f (x%.3f of a)   (c) forward_u8 + logits_conf %.1f (x%.3f of a; b is x%.3f of c)   launches a/b/c %d/%d/%d(+1)"
              % (H, W, Hs, Ws, a.frames, a.rounds, a.warmup, med["a"], med["a'"], 100 * noise, med["b"], med["b"] / med["a"], med["c"], med["c"] / med["a"], med["b"] / med["c"],
                 models["a"].engine.last_launch_count(), models["b"].engine.last_launch_count(), models["c"].engine.last_launch_count()))
        for f in forms:
            print("    rounds (%s): %s" % (f, " ".join("%.1f" % v for v in fps[f])))
        lb, cb = (v[0].cpu().numpy().astype(np.int64) for v in last["b"])
        lc, cc = (v[0].cpu().numpy().astype(np.int64) for v in last["c"])
        la = last["a"][0].cpu().numpy()
        print("    last frame: labels of (a), (b), (c) equal: %s; confidence bytes of (b) and (c) differ at %d of %d pixels (by at most %d); bytes %d..%d, mean %.1f"
              % (bool((la == lb).all() and (lb == lc).all()), int((cb != cc).sum()), cb.size, int(np.abs(cb - cc).max()), cb.min(), cb.max(), cb.mean()))
        assert (la == lb).all() and (lb == lc).all() and np.abs(cb - cc).max() <= 1

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

        fam = {f: family(f) for f in ("a", "b", "a'")}
        print("family %dx%d: device ms of the frame's family-2 kernels (the last launch is the only difference): (a) labels_u8 %.4f   (a') %.4f   (b) labels + confidence %.4f"
              "   difference b - a %+.1f us (a' - a %+.1f us)" % (H, W, fam["a"], fam["a'"], fam["b"], 1e3 * (fam["b"] - fam["a"]), 1e3 * (fam["a'"] - fam["a"])))

        # the network's own low-resolution logits (steady state) through the operator entries
        h, w = models["a"].engine.feature_dims()
        torch.cuda.synchronize()
        lowres = torch.from_numpy(models["a"].engine.stage("lowres", (C, h, w))).to(dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        lab = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        conf = torch.zeros((H, W), dtype=torch.uint8, device=dev)

        def op_ms(passes, n, HH=H, WW=W, hh=h, ww=w):
            if passes:
                os.environ["TDNET_CONF_PASSES"] = str(passes)
            ms = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if passes:
                    tlib.check(tlib.tdnet_op_upsample_argmax_conf(lowres.data_ptr(), C, hh, ww, HH, WW, lab.data_ptr(), conf.data_ptr(), 0, 255, None, s))
                else:
                    tlib.check(tlib.tdnet_op_upsample_argmax(lowres.data_ptr(), C, hh, ww, HH, WW, None, lab.data_ptr(), s))
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms)

        over = op_ms(1, 15, 1, 4, 1, 1)
        res = {k: [op_ms(k, 15), op_ms(k, 15)] for k in (0, 1, 2, 0, 1, 2)}
        print("kernel %dx%d: operator entries on the network's own logits, HIP events around the call, median of 15, twice; overhead (1 x 4 image) %.1f us" % (H, W, 1e3 * over))
        for k, what in ((0, "uint8 labels only (k_upsample_argmax_u8)"), (1, "labels + confidence, one pass"), (2, "labels + confidence, two passes")):
            print("    %-42s %.1f / %.1f us   (minus overhead %.1f)" % (what, 1e3 * res[k][0], 1e3 * res[k][1], 1e3 * (min(res[k]) - over)))
        os.environ.pop("TDNET_CONF_PASSES", None)
        for m in list(models.values()) + [owner]:
            m.engine.close()


if __name__ == "__main__":
    main()
