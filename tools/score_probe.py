#!/usr/bin/env python3
"""GPU-box probe for the score output (csrc/td_score.h; include/tdnet.h "score out"): what does scoring a clip on the device cost, against the
label entry it extends and against what Training/validate.py does on the host?  td4-psp18 fp32 on synthetic weights, frames resident on the device.

  loop     frames/s of four forms, interleaved in one process (a b c d a b c d ..., a fresh handle per form and round, `--warmup` frames first):
             (a) forward_labels_u8                      -- not changed by the score entries: the parent's number, measured here
             (b) forward_score_u8                       -- the fused form (the label map is not asked for)
             (c) forward_labels_u8 + score_labels       -- the unfused form, one more launch
             (d) forward_labels_u8, labels to the host, np.bincount per frame -- validate.py:59-70
           and the matrices of (b), (c), (d) compared.
  family   device ms of the frame's "everything else" kernels (tdnet_last_ms(h, 2); the last kernel is the only difference) for (a) and for (b)
           on three ground truths: the network's own labels, 8 x 16 blocks, noise.
  kernel   the score kernel alone through tdnet_op_upsample_argmax_score on the network's own low-resolution logits, on the same three ground
           truths, with and without the wave-uniform path (TDNET_SCORE_WAVE_UNIFORM=0, read by that entry): HIP events around the call, which
           include the entry's 256-byte upload and synchronisation -- `overhead` is the same call on a 1 x 4 image.  For the kernels' own times
           run `--kernel-only KIND` under `rocprofv3 --kernel-trace --stats`: the two instantiations are two kernel names.

    python tools/score_probe.py [--sizes 1024x2048,769x1537] [--src-size 1024x2048] [--frames 48] [--warmup 8] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d OUT -o score -- python tools/score_probe.py --sizes 1024x2048 --kernel-only blocky"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x2048,769x1537", help="network sizes HxW, comma separated")
    ap.add_argument("--src-size", default="1024x2048", help="size of the decoded frames HsxWs")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", default=None, metavar="KIND", help="only the operator entry, 50 calls with and 50 without the wave-uniform path, on ground truth own|blocky|noise")
    a = ap.parse_args()
    import numpy as np
    import torch
    import score_cases as cases
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

        def model():
            m = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev)
            m.load_state_dict(sd)
            return m

        # the network's own output: labels and low-resolution logits of frame 2 P - 1 (steady state)
        with torch.no_grad():
            m = model()
            for t in range(2 * P):
                own = m.forward_labels_u8(srcs[t % NF], pos_id=t % P, in_size=(H, W))
            torch.cuda.synchronize()
            h, w = m.engine.feature_dims()
            lowres = torch.from_numpy(m.engine.stage("lowres", (C, h, w))).to(dev)
            own_np = own[0].cpu().numpy()
            m.engine.close()
        gts = {"own": own_np, "blocky": cases.ground_truth("blocky", C, own_np), "noise": cases.ground_truth("noise", C, own_np)}
        gts_dev = {k: torch.from_numpy(np.ascontiguousarray(v)[None]).to(dev) for k, v in gts.items()}
        s = torch.cuda.current_stream(dev).cuda_stream

        def op_ms(kind, uniform, n, HH=H, WW=W, hh=h, ww=w):
            os.environ["TDNET_SCORE_WAVE_UNIFORM"] = "1" if uniform else "0"
            cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
            gt = gts_dev[kind] if HH == H else torch.zeros((1, HH, WW), dtype=torch.uint8, device=dev)
            ms = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tlib.check(tlib.tdnet_op_upsample_argmax_score(lowres.data_ptr(), C, hh, ww, HH, WW, gt.data_ptr(), None, None, cm.data_ptr(), None, s))
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            if HH == H:
                assert np.array_equal(cm.cpu().numpy(), n * cases.expected_matrix(gts[kind], own_np, C)), (kind, uniform)
            return statistics.median(ms)

        if a.kernel_only:
            for uniform in (True, False, True, False):
                print("kernel-only %dx%d gt=%s wave-uniform=%d: %.1f us per call (events, entry overhead included), 25 calls"
                      % (H, W, a.kernel_only, uniform, 1e3 * op_ms(a.kernel_only, uniform, 25)))
            continue

        def run(form, gt_kind="blocky", prof=False):
            """(frames/s, matrix or None, family-2 ms of the last frame or None) of one form on a fresh handle"""
            m = model()
            gt, gt_np = gts_dev[gt_kind], gts[gt_kind]
            host = np.zeros((C, C), np.int64)

            def frame(t, count):
                img = srcs[t % NF]
                if form == "b":
                    m.forward_score_u8(img, gt, t % P, (H, W))
                    return
                l8 = m.forward_labels_u8(img, pos_id=t % P, in_size=(H, W))
                if form == "c":
                    m.score_labels(l8, gt)
                elif form == "d":
                    pred = l8.cpu().numpy()                            # validate.py:69-70: synchronous download, then the host counts
                    if count:
                        host[...] += cases.expected_matrix(gt_np, pred[0], C)
            with torch.no_grad():
                for t in range(a.warmup):
                    frame(t, False)
                if form in "bc":
                    m.reset_score()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(a.warmup, a.warmup + a.frames):
                    frame(t, True)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                cm = m.confusion_matrix() if form in "bc" else host if form == "d" else None
                fam = None
                if prof:
                    m.engine.set_profiling(True)
                    vals = []
                    for t in range(a.warmup + a.frames, a.warmup + a.frames + 2 * P):
                        frame(t, False)
                        torch.cuda.synchronize()
                        vals.append(m.engine.last(2)[0])
                    fam = statistics.median(vals)
            launches = m.engine.last_launch_count()
            m.engine.close()
            return a.frames / dt, cm, fam, launches

        fps = {f: [] for f in "abcd"}
        cms, launches = {}, {}
        for r in range(a.rounds):
            for f in "abcd":
                v, cm, _, launches[f] = run(f)
                fps[f].append(v)
                if cm is not None:
                    cms[f] = cm
        med = {f: statistics.median(fps[f]) for f in "abcd"}
        print("loop %dx%d from %dx%d bytes, td4-psp18 fp32, %d frames x %d rounds after %d warm-up frames, gt = blocks: frames/s  (a) labels_u8 %.1f   (b) score fused %.1f (x%.3f)"
              "   (c) labels_u8 + score_labels %.1f (x%.3f)   (d) labels to host + bincount %.1f (x%.3f)   launches a/b/c %d/%d/%d(+1)"
              % (H, W, Hs, Ws, a.frames, a.rounds, a.warmup, med["a"], med["b"], med["b"] / med["a"], med["c"], med["c"] / med["a"], med["d"], med["d"] / med["a"],
                 launches["a"], launches["b"], launches["c"]))
        for f in "abcd":
            print("    rounds (%s): %s" % (f, " ".join("%.1f" % v for v in fps[f])))
        same = np.array_equal(cms["b"], cms["c"]) and np.array_equal(cms["b"], cms["d"]) and cms["b"].sum() > 0
        print("    matrices of (b), (c), (d) equal: %s (%d pixels counted)" % (same, cms["b"].sum()))
        assert same
        fam_a = run("a", prof=True)[2]
        print("family %dx%d: device ms of the frame's family-2 kernels (the last kernel is the only difference): (a) labels_u8 %.4f" % (H, W, fam_a))
        for kind in ("own", "blocky", "noise"):
            fam_b = run("b", kind, prof=True)[2]
            print("    (b) score fused, gt = %-6s %.4f   difference %+.1f us" % (kind, fam_b, 1e3 * (fam_b - fam_a)))
        over = op_ms("own", True, 15, 1, 4, 1, 1)
        print("kernel %dx%d: tdnet_op_upsample_argmax_score on the network's own logits, HIP events around the call, median of 15; overhead (1 x 4 image) %.1f us" % (H, W, 1e3 * over))
        for kind in ("own", "blocky", "noise"):
            on, off = op_ms(kind, True, 15), op_ms(kind, False, 15)
            on2, off2 = op_ms(kind, True, 15), op_ms(kind, False, 15)
            print("    gt = %-6s wave-uniform on %.1f / %.1f us   off %.1f / %.1f us   (minus overhead: on %.1f, off %.1f)"
                  % (kind, 1e3 * on, 1e3 * on2, 1e3 * off, 1e3 * off2, 1e3 * (min(on, on2) - over), 1e3 * (min(off, off2) - over)))
        os.environ.pop("TDNET_SCORE_WAVE_UNIFORM", None)


if __name__ == "__main__":
    main()
