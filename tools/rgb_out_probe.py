#!/usr/bin/env python3
"""GPU-box probe for the colour-map output (csrc/td_out.h k_picture_rows<false, TD_SRC_NONE, TD_DST_RGB>, before the byte ends were unified k_upsample_argmax_rgb; include/tdnet.h "colour map out"): what does asking a frame
for its quarter-size picture instead of its uint8 label map change, on the device and in the frame loop?

  frame    device ms per steady-state frame (HIP events around `--frames` frames, no host work between them) of forward_labels_u8 against
           forward_rgb_u8: every launch but the last is the same, so the difference is the last kernel's (k_upsample_argmax_u8 against
           the fused colour-map kernel).  For the two kernels' own times run the probe under `rocprofv3 --kernel-trace --stats`.
  loop     frames/s of the `tdnet_amd.test --prefetch --u8` loop -- prefetched uint8 upload, forward_labels_u8, asynchronous label download,
           nearest resize + decode_segmap on the host -- against the `--rgb` loop (forward_rgb_u8, picture download, nothing on the host),
           both without and with the PNG encoder (PIL, into memory) behind them.

One process; per round every variant gets a fresh handle (an idle handle's streams slow a busy one) and the rounds interleave the variants
(A B A B ...) as tools/ab_opts.py does.  The pictures of the two loops are compared once per size.

    python tools/rgb_out_probe.py [--sizes 769x1537,1024x2048] [--src-size 1024x2048] [--frames 48] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d OUT -o rgb -- python tools/rgb_out_probe.py --skip-loop --rounds 1"""
import argparse
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="769x1537,1024x2048", help="network sizes HxW, comma separated; the picture is (H // 4) x (W // 4)")
    ap.add_argument("--src-size", default="1024x2048", help="size of the decoded frames HsxWs")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true", help="the `frame` part only (the run to put under rocprofv3)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from tdnet_amd import arch, weights
    from tdnet_amd.dataloader import DevicePrefetcher, LabelDownloader, cityscapesLoader, nearest_index
    from tdnet_amd.model import td4_psp18
    dev = torch.device("cuda", 0)
    Hs, Ws = (int(v) for v in a.src_size.lower().split("x"))
    rng = np.random.default_rng(0)
    NF, P = 8, 4
    srcs = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).pin_memory() for _ in range(NF)]
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.lower().split("x"))
        oh, ow = H // 4, W // 4
        spec = arch.model_spec("td4", 19, "resnet18")
        sd = weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0)
        loader = cityscapesLoader(img_path=os.devnull, in_size=(H, W))
        items = [[srcs[t % NF], "f%d.png" % t, "vid", (W, H)] for t in range(a.frames)]
        on_dev = [s.to(dev) for s in srcs]

        def model():
            m = td4_psp18.td4_psp18(nclass=19, path_num=P, model_path=None, backbone="resnet18").eval().to(dev)
            m.load_state_dict(sd)
            return m

        def frame(m, rgb, img, t):
            return m.forward_rgb_u8(img, t % P, (H, W), (oh, ow)) if rgb else m.forward_labels_u8(img, pos_id=t % P, in_size=(H, W))

        def host_side(rgb, arr, png):
            if rgb:
                pic = np.squeeze(arr, axis=0)
            else:                                                      # tdnet_amd/test.py save()
                pred = np.squeeze(arr, axis=0).astype(np.int8)
                pic = loader.decode_segmap(pred[nearest_index(H, oh)][:, nearest_index(W, ow)]).astype(np.uint8)
            if png:
                Image.fromarray(pic).save(io.BytesIO(), format="PNG")
            return pic

        def device_ms(rgb):
            m = model()
            with torch.no_grad():
                for t in range(2 * P):
                    frame(m, rgb, on_dev[t % NF], t)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for t in range(a.frames):
                    frame(m, rgb, on_dev[t % NF], t)
                e1.record()
                torch.cuda.synchronize()
            n = m.engine.last_launch_count()
            m.engine.close()
            return e0.elapsed_time(e1) / a.frames, n

        def loop_fps(rgb, png, keep=None):
            m = model()
            with torch.no_grad():
                for t in range(2 * P):
                    frame(m, rgb, on_dev[t % NF], t)
                down = LabelDownloader(dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t, (img, name, folder, size_) in enumerate(DevicePrefetcher(items, dev)):
                    for tag, arr in down.submit(frame(m, rgb, img, t), t):
                        pic = host_side(rgb, arr, png)
                        if keep is not None and tag < NF:
                            keep[tag] = pic.copy()
                for tag, arr in down.drain():
                    host_side(rgb, arr, png)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            m.engine.close()
            return a.frames / dt

        ms = {False: [], True: []}
        launches = {}
        for r in range(a.rounds):
            for rgb in (False, True):
                v, launches[rgb] = device_ms(rgb)
                ms[rgb].append(v)
        print("frame %dx%d from %dx%d bytes, td4-psp18 fp32, %d frames x %d rounds: device ms per frame  labels_u8 %.4f (%d launches)   rgb %dx%d %.4f (%d launches)"
              "   difference %+.1f us" % (H, W, Hs, Ws, a.frames, a.rounds, statistics.median(ms[False]), launches[False], oh, ow,
                                          statistics.median(ms[True]), launches[True], 1e3 * (statistics.median(ms[True]) - statistics.median(ms[False]))))
        print("    rounds: labels_u8 %s   rgb %s" % (" ".join("%.4f" % v for v in ms[False]), " ".join("%.4f" % v for v in ms[True])))
        pics = ({}, {})
        if a.skip_loop:
            continue
        for png in (False, True):
            fps = {False: [], True: []}
            for r in range(a.rounds):
                for rgb in (False, True):
                    fps[rgb].append(loop_fps(rgb, png, pics[rgb] if r == 0 and not png else None))
            print("loop  %dx%d -> %dx%d, prefetched uint8 upload + asynchronous download, host %s: frames/s  labels_u8 + host decode %.1f   rgb %.1f   (x%.3f)"
                  % (H, W, oh, ow, "decode + PNG encode" if png else "decode only", statistics.median(fps[False]), statistics.median(fps[True]),
                     statistics.median(fps[True]) / statistics.median(fps[False])))
            print("    rounds: labels_u8 %s   rgb %s" % (" ".join("%.1f" % v for v in fps[False]), " ".join("%.1f" % v for v in fps[True])))
        same = sorted(pics[0]) == sorted(pics[1]) and len(pics[0]) > 0 and all(np.array_equal(pics[0][k], pics[1][k]) for k in pics[0])
        print("    pictures of the two loops equal (%d frames compared): %s" % (len(pics[0]), same))
        assert same


if __name__ == "__main__":
    main()
