#!/usr/bin/env python3
"""GPU-box probe for overlay out (csrc/td_out.h k_picture_rows<false, SRC, TD_DST_RGB>, before the byte ends were unified k_upsample_argmax_overlay<SRC, VIEW>; include/tdnet.h "overlay out").

Device milliseconds per steady-state td4-psp18 frame with three last launches on the same frames, interleaved in one process (three handles on
one weight block, --rounds rounds of --frames frames each, the order rotating, HIP events around each round):
    labels   forward_u8_labels
    rgb      forward_u8_rgb at out_size = the source size: the same sampling and the same number of output bytes as the overlay (the baseline)
    overlay  forward_u8_overlay
and, in the same run, a plain device-to-device copy of the source extent: the floor of what reading the source can cost.  Per-round figures,
medians and spreads (max - min), the overlay - rgb difference against copy + the rgb frame's own spread, and the labels / rgb pair.

    python tools/overlay_out_probe.py --size 769x1537 --src-size 1024x2048 [--nv12] [--rounds 6] [--frames 40]
    rocprofv3 --kernel-trace --stats -d OUT -o r1 -- python tools/overlay_out_probe.py --size 769x1537 --src-size 1024x2048 --rounds 1   (the tail kernels' own times)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="769x1537", help="network size HxW")
    ap.add_argument("--src-size", default="1024x2048", help="source size HsxWs = the overlay's size")
    ap.add_argument("--nv12", action="store_true", help="the source is an NV12 surface (pitch = the row rounded up to 256) instead of packed RGB")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.lower().split("x"))
    Hs, Ws = (int(v) for v in a.src_size.lower().split("x"))
    import numpy as np
    import torch
    from tdnet_amd import arch, weights
    from tdnet_amd.dataloader import cityscapesLoader, rgb_to_nv12
    from tdnet_amd.engine import Engine
    spec = arch.model_spec("td4", 19, "resnet18")
    owner = Engine(4, 18, 19, H, W, torch.cuda.current_device())
    owner.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    eng = {"labels": owner, "rgb": owner.share(), "overlay": owner.share()}
    rgb = np.random.default_rng(0).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    if a.nv12:
        surf = rgb_to_nv12(rgb)
        src = torch.from_numpy(surf).cuda()
        for e in eng.values():
            e.set_input_nv12(Hs, Ws, surf.shape[1])
    else:
        src = torch.from_numpy(rgb).cuda()
        for e in eng.values():
            e.set_input_u8(Hs, Ws)
    pal = np.array(cityscapesLoader.colors, np.uint8)
    eng["rgb"].set_output_rgb(Hs, Ws, pal)
    eng["overlay"].set_output_overlay(np.concatenate([pal, np.full((19, 1), 128, np.uint8)], axis=1))
    out = {"labels": torch.empty((H, W), dtype=torch.uint8, device="cuda"), "rgb": torch.empty((Hs, Ws, 3), dtype=torch.uint8, device="cuda"),
           "overlay": torch.empty((Hs, Ws, 3), dtype=torch.uint8, device="cuda")}
    dst = torch.empty_like(src)
    s = torch.cuda.current_stream().cuda_stream
    call = {"labels": lambda t: eng["labels"].forward_u8_labels(src.data_ptr(), t % 4, out["labels"].data_ptr(), s),
            "rgb": lambda t: eng["rgb"].forward_u8_rgb(src.data_ptr(), t % 4, out["rgb"].data_ptr(), s),
            "overlay": lambda t: eng["overlay"].forward_u8_overlay(src.data_ptr(), t % 4, out["overlay"].data_ptr(), s),
            "copy": lambda t: dst.copy_(src)}
    kinds = ["labels", "rgb", "overlay", "copy"]

    def run(kind, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for t in range(n):
            call[kind](t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    for kind in kinds:                                                  # warm-up: the FIFOs reach their steady state, the streams are placed
        run(kind, 8)
    ms = {k: [] for k in kinds}
    for r in range(a.rounds):
        for kind in kinds[r % 4:] + kinds[:r % 4]:
            ms[kind].append(run(kind, a.frames))
    print("td4-psp18 %dx%d, %s source %dx%d (%d bytes), %d rounds of %d frames; device ms per frame" % (H, W, "NV12" if a.nv12 else "packed RGB", Hs, Ws, src.numel(), a.rounds, a.frames))
    med, spread = {}, {}
    for kind in kinds:
        v = np.array(ms[kind])
        med[kind], spread[kind] = float(np.median(v)), float(v.max() - v.min())
        print("%-8s %s  median %.4f  spread %.4f" % (kind, " ".join("%.4f" % x for x in v), med[kind], spread[kind]))
    diff, allow = med["overlay"] - med["rgb"], med["copy"] + spread["rgb"]
    print("overlay - rgb = %+.4f ms; allowed: copy %.4f + rgb spread %.4f = %.4f ms: %s" % (diff, med["copy"], spread["rgb"], allow, "WITHIN" if diff <= allow else "ABOVE"))
    print("rgb - labels = %+.4f ms (labels spread %.4f)" % (med["rgb"] - med["labels"], spread["labels"]))
    print("csv,%s,%dx%d,%dx%d,%s" % ("nv12" if a.nv12 else "rgb", H, W, Hs, Ws, ",".join("%s=%.4f/%.4f" % (k, med[k], spread[k]) for k in kinds)))


if __name__ == "__main__":
    main()
