#!/usr/bin/env python3
"""GPU-box probe for the regions output (csrc/td_regions.h; include/tdnet.h "regions out"): what do the seven region launches cost behind a frame,
and which of them is furthest from the bytes it has to move?  td4-psp18 fp32 on synthetic weights, frames resident on the device.

  loop      frames/s of three measurements, interleaved in one process (a a' r a a' r ..., one handle per form on one weight block, reset and
            `--warmup` frames before every round):
              (a), (a')  tdnet_forward_u8_labels, twice   -- the yardstick, and the noise actually seen between two measurements of the same thing
              (r)        tdnet_forward_u8_regions         -- labels + id map + table of Cityscapes train ids 11..18 (the "things"), 8 neighbours
            The entries are called on the engine with buffers allocated once: nothing is downloaded inside the timed window.
  unfused   tdnet_labels_regions alone on four label maps at the network size -- one class everywhere, the checkerboard of two member classes at 4
            neighbours, the 1-pixel spiral, seeded noise at 0.6 density -- HIP events around `--reps` calls: the seven launches together, per map.
            The bytes every launch must move (int32 maps read and written x H W x 4, the label bytes beside them) over STREAM_TBS give its floor.
  trace     (--trace MAP: the run to put under the profiler, nothing is timed by the script) `--reps` calls of tdnet_labels_regions on that one map
            (one | checker | spiral | noise), so that the kernel statistics are the per-launch times of that map:
                rocprofv3 --kernel-trace --stats -d OUT -o regions_MAP -- python tools/regions_probe.py --trace MAP
            and (--trace frame) 24 frames of tdnet_forward_u8_regions for the launches' times inside a frame.
  baseline  (--baseline: uses nothing this feature added, so the same file runs in a checkout of the parent commit) frames/s of
            tdnet_forward_u8_labels alone, `--rounds` rounds.

    timeout 600 python tools/regions_probe.py [--size 1024x2048] [--src-size 1080x1920] [--frames 48] [--warmup 8] [--rounds 3] [--reps 20]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

THINGS = tuple(range(11, 19))
MAX_REGIONS = 256
STREAM_TBS = 5.0                                                       # the bytes-once kernels of this tree stream at 4.2 - 7 TB/s
# int32 maps (read, written) and label-byte maps read per launch: K1 labels -> parent, area; K2 border pixels only; K3 parent -> root (+ area atomics);
# K4 root, area; K5 block counts; K6 root, area -> num; K7 root (+ num gathers) -> ids
FLOOR_MAPS = (("k_regions_tile", 0, 2, 1), ("k_regions_merge", 0, 0, 0), ("k_regions_flatten", 1, 1, 0), ("k_regions_count", 2, 0, 0), ("k_regions_scan", 0, 0, 0),
              ("k_regions_number", 2, 1, 0), ("k_regions_stats", 1, 1, 0))


def label_map(name, H, W):
    import regions_cases as cases
    if name == "noise":
        return cases.noise(H, W), (3, 7, 11), 8
    labels, classes = cases.pattern(name, H, W, 16, 64)
    return labels, classes, 4 if name == "checker" else 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x2048", help="network size HxW")
    ap.add_argument("--src-size", default="1080x1920", help="size of the decoded frames HsxWs")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", default=None, help="one | checker | spiral | noise | frame: the calls to put under rocprofv3 --kernel-trace --stats; nothing is timed here")
    ap.add_argument("--baseline", action="store_true", help="frames/s of the label entry only (runs in the parent commit's checkout too)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from tdnet_amd import arch, weights
    from tdnet_amd.model import td4_psp18
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in a.size.lower().split("x"))
    Hs, Ws = (int(v) for v in a.src_size.lower().split("x"))
    P, C, NF = 4, 19, 8
    rng = np.random.default_rng(0)
    srcs = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).to(dev) for _ in range(NF)]
    sd = weights.synth_state_dict(arch.model_spec("td4", C, "resnet18"), arch.feat_size(H), arch.feat_size(W), 0)
    owner = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev)
    owner.load_state_dict(sd)
    owner.ensure_engine(H, W, dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def shared():
        m = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev).share_weights_with(owner)
        with torch.no_grad():
            m.forward_labels_u8(srcs[0], pos_id=0, in_size=(H, W))     # creates the handle and configures its byte input
        return m

    lab = torch.zeros((H, W), dtype=torch.uint8, device=dev)

    def loop(call, m):
        m.reset()
        for t in range(a.warmup):
            call(t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(a.warmup, a.warmup + a.frames):
            call(t)
        torch.cuda.synchronize()
        return a.frames / (time.perf_counter() - t0)

    if a.baseline:
        m = shared()
        e = m.engine
        fps = [loop(lambda t: e.forward_u8_labels(srcs[t % NF].data_ptr(), t % P, lab.data_ptr(), s), m) for _ in range(a.rounds)]
        print("baseline %dx%d from %dx%d bytes, %d frames x %d rounds: forward_u8_labels frames/s %s   median %.1f"
              % (H, W, Hs, Ws, a.frames, a.rounds, " ".join("%.1f" % v for v in fps), statistics.median(fps)))
        return
    ids = torch.zeros((H, W), dtype=torch.int32, device=dev)
    table = torch.zeros((2 + 6 * MAX_REGIONS,), dtype=torch.int64, device=dev)
    if a.trace == "frame":
        m = shared()
        m.engine.set_regions(THINGS, 8, MAX_REGIONS, 1)
        for t in range(24):
            m.engine.forward_u8_regions(srcs[t % NF].data_ptr(), t % P, lab.data_ptr(), ids.data_ptr(), table.data_ptr(), s)
        torch.cuda.synchronize()
        print("trace: 24 frames of forward_u8_regions at %dx%d from %dx%d bytes" % (H, W, Hs, Ws))
        return
    from tdnet_amd.dataloader import region_table
    if a.trace:
        m = shared()
        labels, classes, conn = label_map(a.trace, H, W)
        dl = torch.from_numpy(np.array(labels)).to(dev)
        m.engine.set_regions(classes, conn, MAX_REGIONS, 1)
        for _ in range(a.reps):
            m.engine.labels_regions(dl.data_ptr(), ids.data_ptr(), table.data_ptr(), s)
        torch.cuda.synchronize()
        t = region_table(table.cpu().numpy(), MAX_REGIONS)
        print("trace: %d calls of labels_regions on the %s map at %dx%d, %d neighbours: %d regions, status %d" % (a.reps, a.trace, H, W, conn, t.count, t.status))
        return

    forms = ("a", "a'", "r")
    models = {f: shared() for f in forms}
    models["r"].engine.set_regions(THINGS, 8, MAX_REGIONS, 1)

    def frame(f):
        e = models[f].engine
        if f == "r":
            return lambda t: e.forward_u8_regions(srcs[t % NF].data_ptr(), t % P, lab.data_ptr(), ids.data_ptr(), table.data_ptr(), s)
        return lambda t: e.forward_u8_labels(srcs[t % NF].data_ptr(), t % P, lab.data_ptr(), s)

    fps = {f: [] for f in forms}
    for r in range(a.rounds):
        for f in forms:
            fps[f].append(loop(frame(f), models[f]))
    med = {f: statistics.median(fps[f]) for f in forms}
    t = region_table(table.cpu().numpy(), MAX_REGIONS)
    print("loop %dx%d from %dx%d bytes, td4-psp18 fp32, %d frames x %d rounds after %d warm-up frames: frames/s  (a) forward_u8_labels %.1f   (a') the same again %.1f (noise %.2f %%)"
          "   (r) forward_u8_regions %.1f (x%.3f of a): %+.1f us per frame   launches a/r %d/%d   last frame: %d regions, status %d"
          % (H, W, Hs, Ws, a.frames, a.rounds, a.warmup, med["a"], med["a'"], 100 * abs(med["a'"] - med["a"]) / med["a"], med["r"], med["r"] / med["a"],
             1e6 * (1 / med["r"] - 1 / med["a"]), models["a"].engine.last_launch_count(), models["r"].engine.last_launch_count(), t.count, t.status))
    for f in forms:
        print("    rounds (%s): %s" % (f, " ".join("%.1f" % v for v in fps[f])))

    e = models["r"].engine
    print("unfused %dx%d: labels_regions alone, HIP events around %d calls, the seven launches together per call" % (H, W, a.reps))
    for name in ("one", "checker", "spiral", "noise"):
        labels, classes, conn = label_map(name, H, W)
        dl = torch.from_numpy(np.array(labels)).to(dev)
        e.set_regions(classes, conn, MAX_REGIONS, 1)
        for _ in range(3):
            e.labels_regions(dl.data_ptr(), ids.data_ptr(), table.data_ptr(), s)
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                e.labels_regions(dl.data_ptr(), ids.data_ptr(), table.data_ptr(), s)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
        t = region_table(table.cpu().numpy(), MAX_REGIONS)
        print("    %-8s %d neighbours: %8d regions, status %d   %s us per call" % (name, conn, t.count, t.status, " / ".join("%.1f" % (1e3 * v) for v in ms)))
    print("floors %dx%d at %.1f TB/s: " % (H, W, STREAM_TBS) + "   ".join(
        "%s %.1f us" % (k, ((rd + wr) * 4 * H * W + by * H * W) / (STREAM_TBS * 1e12) * 1e6) for k, rd, wr, by in FLOOR_MAPS))
    for m in list(models.values()) + [owner]:
        m.engine.close()


if __name__ == "__main__":
    main()
