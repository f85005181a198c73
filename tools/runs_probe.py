#!/usr/bin/env python3
"""GPU-box probe for the runs output (csrc/td_runs.h; include/tdnet.h "runs out"): what do the coding launches cost on a map, beside the three launches of
the regions pipeline that do the same kind of work (k_regions_count / _scan / _number), and what does a frame with runs cost?  td4-psp18 fp32 on
synthetic weights, frames resident on the device, max_runs = H W.  Three maps at the network size: `frame` -- the labels of a steady-state frame of the
bench clip (weights.synth_video seed 100; synthetic weights: their labels are close to noise, the WORST case for a run-length code, not a street scene) --,
`constant` (H runs) and `alternating` (H W runs).

  default   per map: count, table bytes / map bytes, and HIP events around `--reps` calls of tdnet_labels_runs (count + scan + emit), of tdnet_runs_labels
            (decode) and of tdnet_labels_regions (all seven region launches, every class a member: the context of the per-launch figures below), three
            times each.  Then frames/s of three measurements interleaved in one process (a a' r a a' r ..., one handle per form on one weight block):
              (a), (a')  tdnet_forward_labels on the fp32 clip, twice   -- the yardstick, and the noise between two measurements of the same thing
              (r)        tdnet_forward_runs with the label map asked for
  trace     (--trace MAP: the run to put under the profiler; nothing is timed by the script) `--reps` calls each of tdnet_labels_runs, tdnet_runs_labels
            and tdnet_labels_regions on that one map, so that the kernel statistics hold k_runs_count / _scan / _emit / _decode and k_regions_count /
            _scan / _number of the SAME map from the SAME run:
                rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o runs_MAP -- python tools/runs_probe.py --trace MAP
            and (--trace frames) 24 frames of tdnet_forward_runs for the launches' times inside a frame.
  digest    (--digest CSV [CSV ...]) the k_runs_* and the three k_regions_* rows of such statistics files, in launch order, microseconds.  No device.
  baseline  (--baseline: uses nothing this feature added, so the same file runs in a checkout of the parent commit) frames/s of the label entry alone.

    timeout 600 python tools/runs_probe.py [--size 1024x2048] [--frames 48] [--warmup 8] [--rounds 3] [--reps 20]"""
import argparse
import csv
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAPS = ("frame", "constant", "alternating")
ROWS = ("k_runs_count", "k_runs_scan", "k_runs_emit", "k_runs_decode", "k_regions_count", "k_regions_scan", "k_regions_number")


def digest(paths):
    for p in paths:
        with open(p, newline="") as f:
            rows = list(csv.DictReader(f))
        print(os.path.basename(p))
        for key in ROWS:
            for r in rows:
                if key + "(" in r["Name"] or key + "<" in r["Name"]:
                    print("   %-46s n=%-4s avg %7.1f us  min %7.1f  max %7.1f" % (r["Name"][:46], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                                                                                 float(r["MaxNs"]) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x2048", help="network size HxW")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", default=None, help="frame | constant | alternating | frames: the calls to put under rocprofv3 --kernel-trace --stats; nothing is timed here")
    ap.add_argument("--digest", nargs="+", default=None, help="kernel statistics CSVs of --trace runs: print the runs and regions rows")
    ap.add_argument("--baseline", action="store_true", help="frames/s of the label entry only (runs in the parent commit's checkout too)")
    a = ap.parse_args()
    if a.digest:
        return digest(a.digest)
    import numpy as np
    import torch
    from tdnet_amd import arch, weights
    from tdnet_amd.model import td4_psp18
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in a.size.lower().split("x"))
    P, C, NF = 4, 19, 8
    clip = [torch.from_numpy(x).to(dev) for x in weights.synth_video(H, W, NF, seed=100)]   # bench.py's clip
    sd = weights.synth_state_dict(arch.model_spec("td4", C, "resnet18"), arch.feat_size(H), arch.feat_size(W), 0)
    owner = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev)
    owner.load_state_dict(sd)
    owner.ensure_engine(H, W, dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def shared():
        m = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev).share_weights_with(owner)
        with torch.no_grad():
            m.forward_labels(clip[0], pos_id=0)                        # creates the handle
        return m

    lab32 = torch.zeros((H, W), dtype=torch.int32, device=dev)
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
        fps = [loop(lambda t: e.forward_labels(clip[t % NF].data_ptr(), t % P, lab32.data_ptr(), s), m) for _ in range(a.rounds)]
        print("baseline %dx%d, %d frames x %d rounds: forward_labels frames/s %s   median %.1f" % (H, W, a.frames, a.rounds, " ".join("%.1f" % v for v in fps), statistics.median(fps)))
        return

    from tdnet_amd.dataloader import RUNS_HEADER_DTYPE
    MAXR = H * W
    table = torch.zeros((2 + MAXR + 1,), dtype=torch.int64, device=dev)
    back = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    ids = torch.zeros((H, W), dtype=torch.int32, device=dev)
    rtable = torch.zeros((2 + 6 * 256,), dtype=torch.int64, device=dev)
    if a.trace == "frames":
        m = shared()
        m.engine.set_runs(MAXR)
        for t in range(24):
            m.engine.forward_runs(clip[t % NF].data_ptr(), t % P, lab.data_ptr(), table.data_ptr(), s)
        torch.cuda.synchronize()
        print("trace: 24 frames of forward_runs at %dx%d" % (H, W))
        return

    def the_map(name, m):
        if name == "constant":
            return torch.full((H, W), 5, dtype=torch.uint8, device=dev)
        if name == "alternating":
            return (3 + 4 * (torch.arange(W, device=dev) % 2)).to(torch.uint8).repeat(H, 1).contiguous()
        m.reset()
        for t in range(2 * P + 1):                                     # a steady-state frame of the clip
            m.engine.forward_runs(clip[t % NF].data_ptr(), t % P, lab.data_ptr(), table.data_ptr(), s)
        torch.cuda.synchronize()
        return lab.clone()

    def header():
        return table[:2].cpu().numpy().view(RUNS_HEADER_DTYPE)[0]

    e_m = shared()
    e = e_m.engine
    e.set_runs(MAXR)
    e.set_regions(tuple(range(C)), 8, 256, 1)
    calls = {"labels_runs": lambda d: e.labels_runs(d.data_ptr(), table.data_ptr(), s), "runs_labels": lambda d: e.runs_labels(table.data_ptr(), 0, back.data_ptr(), s),
             "labels_regions": lambda d: e.labels_regions(d.data_ptr(), ids.data_ptr(), rtable.data_ptr(), s)}
    if a.trace:
        d = the_map(a.trace, e_m)
        for name in calls:
            for _ in range(a.reps):
                calls[name](d)
        torch.cuda.synchronize()
        assert torch.equal(back, d)
        print("trace: %d calls each of labels_runs, runs_labels and labels_regions on the %s map at %dx%d: %d runs" % (a.reps, a.trace, H, W, int(header()["count"])))
        return

    print("unfused %dx%d, max_runs = H W: HIP events around %d calls, three times; labels_runs = count + scan + emit, runs_labels = decode, labels_regions = all seven launches" % (H, W, a.reps))
    for name in MAPS:
        d = the_map(name, e_m)
        line = []
        for cname, call in calls.items():
            for _ in range(3):
                call(d)
            us = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call(d)
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / a.reps)
            line.append("%s %s us" % (cname, " / ".join("%.1f" % v for v in us)))
        assert torch.equal(back, d)
        count = int(header()["count"])
        nbytes = 16 + 8 * (count + 1)
        print("    %-11s %8d runs   table %9d bytes / map %d bytes = %.4f   %s" % (name, count, nbytes, H * W, nbytes / (H * W), "   ".join(line)))

    forms = ("a", "a'", "r")
    models = {f: shared() for f in forms}
    models["r"].engine.set_runs(MAXR)

    def frame(f):
        eng = models[f].engine
        if f == "r":
            return lambda t: eng.forward_runs(clip[t % NF].data_ptr(), t % P, lab.data_ptr(), table.data_ptr(), s)
        return lambda t: eng.forward_labels(clip[t % NF].data_ptr(), t % P, lab32.data_ptr(), s)

    fps = {f: [] for f in forms}
    for r in range(a.rounds):
        for f in forms:
            fps[f].append(loop(frame(f), models[f]))
    med = {f: statistics.median(fps[f]) for f in forms}
    print("loop %dx%d, td4-psp18 fp32, %d frames x %d rounds after %d warm-up frames: frames/s  (a) forward_labels %.1f   (a') the same again %.1f (noise %.2f %%)"
          "   (r) forward_runs %.1f (x%.3f of a): %+.1f us per frame   launches a/r %d/%d   last frame: %d runs"
          % (H, W, a.frames, a.rounds, a.warmup, med["a"], med["a'"], 100 * abs(med["a'"] - med["a"]) / med["a"], med["r"], med["r"] / med["a"],
             1e6 * (1 / med["r"] - 1 / med["a"]), models["a"].engine.last_launch_count(), models["r"].engine.last_launch_count(), int(header()["count"])))
    for f in forms:
        print("    rounds (%s): %s" % (f, " ".join("%.1f" % v for v in fps[f])))
    for m in list(models.values()) + [e_m, owner]:
        m.engine.close()


if __name__ == "__main__":
    main()
