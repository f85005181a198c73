#!/usr/bin/env python3
"""GPU-box probe for the tracks output (csrc/td_tracks.h; include/tdnet.h "tracks out"): what do the four tracking launches cost behind the regions
pipeline?  td4-psp18 fp32 on synthetic weights, label maps resident on the device.

  unfused   per case, HIP events around `--reps` calls of tdnet_labels_regions (R: the parent commit's entry, the yardstick) and of tdnet_labels_tracks (T)
            on the SAME label maps, interleaved R T R T ... `--rounds` times; the tracking launches cost T - R.  A case is a pair of maps fed in turn, so that
            every call has a previous frame to match against:
              frame    the labels the network gives for two consecutive frames of random bytes (Cityscapes train ids 11..18, the "things", 8 neighbours)
              noise    regions_cases.noise with two seeds (0.6 density, three classes): thousands of regions, thousands of distinct pairs
              checker  the checkerboard of two member classes at 4 neighbours with 65536 records: every stored region a pair of its own -- the most distinct
                       pairs a 1024x2048 frame can have (the table holds a pair per record at most)
              third    one region over a third of the frame, still: the hot slot -- every pixel of the region carries ONE key
              one      one region over the whole frame, still
            The bytes the four launches must move (two id maps read, one written, the pair table read once) over STREAM_TBS give the floor.
  trace     (--trace CASE: the run to put under the profiler, nothing is timed by the script) `--reps` calls of tdnet_labels_tracks on that case, so that
            the kernel statistics are the per-launch times of that case:
                rocprofv3 --kernel-trace --stats -d OUT -o tracks_CASE -- python tools/tracks_probe.py --trace CASE
  baseline  (--baseline: uses nothing this feature added, so the same file runs in a checkout of the parent commit) tdnet_labels_regions alone on the same
            cases.

    timeout 600 python tools/tracks_probe.py [--size 1024x2048] [--src-size 1080x1920] [--rounds 3] [--reps 20]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

THINGS = tuple(range(11, 19))
STREAM_TBS = 5.0                                                       # the bytes-once kernels of this tree stream at 4.2 - 7 TB/s
CASES = ("frame", "noise", "checker", "third", "one")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x2048", help="network size HxW")
    ap.add_argument("--src-size", default="1080x1920", help="size of the decoded frames HsxWs")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", default=None, help="|".join(CASES) + ": the calls to put under rocprofv3 --kernel-trace --stats; nothing is timed here")
    ap.add_argument("--baseline", action="store_true", help="labels_regions only (runs in the parent commit's checkout too)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import regions_cases
    from tdnet_amd import arch, weights
    from tdnet_amd.model import td4_psp18
    dev = torch.device("cuda", 0)
    H, W = (int(v) for v in a.size.lower().split("x"))
    Hs, Ws = (int(v) for v in a.src_size.lower().split("x"))
    P, C = 4, 19
    rng = np.random.default_rng(0)
    sd = weights.synth_state_dict(arch.model_spec("td4", C, "resnet18"), arch.feat_size(H), arch.feat_size(W), 0)
    m = td4_psp18.td4_psp18(nclass=C, path_num=P, model_path=None, backbone="resnet18").eval().to(dev)
    m.load_state_dict(sd)
    m.ensure_engine(H, W, dev)
    e = m.engine
    s = torch.cuda.current_stream(dev).cuda_stream

    def case(name):
        """(two label maps on the device, classes, connectivity, max_regions)"""
        yy, xx = np.mgrid[0:H, 0:W]
        if name == "frame":
            maps = []
            with torch.no_grad():
                for t in range(10):                                    # the last two frames of a short clip: the FIFO is full
                    u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).to(dev)
                    maps.append(m.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))[0].clone())
            return maps[-2:], THINGS, 8, 256
        if name == "noise":
            return [torch.from_numpy(regions_cases.noise(H, W, seed=k)).to(dev) for k in (0, 1)], (3, 7, 11), 8, 65536
        if name == "checker":
            return [torch.from_numpy(np.where((yy + xx) % 2 == 0, 3, 7).astype(np.uint8)).to(dev)] * 2, (3, 7), 4, 65536
        lab = np.full((H, W), 1, np.uint8)
        lab[:H // 3 if name == "third" else H] = 3
        return [torch.from_numpy(lab).to(dev)] * 2, (3,), 8, 256

    ids, tmap = (torch.zeros((H, W), dtype=torch.int32, device=dev) for _ in range(2))

    def tables(maxr):
        return torch.zeros((2 + 6 * maxr,), dtype=torch.int64, device=dev), torch.zeros((2 + 3 * maxr,), dtype=torch.int64, device=dev)

    def timed(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(reps):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps

    if a.trace:
        from tdnet_amd.dataloader import track_table
        maps, classes, conn, maxr = case(a.trace)
        rtab, ttab = tables(maxr)
        e.set_regions(classes, conn, maxr, 1)
        e.set_tracks(1)
        for k in range(a.reps):
            e.labels_tracks(maps[k % 2].data_ptr(), ids.data_ptr(), rtab.data_ptr(), tmap.data_ptr(), ttab.data_ptr(), s)
        torch.cuda.synchronize()
        t = track_table(ttab.cpu().numpy(), maxr)
        print("trace: %d calls of labels_tracks on the %s case at %dx%d, %d neighbours: %d regions with a record, matched %d, ended %d, status %d"
              % (a.reps, a.trace, H, W, conn, len(t), t.matched, t.ended, t.status))
        return

    print("unfused %dx%d: HIP events around %d calls, %d rounds interleaved; us per call" % (H, W, a.reps, a.rounds))
    for name in CASES:
        maps, classes, conn, maxr = case(name)
        rtab, ttab = tables(maxr)
        e.set_regions(classes, conn, maxr, 1)
        run_r = lambda k: e.labels_regions(maps[k % 2].data_ptr(), ids.data_ptr(), rtab.data_ptr(), s)
        if a.baseline:
            timed(run_r, 4)
            us = [timed(run_r, a.reps) for _ in range(a.rounds)]
            print("    %-8s labels_regions %s   median %.1f" % (name, " / ".join("%.1f" % v for v in us), statistics.median(us)))
            continue
        from tdnet_amd.dataloader import track_table
        e.set_tracks(1)
        run_t = lambda k: e.labels_tracks(maps[k % 2].data_ptr(), ids.data_ptr(), rtab.data_ptr(), tmap.data_ptr(), ttab.data_ptr(), s)
        timed(run_r, 4)
        timed(run_t, 4)
        r_us, t_us = [], []
        for _ in range(a.rounds):
            r_us.append(timed(run_r, a.reps))
            t_us.append(timed(run_t, a.reps))
        t = track_table(ttab.cpu().numpy(), maxr)
        mr, mt = statistics.median(r_us), statistics.median(t_us)
        print("    %-8s %d neighbours, %6d records: matched %6d ended %6d status %d   labels_regions %s   labels_tracks %s   tracking launches %+.1f us (medians %.1f -> %.1f)"
              % (name, conn, len(t), t.matched, t.ended, t.status, " / ".join("%.1f" % v for v in r_us), " / ".join("%.1f" % v for v in t_us), mt - mr, mr, mt))
    if not a.baseline:
        cap = 2
        while cap < 2 * H * W:
            cap *= 2
        print("floor %dx%d at %.1f TB/s: T1 two id maps read %.1f us   T2 the pair table (%d slots) read %.1f us   T4 one id map read, one (two with the track map) written %.1f us"
              % (H, W, STREAM_TBS, 8 * H * W / (STREAM_TBS * 1e12) * 1e6, cap, 8 * cap / (STREAM_TBS * 1e12) * 1e6, 12 * H * W / (STREAM_TBS * 1e12) * 1e6))
    e.close()


if __name__ == "__main__":
    main()
