#!/usr/bin/env python3
"""GPU-box probe: the refined matte's two launches (td_refine.h: k_refine_coeff, k_refine_apply) through tdnet_refine_matte at a 1024 x 2048 and a
1080 x 1920 source for r = 4, 8, 16.  Prints the time of the pair from events (the mean of REPS calls behind a warm-up) and, per launch, the bytes it must
move -- 2 in + 6 out per pixel for the coefficients, 7 in + 1 out for the apply -- so that a duration gives the HBM rate it implies.
The per-kernel durations come from a run of its own under the profiler, one configuration per run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/refine_probe.py --only 1080x1920,16
--only HxW,R: that configuration alone."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tdnet_amd import _capi
from tdnet_amd.engine import Engine

REPS = 50
ap = argparse.ArgumentParser()
ap.add_argument("--only", default=None, help="HxW,R")
args = ap.parse_args()
configs = [((1024, 2048), r) for r in (4, 8, 16)] + [((1080, 1920), r) for r in (4, 8, 16)]
if args.only:
    size, r = args.only.split(",")
    configs = [(tuple(int(v) for v in size.split("x")), int(r))]
lib = _capi.lib()
eng = Engine(2, 18, 19, 33, 65, 0, lib=lib)                            # the operator needs a handle for its device, nothing else
s = torch.cuda.current_stream().cuda_stream
for (h, w), r in configs:
    rng = np.random.default_rng(h + r)
    x = np.arange(w)[None, :]
    g = torch.from_numpy((100 + 40 * (x >= w // 2) + rng.integers(-3, 4, (h, w))).astype(np.uint8)).cuda()
    m = torch.from_numpy(np.clip((x - (w // 2 - 8)) * 16, 0, 255).astype(np.uint8).repeat(h, 0)).cuda()
    out = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    scratch = torch.empty((eng.refine_scratch_bytes(h, w) // 4,), dtype=torch.int32, device="cuda")
    call = lambda: eng.refine_matte(g.data_ptr(), w, m.data_ptr(), w, out.data_ptr(), w, h, w, r, 65, scratch.data_ptr(), s)
    for _ in range(5):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / REPS
    px = h * w
    print("refine %dx%d r=%2d: %7.1f us per call (2 launches, events, mean of %d);  must move: coeff %5.1f MB (2 in + 6 out / px), apply %5.1f MB (7 in + 1 out / px); "
          "both at this time: %6.1f GB/s" % (h, w, r, us, REPS, 8 * px / 1e6, 8 * px / 1e6, 16 * px / us / 1e3), flush=True)
eng.close()
