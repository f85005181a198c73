#!/usr/bin/env python3
"""GPU-box probe: ResNet layer1's 64 -> 64 3x3 conv on the direct kernel (k_conv_adirect), the unfused Winograd F(4x4) route (winograd = 4: input
transform, 36 GEMMs, output transform through HBM) and the fused kernel (k_wino4_f64, tdnet_bench_conv tile -2: at any map size), in one run.
TD_WINO_F64_MIN_PIXELS (td_wino_f64.h) is the smallest of these sizes at which the fused kernel beats the direct one by more than 5 %."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tdnet_amd import _capi
lib = _capi.test_lib(); torch.zeros(1, device="cuda")
WINO_F64 = 4194304
off = lib.opts().fusion & ~WINO_F64
for (H, W) in [(256, 512), (193, 385), (128, 256)]:
    gf = 2.0 * H * W * 64 * 64 * 9 / 1e9
    row = []
    for nm, o, tile in (("direct", lib.opts(fusion=off), -1), ("unfused F4", lib.opts(winograd=4, fusion=off), -1), ("fused F4", lib.opts(), -2)):
        ms = min(lib.tdnet_bench_conv(H, W, 64, 64, 3, 1, 1, tile, 20, ctypes.byref(o), None) for _ in range(5))
        if ms < 0:
            raise SystemExit(lib.tdnet_last_error().decode())
        row.append((nm, ms))
    d = row[0][1]
    print("64->64 3x3 @%dx%d (%6d px, %5.2f GFLOP direct)  " % (H, W, H * W, gf) +
          "   ".join("%s %6.1f us %5.1f TF-equivalent" % (nm, ms * 1e3, gf / ms) for nm, ms in row) + "   fused / direct %.3f" % (row[2][1] / d), flush=True)
