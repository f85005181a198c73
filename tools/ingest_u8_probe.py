#!/usr/bin/env python3
"""GPU-box probe for the byte ends of a frame (csrc/td_ingest.h in, csrc/td_out.h out), to be run under `rocprofv3 --kernel-trace --stats` for the per-kernel times
(the ops themselves allocate and synchronise):

  ingest    the packed ingest (k_ingest<IngestPacked<3, false>>; before the byte ends were unified: k_ingest_u8) at HxW same-size and from --src-size, beside k_nchw3_to_rgbpad / k_nchw3_to_nhwc4 on an fp32 image of the same
            network size (tdnet_op_stem_image, both layouts)
  labels    k_upsample_argmax_u8 beside k_upsample_argmax on the same low-resolution logits (tdnet_op_upsample_argmax)

It also checks, at these sizes, that the byte path writes the same buffer and the same labels.

    rocprofv3 --kernel-trace --stats -d OUT -o r1 -- python tools/ingest_u8_probe.py [--size 1024x2048] [--src-size 1024x2048] [--iters 20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x2048", help="network size HxW")
    ap.add_argument("--src-size", default=None, help="source size HsxWs (default: the network size = the lookup-only branch)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nclass", type=int, default=19)
    a = ap.parse_args()
    import numpy as np
    import torch
    from tdnet_amd import _capi, arch
    from tdnet_amd.dataloader import cityscapesLoader, resize_linear_u8
    lib = _capi.test_lib()
    H, W = (int(v) for v in a.size.lower().split("x"))
    Hs, Ws = (int(v) for v in (a.src_size or a.size).lower().split("x"))
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    img = cityscapesLoader(img_path=os.devnull, in_size=(H, W)).normalise(resize_linear_u8(src, (W, H))).cuda()
    src_d = torch.from_numpy(src).cuda()
    for rows in (1, 0):
        n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))
        o32, o8 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_stem_image(img.data_ptr(), None, 0, 0, H, W, None, None, rows, o32.data_ptr(), n, s))
            lib.check(lib.tdnet_op_stem_image(None, src_d.data_ptr(), Hs, Ws, H, W, None, None, rows, o8.data_ptr(), n, s))
        same = torch.equal(o32.view(torch.int32), o8.view(torch.int32))
        print("ingest %dx%d -> %dx%d, %s: byte path == fp32 path: %s" % (Hs, Ws, H, W, "packed rows" if rows else "NHWC4", same))
        assert same
    h, w = arch.feat_size(H), arch.feat_size(W)
    x = torch.from_numpy(rng.standard_normal((a.nclass, h, w)).astype(np.float32)).cuda()
    l32 = torch.empty((H, W), dtype=torch.int32, device="cuda")
    l8 = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    for _ in range(a.iters):
        lib.check(lib.tdnet_op_upsample_argmax(x.data_ptr(), a.nclass, h, w, H, W, l32.data_ptr(), l8.data_ptr(), s))
    same = torch.equal(l8.to(torch.int32), l32)
    print("labels %dx%d -> %dx%d, %d classes: uint8 == int32: %s" % (h, w, H, W, a.nclass, same))
    assert same


if __name__ == "__main__":
    main()
