#!/usr/bin/env python3
"""GPU-box probe for NV12 frames in (csrc/td_ingest.h k_ingest<IngestYuv<false, YuvFormNv12>>, in a build from before the byte ends were unified k_ingest_nv12; include/tdnet.h "NV12 frames in").

  --mode ingest   the NV12 ingest beside the packed one (k_ingest<IngestPacked<3, false>>; before: k_ingest_u8) on the same picture (tdnet_op_stem_image_nv12 / tdnet_op_stem_image, both layouts), and a
                  check that the two buffers are identical.  The ops allocate and synchronise: run it under
                  `rocprofv3 --kernel-trace --stats` for the per-kernel times.  --lib PATH loads another build's test library (e.g. the
                  parent commit's, for its packed ingest; the NV12 half is skipped when that library lacks the entry).
  --mode frames   whole td4-psp18 frames per second with NV12 surfaces against RGB bytes, interleaved in one process: two handles on one
                  weight block, --rounds rounds of --frames frames each, alternating; per-round rates, medians and the spread.

    rocprofv3 --kernel-trace --stats -d OUT -o r1 -- python tools/nv12_in_probe.py --mode ingest [--size 1024x2048] [--src-size 1080x1920]
    python tools/nv12_in_probe.py --mode frames [--size 1024x2048] [--src-size 1080x1920] [--rounds 6] [--frames 40]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ingest(a, H, W, Hs, Ws):
    import numpy as np
    import torch
    from tdnet_amd import _capi
    from tdnet_amd.dataloader import nv12_to_rgb_u8, rgb_to_nv12
    if a.lib:                                                          # another build: bind only the entries this probe calls
        import ctypes
        import types
        dll = ctypes.CDLL(a.lib)
        dll.tdnet_last_error.restype = ctypes.c_char_p

        def check(rc):
            if rc < 0:
                raise RuntimeError(dll.tdnet_last_error().decode())
            return rc
        lib = types.SimpleNamespace(check=check)
        has_nv12 = hasattr(dll, "tdnet_op_stem_image_nv12")
        for name in ("tdnet_op_stem_image",) + (("tdnet_op_stem_image_nv12",) if has_nv12 else ()):
            fn = getattr(dll, name)
            fn.restype, fn.argtypes = _capi.TEST_SYMBOLS[name]
            setattr(lib, name, fn)
    else:
        lib, has_nv12 = _capi.test_lib(), True
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    surf = rgb_to_nv12(rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8))
    pitch = surf.shape[1]
    rgb = nv12_to_rgb_u8(surf, Hs, Ws, pitch, Hs * pitch)
    surf_d, rgb_d = torch.from_numpy(surf).cuda(), torch.from_numpy(rgb).cuda()
    for rows in (1, 0):
        n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))
        o8, on = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_stem_image(None, rgb_d.data_ptr(), Hs, Ws, H, W, None, None, rows, o8.data_ptr(), n, s))
            if has_nv12:
                lib.check(lib.tdnet_op_stem_image_nv12(surf_d.data_ptr(), Hs, Ws, pitch, Hs * pitch, 0, H, W, None, None, rows, on.data_ptr(), n, s))
        if has_nv12:
            same = torch.equal(o8.view(torch.int32), on.view(torch.int32))
            print("ingest %dx%d (pitch %d) -> %dx%d, %s: NV12 path == RGB-byte path: %s" % (Hs, Ws, pitch, H, W, "packed rows" if rows else "NHWC4", same))
            assert same
        else:
            print("ingest %dx%d -> %dx%d, %s: RGB-byte path only (%s has no NV12 entry)" % (Hs, Ws, H, W, "packed rows" if rows else "NHWC4", a.lib))


def frames(a, H, W, Hs, Ws):
    import numpy as np
    import torch
    from tdnet_amd.dataloader import nv12_to_rgb_u8, rgb_to_nv12
    from tdnet_amd.model import td4_psp18
    m8 = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, synthetic_seed=0).eval().to("cuda")
    m8.ensure_engine(H, W, "cuda")
    mn = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, synthetic_seed=0).eval().to("cuda").share_weights_with(m8)
    rng = np.random.default_rng(0)
    surf = rgb_to_nv12(rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8))
    pitch = surf.shape[1]
    rgb_d = torch.from_numpy(nv12_to_rgb_u8(surf, Hs, Ws, pitch, Hs * pitch)[None]).cuda()
    surf_d = torch.from_numpy(surf[None]).cuda()

    def run(kind, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(n):
            if kind == "nv12":
                out = mn.forward_labels_nv12(surf_d, t % 4, (Hs, Ws), (H, W))
            else:
                out = m8.forward_labels_u8(rgb_d, t % 4, (H, W))
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), out
    with torch.no_grad():
        (_, l8), (_, ln) = run("u8", 8), run("nv12", 8)                # warm-up, and the same labels
        assert torch.equal(l8, ln)
        rates = {"u8": [], "nv12": []}
        for r in range(a.rounds):
            for kind in (("u8", "nv12") if r % 2 == 0 else ("nv12", "u8")):
                rates[kind].append(run(kind, a.frames)[0])
    for kind in ("u8", "nv12"):
        v = np.array(rates[kind])
        print("%-5s frames/s per round: %s  median %.1f  min %.1f  max %.1f" % (kind, " ".join("%.1f" % x for x in v), np.median(v), v.min(), v.max()))
    print("td4-psp18 %dx%d from %dx%d: NV12 / RGB-byte median ratio %.4f" % (H, W, Hs, Ws, np.median(rates["nv12"]) / np.median(rates["u8"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="ingest", choices=["ingest", "frames"])
    ap.add_argument("--size", default="1024x2048", help="network size HxW")
    ap.add_argument("--src-size", default=None, help="source size HsxWs (default: the network size = the lookup-only branch)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--lib", default=None, help="ingest mode: the test library of another build")
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.lower().split("x"))
    Hs, Ws = (int(v) for v in (a.src_size or a.size).lower().split("x"))
    (ingest if a.mode == "ingest" else frames)(a, H, W, Hs, Ws)


if __name__ == "__main__":
    main()
