#!/usr/bin/env python3
"""GPU-box probe for surfaces (csrc/td_ingest.h k_ingest<IngestYuv<WIDE, YuvFormArgs>>, csrc/td_out.h k_picture_420<.., YuvFormArgs>; include/tdnet.h "surfaces";
DESIGN.md 3.5 has the table of the names these kernels had before: k_ingest_surface, k_ingest_nv12, k_picture_surface, k_picture_nv12).

  --mode ingest    per input layout, --iters launches of the YUV ingest through tdnet_op_stem_image_surface (the packed-row stem image), and a check
                   that the buffer is the RGB-byte path's on the oracle's bytes.  The ops allocate and synchronise: run it under
                   `rocprofv3 --kernel-trace --stats`; the dispatches come in the order the probe prints, `--mode summarize` splits them per layout.
                   --lib PATH loads another build's test library (the parent commit's): its NV12 ingest on the NV12 surface only.
  --mode picture   the same for the four destination layouts: the fused colour map of 19 classes into a whole surface (k_picture_420 with YuvFormArgs; an NV12
                   surface with one pitch takes YuvFormNv12).  --lib PATH: the parent's NV12 picture kernel through tdnet_op_picture_view.
  --mode frames    whole td4-psp18 frames per second, forward_labels_u8(surface=...) per layout against forward_labels_nv12, alternating on two
                   handles of one weight block: --rounds rounds of --frames frames each; median (min .. max).
  --mode summarize --trace kernel_trace.csv [--plan FILE]: average / minimum per group of --iters consecutive dispatches of the probed kernels.

    rocprofv3 --kernel-trace --stats -d OUT -o r1 -- python tools/surface_probe.py --mode ingest [--size 1024x2048] [--src-size 1080x1920]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYOUTS = ("nv12", "nv21", "i420", "p010", "yuy2", "uyvy")
DST_LAYOUTS = ("nv12", "nv21", "i420", "p010")


def other_lib(path, names):
    """Another build's test library with only the entries this probe calls bound (the parent's lacks the surface entries)."""
    import ctypes
    import types
    from tdnet_amd import _capi
    dll = ctypes.CDLL(path)
    dll.tdnet_last_error.restype = ctypes.c_char_p

    def check(rc):
        if rc < 0:
            raise RuntimeError(dll.tdnet_last_error().decode())
        return rc
    lib = types.SimpleNamespace(check=check)
    for name in names:
        fn = getattr(dll, name)
        fn.restype, fn.argtypes = _capi.TEST_SYMBOLS[name]
        setattr(lib, name, fn)
    return lib


def tight(layout, H, W):
    """The surface a decoder of that layout hands over, no padding: interleaved chroma shares the luma pitch (even widths here)."""
    from tdnet_amd.dataloader import Surface
    return Surface(layout, H, W, standard=1)


def ingest(a, H, W, Hs, Ws):
    import numpy as np
    import torch
    from tdnet_amd import _capi
    from tdnet_amd.dataloader import pack_surface, surface_to_rgb_u8
    from tdnet_amd.engine import surface_struct
    import ctypes
    s = torch.cuda.current_stream().cuda_stream
    rgb0 = np.random.default_rng(0).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    if a.lib:
        lib = other_lib(a.lib, ("tdnet_op_stem_image", "tdnet_op_stem_image_nv12"))
        surf = tight("nv12", Hs, Ws)
        d = torch.from_numpy(pack_surface(rgb0, surf)).cuda()
        n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, 1, None, 0, None))
        out = torch.empty(n, device="cuda")
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_stem_image_nv12(d.data_ptr(), Hs, Ws, surf.row_pitch, surf.u_off, 1, H, W, None, None, 1, out.data_ptr(), n, s))
        print("plan: NV12 ingest x %d (%s), %dx%d -> %dx%d" % (a.iters, a.lib, Hs, Ws, H, W))
        return
    lib = _capi.test_lib()
    n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, 1, None, 0, None))
    for layout in LAYOUTS:
        surf = tight(layout, Hs, Ws)
        b = pack_surface(rgb0, surf)
        d, r = torch.from_numpy(b).cuda(), torch.from_numpy(surface_to_rgb_u8(b, surf)).cuda()
        o8, on = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        t = surface_struct(surf)
        lib.check(lib.tdnet_op_stem_image(None, r.data_ptr(), Hs, Ws, H, W, None, None, 1, o8.data_ptr(), n, s))
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_stem_image_surface(d.data_ptr(), ctypes.byref(t), H, W, None, None, 1, on.data_ptr(), n, s))
        same = torch.equal(o8.view(torch.int32), on.view(torch.int32))
        print("plan: YUV ingest x %d %s, %dx%d -> %dx%d: surface path == RGB-byte path: %s" % (a.iters, layout, Hs, Ws, H, W, same))
        assert same


def picture(a, H, W, Hs, Ws):
    import ctypes
    import numpy as np
    import torch
    from tdnet_amd import _capi
    from tdnet_amd.dataloader import PIX_NV12, SourceView, surface_extent
    from tdnet_amd.engine import surface_struct, view_struct
    s = torch.cuda.current_stream().cuda_stream
    C, h, w = 19, (H + 7) // 8, (W + 7) // 8
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((C, h, w)).astype(np.float32)).cuda()
    pal = np.ascontiguousarray(np.random.default_rng(2).integers(0, 256, (19, 3), dtype=np.uint8))
    if a.lib:
        lib = other_lib(a.lib, ("tdnet_op_picture_view",))
        v = SourceView(PIX_NV12, Hs, Ws, standard=1)
        tv = view_struct(v)
        dst = torch.zeros(Hs * Ws * 3 // 2, dtype=torch.uint8, device="cuda")
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_picture_view(x.data_ptr(), C, h, w, H, W, None, pal.ctypes.data, 19, None, None, Hs, Ws, dst.data_ptr(), ctypes.byref(tv), s))
        print("plan: k_picture_420 (NV12 form) x %d (%s), colour map %dx%d" % (a.iters, a.lib, Hs, Ws))
        return
    lib = _capi.test_lib()
    for layout in DST_LAYOUTS:
        surf = tight(layout, Hs, Ws)
        t = surface_struct(surf)
        dst = torch.zeros(surface_extent(surf), dtype=torch.uint8, device="cuda")
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_picture_surface(x.data_ptr(), C, h, w, H, W, None, pal.ctypes.data, 19, None, None, None, Hs, Ws, dst.data_ptr(), ctypes.byref(t), None, s))
        print("plan: %s x %d %s, colour map %dx%d" % ("k_picture_420 (NV12 form)" if layout == "nv12" else "k_picture_420", a.iters, layout, Hs, Ws))


def frames(a, H, W, Hs, Ws):
    import numpy as np
    import torch
    from tdnet_amd.dataloader import pack_surface
    from tdnet_amd.model import td4_psp18
    mn = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, synthetic_seed=0).eval().to("cuda")
    mn.ensure_engine(H, W, "cuda")
    ms = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, synthetic_seed=0).eval().to("cuda").share_weights_with(mn)
    rgb0 = np.random.default_rng(0).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    nv = tight("nv12", Hs, Ws)
    nv_d = torch.from_numpy(pack_surface(rgb0, nv).reshape(1, -1, nv.row_pitch)).cuda()

    def run(layout, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(n):
            if layout is None:
                out = mn.forward_labels_nv12(nv_d, t % 4, (Hs, Ws), (H, W), standard=1)
            else:
                out = ms.forward_labels_u8(surf_d, t % 4, (H, W), surface=surf)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), out
    with torch.no_grad():
        for layout in LAYOUTS:
            surf = tight(layout, Hs, Ws)
            surf_d = torch.from_numpy(pack_surface(rgb0, surf)[None]).cuda()
            (_, ln), (_, ls) = run(None, 8), run(layout, 8)              # warm-up; NV12 as a surface gives the NV12 entry's labels
            if layout == "nv12":
                assert torch.equal(ln, ls)
            rates = {"ref": [], "surf": []}
            for r in range(a.rounds):
                for kind in (("ref", "surf") if r % 2 == 0 else ("surf", "ref")):
                    rates[kind].append(run(None if kind == "ref" else layout, a.frames)[0])
            vr, vs = np.array(rates["ref"]), np.array(rates["surf"])
            print("td4-psp18 %dx%d from %dx%d  %-4s surface: median %.1f (%.1f .. %.1f) frames/s | forward_labels_nv12: median %.1f (%.1f .. %.1f) | ratio %.4f"
                  % (H, W, Hs, Ws, layout, np.median(vs), vs.min(), vs.max(), np.median(vr), vr.min(), vr.max(), np.median(vs) / np.median(vr)))


def summarize(a):
    """kernel_trace.csv of rocprofv3 -> per group of --iters consecutive dispatches of the probed kernels: average and minimum in microseconds."""
    import csv
    rows = []
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            # the YUV ingest and the 4:2:0 picture kernels, under their present names and those of a build from before the byte ends were unified
            if name.replace("void ", "").startswith(("k_ingest<IngestYuv<", "k_picture_420<", "k_ingest_surface", "k_ingest_nv12", "k_picture_surface", "k_picture_nv12")):
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    plan = [l.strip()[6:] for l in open(a.plan) if l.startswith("plan: ")] if a.plan else []
    for g in range(0, len(rows), a.iters):
        grp = rows[g:g + a.iters]
        us = [t for _, _, t in grp]
        print("%-34s n=%d  avg %.2f us  min %.2f us   %s" % (grp[0][1][:34], len(us), sum(us) / len(us), min(us), plan[g // a.iters] if g // a.iters < len(plan) else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="ingest", choices=["ingest", "picture", "frames", "summarize"])
    ap.add_argument("--size", default="1024x2048", help="network size HxW")
    ap.add_argument("--src-size", default=None, help="source (picture: destination) size HsxWs (default: the network size)")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--lib", default=None, help="ingest / picture: the test library of another build (the parent commit's)")
    ap.add_argument("--trace", default=None, help="summarize: rocprofv3's kernel_trace.csv")
    ap.add_argument("--plan", default=None, help="summarize: the probe's own output of that run (its `plan:` lines name the groups)")
    a = ap.parse_args()
    if a.mode == "summarize":
        return summarize(a)
    H, W = (int(v) for v in a.size.lower().split("x"))
    Hs, Ws = (int(v) for v in (a.src_size or a.size).lower().split("x"))
    {"ingest": ingest, "picture": picture, "frames": frames}[a.mode](a, H, W, Hs, Ws)


if __name__ == "__main__":
    main()
