#!/usr/bin/env python3
"""GPU-box probe for source views (include/tdnet.h "source views"): do the existing byte paths pay for the new ones?

Runs, through the test library's operator entries, the kernels an existing caller reaches -- the packed ingest (k_ingest<IngestPacked<3, false>>; a
build from before the byte ends were unified: k_ingest_u8) at 1024x2048 same-size, the NV12 ingest (k_ingest<IngestYuv<false, YuvFormNv12>>; k_ingest_nv12)
at 1080x1920 -> 769x1537, the fused overlay (k_picture_rows<false, TD_SRC_P24T, TD_DST_RGB>; k_upsample_argmax_overlay) over a 1080x1920 packed-RGB source (network 769x1537, 19 classes) -- --iters times each (--forms existing), or
the new forms for the record (--forms new, a run of its own so that their launches do not land in the same kernel's statistics): a BGRA32 crop (60, 0, 960, 1920) and an NV12 crop at the odd origin
(61, 1, 958, 1916) of a 1080x1920 frame -> 769x1537.  The ops allocate and synchronise: the times come from
`rocprofv3 --kernel-trace --stats`, in runs of their own.  --lib PATH loads another build's test library (the parent commit's).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/parent_1 -- python tools/source_view_probe.py --lib PARENT_TEST_LIB
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/new_1 -- python tools/source_view_probe.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/forms_1 -- python tools/source_view_probe.py --forms new
    python tools/source_view_probe.py --summarize OUT [--runs 3]"""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GATED = (("k_ingest_u8", "k_ingest_u8 1024x2048 same-size"), ("k_ingest_nv12", "k_ingest_nv12 1080x1920 -> 769x1537"),
         ("k_upsample_argmax_overlay", "k_upsample_argmax_overlay 1080x1920 packed RGB"))


def run(a):
    import ctypes
    import types
    import numpy as np
    import torch
    from tdnet_amd import _capi
    from tdnet_amd.dataloader import PIX_BGRA32, PIX_NV12, SourceView, pack_view, rgb_to_nv12
    from tdnet_amd.engine import view_struct
    if a.lib:
        dll = ctypes.CDLL(a.lib)
        dll.tdnet_last_error.restype = ctypes.c_char_p

        def check(rc):
            if rc < 0:
                raise RuntimeError(dll.tdnet_last_error().decode())
            return rc
        lib = types.SimpleNamespace(check=check)
        for name in ("tdnet_op_stem_image", "tdnet_op_stem_image_nv12", "tdnet_op_overlay", "tdnet_op_stem_image_view"):
            if hasattr(dll, name):
                fn = getattr(dll, name)
                fn.restype, fn.argtypes = _capi.TEST_SYMBOLS[name]
                setattr(lib, name, fn)
    else:
        lib = _capi.test_lib()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    rows = 1

    def buf(H, W):
        n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))
        return torch.empty(n, device="cuda"), n
    existing = a.forms == "existing"
    # 1. k_ingest_u8, 1024 x 2048 same-size
    H, W = 1024, 2048
    rgb = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    o, n = buf(H, W)
    for _ in range(a.iters if existing else 0):
        lib.check(lib.tdnet_op_stem_image(None, rgb.data_ptr(), H, W, H, W, None, None, rows, o.data_ptr(), n, s))
    # 2. k_ingest_nv12, 1080 x 1920 -> 769 x 1537
    Hs, Ws, H, W = 1080, 1920, 769, 1537
    frame = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    surf = rgb_to_nv12(frame)
    pitch = surf.shape[1]
    surf_d = torch.from_numpy(surf).cuda()
    o, n = buf(H, W)
    for _ in range(a.iters if existing else 0):
        lib.check(lib.tdnet_op_stem_image_nv12(surf_d.data_ptr(), Hs, Ws, pitch, Hs * pitch, 0, H, W, None, None, rows, o.data_ptr(), n, s))
    # 3. k_upsample_argmax_overlay over the 1080 x 1920 packed-RGB frame
    h, w, C = 97, 193, 19
    x = torch.from_numpy(rng.standard_normal((C, h, w)).astype(np.float32)).cuda()
    pal = np.ascontiguousarray(rng.integers(0, 256, (19, 4), dtype=np.uint8))
    src = torch.from_numpy(frame).cuda()
    out = torch.empty(Hs * Ws * 3, dtype=torch.uint8, device="cuda")
    for _ in range(a.iters if existing else 0):
        lib.check(lib.tdnet_op_overlay(x.data_ptr(), C, h, w, H, W, None, src.data_ptr(), 0, Hs, Ws, 0, 0, 0, pal.ctypes.data, 19, out.data_ptr(), s))
    # 4. the new forms, ungated: BGRA32 crop and NV12 crop at an odd origin
    if not existing:
        v = SourceView(PIX_BGRA32, Hs, Ws, pitch=Ws * 4 + 64, crop=(60, 0, 960, 1920))
        bgra = torch.from_numpy(pack_view(frame, v)).cuda()
        t = view_struct(v)
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_stem_image_view(bgra.data_ptr(), ctypes.byref(t), H, W, None, None, rows, o.data_ptr(), n, s))
        v = SourceView(PIX_NV12, Hs, Ws, pitch=pitch, crop=(61, 1, 958, 1916))
        t = view_struct(v)
        for _ in range(a.iters):
            lib.check(lib.tdnet_op_stem_image_view(surf_d.data_ptr(), ctypes.byref(t), H, W, None, None, rows, o.data_ptr(), n, s))
    torch.cuda.synchronize()
    print("source_view_probe: %d launches of each form done (%s)" % (a.iters, a.lib or "this build"))


def kernel_means(run_dir):
    """{kernel name: (calls, mean us)} of the one *kernel_stats.csv under run_dir."""
    files = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    assert len(files) == 1, (run_dir, files)
    with open(files[0]) as f:
        return {r["Name"]: (int(r["Calls"]), float(r["AverageNs"]) / 1000.0) for r in csv.DictReader(f)}


# a family's kernels since the byte ends became k_ingest<Reader> / k_picture_rows<LABELS, SRC, DST>: a run of a parent build still shows the names on the left
RENAMED = {"k_ingest_u8": "k_ingest<IngestPacked<", "k_ingest_nv12": "k_ingest<IngestYuv<false, YuvFormNv12>", "k_upsample_argmax_overlay": "k_picture_rows<false, 1, 0>"}   # TD_SRC_P24T into TD_DST_RGB: the one overlay form the probe times


def family(stats, key):
    """The one kernel of a family (the name up to its template list or argument list, or the family's present name) a run launched."""
    hits = [(k, v) for k, v in stats.items()
            if k.replace("void ", "").split("<")[0].split("(")[0] == key or k.replace("void ", "").replace("> >", ">>").startswith(RENAMED[key])]
    assert len(hits) == 1, (key, [k for k, _ in hits])
    return hits[0]


def summarize(out_dir, runs):
    """OUT/parent_i, OUT/new_i (--forms existing) and OUT/forms_i (--forms new), i = 1..runs.  Per gated kernel: each run's mean, the median of the runs
    and their spread (max - min); accepted when the new median is within the parent's own spread of the parent's median."""
    ok = True
    for key, title in GATED:
        med = {}
        for tag in ("parent", "new"):
            got = [family(kernel_means(os.path.join(out_dir, "%s_%d" % (tag, i))), key) for i in range(1, runs + 1)]
            us = [v[1] for _, v in got]
            med[tag] = (statistics.median(us), max(us) - min(us))
            print("%-52s %-6s %-34s calls %d  runs %s us  median %.2f  spread %.2f"
                  % (title, tag, got[0][0][:34], got[0][1][0], " ".join("%.2f" % u for u in us), med[tag][0], med[tag][1]))
        inside = abs(med["new"][0] - med["parent"][0]) <= med["parent"][1]
        ok = ok and inside
        print("%-52s new - parent %+.2f us against the parent's spread %.2f: %s" % ("", med["new"][0] - med["parent"][0], med["parent"][1], "inside" if inside else "OUTSIDE"))
    for key, title in (("k_ingest_u8", "BGRA32 crop (60,0,960,1920) of 1080x1920 -> 769x1537"), ("k_ingest_nv12", "NV12 crop (61,1,958,1916) of 1080x1920 -> 769x1537")):
        got = [family(kernel_means(os.path.join(out_dir, "forms_%d" % i)), key) for i in range(1, runs + 1)]
        us = [v[1] for _, v in got]
        print("%-52s new    %-34s calls %d  runs %s us  median %.2f  spread %.2f  (ungated)"
              % (title, got[0][0][:34], got[0][1][0], " ".join("%.2f" % u for u in us), statistics.median(us), max(us) - min(us)))
    print("accepted" if ok else "NOT accepted")
    return ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build's test library (the parent commit's)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--forms", default="existing", choices=("existing", "new"), help="the kernels an existing entry reaches, or the new view forms")
    ap.add_argument("--summarize", default=None, help="OUT: print the table of OUT/parent_i, OUT/new_i, OUT/forms_i")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.runs)
    else:
        run(a)
