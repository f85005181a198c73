#!/usr/bin/env python3
"""GPU-box probe for destination views (csrc/td_out.h k_picture_rows into TD_DST_P24 / TD_DST_P32, k_picture_420; before the byte ends were unified: k_picture_packed / k_picture_nv12; include/tdnet.h "destination views").

Device milliseconds per steady-state td4-psp18 frame over an NV12 source, the variants interleaved in one process (one handle each, --rounds rounds of
--frames frames, the order rotating, HIP events around each round):
    rgb, overlay              the contiguous colour map (at the source's size) and overlay of THIS tree
    overlay_nv12              the overlay into a tight NV12 destination of the source's size
    overlay_bgra              the overlay into a tight BGRA32 destination
    parent_rgb, parent_overlay   with --parent-lib: the same two contiguous frames through a libtdnet_hip.so built from the parent commit
    copy                      a device-to-device copy of 3 Hs Ws bytes: a lower bound on any separate conversion pass behind a contiguous overlay
Per-round figures, medians and spreads (max - min), and the three statements of DESIGN.md 5.12:
    (a) rgb / overlay against parent_rgb / parent_overlay: within the parent's own spread (the old forms are unchanged instantiations)
    (b) overlay_nv12 <= parent_overlay + copy + spread      (c) overlay_bgra likewise
Without --parent-lib this tree's contiguous overlay stands in for the parent's in (b) and (c), and (a) is not stated.  --variants picks a subset: a
process with more than three handles (each owns a side stream and a second chain stream) can see one of them share a hardware queue with its own
chain and run at 4.1 instead of 2.4 ms a frame (td_frame.h place_chain_stream; seen here at 769x1537 with six handles), which says nothing about
the kernels -- so the recorded runs take at most three handles each.

    python tools/dest_view_probe.py --size 769x1537 --src-size 1080x1920 [--parent-lib PATH] [--variants overlay,parent_overlay,overlay_nv12] [--rounds 6] [--frames 40]
    rocprofv3 --kernel-trace --stats -d OUT -o r1 -- python tools/dest_view_probe.py --size 769x1537 --rounds 1   (the tail kernels' own times)"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parent_library(path):
    """A libtdnet_hip.so of another commit: the entry points it has, bound like _capi.Lib binds its own (it may lack the newest ones)."""
    import torch  # noqa: F401  (its HIP runtime first, as _capi.Lib does)
    from tdnet_amd import _capi
    lib = _capi.Lib.__new__(_capi.Lib)
    lib.path, lib.dll = path, ctypes.CDLL(path)
    for name, (res, args) in _capi.SYMBOLS.items():
        fn = getattr(lib.dll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
            setattr(lib, name, fn)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="769x1537", help="network size HxW")
    ap.add_argument("--src-size", default="1080x1920", help="NV12 source size HsxWs = the pictures' size")
    ap.add_argument("--parent-lib", default=None, help="libtdnet_hip.so built from the parent commit")
    ap.add_argument("--variants", default=None, help="comma-separated subset of rgb,overlay,overlay_nv12,overlay_bgra,parent_rgb,parent_overlay (copy always runs)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.lower().split("x"))
    Hs, Ws = (int(v) for v in a.src_size.lower().split("x"))
    import numpy as np
    import torch
    from tdnet_amd import arch, weights
    from tdnet_amd.dataloader import PIX_BGRA32, PIX_NV12, SourceView, cityscapesLoader, rgb_to_nv12, view_extent
    from tdnet_amd.engine import Engine
    spec = arch.model_spec("td4", 19, "resnet18")
    sd = weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0)
    want = a.variants.split(",") if a.variants else ["rgb", "overlay", "overlay_nv12", "overlay_bgra"] + (["parent_rgb", "parent_overlay"] if a.parent_lib else [])
    if any(k.startswith("parent_") for k in want) and not a.parent_lib:
        raise SystemExit("--variants names a parent_ variant: give --parent-lib")
    eng = {}
    for lib, names in ((None, [k for k in want if not k.startswith("parent_")]), (a.parent_lib, [k for k in want if k.startswith("parent_")])):
        for i, k in enumerate(names):                                   # one weight block per library, shared by its variants
            if i == 0:
                owner = Engine(4, 18, 19, H, W, torch.cuda.current_device(), lib=parent_library(lib) if lib else None)
                owner.load_state_dict(sd)
            eng[k] = owner if i == 0 else owner.share()
    surf = rgb_to_nv12(np.random.default_rng(0).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8))
    src = torch.from_numpy(surf).cuda()
    pal = np.array(cityscapesLoader.colors, np.uint8)
    pal4 = np.concatenate([pal, np.full((19, 1), 128, np.uint8)], axis=1)
    views = {"overlay_nv12": SourceView(PIX_NV12, Hs, Ws), "overlay_bgra": SourceView(PIX_BGRA32, Hs, Ws)}
    out = {}
    for k, e in eng.items():
        e.set_input_nv12(Hs, Ws, surf.shape[1])
        if k.endswith("rgb"):
            e.set_output_rgb(Hs, Ws, pal)
        else:
            e.set_output_overlay(pal4)
        if k in views:
            e.set_output_view(views[k])
        out[k] = torch.zeros(view_extent(views[k]) if k in views else Hs * Ws * 3, dtype=torch.uint8, device="cuda")
    cp_src, cp_dst = torch.zeros(Hs * Ws * 3, dtype=torch.uint8, device="cuda"), torch.zeros(Hs * Ws * 3, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = {k: ((lambda t, e=e, k=k: e.forward_u8_rgb(src.data_ptr(), t % 4, out[k].data_ptr(), s)) if k.endswith("rgb") else
                (lambda t, e=e, k=k: e.forward_u8_overlay(src.data_ptr(), t % 4, out[k].data_ptr(), s))) for k, e in eng.items()}
    call["copy"] = lambda t: cp_dst.copy_(cp_src)
    kinds = list(call)

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
    for k in ("rgb", "overlay"):                                        # the contiguous forms compute what the parent computes, byte for byte
        if k in out and "parent_" + k in out:
            assert torch.equal(out[k], out["parent_" + k]), "the contiguous %s differs from the parent's" % k
    ms = {k: [] for k in kinds}
    for r in range(a.rounds):
        o = r % len(kinds)
        for kind in kinds[o:] + kinds[:o]:
            ms[kind].append(run(kind, a.frames))
    print("td4-psp18 %dx%d, NV12 source %dx%d, pictures %dx%d, %d rounds of %d frames; device ms per frame" % (H, W, Hs, Ws, Hs, Ws, a.rounds, a.frames))
    med, spread = {}, {}
    for kind in kinds:
        v = np.array(ms[kind])
        med[kind], spread[kind] = float(np.median(v)), float(v.max() - v.min())
        print("%-15s %s  median %.4f  spread %.4f" % (kind, " ".join("%.4f" % x for x in v), med[kind], spread[kind]))
    base = "parent_overlay" if "parent_overlay" in med else "overlay"
    for k in ("rgb", "overlay"):
        if k in med and "parent_" + k in med:
            d = med[k] - med["parent_" + k]
            print("(a) %s - parent_%s = %+.4f ms; the parent's spread %.4f: %s" % (k, k, d, spread["parent_" + k], "WITHIN" if abs(d) <= spread["parent_" + k] else "OUTSIDE"))
    for tag, k in (("(b)", "overlay_nv12"), ("(c)", "overlay_bgra")):
        if k not in med or base not in med:
            continue
        allow = med[base] + med["copy"] + spread[base]
        print("%s %s = %.4f ms; %s %.4f + copy %.4f + spread %.4f = %.4f ms: %s" % (tag, k, med[k], base, med[base], med["copy"], spread[base], allow,
                                                                                 "WITHIN" if med[k] <= allow else "ABOVE"))
    print("csv,%dx%d,%dx%d,%s" % (H, W, Hs, Ws, ",".join("%s=%.4f/%.4f" % (k, med[k], spread[k]) for k in kinds)))


if __name__ == "__main__":
    main()
