#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REAL reference (imported read-only from /root/reference).

Runs only in the build container (the reference never travels to the GPU box).  The only modification made
to the reference objects is the one SURVEY.md §8c documents: `layer_normN` is re-created for the feature
size of the input, because the shipped modules hard-code LayerNorm([97,193]) (td4_psp18.py:107-110).

    python tools/make_golden.py            # writes tests/golden/
    python tools/make_golden.py --arch     # only the backbone-layout / class-count fixtures (ARCH_CASES) + the pspnet inventory
"""
import hashlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/Testing")

import torch  # noqa: E402
from model.pspnet import td4_psp18 as ref_td4, td2_psp50 as ref_td2, pspnet as ref_psp  # noqa: E402  (the reference itself)

from tdnet_amd import arch, weights  # noqa: E402

THREADS = 8
OUT = os.path.join(ROOT, "tests", "golden")


def build_reference(name, backbone, H, W, seed, nclass=19, dilated=True, multi_grid=True):
    spec = arch.model_spec(name, nclass, backbone, dilated, multi_grid)
    h, w = arch.feat_size(H, dilated), arch.feat_size(W, dilated)
    if name == "td4":
        m = ref_td4.td4_psp18(nclass=nclass, path_num=4, model_path=None, backbone=backbone, dilated=dilated, multi_grid=multi_grid)
        LN = ref_td4.Layer_Norm
    else:
        m = ref_td2.td2_psp50(nclass=nclass, path_num=2, model_path=None, backbone=backbone, dilated=dilated, multi_grid=multi_grid)
        LN = ref_td2.Layer_Norm
    for i in range(1, spec.path_num + 1):
        setattr(m, "layer_norm%d" % i, LN([h, w]))
    sd = weights.synth_state_dict(spec, h, w, seed)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)   # proves key/shape parity
    return spec, m.eval()


def run_traced(spec, m, frames):
    """Run the reference on `frames`, capturing stage outputs with forward hooks."""
    per_frame = []
    cur = {}

    def hook(tag):
        def f(mod, inp, out):
            cur.setdefault(tag, []).append(out)
        return f

    hs = []
    for p in range(1, spec.path_num + 1):
        hs.append(getattr(m, "pretrained%d" % p).register_forward_hook(hook("c4")))
        hs.append(getattr(m, "psp%d" % p).register_forward_hook(hook("z")))
        hs.append(getattr(m, "enc%d" % p).register_forward_hook(hook("enc")))
        hs.append(getattr(m, "layer_norm%d" % p).register_forward_hook(hook("ln")))
        hs.append(getattr(m, "head%d" % p).register_forward_hook(hook("lowres")))
    for names in spec.atn_names.values():
        for a in names:
            hs.append(getattr(m, a).register_forward_hook(hook("atn")))
    with torch.no_grad():
        for t, x in enumerate(frames):
            cur.clear()
            out = m(torch.from_numpy(x), pos_id=t % spec.path_num)
            rec = {"c4": cur["c4"][0], "z": cur["z"][0], "ln": cur["ln"][0], "lowres": cur["lowres"][0], "logits": out}
            (q_cur, v_cur), (cq, ck, cv) = cur["enc"]
            rec.update(q_cur=q_cur, v_cur=v_cur, cache_q=cq, cache_k=ck, cache_v=cv)
            if "atn" in cur:
                a = cur["atn"]
                rec["v4"] = a[-1]
                if len(a) == 3:
                    rec["v2"], rec["v3"] = a[0], a[1]
            per_frame.append({k: v.detach().numpy().copy() for k, v in rec.items()})
    for h in hs:
        h.remove()
    return per_frame


def psp_goldens(meta, digests):
    """Single-frame PSPNet-101 (pspnet.py): traced small case + full-size digest.  No LayerNorm, so nothing is patched."""
    spec = arch.model_spec("psp", 19, "resnet101")
    for H, W, full in [(33, 65, True), (769, 1537, False)]:
        sd = weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0)
        m = ref_psp.pspnet(nclass=19, model_path=None).eval()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        cur = {}
        hs = [m.pretrained.layer4.register_forward_hook(lambda mod, i, o: cur.__setitem__("c4", o)),
              m.head.conv5[0].register_forward_hook(lambda mod, i, o: cur.__setitem__("z", o)),
              m.head.register_forward_hook(lambda mod, i, o: cur.__setitem__("lowres", o))]
        x = weights.synth_video(H, W, 1, seed=1)[0]
        with torch.no_grad():
            out = m(torch.from_numpy(x), pos_id=0)
        for h in hs:
            h.remove()
        if full:
            arrs = {"f0_%s" % k: v.numpy().astype(np.float32) for k, v in cur.items()}
            arrs["f0_logits"] = out.numpy().astype(np.float32)
            fn = os.path.join(OUT, "psp_resnet101_%dx%d.npz" % (H, W))
            np.savez_compressed(fn, __meta__=np.array(meta), **arrs)
            print("wrote", fn, "%.1f MB" % (os.path.getsize(fn) / 1e6))
        else:
            o = out.numpy()
            tag = "psp_resnet101_%dx%d" % (H, W)
            digests[tag + "_last_frame"] = np.array(0)
            digests[tag + "_stats"] = np.array([o.min(), o.max(), o.mean(), np.sqrt((o.astype(np.float64) ** 2).sum())], dtype=np.float64)
            digests[tag + "_sample"] = o[0, :, ::61, ::67].astype(np.float32)
            digests[tag + "_labels_sample"] = o[0].argmax(0)[::61, ::67].astype(np.int16)
            print(tag, digests[tag + "_stats"])


# Backbone layouts and class counts beyond the shipped ones (the constructors' dilated / multi_grid / nclass; pspnet on ResNet-18 / 34).
# (name, backbone, H, W, T, nclass, dilated, multi_grid, kept frames): every frame's low-resolution logits; the full logits and c4 / z of the
# kept frames only (z only where d_model <= 512), so that each fixture stays under 1 MiB.
ARCH_CASES = [("td4", "resnet18", 33, 65, 8, 19, True, False, (0, 3, 7)),     # every path in steady state (t = 3..7 -> paths 3,0,1,2,3)
              ("td2", "resnet50", 33, 65, 4, 19, True, False, (3,)),
              ("td2", "resnet18", 65, 129, 4, 19, False, True, (3,)),         # output stride 32: 3 x 5 features
              ("td2", "resnet18", 33, 65, 3, 40, True, True, (2,)),           # NYUD-v2's 40 classes
              ("psp", "resnet18", 33, 65, 1, 19, True, True, (0,)),
              ("psp", "resnet34", 65, 129, 1, 19, False, True, (0,))]


def arch_tag(name, bb, H, W, nclass, dilated, multi_grid):
    return "%s_%s_%dx%d%s%s%s" % (name, bb, H, W, "" if dilated else "_nodil", "" if (multi_grid or not dilated) else "_nomg",
                                  "" if nclass == 19 else "_nc%d" % nclass)


def arch_goldens(meta, only=()):
    for name, bb, H, W, T, nc, dil, mg, keep in ARCH_CASES:
        tag = arch_tag(name, bb, H, W, nc, dil, mg)
        if only and tag not in only:
            continue
        frames = weights.synth_video(H, W, T, seed=1)
        arrs = {}
        if name == "psp":
            spec = arch.model_spec("psp", nc, bb, dil, mg)
            sd = weights.synth_state_dict(spec, arch.feat_size(H, dil), arch.feat_size(W, dil), 0)
            m = ref_psp.pspnet(nclass=nc, model_path=None, backbone=bb, dilated=dil, multi_grid=mg).eval()
            m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
            cur = {}
            hs = [m.pretrained.layer4.register_forward_hook(lambda mod, i, o: cur.__setitem__("c4", o)),
                  m.head.conv5[0].register_forward_hook(lambda mod, i, o: cur.__setitem__("z", o)),
                  m.head.register_forward_hook(lambda mod, i, o: cur.__setitem__("lowres", o))]
            with torch.no_grad():
                out = m(torch.from_numpy(frames[0]), pos_id=0)
            for h_ in hs:
                h_.remove()
            arrs.update({"f0_%s" % k: v.numpy().astype(np.float32) for k, v in cur.items()})
            arrs["f0_logits"] = out.numpy().astype(np.float32)
        else:
            spec, m = build_reference(name, bb, H, W, 0, nc, dil, mg)
            for t, r in enumerate(run_traced(spec, m, frames)):
                kept = ("logits", "c4") + (("z",) if spec.d_model <= 512 else ()) if t in keep else ()
                for k in ("lowres",) + kept:
                    arrs["f%d_%s" % (t, k)] = r[k].astype(np.float32)
        fn = os.path.join(OUT, tag + ".npz")
        np.savez_compressed(fn, __meta__=np.array(meta), **arrs)
        print("wrote", fn, "%.2f MB" % (os.path.getsize(fn) / 1e6))
    if not only or "psp_state_dict_inventory" in only:
        # name -> shape of the REAL pspnet state dicts on the BasicBlock backbones (the inventory arch.state_dict_shapes must reproduce)
        import json
        inv = {}
        for bb in ("resnet18", "resnet34"):
            m = ref_psp.pspnet(nclass=19, model_path=None, backbone=bb)
            inv[bb] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        fn = os.path.join(OUT, "psp_state_dict_inventory.json")
        with open(fn, "w") as f:
            json.dump(inv, f, indent=0)
        print("wrote", fn)


def main():
    torch.set_num_threads(THREADS)
    os.makedirs(OUT, exist_ok=True)
    meta = "torch %s, threads %d" % (torch.__version__, THREADS)
    if "--arch" in sys.argv:                                        # `make_golden.py --arch [tag ...]`: the backbone-layout / class-count fixtures only
        arch_goldens(meta, [a for a in sys.argv[1:] if not a.startswith("-")])
        return

    # ---- small, fully traced cases (every stage boundary) -------------------------------------------------
    # T: every path in steady state at least twice (td4: warm-up = frames 0..2, so T = 11 gives paths 3,0,1,2 | 3,0,1,2 at t = 3..10;
    # td2: warm-up = frame 0, T = 5 gives paths 1,0,1,0).  forward_path3 (atn3_4 -> atn3_1 -> atn3_2, td4_psp18.py:176-195) first
    # runs in steady state at t = 6.
    cases = [("td4", "resnet18", 33, 65, 11, True), ("td2", "resnet18", 33, 65, 5, True),
             ("td2", "resnet34", 33, 65, 5, False), ("td4", "resnet18", 65, 129, 11, False),
             ("td2", "resnet18", 49, 81, 5, False), ("td2", "resnet50", 33, 65, 5, True),
             ("td4", "resnet34", 33, 65, 11, False),            # td4_psp18.py:52-66 accepts resnet34 too
             ("td4", "resnet50", 33, 65, 7, False)]             # ... and resnet50 (d_model = d_v = 2048; constructible, never shipped)
    only = [a for a in sys.argv[1:] if not a.startswith("-")]       # e.g. `make_golden.py td4_resnet50_33x65`: just those small cases
    if only:
        cases = [c for c in cases if "%s_%s_%dx%d" % c[:4] in only]
    for name, bb, H, W, T, full in cases:
        spec, m = build_reference(name, bb, H, W, seed=0)
        frames = weights.synth_video(H, W, T, seed=1)
        rec = run_traced(spec, m, frames)
        arrs = {}
        for t, r in enumerate(rec):
            keep = r.keys() if full else ("lowres", "logits", "cache_k", "ln")
            for k in keep:
                if k in r:
                    arrs["f%d_%s" % (t, k)] = r[k].astype(np.float32)
        fn = os.path.join(OUT, "%s_%s_%dx%d.npz" % (name, bb, H, W))
        np.savez_compressed(fn, __meta__=np.array(meta), **arrs)
        print("wrote", fn, "%.1f MB" % (os.path.getsize(fn) / 1e6))

    if only:
        return
    # ---- full-size digests (statistics + strided samples only) --------------------------------------------
    digests = {}
    # per-frame digests (tag_f<t>_*) from the first steady-state frame on, so that every path's steady-state wiring is pinned at
    # full size too; the un-suffixed keys describe the last frame.
    for name, bb, H, W, T in [("td2", "resnet18", 512, 1024, 5), ("td4", "resnet18", 1024, 2048, 8),
                              ("td4", "resnet18", 769, 1537, 8), ("td2", "resnet34", 720, 960, 4),
                              ("td2", "resnet50", 769, 1537, 3), ("td2", "resnet18", 1024, 2048, 4)]:
        spec, m = build_reference(name, bb, H, W, seed=0)
        frames = weights.synth_video(H, W, T, seed=1)
        tag = "%s_%s_%dx%d" % (name, bb, H, W)
        with torch.no_grad():
            for t, x in enumerate(frames):
                out = m(torch.from_numpy(x), pos_id=t % spec.path_num).numpy()
                if t >= spec.fifo:
                    digests["%s_f%d_stats" % (tag, t)] = np.array([out.min(), out.max(), out.mean(), np.sqrt((out.astype(np.float64) ** 2).sum())], dtype=np.float64)
                    digests["%s_f%d_sample" % (tag, t)] = out[0, :, ::61, ::67].astype(np.float32)
                    digests["%s_f%d_labels_sample" % (tag, t)] = out[0].argmax(0)[::61, ::67].astype(np.int16)
        lab = out[0].argmax(0)
        top2 = np.sort(out[0], axis=0)[-2:]
        gap = top2[1] - top2[0]
        digests[tag + "_last_frame"] = np.array(T - 1)
        digests[tag + "_stats"] = np.array([out.min(), out.max(), out.mean(), np.sqrt((out.astype(np.float64) ** 2).sum())], dtype=np.float64)
        digests[tag + "_sample"] = out[0, :, ::61, ::67].astype(np.float32)
        digests[tag + "_labels_sample"] = lab[::61, ::67].astype(np.int16)
        digests[tag + "_gap_hist"] = np.array([(gap < 1e-4).sum(), (gap < 1e-3).sum(), gap.size], dtype=np.int64)
        digests[tag + "_label_sha256"] = np.array(hashlib.sha256(lab.astype(np.uint8).tobytes()).hexdigest())
        print(tag, digests[tag + "_stats"], digests[tag + "_gap_hist"])
    psp_goldens(meta, digests)
    fn = os.path.join(OUT, "fullsize_digests.npz")
    np.savez_compressed(fn, __meta__=np.array(meta), **digests)
    print("wrote", fn)
    arch_goldens(meta)


if __name__ == "__main__":
    main()
