"""Matte out on the MI355X: the operator tests of tests/test_emu_matte.py on device memory (plus rows wider than one workgroup's strip and the
real 769x1537 geometry), the composite over every source form and into every packed destination, whole frames through the model classes against
the label entries and the float64 softmax of forward_u8's logits, a batch of three, and a captured pos_id cycle that replays the class set of
capture time.  Labels, the exact properties and every composite are compared exactly; the matte bytes through the gate of tests/matte_cases.py."""
import numpy as np
import pytest
import torch

import matte_cases as cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import PIX_BGRA32, composite_u8, view_extent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


class DevMem:
    """The shared scenarios' memory (tests/matte_cases.py): torch tensors on the device, the current stream."""

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def up(self, a, off=0):
        flat = np.array(a, copy=True).view(np.uint8).reshape(-1)       # a writable copy: the cases' arrays are read-only
        holder = torch.full((flat.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        holder[off:off + flat.size] = torch.from_numpy(flat).cuda()
        return holder, holder.data_ptr() + off

    def get(self, buf):
        return buf.cpu().numpy()


MEM = DevMem()


def check_case(lib, key, x, C, h, w, H, W, offsets, set_names=None):
    """Both kernels of one geometry: every set through the gate, the exact properties, the labels at `offsets`, the label pointer NULL."""
    kx, px = MEM.up(x)
    full = torch.full((C, H, W), float("nan"), dtype=torch.float32, device="cuda")
    lib.check(lib.tdnet_op_upsample(px, C, h, w, H, W, full.data_ptr(), MEM.stream))
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    lib.check(lib.tdnet_op_upsample_argmax(px, C, h, w, H, W, l32.data_ptr(), None, MEM.stream))
    labels, fullh = l32.cpu().numpy(), full.cpu().numpy()
    assert labels.min() >= 0 and labels.max() < C
    kf, pf = MEM.up(fullh, 4)                                          # the unfused kernel's logits at a non-16-byte-aligned address
    # the logits as ARRAYS: matte_op puts them between guard bands, once per band fill (the 90 MB of the real geometry stay where they are)
    guarded_full = fullh if fullh.nbytes <= (8 << 20) else full.data_ptr()
    got = {}
    sets = {k: v for k, v in cases.class_sets(C).items() if set_names is None or k in set_names}
    for i, (sname, ids) in enumerate(sets.items()):
        want, near = cases.expected(fullh, ids, (key, sname))
        first = None
        for lab_off, mat_off in (offsets if i == 0 else cases.FEW_OFFSETS[i % 4:i % 4 + 1]):
            lab, mat = cases.matte_op(lib, MEM, C, H, W, ids, x, h, w, lab_off=lab_off, mat_off=mat_off)
            assert np.array_equal(lab, labels), (key, sname, lab_off, mat_off)
            cases.gate(mat, want, near, (key, sname, lab_off, mat_off))
            first = mat if first is None else first
            assert np.array_equal(mat, first), (key, sname, lab_off, mat_off)   # one byte per pixel whatever the offsets
        _, only = cases.matte_op(lib, MEM, C, H, W, ids, x, h, w, mat_off=3, want_labels=False)
        assert np.array_equal(only, first), (key, sname)
        got[sname] = first
        lab, umat = cases.matte_op(lib, MEM, C, H, W, ids, full=guarded_full, lab_off=(i + 1) & 3, mat_off=i & 3)
        assert np.array_equal(lab, labels), (key, sname)
        cases.gate(umat, want, near, (key, sname, "unfused"))
        d = np.abs(umat.astype(np.int64) - first)
        assert d.max() <= 1 and not (d != 0)[~near].any(), (key, sname)
        lab, umat2 = cases.matte_op(lib, MEM, C, H, W, ids, full=pf, mat_off=2)
        assert np.array_equal(lab, labels) and np.array_equal(umat2, umat), (key, sname)
        _, comp = cases.matte_op(lib, MEM, C, H, W, cases.complement(C, ids), px, h, w, mat_off=1, want_labels=False)
        assert np.abs(first.astype(np.int64) + comp - 255).max() <= 1, (key, sname)
    assert (got["every"] == 255).all() and (got["empty"] == 0).all()
    return got


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_both_kernels_every_set_labels_and_the_exact_properties(lib, case):
    name, C, (h, w), (H, W), scale = case
    got = check_case(lib, cases.case_id(case), cases.logits(name, C, h, w, scale), C, h, w, H, W, cases.offsets_of(name))
    if C == 256:
        assert got["high"].max() > 0 and got["with_255"].max() > 0     # the last membership word


@pytest.mark.parametrize("name,C,lo,hi", cases.WIDE_CASES, ids=[c[0] for c in cases.WIDE_CASES])
def test_wide_rows_and_the_real_geometry(lib, name, C, lo, hi):
    (h, w), (H, W) = lo, hi
    x = (np.random.default_rng(H + W).standard_normal((C, h, w)) * 6).astype(np.float32)
    check_case(lib, name, x, C, h, w, H, W, cases.FEW_OFFSETS[:2], set_names=("every", "empty", "moving"))


def test_non_finite_logits_leave_the_labels_alone(lib):
    name, C, (h, w), (H, W), scale = cases.CASES[0]
    x = cases.logits(name, C, h, w, scale).copy()
    x[3, 1, 2], x[7, 2, 5], x[0, 4, 8], x[5, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    kx, px = MEM.up(x)
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    lib.check(lib.tdnet_op_upsample_argmax(px, C, h, w, H, W, l32.data_ptr(), None, MEM.stream))
    full = torch.zeros((C, H, W), dtype=torch.float32, device="cuda")
    lib.check(lib.tdnet_op_upsample(px, C, h, w, H, W, full.data_ptr(), MEM.stream))
    assert not torch.isfinite(full).all()
    assert np.array_equal(cases.matte_op(lib, MEM, C, H, W, cases.MOVING, px, h, w, lab_off=1, mat_off=3)[0], l32.cpu().numpy())
    assert np.array_equal(cases.matte_op(lib, MEM, C, H, W, cases.MOVING, full=full.data_ptr(), lab_off=2, mat_off=1)[0], l32.cpu().numpy())


# ---- the composite, operator level ---------------------------------------------------------------------------------------------------------
_mattes = {}


def comp_inputs(lib):
    if not _mattes:
        keep, px = None, cases.logits("odd_w", 19, 5, 9, 6)          # the array: matte_op / op_composite put it between guard bands, once per band fill
        sets = {}
        for sname, ids in (("moving", cases.MOVING), ("every", tuple(range(19))), ("empty", ())):
            sets[sname] = (ids, cases.matte_op(lib, MEM, 19, 33, 65, ids, px, 5, 9, want_labels=False)[1])
        assert (sets["every"][1] == 255).all() and (sets["empty"][1] == 0).all()
        _mattes["v"] = (keep, px, sets)
    return _mattes["v"]


@pytest.mark.parametrize("kind", cases.SOURCE_KINDS)
def test_composite_into_the_block_over_every_source_form(lib, kind):
    keep, px, sets = comp_inputs(lib)
    for size in cases.SIZES.values():
        src = cases.comp_source(kind, size)
        cases.check_composite(lib, MEM, src, None, sets["moving"][1], cases.BG, px, sets["moving"][0], fills=(0xA5,), what=(size, kind))
    for sname in ("every", "empty"):                                   # M = 255 / 0: the source / the background, exactly
        cases.check_composite(lib, MEM, src, None, sets[sname][1], cases.BG, px, sets[sname][0], offsets=(1,), fills=(0xA5,), what=(kind, sname))


@pytest.mark.parametrize("kind", ("rgb24", "bgra32", "nv12", "p010"))
@pytest.mark.parametrize("dst", list(cases.PACKED))
def test_composite_into_every_packed_view_and_the_alpha_mode(lib, dst, kind):
    keep, px, sets = comp_inputs(lib)
    size = cases.SIZES["up_41x83"]
    src = cases.comp_source(kind, size)
    dview = cases.comp_dest(cases.PACKED[dst], size)
    for sname in ("moving", "every", "empty"):
        ids, m = sets[sname]
        offs = range(4) if sname == "moving" else (2,)
        cases.check_composite(lib, MEM, src, dview, m, cases.BG, px, ids, offsets=offs, what=(dst, kind, sname))
        if dst in ("rgba32", "bgra32"):
            cases.check_composite(lib, MEM, src, dview, m, None, px, ids, offsets=offs, fills=(0xA5,), what=(dst, kind, sname, "alpha"))


def test_composite_rows_wider_than_a_workgroups_strip(lib):
    """a 3 x 2051 source over the 33 x 65 network: more than one block per row"""
    keep, px, sets = comp_inputs(lib)
    ids, m = sets["moving"]
    for kind, dst in (("rgb24", None), ("nv12", "bgra32")):
        src = cases.comp_source(kind, (3, 2051))
        dview = None if dst is None else cases.comp_dest(cases.PACKED[dst], (3, 2051))
        cases.check_composite(lib, MEM, src, dview, m, cases.BG, px, ids, offsets=(0, 3), fills=(0xA5,), what=("wide", kind))


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
def make_model(name, kernel_opts=None):
    from tdnet_amd.model import td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0, kernel_opts=kernel_opts)
    else:
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0, kernel_opts=kernel_opts)
    return m.eval().to("cuda")


def _clip(n, Hs, Ws, seed, batch=1):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, 256, (batch, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(n)]


@pytest.mark.parametrize("name,opts", [("td4", None), ("td2", None), ("td4", {"precision": 1})], ids=["td4-psp18-fp32", "td2-psp18-fp32", "td4-psp18-fp16-mode"])
def test_frames_with_a_matte_and_composited_equal_the_label_entries_frames(name, opts):
    """A clip of 2 P + 1 frames at 65x129 from 80x161 bytes.  Model B: forward_labels_u8; L: forward_u8 (the logits of the float64 reference); A:
    forward_matte_u8 throughout; C mixes in turn the matte entry, the composite entry, encode_u8 + propagate(matte=True) and the unfused
    logits_matte of L's logits; D: encode_u8 + propagate(composite=True) and the alpha mode into a BGRA32 view."""
    H, W, Hs, Ws = 65, 129, 80, 161
    b = make_model(name, opts)
    b.ensure_engine(H, W, "cuda")
    lg, a, c, d = (make_model(name, opts).share_weights_with(b) for _ in range(4))
    P = b.path_num
    for m in (a, c, d):
        m.set_matte(cases.MOVING)
    dview = cases.comp_dest(PIX_BGRA32, (Hs, Ws))
    with torch.no_grad():
        for t, u in enumerate(_clip(2 * P + 1, Hs, Ws, 61)):
            l8 = b.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            full = lg.forward_u8(u, pos_id=t % P, in_size=(H, W))
            want, near = cases.expected(full[0].cpu().numpy(), cases.MOVING, (name, opts, t))
            la, ma = a.forward_matte_u8(u, t % P, (H, W))
            assert torch.equal(la, l8), t
            cases.gate(ma[0].cpu().numpy(), want, near, ("frame", t))
            assert a.engine.last_launch_count() == b.engine.last_launch_count() > 0, t
            src, mh = u[0].cpu().numpy(), ma[0].cpu().numpy()
            pic = composite_u8(src, mh, H, W, cases.BG)
            if t % 4 == 0:
                lc, mc = c.forward_matte_u8(u, t % P, (H, W))
                assert c.engine.last_launch_count() == b.engine.last_launch_count()
            elif t % 4 == 1:
                out = c.forward_composite_u8(u, t % P, (H, W), background=cases.BG)
                assert c.engine.last_launch_count() == b.engine.last_launch_count()
                assert np.array_equal(out[0].cpu().numpy(), pic), t
                lc, mc = l8, ma
            elif t % 4 == 2:
                c.encode_u8(u, t % P, in_size=(H, W))
                lc, mc = c.propagate(matte=True)
            else:
                c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
                lc, mc = c.logits_matte(full)                          # the unfused form: within 1 at near-boundary pixels only
                dd = (mc.int() - ma.int()).abs()[0].cpu().numpy()
                assert dd.max() <= 1 and not (dd != 0)[~near].any(), t
                cases.gate(mc[0].cpu().numpy(), want, near, ("unfused frame", t))
                mc = ma
            assert torch.equal(lc, l8) and torch.equal(mc, ma), t      # bit-identical: the FIFO does not care what left the frame
            if t % 2 == 0:
                d.encode_u8(u, t % P, in_size=(H, W))
                out = d.propagate(composite=True, src=u, background=cases.BG)
                assert np.array_equal(out[0].cpu().numpy(), pic), t
            else:
                prefill = np.full(view_extent(dview), 0xA5, np.uint8)
                dst = torch.from_numpy(prefill.copy())[None].cuda()
                d.forward_composite_u8(u, t % P, (H, W), background=None, out_view=dview, out=dst)
                assert d.engine.last_launch_count() == b.engine.last_launch_count()
                rgba = composite_u8(src, mh, H, W, None)
                assert np.array_equal(dst[0].cpu().numpy(), cases.expected_dest(prefill, dview, np.ascontiguousarray(rgba[..., :3]), rgba[..., 3])), t
    assert a.engine.fifo_len() == b.engine.fifo_len() == c.engine.fifo_len() == d.engine.fifo_len()


def test_a_batch_of_three_and_a_set_per_handle():
    H, W, Hs, Ws = 65, 129, 80, 161
    b = make_model("td2")
    b.ensure_engine(H, W, "cuda")
    a, lg = make_model("td2").share_weights_with(b), make_model("td2").share_weights_with(b)
    a.set_matte(cases.MOVING)                                          # before the batch's handles exist: applies to those created later
    with torch.no_grad():
        for t, u in enumerate(_clip(3, Hs, Ws, 62, batch=3)):
            l8 = b.forward_labels_u8(u, pos_id=t % 2, in_size=(H, W))
            full = lg.forward_u8(u, pos_id=t % 2, in_size=(H, W)).cpu().numpy()
            la, ma = a.forward_matte_u8(u, t % 2, (H, W))
            assert la.shape == ma.shape == (3, H, W) and torch.equal(la, l8)
            for i in range(3):
                want, near = cases.expected(full[i], cases.MOVING, ("batch", t, i))
                cases.gate(ma[i].cpu().numpy(), want, near, ("batch", t, i))
            out = a.forward_composite_u8(u, t % 2, (H, W), background=cases.BG) if t == 2 else None
        assert len([a.engine] + list(a._extra_engines)) == 3
        # the set is per handle: another one on the first handle alone
        e0, e1 = a.engine, a._extra_engines[0]
        e0.set_matte(range(19))
        m0, m1 = (torch.full((H, W), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
        s = torch.cuda.current_stream().cuda_stream
        lgt = torch.from_numpy(full[0]).cuda()
        e0.logits_matte(lgt.data_ptr(), None, m0.data_ptr(), s)
        e1.logits_matte(lgt.data_ptr(), None, m1.data_ptr(), s)
        torch.cuda.synchronize()
        assert (m0 == 255).all() and not (m1 == 255).all()
        assert out.shape == (3, Hs, Ws, 3)


def test_errors_name_their_entry_and_leave_a_pending_frame_alone():
    H, W, Hs, Ws = 33, 65, 41, 83
    m, ref = make_model("td2"), make_model("td2")
    u = _clip(2, Hs, Ws, 63)
    with torch.no_grad():
        m.encode_u8(u[0], 0, in_size=(H, W))
        e = m.engine
        lab, mat = (torch.full((H, W), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
        out = torch.full((Hs, Ws, 3), 0xEE, dtype=torch.uint8, device="cuda")
        for name, call in (("tdnet_forward_u8_matte", lambda: e.forward_u8_matte(u[1].data_ptr(), 1, lab.data_ptr(), mat.data_ptr())),
                           ("tdnet_propagate_matte", lambda: e.propagate_matte(lab.data_ptr(), mat.data_ptr())),
                           ("tdnet_propagate_composite", lambda: e.propagate_composite(u[0].data_ptr(), out.data_ptr()))):
            with pytest.raises(_capi.TdnetError, match=name + ".*tdnet_set_matte"):
                call()
        e.set_matte(cases.MOVING)
        with pytest.raises(_capi.TdnetError, match="tdnet_propagate_composite.*tdnet_set_output_composite"):
            e.propagate_composite(u[0].data_ptr(), out.data_ptr())
        with pytest.raises(_capi.TdnetError, match="tdnet_set_matte"):
            e.set_matte((19,))
        with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_matte.*waiting for tdnet_propagate"):
            e.forward_u8_matte(u[1].data_ptr(), 1, lab.data_ptr(), mat.data_ptr())
        torch.cuda.synchronize()
        assert (lab == 0xEE).all() and (mat == 0xEE).all() and (out == 0xEE).all()
        m.set_matte(cases.MOVING)
        ref.set_matte(cases.MOVING)
        got, gm = m.propagate(matte=True)                              # the pending frame is still there, and is the frame it was
        want, wm = ref.forward_matte_u8(u[0], 0, (H, W))
        assert torch.equal(got, want) and torch.equal(gm, wm)
        with pytest.raises(_capi.TdnetError, match="no encoded frame"):
            e.propagate_matte(lab.data_ptr(), mat.data_ptr())


def test_a_captured_cycle_replays_the_class_set_of_capture_time():
    """One pos_id cycle of forward_matte_u8 at 65x129 captured into a hipGraph (tdnet_warmup before the capture) and replayed twice: labels and
    matte of the eager loop.  The set is kernel arguments: the graph keeps the one in force when it was captured."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    warm = 2 * P
    T = warm + cycles * P
    clip = _clip(T, Hs, Ws, 64)
    with torch.no_grad():
        m = make_model("td4")
        m.set_matte(cases.MOVING)
        eager = [tuple(o.clone() for o in m.forward_matte_u8(clip[t], t % P, (H, W))) for t in range(T)]
        assert any(0 < mm.float().mean() < 255 for _, mm in eager)
        m.reset()
        for t in range(warm):
            l, mm = m.forward_matte_u8(clip[t], t % P, (H, W))
            assert torch.equal(l, eager[t][0]) and torch.equal(mm, eager[t][1])
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        m.engine.warmup(stream.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = [m.forward_matte_u8(xin[j], j, (H, W)) for j in range(P)]
        m.set_matte(())                                                # after the capture: the replays do not see it
        m.engine.set_matte(())
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            graph.replay()
            torch.cuda.synchronize()
            for j in range(P):
                assert torch.equal(outs[j][0], eager[t0 + j][0]) and torch.equal(outs[j][1], eager[t0 + j][1]), (c, j)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _cli(tmp_path, name, extra):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / name
    out.mkdir()
    return out, subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0",
                                "--in_size", "65x129"] + extra, cwd=root, capture_output=True, text=True, timeout=120)


def _cli_frames(tmp_path, n=3):
    from PIL import Image
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(17)
    frames = [rng.integers(0, 256, (80, 161, 3), dtype=np.uint8) for _ in range(n)]
    for t, f in enumerate(frames):
        Image.fromarray(f).save(frames_dir / ("frame_%06d.png" % t))
    return frames


IDS = ",".join(str(c) for c in cases.MOVING)


def test_cli_matte_out_writes_the_matte_the_model_class_gives(tmp_path):
    """Three random 80x161 frames, --in_size 65x129, with --u8 and without: `--matte IDS --matte_out DIR` saves the matte of the model class for the same
    frames as an 8-bit PNG beside the usual quarter-size picture; the switches check their arguments before anything is loaded."""
    from PIL import Image
    from tdnet_amd.dataloader import cityscapesLoader, nearest_index
    frames = _cli_frames(tmp_path)
    H, W = 65, 129
    for extra, match in ((["--matte", "11,19", "--matte_out", "x"], "0..18"), (["--matte", IDS, "--composite", "1,2,3"], "--u8, --nv12 or --yuv"),
                         (["--u8", "--matte", IDS, "--matte_out", "x", "--rgb"], "not with --rgb")):
        out, r = _cli(tmp_path, "bad%d" % len(list(tmp_path.iterdir())), extra)
        assert r.returncode != 0 and match in r.stderr, r.stdout + r.stderr
    for u8 in (True, False):
        ld = cityscapesLoader(img_path=str(tmp_path / "data"), in_size=(H, W), as_uint8=u8)
        ld.load_frames()
        m = make_model("td4")
        m.set_matte(cases.MOVING)
        mdir = tmp_path / ("matte_%d" % u8)
        out, r = _cli(tmp_path, "out_%d" % u8, ["--matte", IDS, "--matte_out", str(mdir)] + (["--u8"] if u8 else []))
        assert r.returncode == 0, r.stdout + r.stderr
        with torch.no_grad():
            for t, item in enumerate(ld.data):
                img = item[0].cuda()
                l, mm = m.forward_matte_u8(img, t % 4, (H, W)) if u8 else m.forward_matte(img, t % 4)
                name = "frame_%06d.png" % t
                got = np.array(Image.open(mdir / "vid1" / name))
                assert got.dtype == np.uint8 and np.array_equal(got, mm[0].cpu().numpy()), (u8, t)
                ys, xs = nearest_index(H, item[3][1] // 4), nearest_index(W, item[3][0] // 4)
                small = l[0].cpu().numpy().astype(np.int8)[ys][:, xs]
                assert np.array_equal(np.array(Image.open(out / "vid1" / name)), ld.decode_segmap(small).astype(np.uint8)), (u8, t)
        assert len(frames) == len(ld.data)


def test_cli_composite_writes_the_frame_through_its_matte(tmp_path):
    """`--u8 --matte IDS --composite R,G,B`: the source-size picture is dataloader.composite_u8 of the frame and the model class's matte bytes; the NV12 and
    the --yuv routes write what the model class gives for the same surfaces."""
    from PIL import Image
    from tdnet_amd.dataloader import PIX_NV12, SourceView, cityscapesLoader, view_to_rgb_u8
    frames = _cli_frames(tmp_path)
    H, W, bg = 65, 129, cases.BG
    out, r = _cli(tmp_path, "u8", ["--u8", "--matte", IDS, "--composite", ",".join(str(v) for v in bg)])
    assert r.returncode == 0, r.stdout + r.stderr
    m = make_model("td4")
    m.set_matte(cases.MOVING)
    with torch.no_grad():
        for t, f in enumerate(frames):
            _, mm = m.forward_matte_u8(torch.from_numpy(f[None]).cuda(), t % 4, (H, W))
            got = np.asarray(Image.open(out / "vid1" / ("frame_%06d.png" % t)))
            assert got.shape == (80, 161, 3) and np.array_equal(got, composite_u8(f, mm[0].cpu().numpy(), H, W, bg)), t
    out, r = _cli(tmp_path, "nv12", ["--nv12", "--nv12_standard", "1", "--matte", IDS, "--composite", ",".join(str(v) for v in bg)])
    assert r.returncode == 0, r.stdout + r.stderr
    ld = cityscapesLoader(img_path=str(tmp_path / "data"), in_size=(H, W), as_nv12=True, nv12_standard=1)
    ld.load_frames()
    n = make_model("td4")
    n.set_matte(cases.MOVING)
    with torch.no_grad():
        for t, item in enumerate(ld.data):
            surf, (Hs, Ws) = item[0], item[4]
            view = SourceView(PIX_NV12, Hs, Ws, pitch=int(surf.shape[2]), standard=1)
            whole = surf.reshape(1, -1).cuda()
            _, mm = n.forward_matte_u8(whole, t % 4, (H, W), view=view)
            rgb = view_to_rgb_u8(surf[0].numpy().reshape(-1), view)
            got = np.asarray(Image.open(out / "vid1" / ("frame_%06d.png" % t)))
            assert got.shape == (80, 161, 3) and np.array_equal(got, composite_u8(rgb, mm[0].cpu().numpy(), H, W, bg)), t
    out, r = _cli(tmp_path, "yuv", ["--yuv", "i420", "--matte", IDS, "--composite", "0,0,0"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.asarray(Image.open(out / "vid1" / "frame_000002.png")).shape == (80, 161, 3)
