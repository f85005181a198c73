"""Colour maps out (include/tdnet.h "colour map out"), on the CPU through the kernel emulator: the C index tables against
dataloader.nearest_index, the fused upsample + argmax + palette kernel and the labels -> picture kernel against decode_segmap of the sampled label
map, whole frames asked for as pictures against the same frames asked for as labels, and the error paths.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import emu_util
import opcheck
import rgb_out_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import nearest_index
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


def c_table(lib, n, on):
    out = np.full(on, -7, np.int32)
    lib.check(lib.tdnet_op_nearest_index(n, on, out.ctypes.data))
    return out


def test_nearest_index_is_the_expression_it_replaced():
    for n, on in cases.TABLE_PAIRS:
        got = nearest_index(n, on)
        assert got.dtype == np.int64 and got.shape == (on,) and np.array_equal(got, cases.old_index(n, on)), (n, on)
        assert got.min() >= 0 and got.max() <= n - 1 and (np.diff(got) >= 0).all()


def test_c_tables_equal_nearest_index(lib):
    for n, on in cases.TABLE_PAIRS:
        assert np.array_equal(c_table(lib, n, on), nearest_index(n, on)), (n, on)
    for n in range(1, 41):
        for on in range(1, 41):
            assert np.array_equal(c_table(lib, n, on), nearest_index(n, on)), (n, on)
    with pytest.raises(_capi.TdnetError):
        lib.check(lib.tdnet_op_nearest_index(0, 4, np.zeros(4, np.int32).ctypes.data))


def labels_of(lib, x, C, h, w, H, W):
    l32 = np.full((H, W), -1, np.int32)
    lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
    assert l32.min() >= 0 and l32.max() < C
    return l32


@opcheck.guarded_arg("x", False)
def picture(lib, H, W, oh, ow, palette, off, x=None, C=0, h=0, w=0, labels_u8=None):
    """The picture written `off` bytes into a holder of 0xEE; the guard bytes around it must survive."""
    n = oh * ow * 3
    holder = np.full(n + 16, 0xEE, np.uint8)
    lib.check(lib.tdnet_op_upsample_argmax_rgb(None if x is None else x.ctypes.data, C, h, w, H, W, oh, ow, palette.ctypes.data, len(palette),
                                               holder.ctypes.data + off, None if labels_u8 is None else labels_u8.ctypes.data, None))
    assert (holder[:off] == 0xEE).all() and (holder[off + n:] == 0xEE).all(), (oh, ow, off)
    return holder[off:off + n].reshape(oh, ow, 3)


@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_fused_kernel_equals_labels_sampled_and_decoded(lib, name, C, lo, hi):
    (h, w), (H, W) = lo, hi
    x = cases.lowres_logits(name, C, h, w)
    labels = labels_of(lib, x, C, h, w, H, W)
    pal = cases.palette19()
    for oh, ow in cases.out_sizes(H, W):
        want = cases.expected_picture(labels, oh, ow)
        for off in range(4):
            assert np.array_equal(picture(lib, H, W, oh, ow, pal, off, x, C, h, w), want), (name, oh, ow, off)
    if name == "c256":                                                 # label 255 reaches the grey branch
        assert (picture(lib, H, W, H, W, pal, 0, x, C, h, w) == 255).all(axis=2).any()
    if name == "ties":                                                 # the lower index still wins: labels 4 and 3 at the planted pixels
        got = picture(lib, H, W, H, W, pal, 0, x, C, h, w)[::8, ::16]
        assert (got[[0, 1, 3, 4]] == pal[4]).all() and (got[2] == pal[3]).all()


def test_other_palettes_and_the_grey_branch(lib):
    name, C, (h, w), (H, W) = cases.ARGMAX_CASES[0]
    x = cases.lowres_logits(name, C, h, w)
    labels = labels_of(lib, x, C, h, w, H, W)
    p40 = np.ascontiguousarray(cases.palette40())
    for oh, ow in cases.out_sizes(H, W):
        for off in (0, 3):
            assert np.array_equal(picture(lib, H, W, oh, ow, p40, off, x, C, h, w), cases.expected_picture(labels, oh, ow, p40)), (oh, ow, off)
    x40 = cases.logits40(h, w)                                         # 40 classes against 19 colours: labels 19..39 are grey (l, l, l)
    l40 = labels_of(lib, x40, 40, h, w, H, W)
    assert (l40 >= 19).any()
    for oh, ow in cases.out_sizes(H, W):
        got = picture(lib, H, W, oh, ow, cases.palette19(), 1, x40, 40, h, w)
        assert np.array_equal(got, cases.expected_picture(l40, oh, ow)), (oh, ow)
    full = picture(lib, H, W, H, W, cases.palette19(), 0, x40, 40, h, w)
    grey = l40 >= 19
    assert (full[grey] == l40[grey][:, None]).all()
    one = np.array([[9, 8, 7]], np.uint8)                              # a one-colour palette: label 0 coloured, everything else grey
    assert np.array_equal(picture(lib, H, W, 7, 17, one, 2, x, C, h, w), cases.expected_picture(labels, 7, 17, one))


@pytest.mark.parametrize("name,C,lo,hi", [cases.ARGMAX_CASES[0], cases.ARGMAX_CASES[1], cases.ARGMAX_CASES[3]], ids=["odd_w", "w_mult_of_4", "c256"])
def test_labels_to_picture_kernel(lib, name, C, lo, hi):
    (h, w), (H, W) = lo, hi
    labels = labels_of(lib, cases.lowres_logits(name, C, h, w), C, h, w, H, W)
    l8 = np.ascontiguousarray(labels.astype(np.uint8))
    for pal in (cases.palette19(), np.ascontiguousarray(cases.palette40())):
        for oh, ow in cases.out_sizes(H, W):
            want = cases.expected_picture(labels, oh, ow, pal)
            for off in (0, 1):
                assert np.array_equal(picture(lib, H, W, oh, ow, pal, off, labels_u8=l8), want), (name, oh, ow, off)


def _engine(lib, model=4, H=33, W=65):
    name = {4: "td4", 2: "td2", 1: "psp"}[model]
    spec = arch.model_spec(name, 19, "resnet18")
    e = Engine(model, 18, 19, H, W, 0, lib=lib, arch={})
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


H, W, HS, WS, T = 33, 65, 41, 83, 6


def _size(t):
    return (H // 4, W // 4) if t % 2 == 0 else (7, 17)                # quarter size on even frames, an odd size on odd ones


@pytest.fixture(scope="module")
def clip(lib):
    """td4-resnet18 at 33x65 and six frames of random bytes at 41x83, with the labels forward_u8_labels gives for them on a handle of its own
    (computed once; the tests below run further handles on the same weights) and that handle's launch counts."""
    owner = _engine(lib, 4, H, W)
    owner.set_input_u8(HS, WS)
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, (HS, WS, 3), dtype=np.uint8) for _ in range(T)]
    labels, launches = [], []
    for t, src in enumerate(frames):
        l8 = np.full((H, W), 0xEE, np.uint8)
        owner.forward_u8_labels(src, t % 4, l8)
        labels.append(l8)
        launches.append(owner.last_launch_count())
    for a in frames + labels:
        a.setflags(write=False)
    yield owner, frames, labels, launches
    owner.close()


def test_frames_asked_for_as_pictures_equal_frames_asked_for_as_labels(clip):
    """forward_u8_rgb throughout on a second handle: every picture is decode_segmap of the sampled labels of the first, in as many launches.
    The size changes from frame to frame: a reconfiguration takes effect on the next frame."""
    owner, frames, labels, launches = clip
    a = owner.share()
    a.set_input_u8(HS, WS)
    pal = cases.palette19()
    with pytest.raises(_capi.TdnetError, match="tdnet_set_output_rgb"):   # a shared handle is unconfigured until it is configured itself
        a.forward_u8_rgb(frames[0], 0, np.zeros((8, 16, 3), np.uint8))
    assert a.fifo_len() == 0
    for t, src in enumerate(frames):
        oh, ow = _size(t)
        a.set_output_rgb(oh, ow, pal)
        a.set_output_rgb(oh, ow, pal)                                  # idempotent
        got = np.full((oh, ow, 3), 0xEE, np.uint8)
        a.forward_u8_rgb(src, t % 4, got)
        assert np.array_equal(got, cases.expected_picture(labels[t], oh, ow)), t
        assert a.last_launch_count() == launches[t] > 0, t
    assert a.fifo_len() == owner.fifo_len()
    a.close()


def test_picture_and_label_entries_mixed_on_one_handle(clip):
    """In turn forward_u8_rgb, forward_u8_labels (+ tdnet_labels_rgb of that map) and encode_u8 + propagate_rgb on ONE handle: the labels and
    pictures of the unmixed handles.  The FIFO does not care what left the frame."""
    owner, frames, labels, launches = clip
    c = owner.share()
    c.set_input_u8(HS, WS)
    pal = cases.palette19()
    for t, src in enumerate(frames):
        oh, ow = _size(t)
        c.set_output_rgb(oh, ow, pal)
        got = np.full((oh, ow, 3), 0xEE, np.uint8)
        if t % 3 == 0:
            c.forward_u8_rgb(src, t % 4, got)
            assert c.last_launch_count() == launches[t]
        elif t % 3 == 1:
            l8 = np.full((H, W), 0xEE, np.uint8)
            c.forward_u8_labels(src, t % 4, l8)
            assert np.array_equal(l8, labels[t]), t
            c.labels_rgb(l8, got)                                      # the picture of a label map the caller holds
        else:
            c.encode_u8(src, t % 4)
            c.propagate_rgb(got)
        assert np.array_equal(got, cases.expected_picture(labels[t], oh, ow)), t
    assert c.fifo_len() == owner.fifo_len()
    c.close()


def test_pspnet_and_fp32_frames_through_forward_rgb(lib):
    e = _engine(lib, 1, H, W)
    e.set_output_rgb(8, 16, cases.palette19())
    x = weights.synth_video(H, W, 1, seed=3)[0]
    l32 = np.full((H, W), -1, np.int32)
    e.forward_labels(x, 0, l32)
    n_labels = e.last_launch_count()
    got = np.full((8, 16, 3), 0xEE, np.uint8)
    e.forward_rgb(x, 0, got)
    assert np.array_equal(got, cases.expected_picture(l32, 8, 16)) and e.last_launch_count() == n_labels > 0
    e.close()


def test_errors_leave_the_fifo_and_a_pending_frame_alone(lib, clip):
    owner, frames, labels, launches = clip
    e = owner.share()
    pal = cases.palette19()
    x = np.zeros((1, 3, H, W), np.float32)
    pic, lab = np.zeros((8, 16, 3), np.uint8), np.zeros((H, W), np.uint8)
    e.set_input_u8(HS, WS)
    e.encode_u8(frames[0], 0)                                          # a pending frame: every failure below must leave it pending
    for call in (lambda: e.forward_rgb(x, 1, pic), lambda: e.forward_u8_rgb(frames[1], 1, pic), lambda: e.propagate_rgb(pic), lambda: e.labels_rgb(lab, pic)):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_output_rgb"):   # a frame call before the configuration
            call()
    for bad, match in (((0, 16, pal), "at least 1"), ((8, 0, pal), "at least 1"), ((8, 16, np.zeros((0, 3), np.uint8)), "n_colours"),
                       ((8, 16, np.zeros((257, 3), np.uint8)), "n_colours")):
        with pytest.raises(_capi.TdnetError, match=match):
            e.set_output_rgb(*bad)
    assert lib.tdnet_set_output_rgb(e.h, 8, 16, None, 19) < 0 and b"NULL" in lib.tdnet_last_error()   # a NULL palette
    with pytest.raises(_capi.TdnetError, match="tdnet_set_output_rgb"):   # a rejected configuration configures nothing
        e.propagate_rgb(pic)
    e.set_output_rgb(8, 16, pal)
    with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):   # the forward forms respect the pending frame like their siblings
        e.forward_u8_rgb(frames[1], 1, pic)
    assert e.fifo_len() == 0
    e.propagate_rgb(pic)                                               # ... which is still there, and is the frame it was
    assert e.fifo_len() == 1 and np.array_equal(pic, cases.expected_picture(labels[0], 8, 16))
    with pytest.raises(_capi.TdnetError, match="no encoded frame"):    # nothing encoded any more
        e.propagate_rgb(pic)
    assert e.fifo_len() == 1
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_output_rgb(8, 16, pal)
    fresh.close()
    e.close()


def test_model_classes_check_their_arguments():
    import torch
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    with pytest.raises(RuntimeError, match="uint8"):
        m.forward_rgb_u8(torch.zeros(1, 41, 83, 3), 0, (33, 65), (8, 16))
    with pytest.raises(RuntimeError, match="out_size"):
        m.forward_rgb_u8(torch.zeros(1, 41, 83, 3, dtype=torch.uint8), 0, (33, 65), (0, 16))
    with pytest.raises(_capi.TdnetError):                               # no CPU fallback
        m.forward_rgb(torch.zeros(1, 3, 33, 65), 0, (8, 16))
    with pytest.raises(_capi.TdnetError):
        m.forward_rgb_u8(torch.zeros(1, 41, 83, 3, dtype=torch.uint8), 0, (33, 65), (8, 16))
    with pytest.raises(RuntimeError, match="no encoded frame"):
        m.propagate(labels="rgb", out_size=(8, 16))
    assert m.engine is None
