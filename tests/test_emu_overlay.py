"""Overlay out (include/tdnet.h "overlay out") on the CPU: the host oracle pinned by hand, then through the kernel emulator the fused and the
label-map kernels over packed-RGB and NV12 sources against that oracle, whole frames asked for as overlays against the same frames asked for
as labels, and the error paths.  Every comparison is exact."""
import numpy as np
import pytest

import emu_util
import overlay_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import nearest_index, overlay_u8
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


class HostMem:
    """The scenarios' memory: numpy arrays stand in for HBM."""
    stream = None

    def up(self, a, off=0):
        flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        holder = np.full(flat.size + 64, 0xA5, np.uint8)
        holder[off:off + flat.size] = flat
        return holder, holder.ctypes.data + off

    def out(self, nbytes):
        return np.full(nbytes, 0xEE, np.uint8)

    def addr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf


MEM = HostMem()


# ---- host only: the oracle ---------------------------------------------------------------------------------------------------------------
def test_oracle_is_pinned_by_hand_computed_values():
    for a, A in cases.WEIGHT_PINS.items():
        assert a + (a >> 7) == A
    for (c, s, a), want in cases.BLEND_PINS:
        src = np.full((1, 1, 3), s, np.uint8)
        got = overlay_u8(src, np.zeros((1, 1), np.uint8), np.array([[c, c, c, a]], np.uint8))
        assert got.dtype == np.uint8 and got.shape == (1, 1, 3) and (got == want).all(), (c, s, a, got, want)
    # the channels are independent, and the label selects the row
    pal = np.array([[200, 255, 0, 127], [255, 0, 3, 128]], np.uint8)
    src = np.array([[[100, 0, 255], [0, 255, 250]]], np.uint8)
    got = overlay_u8(src, np.array([[0, 1]], np.uint8), pal)
    assert got.tolist() == [[[150, 127, 128], [128, 127, 126]]]           # (3 * 129 + 250 * 127 + 128) >> 8 = 32265 >> 8 = 126


def test_oracle_returns_source_and_palette_at_the_extremes_and_samples_with_nearest_index():
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 19, (33, 65), dtype=np.uint8)
    for Hs, Ws in cases.out_sizes(33, 65):
        src = cases.source_rgb(Hs, Ws)
        assert np.array_equal(overlay_u8(src, labels, cases.rgba(cases.palette19(), 0)), src)
        full = overlay_u8(src, labels, cases.rgba(cases.palette19(), 255))
        assert np.array_equal(full, cases.expected_picture(labels, Hs, Ws, cases.palette19()))
        assert np.array_equal(full, cases.palette19()[labels[nearest_index(33, Hs)][:, nearest_index(65, Ws)]])
        mixed = overlay_u8(src, labels, cases.pal_mixed())
        sampled = labels[nearest_index(33, Hs)][:, nearest_index(65, Ws)]
        zero = cases.pal_mixed()[sampled][..., 3] == 0
        assert np.array_equal(mixed[zero], src[zero])
    l40 = rng.integers(0, 40, (33, 65), dtype=np.uint8)                  # labels outside the table show the source
    got = overlay_u8(cases.source_rgb(33, 65), l40, cases.rgba(cases.palette19(), 255))
    assert np.array_equal(got[l40 >= 19], cases.source_rgb(33, 65)[l40 >= 19]) and (l40 >= 19).any()


# ---- operator level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_kernels_equal_the_oracle_over_rgb_and_nv12_sources(lib, name, C, lo, hi):
    labels = cases.run_operator_case(lib, MEM, name, C, lo, hi)
    if name == "c256":
        assert (labels == 255).any()                                     # label 255 >= n_colours: the source shows through (checked by the oracle)
    if name == "ties":
        assert (labels[::8, ::16][[0, 1, 3, 4]] == 4).all() and (labels[::8, ::16][2] == 3).all()


def test_nv12_layouts_standards_and_poisoned_padding(lib):
    cases.run_nv12_layouts_and_standards(lib, MEM)


def test_palettes_per_class_alpha_and_labels_outside_the_table(lib):
    cases.run_palettes(lib, MEM)


def test_every_alpha_and_source_byte_against_python_integers(lib):
    cases.run_exhaustive_blend(lib, MEM)


def test_operator_argument_checks(lib):
    src = cases.source_rgb(8, 16)
    x = cases.lowres_logits("odd_w", 19, 5, 9)
    out = np.zeros(8 * 16 * 3, np.uint8)
    pal = cases.pal_half()
    args = (x.ctypes.data, 19, 5, 9, 33, 65, None, src.ctypes.data, 0, 8, 16, 0, 0, 0)
    for bad_n in (0, 257):
        assert lib.tdnet_op_overlay(*args, pal.ctypes.data, bad_n, out.ctypes.data, None) < 0 and b"n_colours" in lib.tdnet_last_error()
    assert lib.tdnet_op_overlay(*args, None, 19, out.ctypes.data, None) < 0 and b"NULL" in lib.tdnet_last_error()
    nv = (x.ctypes.data, 19, 5, 9, 33, 65, None, src.ctypes.data, 1, 8, 16, 14, 8 * 16, 0)       # pitch below the row
    assert lib.tdnet_op_overlay(*nv, pal.ctypes.data, 19, out.ctypes.data, None) < 0 and b"pitch" in lib.tdnet_last_error()
    assert (out == 0).all()


# ---- frame level ---------------------------------------------------------------------------------------------------------------------------
def _engine(lib, model=4):
    name = {4: "td4", 1: "psp"}[model]
    spec = arch.model_spec(name, 19, "resnet18")
    e = Engine(model, 18, 19, cases.H, cases.W, 0, lib=lib, arch={})
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(cases.H), arch.feat_size(cases.W), 0))
    return e


@pytest.fixture(scope="module")
def owner(lib):
    e = _engine(lib, 4)
    yield e
    e.close()


@pytest.mark.parametrize("overlay_first", [True, False], ids=["overlay_configured_first", "input_configured_first"])
def test_overlay_frames_follow_the_input_configuration(owner, overlay_first):
    cases.run_frames_follow_the_input(owner, MEM, overlay_first)


def test_overlay_entries_mixed_on_one_handle(owner):
    cases.run_entries_mixed(owner, MEM)


def test_alpha_extremes_colour_map_equivalence_and_rejected_pixels(owner):
    cases.run_alpha_extremes_and_rejection(owner, MEM)


def test_single_frame_pspnet(lib):
    e = _engine(lib, 1)
    cases.run_pspnet_single_frame(e, MEM)
    e.close()


def test_errors_leave_the_fifo_and_a_pending_frame_alone(lib, owner):
    cases.run_errors(owner, MEM, lib, lambda: Engine(2, 18, 19, cases.H, cases.W, 0, lib=lib), _capi.TdnetError)


def test_model_classes_check_their_arguments():
    import torch
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    u8 = torch.zeros(1, 41, 83, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="uint8"):
        m.forward_overlay_u8(torch.zeros(1, 41, 83, 3), 0, (33, 65))
    with pytest.raises(RuntimeError, match="alpha"):
        m.forward_overlay_u8(u8, 0, (33, 65), alpha=1.5)
    with pytest.raises(RuntimeError, match="alpha"):
        m.forward_overlay_u8(u8, 0, (33, 65), alpha=[0.5, 0.5])          # per class: one per colour
    with pytest.raises(RuntimeError, match="palette"):
        m.forward_overlay_u8(u8, 0, (33, 65), palette=np.zeros((19, 5), np.uint8))
    with pytest.raises(RuntimeError, match="src_size"):
        m.forward_overlay_nv12(torch.zeros(1, 62, 96, dtype=torch.uint8), 0, None, (33, 65))
    with pytest.raises(_capi.TdnetError):                               # no CPU fallback
        m.forward_overlay_u8(u8, 0, (33, 65))
    with pytest.raises(_capi.TdnetError):
        m.forward_overlay_nv12(torch.zeros(1, 62, 96, dtype=torch.uint8), 0, (41, 83), (33, 65))
    with pytest.raises(RuntimeError, match="no encoded frame"):
        m.propagate(labels="overlay", src=u8)
    with pytest.raises(RuntimeError, match="no handle"):
        m.labels_overlay(torch.zeros(1, 33, 65, dtype=torch.uint8), u8)
    assert m.engine is None
    # the palette rule: [n, 3] + alpha in 0..1 -> the byte rint(255 alpha); [n, 4] bytes as they are
    p = m._palette_rgba(None, 0.5)
    assert p.shape == (19, 4) and (p[:, 3] == 128).all() and np.array_equal(p[:, :3], cases.palette19())
    p = m._palette_rgba(cases.palette19(), np.linspace(0, 1, 19))
    assert p[0, 3] == 0 and p[18, 3] == 255 and np.array_equal(p[:, 3], np.rint(255 * np.linspace(0, 1, 19)).astype(np.uint8))
    assert np.array_equal(m._palette_rgba(cases.pal_mixed(), 0.123), cases.pal_mixed())
