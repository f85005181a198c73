"""Matte out, what needs no device: tdnet_set_matte's validation (plain host state of a handle that is not even finalized), the two numpy oracles
pinned by hand (dataloader.matte_u8, dataloader.composite_u8), and the model classes' argument checks."""
import numpy as np
import pytest

import emu_util
import matte_cases as cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import composite_u8, matte_u8, nearest_index
from tdnet_amd.engine import Engine


def test_set_matte_is_plain_host_state_and_validates_by_name():
    lib = emu_util.emu_lib()
    e = Engine(2, 18, 19, 33, 65, 0, lib=lib)                          # not finalized: only cfg.nclass is needed
    ok = cases.ids_array((11, 12, 12, 18))
    assert lib.tdnet_set_matte(e.h, ok.ctypes.data, 4) == 0            # duplicates are legal
    assert lib.tdnet_set_matte(e.h, None, 0) == 0                      # the empty set
    assert lib.tdnet_set_matte(e.h, ok.ctypes.data, 0) == 0
    every = cases.ids_array(tuple(range(19)) * 13 + tuple(range(9)))
    assert every.size == 256 and lib.tdnet_set_matte(e.h, every.ctypes.data, 256) == 0
    for args, match in (((cases.ids_array((11, 19)).ctypes.data, 2), r"classes\[1\] = 19.*nclass = 19"), ((cases.ids_array((255,)).ctypes.data, 1), r"classes\[0\] = 255"),
                        ((ok.ctypes.data, 257), "n = 257"), ((ok.ctypes.data, -1), "n = -1"), ((None, 3), "NULL")):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_matte.*" + match):
            lib.check(lib.tdnet_set_matte(e.h, *args))
    with pytest.raises(_capi.TdnetError, match="tdnet_set_matte.*null handle"):
        lib.check(lib.tdnet_set_matte(None, ok.ctypes.data, 4))
    with pytest.raises(_capi.TdnetError, match="set_matte"):
        e.set_matte((3, 256))
    e.set_matte(range(11, 19))
    e.close()


def test_matte_oracle_by_hand():
    # two pixels, three classes: logits (0, ln 2, ln 5) -> masses 1/8, 2/8, 5/8; a pixel of equal logits -> thirds
    v = np.array([[[0.0, 7.0]], [[np.log(2.0), 7.0]], [[np.log(5.0), 7.0]]], np.float32)
    assert matte_u8(v, (0,)).tolist() == [[32, 85]]                    # 255 / 8 = 31.875 -> 32; 85
    assert matte_u8(v, (1, 2, 2)).tolist() == [[223, 170]]             # 255 * 7 / 8 = 223.125
    assert matte_u8(v, (2,)).tolist() == [[159, 85]]                   # 159.375
    rng = np.random.default_rng(3)
    big = (rng.standard_normal((19, 9, 11)) * 300).astype(np.float32)  # +-1000: nothing overflows
    assert (matte_u8(big, range(19)) == 255).all() and (matte_u8(big, ()) == 0).all()
    m, c = matte_u8(big / 100, cases.MOVING).astype(int), matte_u8(big / 100, cases.complement(19, cases.MOVING)).astype(int)
    assert np.abs(m + c - 255).max() <= 1 and 0 < m.mean() < 255
    with pytest.raises(AssertionError):
        matte_u8(big, (19,))
    wide = (rng.standard_normal((19, 40, 50)) * 3).astype(np.float32)  # 2000 pixels: enough for the reference's cap on its near-boundary share to mean something
    want, near = cases.expected(wide, cases.MOVING)
    assert np.array_equal(want, matte_u8(wide, cases.MOVING))          # the tests' reference is this oracle


def test_composite_oracle_by_hand():
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (7, 10, 3), dtype=np.uint8)
    H, W = 3, 4
    bg = (200, 30, 90)
    assert np.array_equal(composite_u8(src, np.full((H, W), 255, np.uint8), H, W, bg), src)             # M = 255: the source, exactly
    assert (composite_u8(src, np.zeros((H, W), np.uint8), H, W, bg) == np.array(bg, np.uint8)).all()    # M = 0: the background, exactly
    m = rng.integers(0, 256, (H, W), dtype=np.uint8)
    out = composite_u8(src, m, H, W, bg)
    ys, xs = nearest_index(H, 7), nearest_index(W, 10)
    for (y, x) in ((0, 0), (6, 9), (3, 5)):
        M = int(m[ys[y], xs[x]])
        A = M + (M >> 7)
        assert out[y, x].tolist() == [(int(src[y, x, c]) * A + bg[c] * (256 - A) + 128) >> 8 for c in range(3)]
    assert composite_u8(src[:1, :1], np.array([[128]], np.uint8), 1, 1, (0, 0, 255))[0, 0].tolist() == \
        [(int(src[0, 0, 0]) * 129 + 128) >> 8, (int(src[0, 0, 1]) * 129 + 128) >> 8, (int(src[0, 0, 2]) * 129 + 255 * 127 + 128) >> 8]
    rgba = composite_u8(src, m, H, W, None)                            # the alpha mode: colour bytes unchanged, M as the fourth
    assert rgba.shape == (7, 10, 4) and np.array_equal(rgba[..., :3], src) and np.array_equal(rgba[..., 3], m[ys][:, xs])


def test_model_classes_check_their_arguments():
    import torch
    from tdnet_amd.dataloader import PIX_RGB24, SourceView
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    u8 = torch.zeros(1, 41, 83, 3, dtype=torch.uint8)
    for call in (lambda: m.forward_matte(torch.zeros(1, 3, 33, 65), 0), lambda: m.forward_matte_u8(u8, 0, (33, 65)),
                 lambda: m.forward_composite_u8(u8, 0, (33, 65)), lambda: m.logits_matte(torch.zeros(1, 19, 33, 65))):
        with pytest.raises(RuntimeError, match="set_matte"):
            call()
    assert m.set_matte([12, 11, 12]) == (11, 12) and m.set_matte(()) == () and m.set_matte(range(11, 19)) == cases.MOVING
    for bad in ((19,), (-1,), (1.5,), 7, (True,), ("a",), (None,), ([1],)):
        with pytest.raises(RuntimeError, match="set_matte"):
            m.set_matte(bad)
    assert m._matte == cases.MOVING
    with pytest.raises(RuntimeError, match="uint8 image"):
        m.forward_matte_u8(torch.zeros(1, 41, 83, 3), 0, (33, 65))
    with pytest.raises(RuntimeError, match="background"):
        m.forward_composite_u8(u8, 0, (33, 65), background=(1, 2))
    with pytest.raises(RuntimeError, match="background"):
        m.forward_composite_u8(u8, 0, (33, 65), background=(1, 2, 256))
    with pytest.raises(RuntimeError, match="32-bit out_view"):
        m.forward_composite_u8(u8, 0, (33, 65), background=None)
    with pytest.raises(RuntimeError, match="32-bit out_view"):
        m.forward_composite_u8(u8, 0, (33, 65), background=None, out_view=SourceView(PIX_RGB24, 41, 83))
    with pytest.raises(_capi.TdnetError):                               # no CPU fallback
        m.forward_matte(torch.zeros(1, 3, 33, 65), 0)
    with pytest.raises(_capi.TdnetError):
        m.forward_matte_u8(u8, 0, (33, 65))
    with pytest.raises(_capi.TdnetError):
        m.forward_composite_u8(u8, 0, (33, 65), background=(1, 2, 3))
    with pytest.raises(RuntimeError, match="no encoded frame"):
        m.propagate(matte=True)
    with pytest.raises(RuntimeError, match="no encoded frame"):
        m.propagate(composite=True, src=u8)
    with pytest.raises(RuntimeError, match="no handle"):
        m.logits_matte(torch.zeros(1, 19, 33, 65))
    assert m.engine is None
