"""The new kernel and host paths of the backbone-layout / class-count feature through the test-only fiber emulator (tests/emu/): the
class-tiled classifier (NC > 32) on ragged shapes, and whole frames of td4-r18 multi_grid=False and td2-r18 nclass=40 against the
fixtures captured from the real reference.  CPU only."""
import os

import numpy as np
import pytest

import emu_util
import opcheck
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine

MEM = opcheck.NumpyMem()


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


def _classifier(lib, x, wt, b):
    HW, C = x.shape
    NC = wt.shape[0]
    out = MEM.empty((NC, HW))
    lib.check(lib.tdnet_op_classifier(MEM.ptr(MEM.put(x)), HW, C, MEM.ptr(MEM.put(wt)), MEM.ptr(MEM.put(b)), NC, MEM.ptr(out), None))
    return out


@pytest.mark.parametrize("NC", [33, 40, 150, 256])
def test_class_tiled_classifier_ragged(lib, NC):
    rng = np.random.default_rng(NC)
    for C, HW in ((64, 45), (128, 131), (512, 70)):                  # HW not a multiple of the 64-pixel block
        x = rng.standard_normal((HW, C)).astype(np.float32)
        wt = (rng.standard_normal((NC, C)) / np.sqrt(C)).astype(np.float32)
        b = rng.standard_normal(NC).astype(np.float32)
        out = _classifier(lib, x, wt, b)
        ref = (wt.astype(np.float64) @ x.astype(np.float64).T) + b[:, None]
        assert np.abs(out - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (NC, C, HW)
        # every class tile forms the sum k_classifier forms: the first 32 classes bit for bit as a 32-class classifier
        assert np.array_equal(out[:32], _classifier(lib, x, wt[:32].copy(), b[:32].copy())), (NC, C, HW)
    with pytest.raises(_capi.TdnetError):
        _classifier(lib, np.zeros((4, 64), np.float32), np.zeros((257, 64), np.float32), np.zeros(257, np.float32))


@pytest.mark.parametrize("tag,name,bb,H,W,nc,dil,mg", [("td4_resnet18_33x65_nomg", "td4", "resnet18", 33, 65, 19, True, False),
                                                       ("td2_resnet18_33x65_nc40", "td2", "resnet18", 33, 65, 40, True, True)])
def test_frames_against_reference_goldens(lib, golden_dir, tag, name, bb, H, W, nc, dil, mg):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    T = 1 + max(int(k.split("_")[0][1:]) for k in g.files if k.startswith("f"))
    spec = arch.model_spec(name, nc, bb, dil, mg)
    h, w = arch.feat_size(H, dil), arch.feat_size(W, dil)
    e = Engine(spec.path_num, int(bb[6:]), nc, H, W, 0, lib=lib, arch={"dilated": dil, "multi_grid": mg})
    assert e.feature_dims() == (h, w) and e.arch() == {"dilated": int(dil), "multi_grid": int(mg)}
    e.load_state_dict(weights.synth_state_dict(spec, h, w, 0))
    shapes = {"c4": (1, spec.d_model, h, w), "z": (1, spec.d_model, h, w), "lowres": (1, nc, h, w)}
    for t, x in enumerate(weights.synth_video(H, W, T, seed=1)):
        out = np.full((1, nc, H, W), 7e7, np.float32)
        e.forward(x, t % spec.path_num, out)
        for st, shp in shapes.items():
            key = "f%d_%s" % (t, st)
            if key in g.files:
                got = e.stage(st, shp)
                assert np.abs(got - g[key]).max() <= 1e-4 * max(1.0, np.abs(g[key]).max()), key
        key = "f%d_logits" % t
        if key in g.files:
            ref = g[key]
            err = float(np.abs(out - ref).max())
            assert err <= 1e-3, (key, err)
            bad = out[0].argmax(0) != ref[0].argmax(0)
            if bad.any():
                top2 = np.sort(ref[0], axis=0)[-2:]
                assert ((top2[1] - top2[0])[bad] <= 2 * err).all(), key
            lab = np.zeros((H, W), np.int32)
            e.argmax(out, lab)
            assert (lab == out[0].argmax(0)).all()
    e.close()


def test_arch_entry_points_refuse_bad_arguments(lib):
    a = lib.arch()
    a.dilated = 2
    with pytest.raises(_capi.TdnetError, match="0 or 1"):
        Engine(2, 18, 19, 33, 65, 0, lib=lib, arch=a)
    a = lib.arch()
    a.reserved[3] = 1
    with pytest.raises(_capi.TdnetError, match="reserved"):
        Engine(2, 18, 19, 33, 65, 0, lib=lib, arch=a)
    for nc in (0, 257):
        with pytest.raises(_capi.TdnetError, match="nclass"):
            Engine(2, 18, nc, 33, 65, 0, lib=lib, arch={})
    Engine(2, 18, 256, 33, 65, 0, lib=lib, arch={}).close()
    with pytest.raises(_capi.TdnetError):                            # tdnet_create_opts keeps refusing pspnet on BasicBlock backbones
        Engine(1, 18, 19, 33, 65, 0, lib=lib)
    e = Engine(1, 34, 19, 769, 1537, 0, lib=lib, arch={"dilated": False})
    assert e.feature_dims() == (25, 49) and e.arch() == {"dilated": 0, "multi_grid": 1}
    e.close()
