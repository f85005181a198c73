"""GPU parity of the backbone layouts and class counts beyond the shipped ones (dilated / multi_grid / nclass, pspnet on ResNet-18 / 34):
the fixtures captured from the real reference, the CPU oracle where the production routings engage (row-parity chains, stride-32 maps,
the class-tiled classifier), the fp16 and split-bf16 precision modes, and the C ABI's arch entry points.  Gates of test_gpu_model.py:
stages <= 1e-4 relative, logits <= 1e-3 plus the top-2 tie band, clip mIoU >= 0.9995."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import tdnet_ref
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine
from tdnet_amd.model import pspnet, td2_psp50, td4_psp18

pytestmark = pytest.mark.gpu


def blocks_for(bb, dilated, multi_grid):
    """The oracle's block list, restated from resnet.py:138-200 (tests/test_arch_variants.py) and assigned to ref.blocks."""
    from test_arch_variants import restated_blocks
    return restated_blocks(bb, dilated, multi_grid)


def make(name, bb, nclass=19, dilated=True, multi_grid=True, kernel_opts=None):
    kw = dict(nclass=nclass, model_path=None, backbone=bb, dilated=dilated, multi_grid=multi_grid, synthetic_seed=0, kernel_opts=kernel_opts)
    if name == "td4":
        return td4_psp18.td4_psp18(path_num=4, **kw).eval()
    if name == "td2":
        return td2_psp50.td2_psp50(path_num=2, **kw).eval()
    return pspnet.pspnet(**kw).eval()


def make_ref(name, bb, H, W, nclass=19, dilated=True, multi_grid=True):
    spec = arch.model_spec(name, nclass, bb, dilated, multi_grid)
    sd = weights.synth_state_dict(spec, arch.feat_size(H, dilated), arch.feat_size(W, dilated), 0)
    ref = (tdnet_ref.PSPNetRef if name == "psp" else tdnet_ref.TDNetRef)(spec, sd)
    ref.blocks = blocks_for(bb, dilated, multi_grid)
    return spec, ref


def check_frame(out, ref, tag, hist, nclass, atol=1e-3, min_equal=None):
    err = float(np.abs(out - ref).max())
    assert err <= atol, (tag, err)
    lo, lr = out[0].argmax(0), ref[0].argmax(0)
    bad = lo != lr
    if min_equal is not None:
        assert 1.0 - bad.mean() >= min_equal, (tag, bad.mean())
    elif bad.any():
        top2 = np.sort(ref[0], axis=0)[-2:]
        assert ((top2[1] - top2[0])[bad] <= 2 * err).all(), (tag, "label flip outside the tie band")
    hist += tdnet_ref.confusion_miou(lo, lr, nclass)[1]
    return err


def clip_miou(hist):
    with np.errstate(divide="ignore", invalid="ignore"):
        iu = np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))
    return float(np.nanmean(iu))


GOLDENS = [("td4_resnet18_33x65_nomg", "td4", "resnet18", 33, 65, 19, True, False),
           ("td2_resnet50_33x65_nomg", "td2", "resnet50", 33, 65, 19, True, False),
           ("td2_resnet18_65x129_nodil", "td2", "resnet18", 65, 129, 19, False, True),
           ("td2_resnet18_33x65_nc40", "td2", "resnet18", 33, 65, 40, True, True),
           ("psp_resnet18_33x65", "psp", "resnet18", 33, 65, 19, True, True),
           ("psp_resnet34_65x129_nodil", "psp", "resnet34", 65, 129, 19, False, True)]


@pytest.mark.parametrize("tag,name,bb,H,W,nc,dil,mg", GOLDENS)
def test_against_reference_goldens(golden_dir, tag, name, bb, H, W, nc, dil, mg):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    T = 1 + max(int(k.split("_")[0][1:]) for k in g.files if k.startswith("f"))
    spec = arch.model_spec(name, nc, bb, dil, mg)
    h, w = arch.feat_size(H, dil), arch.feat_size(W, dil)
    zc = 2 * spec.d_model if name == "psp" else spec.d_model
    shapes = {"c4": (1, spec.d_model, h, w), "z": (1, zc, h, w), "lowres": (1, nc, h, w)}
    m = make(name, bb, nc, dil, mg)
    hist = np.zeros((nc, nc), np.int64)
    with torch.no_grad():
        for t, x in enumerate(weights.synth_video(H, W, T, seed=1)):
            out = m(torch.from_numpy(x).cuda(), pos_id=t % spec.path_num).cpu().numpy()
            assert m.engine.feature_dims() == (h, w)
            for st, shp in shapes.items():
                key = "f%d_%s" % (t, st)
                if key in g.files:
                    got = m.engine.stage(st, shp)
                    assert np.abs(got - g[key]).max() <= 1e-4 * max(1.0, np.abs(g[key]).max()), key
            if "f%d_logits" % t in g.files:
                check_frame(out, g["f%d_logits" % t], (tag, t), hist, nc)
    assert clip_miou(hist) >= 0.9995


def _vs_oracle(name, bb, H, W, T, nclass=19, dilated=True, multi_grid=True, kernel_opts=None, atol=1e-3, min_equal=None, labels=False):
    spec, ref = make_ref(name, bb, H, W, nclass, dilated, multi_grid)
    m = make(name, bb, nclass, dilated, multi_grid, kernel_opts)
    tdnet_ref.tune_threads()
    hist = np.zeros((nclass, nclass), np.int64)
    worst = 0.0
    with torch.no_grad():
        for t, x in enumerate(weights.synth_video(H, W, T, seed=1)):
            xt = torch.from_numpy(x)
            out_t = m(xt.cuda(), pos_id=t % spec.path_num)
            out = out_t.cpu().numpy()
            exp = ref.forward(xt, t % spec.path_num).numpy()
            worst = max(worst, check_frame(out, exp, (name, bb, H, W, t), hist, nclass, atol, min_equal))
            if labels:
                lab = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
                m.engine.argmax(out_t.data_ptr(), lab.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert (lab.cpu().numpy()[0] == out[0].argmax(0)).all()
    miou = clip_miou(hist)
    print("%s-%s %dx%d dil=%d mg=%d nc=%d %s: worst |dlogit| %.2e, clip mIoU %.6f, launches %d"
          % (name, bb, H, W, dilated, multi_grid, nclass, kernel_opts or "", worst, miou, m.engine.last_launch_count()))
    if min_equal is None:
        assert miou >= 0.9995, miou
    return m


def test_td4_r18_no_multi_grid_with_and_without_chains():
    _vs_oracle("td4", "resnet18", 385, 769, 6, multi_grid=False)
    m = _vs_oracle("td4", "resnet18", 385, 769, 6, multi_grid=False, kernel_opts={"overlap": 41 | 4})   # row-parity chains at any size
    assert m.engine.opts()["overlap"] & 4


def test_td2_r50_no_multi_grid():
    _vs_oracle("td2", "resnet50", 385, 769, 3, multi_grid=False)


def test_stride32_maps():
    _vs_oracle("td2", "resnet18", 769, 1537, 3, dilated=False)      # 25 x 49 features
    _vs_oracle("td4", "resnet34", 1024, 2048, 5, dilated=False)     # 32 x 64 features


def test_pspnet_on_basicblock_backbones():
    _vs_oracle("psp", "resnet18", 769, 1537, 1)
    _vs_oracle("psp", "resnet34", 769, 1537, 1, dilated=False)


@pytest.mark.parametrize("nc", [33, 40, 150, 256])
def test_class_counts(nc):
    m = _vs_oracle("td2", "resnet18", 129, 257, 3, nclass=nc, labels=True)
    if nc == 256:
        x = torch.from_numpy(weights.synth_video(129, 257, 1, seed=7)[0]).cuda()
        m.reset()
        out = m(x, 0)
        m.reset()
        lab = m.forward_labels(x, 0)
        assert torch.equal(lab[0].cpu(), out[0].argmax(0).int().cpu())


@pytest.mark.parametrize("precision", [1, 2])
def test_precision_modes(precision):
    gate = dict(atol=3e-2, min_equal=0.995) if precision == 1 else {}
    _vs_oracle("td4", "resnet18", 385, 769, 5, multi_grid=False, kernel_opts={"precision": precision}, **gate)
    _vs_oracle("td2", "resnet18", 385, 769, 3, dilated=False, kernel_opts={"precision": precision}, **gate)


def test_create_arch_default_is_bit_identical_to_create_opts():
    H, W, T = 129, 257, 5
    spec = arch.model_spec("td4", 19, "resnet18")
    sd = weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0)
    lib = _capi.lib()
    outs = []
    for a in (None, {"dilated": True, "multi_grid": True}, "null"):
        if a == "null":                                               # tdnet_create_arch(cfg, NULL, opts)
            e = Engine(4, 18, 19, H, W, 0)
            lib.tdnet_destroy(e.h)
            h = ctypes.c_void_p()
            o = lib.opts()
            lib.check(lib.tdnet_create_arch(ctypes.byref(e.cfg), None, ctypes.byref(o), ctypes.byref(h)))
            e.h = h
        else:
            e = Engine(4, 18, 19, H, W, 0, arch=a)
        e.load_state_dict(sd)
        res = []
        for t, x in enumerate(weights.synth_video(H, W, T, seed=1)):
            xi = torch.from_numpy(x).cuda()
            out = torch.empty((1, 19, H, W), device="cuda")
            e.forward(xi.data_ptr(), t % 4, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            res.append(out.cpu().numpy())
        assert e.arch() == {"dilated": 1, "multi_grid": 1}
        e.close()
        outs.append(res)
    for other in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], other))


def test_refusals():
    lib = _capi.lib()
    a = lib.arch()
    a.multi_grid = 3
    with pytest.raises(_capi.TdnetError, match="0 or 1"):
        Engine(2, 18, 19, 65, 129, 0, arch=a)
    for nc in (0, 257):
        with pytest.raises(_capi.TdnetError, match="nclass"):
            Engine(2, 18, nc, 65, 129, 0, arch={})
