"""Backbone layouts and class counts beyond the shipped ones (the reference constructors' dilated / multi_grid / nclass, and pspnet
on ResNet-18 / 34): block lists restated from the reference, the CPU oracle against the fixtures captured from the real reference
(tools/make_golden.py ARCH_CASES), the pspnet state-dict inventory, the model classes' constructors, and the unchanged defaults.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import tdnet_ref
from tdnet_amd import arch, weights

BACKBONES = ("resnet18", "resnet34", "resnet50", "resnet101")
COUNTS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3), "resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3)}


def restated_blocks(bb, dilated, multi_grid):
    """resnet.py:138-200 read on its own (not through arch.py): oracle RefBlocks (name kind stride dil1 dil2 downsample)."""
    kind = "bottleneck" if bb in ("resnet50", "resnet101") else "basic"
    exp = 4 if kind == "bottleneck" else 1
    inplanes = 128 if kind == "bottleneck" else 64
    if dilated:
        layers = [(64, 1, 1, False), (128, 2, 1, False), (256, 1, 2, False), (512, 1, 4, multi_grid)]
    else:                                                           # for_seg is never passed: dilation = [1, 1] (resnet.py:150-158)
        layers = [(64, 1, 1, False), (128, 2, 1, False), (256, 2, 1, False), (512, 2, 1, False)]
    out = []
    for li, ((planes, stride, dilation, mg), n) in enumerate(zip(layers, COUNTS[bb]), 1):
        ds = stride != 1 or inplanes != planes * exp
        first = 4 if mg else 1 if dilation in (1, 2) else 2        # :181-190
        out.append(tdnet_ref.RefBlock("layer%d.0" % li, kind, stride, first, dilation, ds))
        inplanes = planes * exp
        for i in range(1, n):                                       # :194-200
            out.append(tdnet_ref.RefBlock("layer%d.%d" % (li, i), kind, 1, (4, 8, 16)[i] if mg else dilation, dilation, False))
    return out


@pytest.mark.parametrize("bb", BACKBONES)
def test_restated_block_lists_equal_arch(bb):
    for dilated in (True, False):
        for mg in (True, False):
            a = arch.backbone_blocks(bb, dilated, mg)
            b = restated_blocks(bb, dilated, mg)
            assert [(x.name, x.kind, x.stride, x.dil1, x.dil2, x.downsample) for x in a] == [tuple(y) for y in b], (bb, dilated, mg)
    # spot checks of the issue's statement: multi_grid=False layer 4 is (2, 4), (4, 4) ...; not dilated: stride-2 layer3.0 / layer4.0
    nomg = {b.name: b for b in arch.backbone_blocks(bb, True, False)}
    assert (nomg["layer4.0"].dil1, nomg["layer4.1"].dil1) == (2, 4) and nomg["layer4.0"].dil2 == 4
    nodil = {b.name: b for b in arch.backbone_blocks(bb, False, True)}
    assert nodil["layer3.0"].stride == nodil["layer4.0"].stride == 2 and nodil["layer3.0"].downsample and nodil["layer4.0"].downsample
    assert all(b.dil1 == b.dil2 == 1 for b in nodil.values())


def test_feature_size_follows_the_strides():
    assert arch.feat_size(769, False) == 25 and arch.feat_size(1537, False) == 49
    assert arch.feat_size(1024, False) == 32 and arch.feat_size(2048, False) == 64
    assert (arch.feat_size(65, False), arch.feat_size(129, False)) == (3, 5)
    for n in (33, 65, 97, 769, 1024):
        assert arch.feat_size(n) == arch.feat_size(n, True) == (((n - 1) // 2) // 2) // 2 + 1


# (tag, name, backbone, H, W, nclass, dilated, multi_grid): the fixtures of tools/make_golden.py ARCH_CASES
GOLDENS = [("td4_resnet18_33x65_nomg", "td4", "resnet18", 33, 65, 19, True, False),
           ("td2_resnet50_33x65_nomg", "td2", "resnet50", 33, 65, 19, True, False),
           ("td2_resnet18_65x129_nodil", "td2", "resnet18", 65, 129, 19, False, True),
           ("td2_resnet18_33x65_nc40", "td2", "resnet18", 33, 65, 40, True, True),
           ("psp_resnet18_33x65", "psp", "resnet18", 33, 65, 19, True, True),
           ("psp_resnet34_65x129_nodil", "psp", "resnet34", 65, 129, 19, False, True)]


def frames_in(g):
    return 1 + max(int(k.split("_")[0][1:]) for k in g.files if k.startswith("f"))


@pytest.mark.parametrize("tag,name,bb,H,W,nc,dil,mg", GOLDENS)
def test_oracle_matches_reference_goldens(golden_dir, tag, name, bb, H, W, nc, dil, mg):
    torch.set_num_threads(8)
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    spec = arch.model_spec(name, nc, bb, dil, mg)
    h, w = arch.feat_size(H, dil), arch.feat_size(W, dil)
    sd = weights.synth_state_dict(spec, h, w, 0)
    net = (tdnet_ref.PSPNetRef if name == "psp" else tdnet_ref.TDNetRef)(spec, sd)
    net.blocks = restated_blocks(bb, dil, mg)                        # the oracle reads its block list from here
    checked = 0
    for t, x in enumerate(weights.synth_video(H, W, frames_in(g), seed=1)):
        net.trace = {}
        out = net.forward(torch.from_numpy(x), t % spec.path_num).numpy()
        got = {k: v.numpy() for k, v in net.trace.items()}
        got["logits"] = out
        for st in ("c4", "z", "lowres", "logits"):
            key = "f%d_%s" % (t, st)
            if key not in g.files:
                continue
            ref = g[key]
            assert got[st].shape == ref.shape, key
            assert np.abs(got[st] - ref).max() <= 1e-4 * max(1.0, float(np.abs(ref).max())), (key, np.abs(got[st] - ref).max())
            checked += 1
        key = "f%d_logits" % t
        if key in g.files:
            ref = g[key][0]
            bad = ref.argmax(0) != out[0].argmax(0)
            if bad.any():                                                  # tie-tolerant argmax
                top2 = np.sort(ref, axis=0)[-2:]
                assert ((top2[1] - top2[0])[bad] <= 1e-4).all(), key
    assert checked >= frames_in(g) + 1
    assert g["f0_lowres"].shape == (1, nc, h, w)


def test_psp_state_dict_inventory_matches_the_reference(golden_dir):
    inv = json.load(open(os.path.join(golden_dir, "psp_state_dict_inventory.json")))
    for bb in ("resnet18", "resnet34"):
        for dil in (True, False):
            got = arch.state_dict_shapes(arch.model_spec("psp", 19, bb, dil), 1, 1)
            assert [(k, list(s)) for k, s in got.items()] == [(k, s) for k, s in inv[bb]], bb


def test_model_classes_construct_with_the_reference_arguments():
    """Before this feature dilated=False / multi_grid=False, pspnet on ResNet-18 / 34 raised NotImplementedError (and nclass > 32
    was refused by the library)."""
    from tdnet_amd.model import pspnet, td2_psp50, td4_psp18
    m = td4_psp18.td4_psp18(nclass=19, path_num=4, backbone="resnet18", multi_grid=False, synthetic_seed=0)
    assert (m.spec.dilated, m.spec.multi_grid) == (True, False)
    assert [b.dil1 for b in arch.spec_blocks(m.spec)][-2:] == [2, 4]
    m = td2_psp50.td2_psp50(nclass=40, path_num=2, backbone="resnet18", dilated=False, synthetic_seed=0)
    assert m.spec.dilated is False and m.nclass == 40
    assert m.cache_entry_numel_for(769, 1537) == (7 * 13 * 64, 7 * 13 * 64, 7 * 13 * 128)   # 25 x 49 features -> 7 x 13 keys
    for bb in ("resnet18", "resnet34"):
        p = pspnet.pspnet(nclass=19, backbone=bb, synthetic_seed=0)
        assert (p.spec.d_model, p.spec.head_mid) == (512, 128)
    p = pspnet.pspnet(nclass=19, backbone="resnet34", dilated=False, multi_grid=False, synthetic_seed=0)
    assert p.spec.dilated is False
    with pytest.raises(RuntimeError):
        pspnet.pspnet(nclass=19, backbone="vgg16")
    # the LayerNorm plane must be the map's own: a td2 stride-32 checkpoint made for another input size fails like the reference
    sd = weights.synth_state_dict(arch.model_spec("td2", 19, "resnet18", False), 3, 5, 0)
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, backbone="resnet18", dilated=False)
    m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="normalized_shape"):
        m._build_engine(97, 193, 0)


def _sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        a = np.ascontiguousarray(np.asarray(sd[k]))
        h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def test_defaults_are_unchanged():
    for bb in BACKBONES:
        assert arch.backbone_blocks(bb) == arch.backbone_blocks(bb, True, True)
        assert [tuple(x) for x in tdnet_ref.ref_backbone_blocks(bb)] == [tuple(y) for y in restated_blocks(bb, True, True)]
    assert arch.model_spec("td4", 19, "resnet18") == arch.model_spec("td4", 19, "resnet18", True, True)
    assert arch.model_spec("psp")[:12] == ("psp", 1, "resnet101", 2048, 0, 0, 1, (0,), 512, 19, 0, {})
    # synth_state_dict of the shipped specs, byte for byte as the parent commit generated them (hashes recorded there)
    assert _sha(weights.synth_state_dict(arch.model_spec("td4", 19, "resnet18"), 5, 9, 0)) == \
        "b94bff679e949fd7e7e1d7c6f9ab33d625b4cfe04c5c1b221004822359cf7d99"
    assert _sha(weights.synth_state_dict(arch.model_spec("td2", 19, "resnet50"), 5, 9, 0)) == \
        "1b228ec8f034bf4161db759b4a599fc75b005dcf867123d3d6cd3cc23e37680c"
