"""tests/wino_f64_cases.py on the device: the fused Winograd F(4x4) kernel of the 64 -> 64 3x3 convs (k_wino4_f64, tdnet_opts.fusion bit 4194304) -- the
operator entry inside guard bands at the smallest maps its index math can go wrong at, and a whole td4 clip at the smallest frame whose layer1 the size
rule gives to the kernel, with the bit on and off."""
import numpy as np
import pytest
import torch

import opcheck
import wino_f64_cases as cases
from tdnet_amd import _capi, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()                      # the in-tree libtdnet_hip_test.so; raises if it is missing


@pytest.fixture()
def mem():
    return opcheck.GuardedTorchMem()


@pytest.mark.parametrize("resid,act", cases.VARIANTS)
@pytest.mark.parametrize("hw", cases.MAPS, ids=lambda hw: "%dx%d" % hw)
def test_fused_kernel_against_fp64_and_the_unfused_route(lib, mem, hw, resid, act):
    cases.conv(lib, mem, hw[0], hw[1], resid, act)


@pytest.mark.parametrize("shape", cases.REFUSED, ids=lambda s: "%d-%d-k%d-s%d-d%d-a%d" % s)
def test_entry_refuses_what_the_route_does_not_take(lib, mem, shape):
    cases.refused(lib, mem, shape)


def test_entry_refuses_a_map_past_the_32_bit_offsets(lib, mem):
    cases.refused_size(lib, mem)


def test_small_maps_keep_the_direct_kernel(lib, mem):
    cases.plan_keeps_small_maps(lib, mem)


def test_frames_with_the_bit_on_and_off(lib):
    """td4-resnet18 at 509 x 1021: layer1's map is 128 x 256 = 32768 pixels, the smallest the size rule (TD_WINO_F64_MIN_PIXELS) hands to the fused kernel.
    Both settings pass test_gpu_model's oracle gate; their logits differ in bits -- the route was taken."""
    import test_gpu_model as tm
    H, W = 509, 1021
    assert ((H - 1) // 2 // 2 + 1) * ((W - 1) // 2 // 2 + 1) == cases.MIN_PIXELS
    default = lib.opts().fusion
    on, off = {"fusion": default | cases.WINO_F64}, {"fusion": default & ~cases.WINO_F64}
    for opts in (on, off):
        tm._vs_oracle("td4", "resnet18", H, W, 1, kernel_opts=opts)
    x = torch.from_numpy(next(iter(weights.synth_video(H, W, 1, seed=1)))).cuda()
    with torch.no_grad():
        a, b = (tm.make_model("td4", "resnet18", kernel_opts=o)(x, pos_id=0).cpu().numpy() for o in (on, off))
    d = float(np.abs(a - b).max())
    print("509x1021 frame 0, bit on against bit off: max |dlogit| %.2e" % d)
    assert not np.array_equal(a, b) and d <= 1e-3
