"""Refined matte (include/tdnet.h "refined matte"), on the CPU through the kernel emulator: the operator entry and its coefficient launch against the
oracle dataloader.refine_matte_u8, EXACTLY -- the definition is integers and single correctly rounded fp32 operations, so the tiling cannot show.  Every
map sits at a byte offset inside guard bands, with padded rows (tests/refine_cases.py); the exact properties; every refused argument by message."""
import numpy as np
import pytest

import emu_util
import refine_cases as cases
from tdnet_amd import _capi
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


@pytest.fixture(scope="module")
def eng(lib):
    e = Engine(2, 18, 19, 33, 65, 0, lib=lib)                         # the operator needs a handle for its device, nothing else: no weights
    yield e
    e.close()


class HostMem:
    """The shared scenarios' memory (tests/refine_cases.py): numpy arrays stand in for HBM."""
    stream = None

    def up(self, a, off=0):
        flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        raw = np.full(off + flat.size + 16, 0xA5, np.uint8)
        pad = (-raw.ctypes.data) % 16
        holder = raw[pad:pad + off + flat.size]
        holder[off:] = flat
        return holder, holder.ctypes.data + off

    def get(self, buf):
        return buf


MEM = HostMem()


def test_tile_geometry_and_scratch_size(lib, eng):
    assert cases.tile(lib) == cases.TILE                               # the cases are sized from it
    assert eng.refine_scratch_bytes(41, 83) == 6 * 41 * 83 and eng.refine_scratch_bytes(0, 5) == 0 and eng.refine_scratch_bytes(5, -1) == 0


@pytest.mark.parametrize("case", cases.exact_cases(), ids=cases.case_id)
def test_operator_and_coefficients_equal_the_oracle(lib, eng, case):
    cases.check_operator(lib, eng, MEM, case, cases.FEW_OFFSETS)


def test_every_byte_offset_of_each_of_the_three_maps(lib, eng):
    """independent of the byte address and pitch of any of the three maps: the 64 offset triples at a size with a partial tile in both axes"""
    cases.check_operator(lib, eng, MEM, ("random", 5, 9, 16, 65), cases.ALL_OFFSETS, fills=cases.FILLS[:1])
    cases.check_operator(lib, eng, MEM, ("ramp", 17, 29, 4, 65), cases.ALL_OFFSETS[::5], fills=cases.FILLS)


def test_the_exact_properties(lib, eng):
    tx, cy, ay = cases.tile(lib)
    cases.check_exact_properties(eng, MEM, 5, 9)
    cases.check_exact_properties(eng, MEM, max(cy, ay) + 1, tx + 1)


def test_every_refused_argument_by_message_and_nothing_written(lib, eng):
    calls, (o, keep) = cases.refused(eng, MEM)
    for call, msg in calls:
        with pytest.raises(_capi.TdnetError, match="tdnet_refine_matte.*" + msg):
            call()
    assert np.array_equal(np.asarray(MEM.get(o.holder)), o.host)
    G, M = cases.inputs("random", 5, 9)
    g, m = cases.place(MEM, G), cases.place(MEM, M)
    aq, bq = np.zeros((5, 9), np.int16), np.zeros((5, 9), np.int32)
    for args, msg in (((g.addr, g.pitch, m.addr, m.pitch, 5, 9, 0, 65, aq.ctypes.data, bq.ctypes.data, None), "radius = 0"),
                      ((g.addr, g.pitch, m.addr, 8, 5, 9, 4, 65, aq.ctypes.data, bq.ctypes.data, None), "matte_pitch = 8"),
                      ((g.addr, g.pitch, m.addr, m.pitch, 5, 9, 4, 65, None, bq.ctypes.data, None), "null")):
        with pytest.raises(_capi.TdnetError, match="tdnet_op_refine_coeff.*" + msg):
            lib.check(lib.tdnet_op_refine_coeff(*args))
    with pytest.raises(_capi.TdnetError, match="tdnet_refine_matte: null handle"):
        lib.check(lib.tdnet_refine_matte(None, g.addr, g.pitch, m.addr, m.pitch, o.addr, o.pitch, 5, 9, 4, 65, 16, None))


# ---- the frame's end ---------------------------------------------------------------------------------------------------------------------------
import matte_cases as mc  # noqa: E402
from tdnet_amd import arch, weights  # noqa: E402


class HostDev:
    """tests/refine_cases.py check_frames' memory: numpy arrays"""
    stream = None

    def put(self, a):
        return np.array(a, copy=True)

    def ptr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf.reshape(-1) if buf.ndim == 1 else buf


_gather = {}


def gather_inputs(lib):
    """(keepalive, address of logits [19, 5, 9], the matte operator's bytes [33, 65] for the set `moving`), computed once"""
    if not _gather:
        x = mc.logits("odd_w", 19, 5, 9, 6)
        keep, px = MEM.up(x)
        _, m = mc.matte_op(lib, MEM, 19, 33, 65, mc.MOVING, px, 5, 9, want_labels=False)
        m.setflags(write=False)
        assert len(np.unique(m)) > 100
        _gather["v"] = (keep, px, m)
    return _gather["v"]


@pytest.mark.parametrize("kind", mc.SOURCE_KINDS)
@pytest.mark.parametrize("size", [(41, 83), (17, 29)], ids=["41x83", "17x29"])
def test_gather_planes_equal_luma_and_the_sampled_matte(lib, size, kind):
    keep, px, m = gather_inputs(lib)
    cases.check_gather(lib, MEM, kind, size, px, mc.MOVING, m)


def test_whole_frames_refined_entry_composite_counts_and_errors(lib):
    spec = arch.model_spec("td4", 19, "resnet18")
    owner = Engine(4, 18, 19, cases.H, cases.W, 0, lib=lib, arch={})
    owner.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(cases.H), arch.feat_size(cases.W), 0))
    rng = np.random.default_rng(45)
    frames = [rng.integers(0, 256, (cases.HS, cases.WS, 3), dtype=np.uint8) for _ in range(3)]
    cases.check_frames(HostDev(), owner, frames, 4)
    owner.close()
