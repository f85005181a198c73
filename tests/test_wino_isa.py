"""Instruction counts of the Winograd F(4x4) transform kernels (tdnet_amd/csrc/td_wino.h) in the gfx950 code the library's flags produce.

The transforms are VALU-bound wherever they share a SIMD with the fp32 GEMM, and twice the compiler was found issuing three times the
instructions the arithmetic needs: a four-wide fp32 expression is split into single-lane v_sub_f32 instead of v_pk_add_f32, and a
multiplication by 2, 4 or 8 in front of an addition stays an instruction of its own with contraction off.  These limits guard against
either coming back silently with a compiler release or an edit of the header.  Skips without hipcc."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r"""
#include "td_wino.h"
template __global__ void k_wino4_out<false>(WinoArgs);
template __global__ void k_wino4_out<true>(WinoArgs);
template __global__ void k_wino4_in_c<1>(WinoArgs);
template __global__ void k_wino4_in_c<2>(WinoArgs);
template __global__ void k_wino4_in_c<4>(WinoArgs);
template __global__ void k_wino4_out_c<1, false>(WinoArgs);
template __global__ void k_wino4_out_c<2, false>(WinoArgs);
template __global__ void k_wino4_out_c<4, false>(WinoArgs);
template __global__ void k_wino4_out_c<2, true>(WinoArgs);
template __global__ void k_wino4_out_c<4, true>(WinoArgs);
template __global__ void k_wino4_out_cls<1>(WinoArgs, ClsArgs);
template __global__ void k_wino4_out_cls<2>(WinoArgs, ClsArgs);
"""
# mangled name -> what it is.  k_wino4_out / _out_c: <.., false> is the instance of ReLU and identity (every conv of the frame), <.., true> the leaky one.
KERNELS = {
    "_Z10k_wino4_in8WinoArgs": "k_wino4_in",
    "_Z11k_wino4_outILb0EEv8WinoArgs": "k_wino4_out<false>",
    "_Z11k_wino4_outILb1EEv8WinoArgs": "k_wino4_out<true>",
    "_Z12k_wino4_in_cILi2EEv8WinoArgs": "k_wino4_in_c<2>",
    "_Z12k_wino4_in_cILi4EEv8WinoArgs": "k_wino4_in_c<4>",
    "_Z13k_wino4_out_cILi2ELb0EEv8WinoArgs": "k_wino4_out_c<2, false>",
    "_Z13k_wino4_out_cILi4ELb0EEv8WinoArgs": "k_wino4_out_c<4, false>",
    "_Z13k_wino4_out_cILi2ELb1EEv8WinoArgs": "k_wino4_out_c<2, true>",
    "_Z13k_wino4_out_cILi4ELb1EEv8WinoArgs": "k_wino4_out_c<4, true>",
    "_Z15k_wino4_out_clsILi2EEv8WinoArgs7ClsArgs": "k_wino4_out_cls<2>",
}


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from tdnet_amd import build as b
    d = tmp_path_factory.mktemp("wino_isa")
    src, out = str(d / "wino_tu.hip"), str(d / "wino_tu.s")
    with open(src, "w") as f:
        f.write(TU)
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-I", b.CSRC, src, "-o", out], check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        asm = f.read()
    res = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        if m.group(1) in KERNELS:
            ins = [l.split()[0] for l in m.group(2).split("\n") if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
            res[KERNELS[m.group(1)]] = collections.Counter(ins)
    assert set(res) == set(KERNELS.values()), sorted(set(KERNELS.values()) - set(res))
    for name in sorted(res):
        c = res[name]
        print("%-26s v_* %4d  v_pk_* %4d  v_sub_f32 %3d  v_add_f32 %3d  v_max* %3d  s_* %4d" % (
            name, _n(c, "v_"), _n(c, "v_pk_"), _n(c, "v_sub_f32"), _n(c, "v_add_f32"), _n(c, "v_max"), _n(c, "s_")))
    return res


def _n(counter, prefix):
    return sum(n for k, n in counter.items() if k.startswith(prefix))


def test_transform_arithmetic_is_packed(counts):
    """Two or four channels per lane: every addition and subtraction of the transforms, of bias and residual and of the fused LayerNorm is a
    v_pk_add_f32 (a subtraction is one with a negated operand).  Only the classifier kernel has single-lane additions of its own: the four of
    ((s0 + s1) + s2) + s3 + bias per output, at most twice if the compiler unrolls that loop by two."""
    for name, c in counts.items():
        assert _n(c, "v_sub_f32") == 0, (name, _n(c, "v_sub_f32"))
        assert _n(c, "v_add_f32") <= (8 if name == "k_wino4_out_cls<2>" else 0), (name, _n(c, "v_add_f32"))


def test_instruction_totals(counts):
    """All VALU instructions in the text of the frame's two transforms.  Input: 12 1-D transforms x 14 operations x 2 halves = 336, the fused
    LayerNorm path on top of it, addressing; it was 1299.  Output: (6 + 4) x 10 x 2 = 200, bias + residual 64, ReLU 64 (one v_maximum3_f32 per value), addressing: about 330; it was 765."""
    assert _n(counts["k_wino4_in_c<4>"], "v_") <= 650, _n(counts["k_wino4_in_c<4>"], "v_")
    assert _n(counts["k_wino4_out_c<4, false>"], "v_") <= 420, _n(counts["k_wino4_out_c<4, false>"], "v_")
