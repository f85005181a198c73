"""Operator-level parity checks shared by the emulator tests (CPU, numpy "HBM") and the GPU tests (torch-ROCm HBM).
Each check builds seeded inputs, runs ONE C-ABI op, and compares with the same op in plain PyTorch fp32 (or fp64) on CPU.
The Guarded* mems put every tensor between guard bands and check them in verify() (tests/ops_edge_cases.py).
conv_group / cache_subsample / conv1x1_rows check launch forms of a frame -- several convs in one grid, both cache entries in one launch, a
conv on one row class -- against the single-operator form of the same arithmetic bit for bit; the gate against fp64 is that form's."""
import numpy as np
import torch
import torch.nn.functional as F


class NumpyMem:
    """'device' memory for the emulator: host arrays."""
    def put(self, a):
        return np.ascontiguousarray(a, dtype=np.float32)

    def empty(self, shape):
        return np.full(shape, 7e7, np.float32)

    def ptr(self, a):
        return None if a is None else a.ctypes.data

    def get(self, a):
        return a

    stream = None


class TorchMem:
    """device memory on cuda:0 through torch-ROCm (plumbing only)."""
    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def empty(self, shape):
        return torch.full(tuple(shape), 7e7, dtype=torch.float32, device="cuda")

    def ptr(self, a):
        return None if a is None else a.data_ptr()

    def get(self, a):
        torch.cuda.synchronize()
        return a.cpu().numpy()

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream


class _Guarded:
    """Guard bands around every tensor a mem hands out: the tensor is the interior of a larger allocation with GUARD bytes in front and
    behind (a multiple of 256, so the interior keeps a fresh allocation's 256-byte alignment).  The bands of an input (put) hold quiet
    NaNs -- an out-of-range read that reaches a result poisons it; one that is discarded is allowed -- and those of an output (empty) a
    fixed pattern, itself a NaN.  A NaN cannot poison a MAXIMUM written as a comparison (`v > best`, td_out.h td_first_max: false with a
    NaN on either side), so put(a, poison=BIG_BITS) fills the bands with 2^127 instead: finite -- a tap read with weight exactly 0 is still
    discarded (0 * 2^127 = 0, where 0 * inf would be a NaN) -- and larger than any logit, so a maximum that takes it in names another
    class.  What feeds a maximum runs once per fill of POISONS and must give the same bytes both times.
    verify() asserts that every band of every tensor handed out since the last verify() still holds its fill bit for bit, and that every
    output interior is finite and free of the 7e7 fill; then the mem forgets those tensors.  The mem owns the allocations until then:
    mem.ptr(mem.put(x)) on a temporary stays valid through the kernel call.
    empty(shape, unwritten_rows=mask): an output of which the call writes only some rows (a boolean per index of the first axis, True = must
    NOT be written): verify() holds those rows to the 7e7 fill bit for bit and every other row to "finite and fully written" as usual."""
    GUARD = 4096                     # bytes per band
    IN_BITS = 0x7FC00000             # quiet NaN
    BIG_BITS = 0x7F000000            # 2^127: the input fill a comparison cannot swallow
    POISONS = (IN_BITS, BIG_BITS)
    OUT_BITS = 0x7FC5A5A5            # a quiet NaN with a payload: a fixed pattern no kernel produces
    FILL = 7e7

    def __init__(self):
        self._live = []

    def _new(self, shape, bits, is_out, keep=None):
        shape = tuple(int(d) for d in shape)
        n, g = int(np.prod(shape, dtype=np.int64)), self.GUARD // 4
        buf = self._words(g + n + g, bits)
        inner = self._interior(buf, g, n, shape)
        assert self.ptr(inner) % 256 == 0, "interior lost the allocation's alignment"
        if keep is not None:
            keep = np.asarray(keep, bool)
            assert keep.shape == shape[:1], "unwritten_rows: one boolean per index of the first axis"
        self._live.append((buf, n, bits, is_out, shape, keep))
        return inner

    def put(self, a, poison=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert poison is None or poison in self.POISONS, poison
        t = self._new(a.shape, self.IN_BITS if poison is None else poison, False)
        self._store(t, a)
        return t

    def empty(self, shape, unwritten_rows=None):
        t = self._new(shape, self.OUT_BITS, True, unwritten_rows)
        self._store(t, np.float32(self.FILL))
        return t

    def verify(self, untouched=False, finite=True):
        """untouched: the calls since the last verify() were refused -- every output interior must still hold its fill instead.
        finite = False: the inputs held non-finite values on purpose (tests/nonfinite_cases.py), so the outputs may; the bands and "fully
        written" are checked as always."""
        live, self._live = self._live, []
        g = self.GUARD // 4
        for i, (buf, n, bits, is_out, shape, keep) in enumerate(live):
            words = self._host_words(buf)
            what = "%s #%d %s" % ("output" if is_out else "input", i, shape)
            for name, band, base in (("in front of", words[:g], -g), ("behind", words[g + n:], n)):
                bad = np.flatnonzero(band != bits)
                assert bad.size == 0, "guard band %s %s overwritten: %d words, the first at element %d (0x%08x)" % (
                    name, what, bad.size, base + int(bad[0]), int(band[bad[0]]) & 0xFFFFFFFF)
            if is_out and untouched:
                assert (words[g:g + n].view(np.float32) == np.float32(self.FILL)).all(), "%s was written by a call that should have launched nothing" % what
            elif is_out:
                f = words[g:g + n].view(np.float32)
                if keep is not None:                                   # rows the call must leave alone: still the fill; the others as any output
                    f = f.reshape(shape[0], -1)
                    kept = f[keep].view(np.int32) != np.float32(self.FILL).view(np.int32)
                    assert not kept.any(), "%s: %d elements in %d rows that must stay unwritten were written" % (what, int(kept.sum()), int(kept.any(1).sum()))
                    f = f[~keep]
                assert not finite or np.isfinite(f).all(), "%s: %d non-finite values (a read outside an input reached the result)" % (what, int((~np.isfinite(f)).sum()))
                assert not (f == np.float32(self.FILL)).any(), "%s: %d elements were never written" % (what, int((f == np.float32(self.FILL)).sum()))


class GuardedNumpyMem(_Guarded, NumpyMem):
    """NumpyMem with guard bands (see _Guarded): for the emulator."""
    def _words(self, total, bits):
        raw = np.empty(total + 64, np.int32)
        off = (-(raw.ctypes.data // 4)) % 64                   # the first 256-byte boundary
        buf = raw[off:off + total]
        buf[:] = bits
        return buf

    def _interior(self, buf, g, n, shape):
        return buf[g:g + n].view(np.float32).reshape(shape)

    def _store(self, t, a):
        t[...] = a

    def _host_words(self, buf):
        return buf


class GuardedTorchMem(_Guarded, TorchMem):
    """TorchMem with guard bands (see _Guarded): device memory."""
    def _words(self, total, bits):
        return torch.full((total,), bits, dtype=torch.int32, device="cuda")

    def _interior(self, buf, g, n, shape):
        return buf[g:g + n].view(torch.float32).view(shape)

    def _store(self, t, a):
        if np.ndim(a) == 0:
            t.fill_(float(a))
        else:
            t.copy_(torch.from_numpy(a))

    def _host_words(self, buf):
        torch.cuda.synchronize()
        return buf.cpu().numpy()


def conv(lib, mem, H, W, Cin, Cout, KS, stride, dil, act, resid, tile=None, seed=0, tol=1e-4, opts=None):
    """opts: dict of tdnet_opts fields for this one call (e.g. {"winograd": 0}); None = library defaults."""
    import ctypes
    g = np.random.default_rng(seed)
    x = g.standard_normal((H, W, Cin)).astype(np.float32)
    w = (g.standard_normal((Cout, Cin, KS, KS)) * (1.0 / np.sqrt(Cin * KS * KS))).astype(np.float32)
    b = g.standard_normal(Cout).astype(np.float32)
    pad = dil * (KS // 2)
    ref = F.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w), torch.from_numpy(b), stride, pad, dil)
    Ho, Wo = ref.shape[-2:]
    r = None
    if resid:
        r = g.standard_normal((Ho, Wo, Cout)).astype(np.float32)
        ref = ref + torch.from_numpy(r).permute(2, 0, 1)[None]
    if act == 1:
        ref = F.relu(ref)
    elif act == 2:
        ref = F.leaky_relu(ref, 0.01)
    dx, dr, out = mem.put(x), (mem.put(r) if resid else None), mem.empty((Ho, Wo, Cout))
    o = lib.opts(**(opts or {}))
    rc = lib.tdnet_op_conv2d(mem.ptr(dx), H, W, Cin, w.ctypes.data, b.ctypes.data, Cout, KS, stride, dil, mem.ptr(dr), act,
                             ctypes.byref(o), -1 if tile is None else tile, mem.ptr(out), mem.stream)
    lib.check(rc)
    err = float(np.abs(mem.get(out) - ref[0].permute(1, 2, 0).numpy()).max())
    assert err <= tol, ("conv", H, W, Cin, Cout, KS, stride, dil, act, resid, tile, err)
    return err


def half(a):
    """fp32 -> fp16, round to nearest even, widened to fp64: what k_f2h, the kernels' staging converts and the host weight packing do."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def t16(ref):
    """The gate of an fp16-MFMA product with fp32 accumulation and an fp32 result against fp64 on the same rounded operands
    (test_gpu_fp16._conv16's): what is left is the fp32 summation."""
    return 3e-5 * max(1.0, float(np.abs(ref).max()))


def gate_f16(ref):
    """Per-element gate of a result STORED as fp16: half an fp16 ulp of the value (2^-11 relative) + t16, the fp32 value's own error, which may
    also have put it on the other side of a rounding boundary."""
    return 2.0 ** -11 * np.abs(ref) + t16(ref)


def assert_within(got, ref, gate, what):
    """|got - ref| <= gate (a scalar or per element); the message carries the worst element.  Returns max(err / gate)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = err / gate
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[i] <= 1.0, what + ("worst element %s: got %.9g, reference %.9g, error %.3e, gate %.3e; %d of %d outside" % (
        i, float(np.asarray(got)[i]), float(ref[i]), float(err[i]), float(np.broadcast_to(gate, err.shape)[i]), int((ratio > 1.0).sum()), err.size),)
    return float(ratio[i])


def conv_f16_inputs(seed, H, W, Cin, Cout, KS, x=None):
    """The seeded (generator, input, weight, bias) of conv_f16io; x: an input given by the caller (members of a group that read one map)."""
    g = np.random.default_rng(seed)
    drawn = g.standard_normal((H, W, Cin)).astype(np.float32)          # drawn either way: the weights do not depend on whether x was given
    x = drawn if x is None else x
    w = (g.standard_normal((Cout, Cin, KS, KS)) / np.sqrt(Cin * KS * KS)).astype(np.float32)
    b = g.standard_normal(Cout).astype(np.float32)
    return g, x, w, b


def conv_f16io(lib, mem, H, W, Cin, Cout, KS, stride, dil, act, resid, tile=None, seed=0, want_out=False, in16=True, out16=True, resid16=False,
               x=None, bias=True):
    """The fp16-MFMA conv of tdnet_opts.precision = 1 (fp32 accumulate) against an fp64 evaluation on the operands as the kernel rounds them:
    the weights (host packing) and the input (k_f2h for an fp16 map, the staging convert for an fp32 one) to fp16; the residual to fp16 only
    where it is an fp16 map (in16); the bias not at all.  An fp32 result (out16 = False) is gated at t16, an fp16 map per element at gate_f16.
    in16 = out16 = True: tdnet_op_conv2d_f16io, else tdnet_op_conv2d_f16mix.  resid16: the residual holds fp16 values already, so that the
    in16 and in32 forms add the same numbers.  x: the input instead of the seeded one; bias = False: a NULL bias.  Returns max(error / gate)."""
    g, x, w, b = conv_f16_inputs(seed, H, W, Cin, Cout, KS, x)
    pad = dil * (KS // 2)
    ref = F.conv2d(torch.from_numpy(half(x)).permute(2, 0, 1)[None], torch.from_numpy(half(w)), torch.from_numpy(b).double() if bias else None, stride, pad, dil)
    Ho, Wo = ref.shape[-2:]
    r = None
    if resid:
        r = g.standard_normal((Ho, Wo, Cout)).astype(np.float32)
        if resid16:
            r = r.astype(np.float16).astype(np.float32)
        ref = ref + torch.from_numpy(half(r) if in16 else r.astype(np.float64)).permute(2, 0, 1)[None]
    if act == 1:
        ref = F.relu(ref)
    elif act == 2:
        ref = F.leaky_relu(ref, 0.01)
    ref = ref[0].permute(1, 2, 0).numpy()
    dx, dr, out = mem.put(x), (mem.put(r) if resid else None), mem.empty((Ho, Wo, Cout))
    t, pb = -1 if tile is None else tile, b.ctypes.data if bias else None
    if in16 and out16:
        lib.check(lib.tdnet_op_conv2d_f16io(mem.ptr(dx), H, W, Cin, w.ctypes.data, pb, Cout, KS, stride, dil, mem.ptr(dr), act, t,
                                            mem.ptr(out), mem.stream))
    else:
        lib.check(lib.tdnet_op_conv2d_f16mix(mem.ptr(dx), H, W, Cin, w.ctypes.data, pb, Cout, KS, stride, dil, mem.ptr(dr), act, t,
                                             int(in16), int(out16), mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    ratio = assert_within(got, ref, gate_f16(ref) if out16 else t16(ref), ("conv_f16io", H, W, Cin, Cout, KS, stride, dil, act, resid, tile, in16, out16))
    return (ratio, got) if want_out else ratio


def conv_group(lib, mem, members, tile, in16=True, out16=True, fusion=None, grouped=True, seed=0):
    """tdnet_op_conv_group_f16 -- run_conv_group, the grouping decision and the launch of a frame -- on up to three members
    (H, W, Cin, Cout, KS, stride, dil, act, bias, share): bias False = a NULL bias; share = None or the index of an EARLIER member whose
    input map this one reads (one device tensor).  Every member's output equals BIT FOR BIT the output of conv_f16io on that member alone at
    the same tile and storage (which holds it to the rounding-aware fp64 gate): k_conv_igemm_h_group runs the body of k_conv_igemm_h on a
    member-local block index, the same products in the same order.  The entry's flag must say `grouped`.  fusion: tdnet_opts.fusion, None =
    the library default.  Members draw their weights and inputs from different seeds, so one that ran on a neighbour's arguments shows."""
    import ctypes
    ng = len(members)
    xs, ws, bs, singles, shapes = [], [], [], [], []
    for i, (H, W, Cin, Cout, KS, stride, dil, act, bias, share) in enumerate(members):
        x = None
        if share is not None:
            assert share < i and members[share][:3] == (H, W, Cin), ("conv_group: a shared input needs an earlier member of the same map", members)
            x = xs[share]
        _, x, w, b = conv_f16_inputs(seed + 101 * i, H, W, Cin, Cout, KS, x)
        _, one = conv_f16io(lib, mem, H, W, Cin, Cout, KS, stride, dil, act, False, tile, seed=seed + 101 * i, want_out=True, in16=in16, out16=out16,
                            x=x, bias=bias)
        xs.append(x); ws.append(w); bs.append(b if bias else None); singles.append(one); shapes.append(one.shape)
    dxs = []
    for i, m in enumerate(members):
        dxs.append(dxs[m[9]] if m[9] is not None else mem.put(xs[i]))
    outs = [mem.empty(sh) for sh in shapes]
    ints = lambda j: (ctypes.c_int * ng)(*[int(m[j]) for m in members])
    ptrs = lambda v: (ctypes.c_void_p * ng)(*v)
    flag = ctypes.c_int(-1)
    fus = lib.opts().fusion if fusion is None else int(fusion)
    lib.check(lib.tdnet_op_conv_group_f16(ng, ptrs([mem.ptr(d) for d in dxs]), ints(0), ints(1), ints(2), ptrs([w.ctypes.data for w in ws]),
                                          ptrs([None if b is None else b.ctypes.data for b in bs]), ints(3), ints(4), ints(5), ints(6), ints(7),
                                          ptrs([mem.ptr(o) for o in outs]), -1 if tile is None else tile, int(in16), int(out16), fus,
                                          ctypes.byref(flag), mem.stream))
    assert flag.value == int(grouped), ("conv_group: grouped flag", flag.value, "expected", int(grouped), members, tile, in16, out16, fus)
    for i, (o, one) in enumerate(zip(outs, singles)):
        got = np.array(mem.get(o))
        assert np.array_equal(got, one), ("conv_group: member %d != the single launch" % i, members, tile, in16, out16, int((got != one).sum()),
                                          float(np.nanmax(np.abs(got - one))))
    return flag.value


def cache_subsample(lib, mem, h, w, C1, C2, seed=0):
    """tdnet_op_cache_subsample (k_subsample2 through encode_frame's launch): both outputs equal x[::4, ::4] BIT FOR BIT."""
    g = np.random.default_rng(seed + 131 * h + w)
    q = g.random((h, w, C1), dtype=np.float32) - 0.5
    v = g.random((h, w, C2), dtype=np.float32) - 0.5
    hk, wk = (h - 1) // 4 + 1, (w - 1) // 4 + 1
    dq, dv, oq, ov = mem.put(q), mem.put(v), mem.empty((hk, wk, C1)), mem.empty((hk, wk, C2))
    lib.check(lib.tdnet_op_cache_subsample(mem.ptr(dq), mem.ptr(dv), h, w, C1, C2, mem.ptr(oq), mem.ptr(ov), mem.stream))
    for name, got, src in (("q", mem.get(oq), q), ("v", mem.get(ov), v)):
        exp = src[::4, ::4]
        assert exp.shape == (hk, wk, src.shape[2])
        bad = np.asarray(got) != exp
        assert not bad.any(), ("cache_subsample: %s != x[::4, ::4]" % name, h, w, C1, C2, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))


def conv1x1_rows(lib, mem, H, W, Cin, Cout, opts, ny, cy, act=1, seed=0, stays_exact=False):
    """tdnet_op_conv1x1_rows -- run_ds_rows, the 1x1 downsample conv of one row-parity chain: a batched GEMM, batch = image row, one weight set --
    on the rows y % ny == cy of an H x W map.  Three checks:
      1. the written rows equal BIT FOR BIT the same rows of tdnet_op_conv2d on the whole map with the same opts: the plan is the same, and the
         K order of a dot product does not depend on where its row sits in a tile;
      2. those rows -- and only those go to the comparison -- pass the gate a 1x1 conv on that kernel already has: conv()'s 1e-4 against the fp32
         torch conv with bias and activation; with precision >= 2 also split_conv()'s: the products alone (no bias, no activation) against
         fp64 at SPLIT_GATE over the fp32 CPU evaluation's error on the same rows, and the split kernel really ran (its bits are not the
         exact-fp32 kernel's), or, stays_exact, the plan has no split kernel for this conv and it keeps the exact kernel's bits;
      3. the rows of the other classes still hold the output's fill: asserted here, and again by mem.verify() through unwritten_rows.
    A class without rows (H <= cy) launches nothing.  Returns {"cpu32" | "exact" | "split": (max, rms)} with precision >= 2, else the max error."""
    import ctypes
    g = np.random.default_rng(seed)
    x = g.standard_normal((H, W, Cin)).astype(np.float32)
    w = (g.standard_normal((Cout, Cin, 1, 1)) / np.sqrt(Cin)).astype(np.float32)
    b = g.standard_normal(Cout).astype(np.float32)
    tx, tw = torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w)
    nhwc = lambda t: t[0].permute(1, 2, 0).numpy()
    ref32 = F.conv2d(tx, tw, torch.from_numpy(b))
    ref32 = nhwc(F.relu(ref32) if act == 1 else F.leaky_relu(ref32, 0.01) if act == 2 else ref32)
    other = np.arange(H) % ny != cy
    dx = mem.put(x)

    def rows(kw, bias, a):
        out = mem.empty((H, W, Cout), unwritten_rows=other)
        lib.check(lib.tdnet_op_conv1x1_rows(mem.ptr(dx), H, W, Cin, w.ctypes.data, b.ctypes.data if bias else None, Cout, a, ctypes.byref(lib.opts(**kw)),
                                            ny, cy, mem.ptr(out), mem.stream))
        got = np.array(mem.get(out))
        assert (got[other].view(np.int32) == np.float32(mem.FILL).view(np.int32)).all(), ("conv1x1_rows: rows of another class were written", H, W, Cin, Cout, kw, ny, cy)
        return got[cy::ny]

    whole = mem.empty((H, W, Cout))
    lib.check(lib.tdnet_op_conv2d(mem.ptr(dx), H, W, Cin, w.ctypes.data, b.ctypes.data, Cout, 1, 1, 1, None, act, ctypes.byref(lib.opts(**opts)), -1,
                                  mem.ptr(whole), mem.stream))
    whole = np.array(mem.get(whole))
    got = rows(opts, True, act)
    what = ("conv1x1_rows", H, W, Cin, Cout, opts, ny, cy)
    assert got.shape[0] == len(range(cy, H, ny))
    assert np.array_equal(got, whole[cy::ny]), what + ("!= the rows of the whole-map conv", int((got != whole[cy::ny]).sum()))
    if got.shape[0] == 0:
        return None
    err = float(np.abs(got - ref32[cy::ny]).max())
    assert err <= 1e-4, what + (err,)
    if opts.get("precision", 0) < 2:
        return err
    ref = nhwc(F.conv2d(tx.double(), tw.double()))[cy::ny]
    errs = {"cpu32": max_rms(nhwc(F.conv2d(tx, tw))[cy::ny], ref)}
    outs = {name: rows(kw, False, 0) for name, kw in (("exact", dict(opts, precision=0)), ("split", opts))}
    for name in outs:
        errs[name] = max_rms(outs[name], ref)
    label = "conv1x1_rows %dx%d %d->%d %s rows %d mod %d" % (H, W, Cin, Cout, opts, cy, ny)
    if stays_exact:
        assert np.array_equal(outs["exact"], outs["split"]), ("not the bits of the exact-fp32 kernel", label)
    else:
        assert not np.array_equal(outs["exact"], outs["split"]), ("the split kernel did not run: the bits of the exact-fp32 kernel", label)
    return _split_gate(label, errs, "cpu32", SPLIT_GATE)


def _stem_case(H, W, seed, rounded):
    """Inputs of the stem checks and the fp64 conv -> ReLU -> max-pool, NHWC; rounded: on the image and the weights as the fp16-MFMA stem
    rounds them (the image while staging, the weights when packed)."""
    g = np.random.default_rng(seed)
    img = g.standard_normal((3, H, W)).astype(np.float32)
    w = (g.standard_normal((64, 3, 7, 7)) * 0.1).astype(np.float32)
    b = g.standard_normal(64).astype(np.float32)
    cast = half if rounded else (lambda a: a.astype(np.float64))
    ref = F.max_pool2d(F.relu(F.conv2d(torch.from_numpy(cast(img))[None], torch.from_numpy(cast(w)), torch.from_numpy(b).double(), 2, 3)), 3, 2, 1)
    return img, w, b, ref[0].permute(1, 2, 0).numpy()


def stem(lib, mem, H, W, seed=0, tol=1e-4, opts=None, want_out=False):
    """tdnet_op_stem against fp64.  precision = 1 (the fp16-MFMA stem writing fp32): the reference is evaluated on the rounded image and
    weights and the gate is t16 instead of tol (the max-pool picks, it adds no error)."""
    import ctypes
    f16 = (opts or {}).get("precision") == 1
    img, w, b, ref = _stem_case(H, W, seed, f16)
    di, out = mem.put(img), mem.empty(ref.shape)
    lib.check(lib.tdnet_op_stem(mem.ptr(di), H, W, w.ctypes.data, b.ctypes.data, ctypes.byref(lib.opts(**(opts or {}))), mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    err = float(np.abs(got - ref).max())
    assert err <= (t16(ref) if f16 else tol), ("stem", H, W, opts, err)
    return (err, got) if want_out else err


def stem_f16(lib, mem, H, W, seed=0, tile=None):
    """tdnet_op_stem_f16 (the fp16-MFMA stem writing an fp16 map, the fp16 max-pool) against fp64 on the rounded image and weights, per
    element at gate_f16: the stored map is half an ulp from the fp32 value, the pool picks (the values are >= 0 behind the ReLU, so the
    largest gate of a window is that of its maximum).  And bit for bit half() of tdnet_op_stem with precision = 1 on the same tile: the
    OUT16 epilogue rounds the value the fp32 epilogue stores, and the maximum commutes with a monotone rounding."""
    img, w, b, ref = _stem_case(H, W, seed, True)
    di, out = mem.put(img), mem.empty(ref.shape)
    lib.check(lib.tdnet_op_stem_f16(mem.ptr(di), H, W, w.ctypes.data, b.ctypes.data, -1 if tile is None else tile, mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    ratio = assert_within(got, ref, gate_f16(ref), ("stem_f16", H, W, tile))
    if tile is None:
        _, wide = stem(lib, mem, H, W, seed, opts={"precision": 1}, want_out=True)
        assert np.array_equal(got, wide.astype(np.float16).astype(np.float32)), ("stem_f16 != half(fp32-output stem)", H, W)
    return ratio


def maxpool(lib, mem, H, W, C, mode, seed=0):
    """tdnet_op_maxpool on N(0, 1) data -- negative values, so a padding value of 0 instead of -inf shows at every border -- against
    F.max_pool2d, BIT FOR BIT: mode 0 the fp32 maximum; modes 1 and 2 half() of it (the maximum commutes with a monotone rounding, so
    rounding the input first (2) or the result (1) is the same)."""
    g = np.random.default_rng(seed + 1000 * mode + H * 131 + W)
    x = g.standard_normal((H, W, C)).astype(np.float32)
    ref = F.max_pool2d(torch.from_numpy(x).permute(2, 0, 1)[None], 3, 2, 1)[0].permute(1, 2, 0).numpy()
    assert (ref < 0).any()
    if mode:
        ref = ref.astype(np.float16).astype(np.float32)
    dx, out = mem.put(x), mem.empty(ref.shape)
    lib.check(lib.tdnet_op_maxpool(mem.ptr(dx), H, W, C, mode, mem.ptr(out), mem.stream))
    got = np.array(mem.get(out))
    assert np.array_equal(got, ref), ("maxpool", H, W, C, mode, int((got != ref).sum()), float(np.abs(got - ref).max()))


def attention(lib, mem, Lq, Lk, DV, bias=True, resid=True, seed=0, tol=1e-4, qk_scale=1.0, spike=False, online=0, ln=False, ramp=False):
    """online: the single-pass schedule; ln: also check the plane LayerNorm computed from the epilogue's strip statistics;
    ramp: keys sorted by growing score for every query, so the online reference has to move again and again.
    online = 16 (the fp16-MFMA kernel): the reference is fp64 on q, k, v' rounded to fp16, gated per element (below); tol is not used."""
    g = np.random.default_rng(seed)
    q = (qk_scale * g.standard_normal((Lq, 64))).astype(np.float32)
    k = (qk_scale * g.standard_normal((Lk, 64))).astype(np.float32)
    if spike:                                  # one key dominating one query row: exercises the max subtraction
        k[Lk // 2] = 6.0 * q[Lq // 3] / max(1e-6, float(np.linalg.norm(q[Lq // 3]))) * 8.0
    if ramp:                                   # k_j = (j / Lk) * 40 * u with q . u > 0 for all q: scores grow along the key axis by ~100 log2 units
        u = np.ones(64, np.float32) / 8.0
        q = np.abs(q) + 0.5
        k = (np.arange(Lk, dtype=np.float32)[:, None] / max(1, Lk - 1)) * 40.0 * u[None, :] + 0.1 * k
    v = g.standard_normal((Lk, DV)).astype(np.float32)
    b = g.standard_normal(DV).astype(np.float32)
    r = g.standard_normal((Lq, DV)).astype(np.float32)
    f16 = (int(online) & ~(32 | 64)) == 16
    if f16:
        # the fp16-MFMA kernel rounds q, k and v' on the way into the MFMAs (td_attn_h.h); q is rounded AFTER its fp32 multiplication by
        # log2(e) / 8, so the scores are in log2 units and the softmax is 2^s: softmax(ln 2 * qs k^T) with qs = half(q * log2(e) / 8)
        qs = half(q * (np.float32(1.4426950408889634) / np.float32(8.0)))
        prob = torch.softmax(float(np.log(2.0)) * (torch.from_numpy(qs) @ torch.from_numpy(half(k)).T), 1)
        ref = prob @ torch.from_numpy(half(v))
        amp = (prob @ torch.from_numpy(np.abs(half(v)))).numpy()          # A = sum_j p_j |v'_j| >= |R|
    else:
        ref = torch.softmax(torch.from_numpy(q).double() @ torch.from_numpy(k).double().T / 8.0, 1) @ torch.from_numpy(v).double()
    if bias:
        ref = ref + torch.from_numpy(b)
    if resid:
        ref = ref + torch.from_numpy(r)
    dq, dk, dv_, db, dr = mem.put(q), mem.put(k), mem.put(v), mem.put(b), mem.put(r)
    out = mem.empty((Lq, DV))
    gg = g.uniform(0.5, 1.5, Lq).astype(np.float32)
    bb = g.standard_normal(Lq).astype(np.float32)
    dg, dbb, lnout = (mem.put(gg), mem.put(bb), mem.empty((Lq, DV))) if ln else (None, None, None)
    lib.check(lib.tdnet_op_attention(mem.ptr(dq), mem.ptr(dk), mem.ptr(dv_), mem.ptr(db) if bias else None,
                                     mem.ptr(dr) if resid else None, Lq, Lk, DV, int(online), mem.ptr(dg), mem.ptr(dbb), mem.ptr(lnout),
                                     mem.ptr(out), mem.stream))
    if f16:
        # P is rounded to fp16 as well, 2^-11 relative per element: numerator and normalisation together move an output by at most 2^-10 A;
        # the rest (fp32 scores, softmax and accumulation) is what the fp32 kernels are held to: 1e-4
        got = np.array(mem.get(out))
        assert_within(got, ref.numpy(), 2.0 ** -10 * amp + 1e-4, ("attention fp16", Lq, Lk, DV, bias, resid, online))
        err = float(np.abs(got - ref.numpy()).max())
        if ln:                                 # the plane LayerNorm of the kernel's OWN output, from the epilogue's strip statistics, at the fp32 LayerNorm tolerance
            g64 = got.astype(np.float64)
            lref = (g64 - g64.mean(0)) / np.sqrt(g64.var(0) + 1e-5) * gg.astype(np.float64)[:, None] + bb.astype(np.float64)[:, None]
            lerr = float(np.abs(mem.get(lnout) - lref).max())
            assert lerr <= 1e-4, ("attention fp16 + layernorm", Lq, Lk, DV, online, lerr)
        return err
    err = float(np.abs(mem.get(out) - ref.float().numpy()).max())
    assert err <= tol, ("attention", Lq, Lk, DV, bias, resid, online, err)
    if ln:
        lref = F.layer_norm(ref.float().T.contiguous(), (Lq,), torch.from_numpy(gg), torch.from_numpy(bb), 1e-5).T.numpy()
        lerr = float(np.abs(mem.get(lnout) - lref).max())
        assert lerr <= 2 * tol, ("attention+layernorm", Lq, Lk, DV, online, lerr)
    return err


# ---- tdnet_opts.precision = 2 / 3: fp32 operands as three bf16 parts, six bf16-MFMA products per product (td_gemm_b3.h, td_conv_ad_b3.h,
# td_attn_b3.h).  A product is carried to ~2^-26; dropping one of the three third-order terms costs ~2^-18 per product, a second-order
# one ~2^-9 -- both far below the 1e-4 of conv() / attention().  So the split kernels are gated against fp64 RELATIVE to a yardstick on
# the same inputs, in max and in rms error (rms is the sharp statistic: a lost third-order term moves it by 5.9x .. 19x, max by 3x .. 10x):
#   * non-Winograd routes: the distance of the plain fp32 torch evaluation on the CPU to fp64.  Under the emulator the unmodified kernels
#     are at most 1.17x (rms) / 1.25x (max) of it; the gate is 2x / 3x because the device's MFMA adds the 16 products of an instruction in
#     its own order.  The rms factor stays below 3.0, half the smallest lost-product ratio.
#   * Winograd routes (both kernels are limited by the transforms, a direct fp32 conv is not comparable): the relation test_gpu_b3 holds
#     the mode to, 1.25x max / 1.1x rms of the exact-fp32 Winograd kernel ({"winograd": 4}).
# The floors are test_gpu_b3's: at Lk = 1 the attention is exact and every error is 0.
SPLIT_GATE = {"max": (3.0, 1e-7), "rms": (2.0, 1e-9)}                  # over the CPU fp32 evaluation's own error
SPLIT_WINO_GATE = {"max": (1.25, 1e-7), "rms": (1.1, 1e-9)}           # over the exact-fp32 Winograd kernel's error
SPLIT_DATA = ("normal", "abs", "scaled")


def pow2_scales(n):
    """Per-channel powers of two from 2^-6 to 2^6, neighbours far apart: the 8 values a lane hands to one MFMA span the whole range."""
    return np.exp2(((np.arange(n) * 5) % 13 - 6).astype(np.float64)).astype(np.float32)


def max_rms(got, ref):
    e = np.abs(np.asarray(got, np.float64) - ref)
    return float(e.max()), float(np.sqrt((e * e).mean()))


def _split_gate(what, errs, yard, gate):
    """errs: {"cpu32" | "exact" | "split": (max, rms)} against fp64; asserts errs["split"] against errs[yard] and prints every figure."""
    (fm, cm), (fr, cr) = gate["max"], gate["rms"]
    s, y = errs["split"], errs[yard]
    ratio = lambda a, b: "x%.2f" % (a / b) if b > 0 else "-"
    print("split gate %s: cpu32 %.2e / %.2e | exact %.2e / %.2e (%s / %s) | split %.2e / %.2e (%s / %s of cpu32%s)" % (
        what, *errs["cpu32"], *errs["exact"], ratio(errs["exact"][0], errs["cpu32"][0]), ratio(errs["exact"][1], errs["cpu32"][1]),
        *s, ratio(s[0], errs["cpu32"][0]), ratio(s[1], errs["cpu32"][1]),
        "" if yard == "cpu32" else "; %s / %s of exact" % (ratio(s[0], y[0]), ratio(s[1], y[1]))))
    assert s[1] <= fr * y[1] + cr, ("split kernel rms error", what, yard, errs)
    assert s[0] <= fm * y[0] + cm, ("split kernel max error", what, yard, errs)
    return errs


def _conv_data(g, H, W, Cin, Cout, KS, data):
    x = g.standard_normal((H, W, Cin)).astype(np.float32)
    w = (g.standard_normal((Cout, Cin, KS, KS)) / np.sqrt(Cin * KS * KS)).astype(np.float32)
    if data == "abs":                                                  # behind a ReLU: the sums of a product row cancel less
        x = np.abs(x)
    elif data == "scaled":                                             # exact in every format: the same products, other exponents per channel
        s = pow2_scales(Cin)
        x, w = x * s, w / s[None, :, None, None]
    else:
        assert data == "normal", data
    return x, w


def split_conv(lib, mem, H, W, Cin, Cout, KS, stride, dil, opts, wino=False, data="normal", seed=0, stays_exact=False):
    """A conv of tdnet_opts.precision = 2 / 3 (opts) through tdnet_op_conv2d without bias, residual or activation -- the products alone --
    against fp64, next to the fp32 torch conv on the CPU and to the exact-fp32 kernel of the same route (opts with precision 0; wino: the
    Winograd kernel {"winograd": 4}) on the same inputs.  Gate: SPLIT_GATE over the CPU evaluation, wino: SPLIT_WINO_GATE over the exact
    kernel.  Also: the split kernel really ran -- its sums are not the fp32 MFMA's bit for bit --, or, stays_exact, the plan has no split
    kernel for this conv and it keeps the exact-fp32 kernel's bits.  Returns the three (max, rms)."""
    import ctypes
    g = np.random.default_rng(seed)
    x, w = _conv_data(g, H, W, Cin, Cout, KS, data)
    tx, tw, pad = torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w), dil * (KS // 2)
    ref = F.conv2d(tx.double(), tw.double(), None, stride, pad, dil)[0].permute(1, 2, 0).numpy()
    errs = {"cpu32": max_rms(F.conv2d(tx, tw, None, stride, pad, dil)[0].permute(1, 2, 0).numpy(), ref)}
    dx, outs = mem.put(x), {}
    for name, kw in (("exact", {"winograd": 4} if wino else dict(opts, precision=0)), ("split", opts)):
        out = mem.empty(ref.shape)
        lib.check(lib.tdnet_op_conv2d(mem.ptr(dx), H, W, Cin, w.ctypes.data, None, Cout, KS, stride, dil, None, 0, ctypes.byref(lib.opts(**kw)), -1,
                                      mem.ptr(out), mem.stream))
        outs[name] = np.array(mem.get(out))
        errs[name] = max_rms(outs[name], ref)
    what = "conv %dx%d %d->%d k%d s%d d%d %s %s" % (H, W, Cin, Cout, KS, stride, dil, opts, data)
    if stays_exact:
        assert np.array_equal(outs["exact"], outs["split"]), ("not the bits of the exact-fp32 kernel", what)
    else:
        assert not np.array_equal(outs["exact"], outs["split"]), ("the split kernel did not run: the bits of the exact-fp32 kernel", what)
    return _split_gate(what, errs, "exact" if wino else "cpu32", SPLIT_WINO_GATE if wino else SPLIT_GATE)


def split_stem(lib, mem, H, W, data="normal", seed=0):
    """The packed-row 7x7 stem of tdnet_opts.precision = 2 (k_conv_adirect_b3<7, 2>) through tdnet_op_stem -- conv -> ReLU -> max-pool, which
    picks and adds no error -- at SPLIT_GATE over the same chain in fp32 torch on the CPU."""
    import ctypes
    img, w, b, _ = _stem_case(H, W, seed, False)
    if data == "abs":
        img = np.abs(img)
    elif data == "scaled":
        s = np.float32([2.0 ** -6, 1.0, 2.0 ** 6])
        img, w = img * s[:, None, None], w / s[None, :, None, None]
    chain = lambda cast: F.max_pool2d(F.relu(F.conv2d(cast(torch.from_numpy(img))[None], cast(torch.from_numpy(w)), cast(torch.from_numpy(b)), 2, 3)), 3, 2, 1)[0].permute(1, 2, 0).numpy()
    ref = chain(lambda t: t.double())
    errs = {"cpu32": max_rms(chain(lambda t: t), ref)}
    di, outs = mem.put(img), {}
    for name, kw in (("exact", {}), ("split", {"precision": 2})):
        out = mem.empty(ref.shape)
        lib.check(lib.tdnet_op_stem(mem.ptr(di), H, W, w.ctypes.data, b.ctypes.data, ctypes.byref(lib.opts(**kw)), mem.ptr(out), mem.stream))
        outs[name] = np.array(mem.get(out))
        errs[name] = max_rms(outs[name], ref)
    what = "stem %dx%d %s" % (H, W, data)
    assert not np.array_equal(outs["exact"], outs["split"]), ("the split kernel did not run: the bits of the exact-fp32 kernel", what)
    return _split_gate(what, errs, "cpu32", SPLIT_GATE)


def split_attention(lib, mem, Lq, Lk, DV, online, spike=False, ramp=False, data="normal", seed=0):
    """The attention of tdnet_opts.precision = 2 (td_attn_b3.h; online 17: the form by size, 18: 64 queries per workgroup, 19: 32) without bias
    and residual against fp64 softmax(q k^T / 8) v', at SPLIT_GATE over the same expression in fp32 torch on the CPU; the exact-fp32
    single-pass kernel (online = 2) runs beside it for the record.  spike / ramp: attention()'s.  data: "abs": q, k, v' >= 0 (every score
    positive, no cancellation in P V'); "scaled": q_d * s_d and k_d / s_d (the same scores from other exponents), key j of v' times s_j."""
    g = np.random.default_rng(seed)
    q = g.standard_normal((Lq, 64)).astype(np.float32)
    k = g.standard_normal((Lk, 64)).astype(np.float32)
    if spike:
        k[Lk // 2] = 6.0 * q[Lq // 3] / max(1e-6, float(np.linalg.norm(q[Lq // 3]))) * 8.0
    if ramp:
        q = np.abs(q) + 0.5
        k = (np.arange(Lk, dtype=np.float32)[:, None] / max(1, Lk - 1)) * 40.0 * (np.ones(64, np.float32) / 8.0)[None, :] + 0.1 * k
    v = g.standard_normal((Lk, DV)).astype(np.float32)
    if data == "abs":
        q, k, v = np.abs(q), np.abs(k), np.abs(v)
    elif data == "scaled":
        s = pow2_scales(64)
        q, k, v = q * s, k / s, v * pow2_scales(Lk)[:, None]
    else:
        assert data == "normal", data
    tq, tk, tv = torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v)
    ref = (torch.softmax(tq.double() @ tk.double().T / 8.0, 1) @ tv.double()).numpy()
    errs = {"cpu32": max_rms((torch.softmax(tq @ tk.T / 8.0, 1) @ tv).numpy(), ref)}
    dq, dk, dv_ = mem.put(q), mem.put(k), mem.put(v)
    for name, code in (("exact", 2), ("split", int(online))):
        out = mem.empty((Lq, DV))
        lib.check(lib.tdnet_op_attention(mem.ptr(dq), mem.ptr(dk), mem.ptr(dv_), None, None, Lq, Lk, DV, code, None, None, None, mem.ptr(out), mem.stream))
        errs[name] = max_rms(np.array(mem.get(out)), ref)
    what = "attention (%d, %d, %d) online %d%s%s %s" % (Lq, Lk, DV, online, " spike" if spike else "", " ramp" if ramp else "", data)
    return _split_gate(what, errs, "cpu32", SPLIT_GATE)


def layernorm(lib, mem, HW, C, seed=0, tol=1e-4):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((HW, C)) * 3 + 1).astype(np.float32)
    gg = g.uniform(0.5, 1.5, HW).astype(np.float32)
    bb = g.standard_normal(HW).astype(np.float32)
    ref = F.layer_norm(torch.from_numpy(x).T.contiguous(), (HW,), torch.from_numpy(gg), torch.from_numpy(bb), 1e-5).T.numpy()
    dx, dg, db, out = mem.put(x), mem.put(gg), mem.put(bb), mem.empty((HW, C))
    lib.check(lib.tdnet_op_layernorm_hw(mem.ptr(dx), HW, C, mem.ptr(dg), mem.ptr(db), mem.ptr(out), mem.stream))
    err = float(np.abs(mem.get(out) - ref).max())
    assert err <= tol, ("layernorm", HW, C, err)
    return err


def layernorm_f16(lib, mem, HW, C, seed=0):
    """tdnet_op_layernorm_hw_f16 (k_ln_apply_h: the map the head conv of an fp16-mode frame reads) is half() of tdnet_op_layernorm_hw's
    output BIT FOR BIT: the same statistics, the same fp32 expression, one rounding (td_misc.h above k_ln_apply_h).  The fp32 output itself
    is held to fp64 by layernorm()."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((HW, C)) * 3 + 1).astype(np.float32)
    gg = g.uniform(0.5, 1.5, HW).astype(np.float32)
    bb = g.standard_normal(HW).astype(np.float32)
    dx, dg, db, wide, out = mem.put(x), mem.put(gg), mem.put(bb), mem.empty((HW, C)), mem.empty((HW, C))
    lib.check(lib.tdnet_op_layernorm_hw(mem.ptr(dx), HW, C, mem.ptr(dg), mem.ptr(db), mem.ptr(wide), mem.stream))
    lib.check(lib.tdnet_op_layernorm_hw_f16(mem.ptr(dx), HW, C, mem.ptr(dg), mem.ptr(db), mem.ptr(out), mem.stream))
    got, exp = np.array(mem.get(out)), np.array(mem.get(wide)).astype(np.float16).astype(np.float32)
    assert np.array_equal(got, exp), ("layernorm_f16", HW, C, int((got != exp).sum()), float(np.abs(got - exp).max()))


def layernorm_flat(lib, mem, HW, C, mean, std, seed=0, factor=4.0):
    """The plane LayerNorm on nearly constant planes (N(mean, std) with std << mean: what the head normalises when the residual is small),
    against an fp64 evaluation.  There the variance is of eps's order and far below mean^2, so a kernel that drops eps or forms a one-pass
    E[x^2] - E[x]^2 is wrong by orders of magnitude -- which opcheck.layernorm's N(1, 3) planes do not show.  The input's own fp32 rounding
    sets the achievable error, so the gate is relative to it: the kernel's max error may be `factor` times that of F.layer_norm in fp32 on
    the CPU on the same input (the factor test_gpu_model grants over the CPU path's own error).  The check first proves that the case
    discriminates: the same fp64 formula without eps is off by more than 100 gates.  Returns kernel error / CPU fp32 error."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((HW, C)) * std + mean).astype(np.float32)
    gg = g.uniform(0.5, 1.5, HW).astype(np.float32)
    bb = g.standard_normal(HW).astype(np.float32)
    x64 = x.astype(np.float64)
    mu, var = x64.mean(0), x64.var(0)
    aff = lambda z: z * gg.astype(np.float64)[:, None] + bb.astype(np.float64)[:, None]
    ref = aff((x64 - mu) / np.sqrt(var + 1e-5))
    no_eps = aff((x64 - mu) / np.sqrt(var))
    cpu = F.layer_norm(torch.from_numpy(x).T.contiguous(), (HW,), torch.from_numpy(gg), torch.from_numpy(bb), 1e-5).T.numpy()
    cpu_err = float(np.abs(cpu - ref).max())
    gate = factor * cpu_err
    sep = float(np.abs(no_eps - ref).max())
    assert cpu_err > 0 and sep > 100 * gate, ("layernorm_flat: the case does not discriminate", HW, C, mean, std, sep, gate)
    dx, dg, db, out = mem.put(x), mem.put(gg), mem.put(bb), mem.empty((HW, C))
    lib.check(lib.tdnet_op_layernorm_hw(mem.ptr(dx), HW, C, mem.ptr(dg), mem.ptr(db), mem.ptr(out), mem.stream))
    err = float(np.abs(mem.get(out) - ref).max())
    print("layernorm_flat HW=%d C=%d mean=%g std=%g: kernel %.3e, CPU fp32 %.3e, ratio %.2f, without eps %.3e" % (HW, C, mean, std, err, cpu_err, err / cpu_err, sep))
    assert err <= gate, ("layernorm_flat", HW, C, mean, std, err, cpu_err)
    return err / cpu_err


def ppm(lib, mem, h, w, pid, seed=0, tol=1e-4):
    g = np.random.default_rng(seed)
    c4 = np.abs(g.standard_normal((h, w, 512))).astype(np.float32)
    W4 = (g.standard_normal((4, 128, 512)) * 0.05).astype(np.float32)
    B4 = g.standard_normal((4, 128)).astype(np.float32)
    x = torch.from_numpy(c4).permute(2, 0, 1)[None]
    feats = []
    for j, o in enumerate((1, 2, 3, 6)):
        p = F.relu(F.conv2d(F.adaptive_avg_pool2d(x, o), torch.from_numpy(W4[j])[:, :, None, None], torch.from_numpy(B4[j])))
        feats.append(F.interpolate(p, (h, w), mode="bilinear", align_corners=True))
    ref = torch.cat([x[:, pid * 256:(pid + 1) * 256]] + [f[:, pid * 64:(pid + 1) * 64] for f in feats], 1)[0].permute(1, 2, 0).numpy()
    dc, out = mem.put(c4), mem.empty((h, w, 512))
    lib.check(lib.tdnet_op_ppm(mem.ptr(dc), h, w, W4.ctypes.data, B4.ctypes.data, 2, pid, mem.ptr(out), mem.stream))
    err = float(np.abs(mem.get(out) - ref).max())
    assert err <= tol, ("ppm", h, w, pid, err)
    return err


def upsample(lib, mem, C, h, w, H, W, seed=0, tol=1e-5):
    g = np.random.default_rng(seed)
    x = g.standard_normal((C, h, w)).astype(np.float32)
    ref = F.interpolate(torch.from_numpy(x)[None], (H, W), mode="bilinear", align_corners=True)[0].numpy()
    dx, out = mem.put(x), mem.empty((C, H, W))
    lib.check(lib.tdnet_op_upsample(mem.ptr(dx), C, h, w, H, W, mem.ptr(out), mem.stream))
    err = float(np.abs(mem.get(out) - ref).max())
    assert err <= tol, ("upsample", C, h, w, H, W, err)
    return err


def _same_bytes(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bytes(p, q) for p, q in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def each_poison(x, device, run):
    """fp32 logits x through an output entry inside guard bands, once per fill of _Guarded.POISONS (the quiet NaN a comparison swallows, the 2^127
    it cannot): run(address) -> an array, or a tuple of arrays and Nones.  The two results must be the same bytes -- an out-of-range read of
    logits shows under one of the fills -- and the bands intact; returns the first.  device: torch-ROCm memory, else numpy (the emulator)."""
    if torch.is_tensor(x):
        x = x.cpu().numpy()
    first = None
    for poison in _Guarded.POISONS:
        mem = GuardedTorchMem() if device else GuardedNumpyMem()
        got = run(mem.ptr(mem.put(x, poison=poison)))
        mem.verify()
        if first is None:
            first = got
        else:
            assert _same_bytes(first, got), "the output depends on what lies around the logits: band fill 0x%08x against 0x%08x" % (poison, _Guarded.POISONS[0])
    return first


class At:
    """The address of a guarded copy where a helper expects the array (x.ctypes.data) or the tensor (x.data_ptr()) itself."""
    def __init__(self, addr):
        self._addr = addr
        self.ctypes = self

    @property
    def data(self):
        return self._addr

    def data_ptr(self):
        return self._addr


GUARDED_ARG_CAP = 8 << 20                                              # bytes: larger logits (the 90 MB of a 769x1537 frame) stay where they are


def guarded_arg(name, device, accumulates=None):
    """Decorator for a test's operator helper: its argument `name` -- fp32 logits as an array or a tensor, or None -- goes through each_poison: the
    helper runs once per band fill on a guarded copy (it sees an At) and must return the same bytes.  accumulates: an argument the entry adds
    into (the score entry's matrix), put back to its state at the call before each run."""
    import functools
    import inspect

    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            x = b.arguments[name]
            nbytes = 0 if x is None or isinstance(x, At) else (x.numel() * x.element_size() if torch.is_tensor(x) else np.asarray(x).nbytes)
            addr = 0 if nbytes == 0 else (x.data_ptr() if torch.is_tensor(x) else np.asarray(x).ctypes.data)
            if nbytes == 0 or nbytes > GUARDED_ARG_CAP or addr % 16:     # (a deliberately misaligned map keeps its address: that is what its test is about)
                return fn(*a, **kw)
            acc = b.arguments.get(accumulates) if accumulates else None
            start = None if acc is None else (acc.clone() if torch.is_tensor(acc) else np.array(acc))

            def run(addr):
                if acc is not None:
                    acc.copy_(start) if torch.is_tensor(acc) else np.copyto(acc, start)
                b.arguments[name] = At(addr)
                return fn(*b.args, **b.kwargs)
            return each_poison(x, device, run)
        return wrapper
    return deco
