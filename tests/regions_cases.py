"""Cases and checks of regions out (include/tdnet.h "regions out"), shared by tests/test_emu_regions.py (CPU, through the emulator) and
tests/test_gpu_regions.py (device memory).  The expected id map, count and table come from tdnet_amd.dataloader.regions_u8, a plain flood fill that
tests/test_regions_host.py holds to hand-written answers and to scipy.ndimage.label.  Every comparison is exact: everything is an integer.

The label map, the id map and the table of an operator call sit between opcheck's guard bands (the maps are bytes and int32 words inside float32
holders: a small integer is a finite float and never the 7e7 fill, so verify()'s "fully written" holds for them as it stands)."""
import functools

import numpy as np

from tdnet_amd.dataloader import REGION_DTYPE, REGIONS_HEADER_DTYPE, REGIONS_OVERFLOW, regions_u8

C = 19                                                                 # nclass of the operator cases
PATTERNS = ("one", "hstripes", "vstripes", "checker", "diag_back", "diag_fwd", "spiral", "comb", "two_classes", "interrupted", "reject255", "noise")
FIXED_SHAPES = ((33, 65), (128, 256))                                  # the latter >= 32 tiles: the merge spans the XCDs on the device


def shapes(th, tw):
    """The map sizes at which the tile-local labelling, the border merge or the numbering can go wrong, from the kernels' real tile (th rows, tw columns)."""
    return ((1, 1), (1, tw + 3), (th + 1, 1), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th + 3, 3 * tw + 5)) + FIXED_SHAPES


def spiral(H, W):
    """A 1-pixel path winding inwards with 1-pixel gaps: rectangles 2 pixels apart, each cut open below its top-left corner and bridged to the next."""
    g = np.zeros((H, W), bool)
    k = 0
    while 2 * k <= H - 1 - 2 * k and 2 * k <= W - 1 - 2 * k:
        a, b, c, d = 2 * k, H - 1 - 2 * k, 2 * k, W - 1 - 2 * k        # rows a..b, columns c..d
        g[a, c:d + 1] = True
        g[b, c:d + 1] = True
        g[a:b + 1, c] = True
        g[a:b + 1, d] = True
        if b - a >= 2 and d - c >= 2:
            g[a + 1, c] = False                                        # the cut
            if a + 2 <= b and c + 2 <= d - 2 and a + 2 <= b - 2:
                g[a + 2, c + 1] = True                                 # the bridge to the next rectangle's corner
        k += 1
    return g


@functools.lru_cache(maxsize=None)
def pattern(name, H, W, th, tw):
    """(labels uint8 [H, W], class set).  Member classes are 3, 7 and 11; 1 is a class outside the set, 255 no class at all."""
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.full((H, W), 1, np.uint8)
    classes = (3,)
    g = int(np.gcd(th, tw))
    if name == "one":
        lab[:] = 3
    elif name == "hstripes":
        lab[yy % 2 == 0] = 3
    elif name == "vstripes":
        lab[xx % 2 == 0] = 3
    elif name == "checker":
        lab[:] = np.where((yy + xx) % 2 == 0, 3, 7)
        classes = (3, 7)
    elif name == "diag_back":                                          # x - y = multiples of gcd(th, tw): through (k th - 1, m tw - 1) -> (k th, m tw)
        lab[(xx - yy) % g == 0] = 3
    elif name == "diag_fwd":                                           # through (k th, m tw - 1) -> (k th - 1, m tw)
        lab[(xx + yy + 1) % g == 0] = 3
    elif name == "spiral":
        lab[spiral(H, W)] = 3
    elif name == "comb":                                               # teeth joined along the bottom row only: their roots are found late
        lab[xx % 2 == 0] = 3
        lab[H - 1, :] = 3
        if H > 1:
            lab[H - 2, 1::2] = 1
    elif name == "two_classes":
        lab[:] = np.where(xx < (W + 1) // 2, 3, 7)
        classes = (3, 7)
    elif name == "interrupted":
        lab[:] = 3
        lab[:, W // 2] = 1
        lab[H // 3, :] = 1
    elif name == "reject255":
        lab[:] = 3
        lab[(yy // 3 + xx // 5) % 3 == 0] = 255
    elif name == "noise":
        lab[:] = noise(H, W)
        classes = (3, 7, 11)
    else:
        raise KeyError(name)
    lab = np.ascontiguousarray(lab)
    lab.setflags(write=False)
    return lab, classes


def noise(H, W, seed=0):
    """about 0.6 of the pixels in one of three member classes (mostly 3): irregular components near the percolation threshold"""
    rng = np.random.default_rng(1000 * H + W + seed)
    member = rng.random((H, W)) < 0.6
    which = rng.choice(np.array([3, 7, 11], np.uint8), size=(H, W), p=[0.8, 0.1, 0.1])
    return np.where(member, which, 1).astype(np.uint8)


_oracle = {}


def oracle(labels, classes, conn, min_area, max_regions):
    """regions_u8 once per distinct question (the emulator and the parameter sweeps ask the same ones again)."""
    key = (labels.shape, labels.tobytes(), tuple(classes), conn, min_area, max_regions)
    if key not in _oracle:
        ids, count, table = regions_u8(labels, classes, conn, min_area, max_regions)
        ids.setflags(write=False)
        table.setflags(write=False)
        _oracle[key] = (ids, count, table)
    return _oracle[key]


def compare(got, labels, classes, conn, min_area, max_regions, what=()):
    """got = (ids or None, header record, records [max_regions]) against the oracle on `labels`; returns the count."""
    ids, hdr, recs = got
    want_ids, count, table = oracle(np.ascontiguousarray(labels), classes, conn, min_area, max_regions)
    stored = min(count, max_regions)
    assert (int(hdr["count"]), int(hdr["stored"]), int(hdr["reserved"])) == (count, stored, 0), what + ("header", hdr, count, stored)
    assert int(hdr["status"]) == (REGIONS_OVERFLOW if count > max_regions else 0), what + ("status", int(hdr["status"]), count, max_regions)
    if ids is not None:
        bad = np.asarray(ids) != want_ids
        assert not bad.any(), what + ("id map", int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))
    assert recs.shape == (max_regions,)
    for f in REGION_DTYPE.names:
        bad = recs[f][:stored] != table[f]
        assert not bad.any(), what + ("record field " + f, int(np.argmax(bad)), recs[:stored][bad][:1], table[bad][:1])
    assert not recs[stored:].view(np.uint8).any(), what + ("records beyond stored are not zero",)
    return count


def words(nbytes):
    return (int(nbytes) + 3) // 4


def put_bytes(mem, a, off=0):
    """uint8 array `a` at byte offset `off` (0..3) of a guarded input: (holder, address)"""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1)
    raw = np.zeros(4 * words(a.size + off), np.uint8)
    raw[off:off + a.size] = a
    t = mem.put(raw.view(np.float32))
    return t, mem.ptr(t) + off


def get_bytes(mem, t, nbytes, off=0):
    return np.ascontiguousarray(np.asarray(mem.get(t))).view(np.uint8).reshape(-1)[off:off + nbytes].copy()


def run_op(lib, mem, H, W, classes, conn, max_regions, min_area, labels=None, logits=None, want_ids=True, want_labels=True, lab_off=0, nclass=C):
    """One call of tdnet_op_regions between guard bands: (ids or None, header, records, labels written or None).  labels: the unfused form (a uint8 map at byte
    offset lab_off of its holder); logits = (x, h, w): from low-resolution logits [nclass, h, w]."""
    ids_t = mem.empty((H, W)) if want_ids else None
    tab_t = mem.empty((words(16 + 48 * max_regions),))
    cls = np.ascontiguousarray(classes, np.uint8)
    lab_t = out_t = x_t = None
    lab_p = None
    if labels is not None:
        lab_t, lab_p = put_bytes(mem, labels, lab_off)
        args = (None, nclass, 0, 0, H, W, lab_p, None)
    else:
        x, h, w = logits
        x_t = mem.put(x)
        out_t = mem.empty((words(H * W),)) if want_labels else None
        args = (mem.ptr(x_t), nclass, h, w, H, W, None, mem.ptr(out_t))
    lib.check(lib.tdnet_op_regions(*args, cls.ctypes.data if cls.size else None, int(cls.size), conn, max_regions, min_area, mem.ptr(ids_t), mem.ptr(tab_t), mem.stream))
    ids = None if ids_t is None else np.ascontiguousarray(np.asarray(mem.get(ids_t))).view(np.int32).reshape(H, W).copy()
    raw = get_bytes(mem, tab_t, 16 + 48 * max_regions)
    written = None if out_t is None else get_bytes(mem, out_t, H * W).reshape(H, W)
    if lab_t is not None:
        assert np.array_equal(get_bytes(mem, lab_t, H * W, lab_off).reshape(H, W), labels)   # the label map is only read
    mem.verify()
    return ids, raw[:16].view(REGIONS_HEADER_DTYPE)[0], raw[16:].view(REGION_DTYPE), written


def tile(lib):
    import ctypes
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    lib.check(lib.tdnet_op_regions_tile(ctypes.byref(th), ctypes.byref(tw)))
    assert th.value > 1 and tw.value > 1
    return th.value, tw.value


def check_pattern(lib, mem, name, H, W, th, tw, conns=(4, 8), max_regions=256):
    """One pattern at one size through the unfused form, at both connectivities: id map, header and records against the oracle."""
    labels, classes = pattern(name, H, W, th, tw)
    counts = []
    for conn in conns:
        ids, hdr, recs, _ = run_op(lib, mem, H, W, classes, conn, max_regions, 1, labels=labels)
        counts.append(compare((ids, hdr, recs), labels, classes, conn, 1, max_regions, (name, H, W, conn)))
    return counts


def check_parameters(lib, mem, H, W):
    """min_area, max_regions, the empty set and the set of every class on the noise map; ids may be left out; the map at every byte offset."""
    labels = noise(H, W)
    classes = (3, 7, 11)
    for conn in (4, 8):
        base = None
        for min_area in (1, 2, 50):
            ids, hdr, recs, _ = run_op(lib, mem, H, W, classes, conn, 4096, min_area, labels=labels)
            n = compare((ids, hdr, recs), labels, classes, conn, min_area, 4096, ("min_area", min_area, conn))
            base = n if base is None else base
            assert n <= base and (min_area == 1 or n < base), (min_area, n, base)   # regions really are dropped and the rest renumbered
            if min_area > 1:
                assert (ids == 0).sum() > (np.isin(labels, classes) == 0).sum()      # dropped regions are id 0
        count = oracle(labels, classes, conn, 1, 4096)[1]
        assert count > 3
        for max_regions in (1, count, count + 1):
            ids, hdr, recs, _ = run_op(lib, mem, H, W, classes, conn, max_regions, 1, labels=labels)
            compare((ids, hdr, recs), labels, classes, conn, 1, max_regions, ("max_regions", max_regions, conn))
            assert ids.max() == count                                  # ids run beyond the table
        ids, hdr, recs, _ = run_op(lib, mem, H, W, (), conn, 8, 1, labels=labels)
        assert compare((ids, hdr, recs), labels, (), conn, 1, 8, ("empty set", conn)) == 0 and not ids.any()
        every = tuple(range(C))
        ids, hdr, recs, _ = run_op(lib, mem, H, W, every, conn, 4096, 1, labels=labels)
        compare((ids, hdr, recs), labels, every, conn, 1, 4096, ("every class", conn))
        assert (ids > 0).all()
        _, hdr, recs, _ = run_op(lib, mem, H, W, classes, conn, 4096, 1, labels=labels, want_ids=False)
        compare((None, hdr, recs), labels, classes, conn, 1, 4096, ("no id map", conn))
    for off in (1, 2, 3):                                              # a label map at any byte address
        ids, hdr, recs, _ = run_op(lib, mem, H, W, classes, 8, 4096, 1, labels=labels, lab_off=off)
        compare((ids, hdr, recs), labels, classes, 8, 1, 4096, ("label map at byte offset", off))


def check_from_logits(lib, mem, x, nclass, h, w, H, W, want_labels):
    """The fused form: the labels written are `want_labels` (tdnet_op_upsample_argmax's), the regions the oracle's on those labels; with and without the
    label map asked for."""
    classes = tuple(c for c in (0, 1, 3, 4, 11) if c < nclass)
    for conn in (4, 8):
        ids, hdr, recs, written = run_op(lib, mem, H, W, classes, conn, 512, 1, logits=(x, h, w), nclass=nclass)
        assert np.array_equal(written, want_labels), ("labels", nclass, H, W, conn)
        compare((ids, hdr, recs), want_labels, classes, conn, 1, 512, ("from logits", nclass, H, W, conn))
    ids, hdr, recs, written = run_op(lib, mem, H, W, classes, 8, 512, 2, logits=(x, h, w), nclass=nclass, want_labels=False)
    assert written is None
    compare((ids, hdr, recs), want_labels, classes, 8, 2, 512, ("from logits, no label map", nclass, H, W))


def check_frame_regions(got, labels, classes, conn, min_area, max_regions, what=()):
    """got = (ids, table bytes) of a frame entry against the oracle on that frame's labels"""
    ids, raw = got
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    return compare((ids, raw[:16].view(REGIONS_HEADER_DTYPE)[0], raw[16:].view(REGION_DTYPE)), labels, classes, conn, min_area, max_regions, what)
