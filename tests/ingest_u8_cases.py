"""Cases and expected values shared by tests/test_emu_ingest_u8.py (CPU, through the emulator) and tests/test_gpu_ingest_u8.py (device memory).

Expected values come from code that predates the uint8 entries: dataloader.resize_linear_u8, cityscapesLoader.normalise, and the library's
fp32 entries.  Every comparison the two test files make is exact."""
import functools

import numpy as np

from tdnet_amd.dataloader import cityscapesLoader, resize_linear_u8

# (name, (Hs, Ws), (H, W)): the op-level ingest cases
STEM_CASES = [
    ("same_33x65_all_bytes", (33, 65), (33, 65)),
    ("same_8x12_w_mult_of_4", (8, 12), (8, 12)),
    ("same_7x31", (7, 31), (7, 31)),
    ("same_1x1", (1, 1), (1, 1)),
    ("down_41x83", (41, 83), (33, 65)),
    ("down_exact_2x", (66, 130), (33, 65)),
    ("up_20x37", (20, 37), (33, 65)),
    ("aniso_50x40", (50, 40), (33, 65)),
    ("one_row_1x9", (1, 9), (5, 9)),
    ("one_col_9x1", (9, 1), (9, 5)),
]
# wider than one workgroup's strip (256 lanes x 4 columns): GPU only (the emulator runs a workgroup's lanes one after the other)
WIDE_CASES = [("same_6x2051", (6, 2051), (6, 2051)), ("down_9x2100", (9, 2100), (8, 2051))]
ALT_MEAN, ALT_STD = (0.31, 0.5, 0.72), (0.11, 0.4, 1.7)

# (name, C, (h, w), (H, W)): upsample + argmax
ARGMAX_CASES = [("odd_w", 19, (5, 9), (33, 65)), ("w_mult_of_4", 19, (4, 8), (32, 64)), ("native", 19, (13, 25), (97, 193)),
                ("c256", 256, (5, 9), (33, 65)), ("c1", 1, (5, 9), (33, 65)), ("ties", 19, (5, 9), (33, 65))]


@functools.lru_cache(maxsize=None)
def source(name, Hs, Ws):
    """Random bytes [Hs, Ws, 3]; the first case holds all 256 byte values in every channel."""
    rng = np.random.default_rng(Hs * 10007 + Ws)
    src = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    if name == "same_33x65_all_bytes":
        flat = src.reshape(-1, 3)
        for c in range(3):
            flat[:256, c] = np.roll(np.arange(256, dtype=np.uint8), 17 * c)
    src.setflags(write=False)
    return src


def offset_copy(src, off):
    """(holder, address): the bytes of src at `off` bytes into a larger buffer whose other bytes are 0xA5 (a read outside the image shows)."""
    holder = np.full(src.size + 64, 0xA5, np.uint8)
    holder[off:off + src.size] = src.reshape(-1)
    return holder, holder.ctypes.data + off


def loader(H, W, mean=None, std=None):
    ld = cityscapesLoader(img_path="/nonexistent-frames", in_size=(H, W))
    if mean is not None:
        ld.mean, ld.std = np.array(mean), np.array(std)
    return ld


def expected_image(src, H, W, mean=None, std=None):
    """The fp32 NCHW tensor the host loader makes of the frame: normalise(resize_linear_u8(src, (W, H))), [1, 3, H, W] numpy."""
    return np.ascontiguousarray(loader(H, W, mean, std).normalise(resize_linear_u8(src, (W, H))).numpy())


def box_average_2x(src):
    """Exact 2x downscale = 2x2 box average, rounded half up (tests/test_dataloader.py)."""
    a = src.astype(np.int64)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def lowres_logits(name, C, h, w):
    rng = np.random.default_rng(C * 1000 + h * 10 + w)
    x = rng.standard_normal((C, h, w)).astype(np.float32)
    if name == "c256":                                                 # the maximum in channel 255 at some pixels: label 255 must survive
        x[255, ::2, ::3] = 9.0
        x[255, 1, 1] = 9.0
    if name == "ties":                                                 # exact ties between two channels, above everything else: the lower index wins
        x[11, :, ::2] = 7.5
        x[4, :, ::2] = 7.5
        x[17, 2, :] = 8.25
        x[3, 2, :] = 8.25
    x.setflags(write=False)
    return x


def double3(v):
    import ctypes
    return None if v is None else (ctypes.c_double * 3)(*v)
