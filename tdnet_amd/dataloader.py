"""Frame loader with the reference's API (Testing/dataloader.py:44-88): cityscapesLoader(img_path, in_size),
.load_frames(), .data = [[img[1,3,H,W] fp32, img_name, folder, (W,H)], ...], .decode_segmap(labels).

imageio / cv2 are not in this image.  PNGs are read with PIL; the resize is `resize_linear_u8`, a restatement of what
`cv2.resize(img, (W, H))` (dataloader.py:64: default INTER_LINEAR on a uint8 image) computes: half-pixel centres, NO antialiasing on
downscale (PIL's BILINEAR widens its support when shrinking, so it is not a stand-in), and OpenCV's 11-bit fixed-point arithmetic, so
the uint8 result is meant to be the one OpenCV's generic path produces.  cv2 itself is absent here, so the function is pinned by
hand-derived known answers, by the float bilinear formula to within one grey level and by the 2x-downscale = 2x2 box-average
identity (tests/test_dataloader.py), not by a cv2-generated fixture.  Normalisation follows dataloader.py:66-67 in float64.
"""
import os

import numpy as np
import torch


def recursive_glob(rootdir=".", suffix=""):
    return [os.path.join(looproot, filename) for looproot, _, filenames in os.walk(rootdir)
            for filename in filenames if filename.endswith(suffix)]


def _linear_coeffs(n_src, n_dst):
    """Source index and the two 11-bit weights per destination index, as OpenCV's resize builds them for INTER_LINEAR:
    fx = (float)((d + 0.5) * scale - 0.5), s = floor(fx), fx -= s, clamped at both borders; weights = round((1 - fx, fx) * 2048)."""
    scale = float(n_src) / float(n_dst)
    d = np.arange(n_dst, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(fx).astype(np.int64)
    fx = (fx - s.astype(np.float32)).astype(np.float32)
    low = s < 0
    fx[low] = 0.0; s[low] = 0
    high = s >= n_src - 1
    fx[high] = 0.0; s[high] = n_src - 1
    w1 = np.rint(fx * np.float32(2048.0)).astype(np.int64)
    w0 = np.rint((np.float32(1.0) - fx) * np.float32(2048.0)).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), w0, w1


def resize_linear_u8(img, size):
    """uint8 [H,W,C] -> uint8 [size[1], size[0], C]; size = (W, H) like cv2.resize's dsize (dataloader.py:52,64).
    Horizontal pass in int32 (pixel * 2048-scale weights), vertical pass with OpenCV's shifts:
        dst = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    Wd, Hd = int(size[0]), int(size[1])
    Hs, Ws = img.shape[:2]
    if (Hs, Ws) == (Hd, Wd):
        return img.copy()
    x0, x1, a0, a1 = _linear_coeffs(Ws, Wd)
    y0, y1, b0, b1 = _linear_coeffs(Hs, Hd)
    src = img.astype(np.int64)
    rows = src[:, x0, :] * a0[None, :, None] + src[:, x1, :] * a1[None, :, None]          # [Hs, Wd, C], <= 255 * 2048
    out = (((b0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- NV12 surfaces (include/tdnet.h "NV12 frames in") ----------------------------------------------------------------------------
# standard -> (yoff, decimal coefficients CY, CUB, CUG, CVG, CVR): BT.601 limited (OpenCV's COLOR_YUV2RGB_NV12), BT.709 limited, BT.601 full, BT.709 full
NV12_STANDARDS = {0: (16, (1.164, 2.018, -0.391, -0.813, 1.596)), 1: (16, (1.164, 2.112, -0.213, -0.533, 1.793)),
                  2: (0, (1.0, 1.772, -0.344136, -0.714136, 1.402)), 3: (0, (1.0, 1.8556, -0.187324, -0.468124, 1.5748))}


def nv12_coeffs(standard):
    """(yoff, CY, CUB, CUG, CVG, CVR): the 20-bit fixed-point constants rint(c * 2^20) of the conversion."""
    yoff, dec = NV12_STANDARDS[int(standard)]
    return (yoff,) + tuple(int(np.rint(c * 1048576.0)) for c in dec)


def nv12_extent(Hs, Ws, pitch, uv_offset):
    """Bytes of a surface from its base to the end of its last chroma pair: nothing behind them is ever read."""
    return int(uv_offset) + ((int(Hs) + 1) // 2 - 1) * int(pitch) + 2 * ((int(Ws) + 1) // 2)


def nv12_to_rgb_u8(surface, Hs, Ws, pitch, uv_offset, standard=0):
    """The oracle of the library's NV12 input: the bytes of a surface (Y plane at 0, row pitch `pitch`; interleaved U, V plane at uv_offset,
    the same pitch, ceil(Hs / 2) rows of ceil(Ws / 2) pairs) -> uint8 RGB [Hs, Ws, 3].  Chroma is replicated (pixel (y, x) takes pair
    (y >> 1, x >> 1)); per pixel, in integers that fit int32 (asserted):
        yy = max(0, Y - yoff) * CY;  u = U - 128;  v = V - 128
        R = clamp8((yy + 2^19 + CVR v) >> 20);  G = clamp8((yy + 2^19 + CVG v + CUG u) >> 20);  B = clamp8((yy + 2^19 + CUB u) >> 20)
    This restates what cv2.cvtColor(COLOR_YUV2RGB_NV12) computes for standard 0; cv2 is absent here, so tests/test_nv12_host.py pins it by
    hand-derived answers."""
    s = np.asarray(surface).reshape(-1)
    Hs, Ws, pitch, uv_offset = int(Hs), int(Ws), int(pitch), int(uv_offset)
    assert s.dtype == np.uint8 and Hs >= 1 and Ws >= 1 and pitch >= 2 * ((Ws + 1) // 2) and uv_offset >= Hs * pitch
    assert s.size >= nv12_extent(Hs, Ws, pitch, uv_offset)
    yoff, CY, CUB, CUG, CVG, CVR = nv12_coeffs(standard)
    ys, xs = np.arange(Hs)[:, None], np.arange(Ws)[None, :]
    Y = s[ys * pitch + xs].astype(np.int64)
    cidx = uv_offset + (ys >> 1) * pitch + (xs >> 1) * 2
    u, v = s[cidx].astype(np.int64) - 128, s[cidx + 1].astype(np.int64) - 128
    yy = np.maximum(0, Y - yoff) * CY + (1 << 19)
    sums = np.stack([yy + CVR * v, yy + CVG * v + CUG * u, yy + CUB * u], axis=-1)
    assert np.abs(sums).max() < 2 ** 31 and np.abs(CVG * v).max() < 2 ** 31
    return np.clip(sums >> 20, 0, 255).astype(np.uint8)


def rgb_to_nv12(img_u8, pitch=None, standard=0):
    """A deterministic NV12 surface of an RGB image [Hs, Ws, 3], for tests and the command line: uint8 [Hs + ceil(Hs / 2), pitch] -- the Y
    plane, then the UV plane at uv_offset = Hs * pitch.  The forward matrix (the inverse of the standard's decimal coefficients) in float64,
    rounded to nearest; chroma is the mean over each 2 x 2 block (over the pixels that exist at an odd edge).  pitch: default the row's bytes
    rounded up to 256, as decoders pad; the padding is zero.  Not an exact inverse of nv12_to_rgb_u8 -- it only has to be a function."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    Hs, Ws = img.shape[:2]
    hc, wc = (Hs + 1) // 2, (Ws + 1) // 2
    pitch = (2 * wc + 255) // 256 * 256 if pitch is None else int(pitch)
    assert pitch >= 2 * wc
    yoff, (cy, cub, cug, cvg, cvr) = NV12_STANDARDS[int(standard)]
    inv = np.linalg.inv(np.array([[cy, 0.0, cvr], [cy, cug, cvg], [cy, cub, 0.0]], dtype=np.float64))   # (Y - yoff, u, v) -> (R, G, B), inverted
    yuv = img.astype(np.float64) @ inv.T
    surf = np.zeros((Hs + hc, pitch), np.uint8)
    surf[:Hs, :Ws] = np.clip(np.rint(yuv[..., 0] + yoff), 0, 255).astype(np.uint8)
    pad = np.full((2 * hc, 2 * wc, 2), np.nan)
    pad[:Hs, :Ws] = yuv[..., 1:]
    chroma = np.nanmean(pad.reshape(hc, 2, wc, 2, 2), axis=(1, 3))
    surf[Hs:, :2 * wc] = np.clip(np.rint(chroma + 128.0), 0, 255).astype(np.uint8).reshape(hc, 2 * wc)
    return surf


# ---- source views (include/tdnet.h "source views") -----------------------------------------------------------------------------------
PIX_RGB24, PIX_BGR24, PIX_RGBA32, PIX_BGRA32, PIX_NV12 = 0, 1, 2, 3, 4
PIX_BPP = {PIX_RGB24: 3, PIX_BGR24: 3, PIX_RGBA32: 4, PIX_BGRA32: 4}
PIX_BGR = (PIX_BGR24, PIX_BGRA32)                        # the colour bytes are b g r: the overlay comes out b g r too


class SourceView:
    """A rectangle of a pitched frame in one of the five pixel formats (tdnet_view).  height, width: the WHOLE frame; pitch 0: tight
    (width * bpp; NV12: 2 * ceil(width / 2)); crop = (y, x, h, w) or None: the whole frame; NV12: standard, and uv_offset None = height * pitch.
    Nothing is validated here beyond what the derived values need: the library's tdnet_set_input_view is the judge."""

    def __init__(self, format, height, width, pitch=0, crop=None, standard=0, uv_offset=None):
        self.format, self.height, self.width, self.standard = int(format), int(height), int(width), int(standard)
        if self.format not in (PIX_RGB24, PIX_BGR24, PIX_RGBA32, PIX_BGRA32, PIX_NV12):
            raise ValueError("SourceView: format %r is not one of PIX_* (0..4)" % (format,))
        self.pitch = int(pitch)
        self.crop = None if crop is None else tuple(int(v) for v in crop)
        if self.crop is not None and len(self.crop) != 4:
            raise ValueError("SourceView: crop is (y, x, height, width)")
        self.uv_offset = None if uv_offset is None else int(uv_offset)

    @property
    def nv12(self):
        return self.format == PIX_NV12

    @property
    def bpp(self):
        return 1 if self.nv12 else PIX_BPP[self.format]

    @property
    def row_pitch(self):
        """The pitch in force: the given one, or the tight one."""
        return self.pitch if self.pitch else (2 * ((self.width + 1) // 2) if self.nv12 else self.width * self.bpp)

    @property
    def uv(self):
        """NV12: the UV plane's offset in force (None or 0: height * pitch, as the C ABI reads 0)."""
        return self.uv_offset if self.uv_offset else self.height * self.row_pitch

    @property
    def rect(self):
        """(y, x, h, w) of the rectangle in force."""
        return (0, 0, self.height, self.width) if self.crop is None or self.crop == (0, 0, 0, 0) else self.crop

    @property
    def size(self):
        return self.rect[2:]

    def key(self):
        return (self.format, self.height, self.width, self.row_pitch) + self.rect + ((self.standard, self.uv) if self.nv12 else (0, 0))

    def __repr__(self):
        return "SourceView(format=%d, %dx%d, pitch=%d, rect=%r)" % (self.format, self.height, self.width, self.row_pitch, self.rect)


def view_extent(view):
    """Bytes from the frame's base to the end of its last pixel (NV12: of its last chroma pair): nothing behind them is ever read."""
    if view.nv12:
        return nv12_extent(view.height, view.width, view.row_pitch, view.uv)
    return (view.height - 1) * view.row_pitch + view.width * view.bpp


def view_to_rgb_u8(buf, view):
    """The oracle of the library's source views: the bytes of a frame -> uint8 RGB [h, w, 3] of the view's rectangle.  Packed formats: the three
    colour bytes of every pixel of the rectangle, reordered to r g b.  NV12: nv12_to_rgb_u8 of the WHOLE surface, then sliced -- chroma goes by
    the frame's coordinates, so an odd origin shifts its phase."""
    s = np.asarray(buf).reshape(-1)
    assert s.dtype == np.uint8 and s.size >= view_extent(view), (s.dtype, s.size, view_extent(view))
    y, x, h, w = view.rect
    assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= view.height and x + w <= view.width
    if view.nv12:
        return np.ascontiguousarray(nv12_to_rgb_u8(s, view.height, view.width, view.row_pitch, view.uv, view.standard)[y:y + h, x:x + w])
    bpp, pitch = view.bpp, view.row_pitch
    assert pitch >= view.width * bpp
    idx = ((y + np.arange(h))[:, None, None] * pitch + (x + np.arange(w))[None, :, None] * bpp +
           (np.array([2, 1, 0]) if view.format in PIX_BGR else np.arange(3))[None, None, :])
    return s[idx]


def pack_view(rgb_frame, view, fill=0):
    """A host generator for the packed formats: the bytes [0, view_extent) of the WHOLE frame rgb_frame [height, width, 3] in the view's format and
    pitch; pitch padding and the x bytes of the 32-bit formats hold `fill`."""
    img = np.asarray(rgb_frame)
    assert not view.nv12 and img.dtype == np.uint8 and img.shape == (view.height, view.width, 3)
    bpp, pitch = view.bpp, view.row_pitch
    assert pitch >= view.width * bpp
    out = np.full(view_extent(view), fill, np.uint8)
    idx = (np.arange(view.height)[:, None, None] * pitch + np.arange(view.width)[None, :, None] * bpp +
           (np.array([2, 1, 0]) if view.format in PIX_BGR else np.arange(3))[None, None, :])
    out[idx] = img
    return out


# ---- destination views (include/tdnet.h "destination views") --------------------------------------------------------------------------
# standard -> (yoff, decimal rows Y, U, V over r, g, b) of the forward matrix
NV12_FORWARD = {0: (16, ((.257, .504, .098), (-.148, -.291, .439), (.439, -.368, -.071))),
                1: (16, ((.183, .614, .062), (-.101, -.339, .439), (.439, -.399, -.040))),
                2: (0, ((.299, .587, .114), (-.168736, -.331264, .5), (.5, -.418688, -.081312))),
                3: (0, ((.2126, .7152, .0722), (-.114572, -.385428, .5), (.5, -.454153, -.045847)))}


def nv12_forward_coeffs(standard):
    """(yoff, K int64 [3, 3]): K = rint(c * 2^20) of the forward matrix, rows Y, U, V over r, g, b."""
    yoff, rows = NV12_FORWARD[int(standard)]
    return yoff, np.array([[int(np.rint(c * 1048576.0)) for c in row] for row in rows], np.int64)


def nv12_from_rgb_u8(rgb, standard=0, planes=False):
    """The integer oracle of the library's NV12 destination: uint8 RGB [H, W, 3] -> the tight NV12 surface uint8 [H + ceil(H / 2), 2 * ceil(W / 2)]
    (the Y plane, then the interleaved U, V plane; an odd W leaves one zero byte behind every Y row), or with planes=True (Y [H, W],
    UV [ceil(H / 2), ceil(W / 2), 2]).  Per pixel and per chroma pair, in integers that fit int32 (asserted), arithmetic shifts:
        Y = clamp8((KYR R + KYG G + KYB B + (yoff << 20) + (1 << 19)) >> 20)
        S = the sum of the n in {1, 2, 4} pixels of the pair's 2 x 2 block that exist, m = 4 / n
        U = clamp8((m (KUR S_R + KUG S_G + KUB S_B) + (128 << 22) + (1 << 21)) >> 22);  V likewise with the V row.
    Not rgb_to_nv12, the float generator of test surfaces: this one is a definition, pinned by hand in tests/test_dst_view_host.py."""
    img = np.asarray(rgb)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] >= 1 and img.shape[1] >= 1
    H, W = img.shape[:2]
    hc, wc = (H + 1) // 2, (W + 1) // 2
    yoff, K = nv12_forward_coeffs(standard)
    p = img.astype(np.int64)
    ysum = p @ K[0] + (yoff << 20) + (1 << 19)
    assert (p @ np.abs(K[0])).max() + (yoff << 20) + (1 << 19) < 2 ** 31
    Y = np.clip(ysum >> 20, 0, 255).astype(np.uint8)
    S, cnt = np.zeros((2 * hc, 2 * wc, 3), np.int64), np.zeros((2 * hc, 2 * wc), np.int64)
    S[:H, :W], cnt[:H, :W] = p, 1
    S, n = S.reshape(hc, 2, wc, 2, 3).sum(axis=(1, 3)), cnt.reshape(hc, 2, wc, 2).sum(axis=(1, 3))
    assert np.isin(n, (1, 2, 4)).all()
    m = (4 // n)[..., None]
    assert (m * (S @ np.abs(K[1:]).T)).max() + (128 << 22) + (1 << 21) < 2 ** 31      # every partial sum, whatever the order
    UV = np.clip((m * (S @ K[1:].T) + (128 << 22) + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    if planes:
        return Y, UV
    surf = np.zeros((H + hc, 2 * wc), np.uint8)
    surf[:H, :W] = Y
    surf[H:] = UV.reshape(hc, 2 * wc)
    return surf


def write_view(frame_bytes, view, picture_rgb):
    """The host oracle of the library's destination views: a COPY of a frame's bytes with picture_rgb [h, w, 3] (true r, g, b) pasted into the view's
    rectangle, in any of the five formats.  Packed: the three colour bytes in the format's order, the x byte of the 32-bit formats 255.  NV12 (even
    origin): nv12_from_rgb_u8 of the picture -- its Y bytes and the chroma pairs covering the rectangle.  Every other byte keeps its value."""
    s = np.array(np.asarray(frame_bytes).reshape(-1), copy=True)
    pic = np.asarray(picture_rgb)
    y, x, h, w = view.rect
    assert s.dtype == np.uint8 and s.size >= view_extent(view) and pic.dtype == np.uint8 and pic.shape == (h, w, 3), (s.dtype, s.size, pic.shape, view.rect)
    assert 0 <= y and 0 <= x and y + h <= view.height and x + w <= view.width
    pitch = view.row_pitch
    if view.nv12:
        assert y % 2 == 0 and x % 2 == 0, "an NV12 destination starts on the chroma grid"
        Y, UV = nv12_from_rgb_u8(pic, view.standard, planes=True)
        s[(y + np.arange(h))[:, None] * pitch + (x + np.arange(w))[None, :]] = Y
        hc, wc = UV.shape[:2]
        s[view.uv + (y // 2 + np.arange(hc))[:, None, None] * pitch + (x + 2 * np.arange(wc))[None, :, None] + np.arange(2)[None, None, :]] = UV
        return s
    bpp = view.bpp
    at = (y + np.arange(h))[:, None] * pitch + (x + np.arange(w))[None, :] * bpp
    s[at[..., None] + (np.array([2, 1, 0]) if view.format in PIX_BGR else np.arange(3))[None, None, :]] = pic
    if bpp == 4:
        s[at + 3] = 255
    return s


# ---- surfaces (include/tdnet.h "surfaces") ----------------------------------------------------------------------------------------------
SURF_NV12, SURF_NV21, SURF_I420, SURF_P010, SURF_YUY2, SURF_UYVY = 0, 1, 2, 3, 4, 5
SURF_NAMES = {"nv12": SURF_NV12, "nv21": SURF_NV21, "i420": SURF_I420, "p010": SURF_P010, "yuy2": SURF_YUY2, "uyvy": SURF_UYVY}
SURF_422 = (SURF_YUY2, SURF_UYVY)
SURF_DST = (SURF_NV12, SURF_NV21, SURF_I420, SURF_P010)          # the layouts a destination may have
# layout -> (bytes between luma samples, the luma sample's offset, bytes between chroma pairs, U's offset in a pair, V's offset in a pair)
_SURF_FORM = {SURF_NV12: (1, 0, 2, 0, 1), SURF_NV21: (1, 0, 2, 1, 0), SURF_I420: (1, 0, 1, 0, 0), SURF_P010: (2, 0, 4, 0, 2),
              SURF_YUY2: (2, 0, 4, 1, 3), SURF_UYVY: (2, 1, 4, 0, 2)}


class Surface:
    """A rectangle of a YUV frame whose planes lie in one allocation (tdnet_surface), every default resolved as include/tdnet.h says: pitch 0 = tight;
    chroma_pitch 0 = pitch (NV12, NV21, P010) or (pitch + 1) // 2 (I420); u_offset None / 0 = height * pitch; v_offset None / 0 = u_offset +
    ceil(height / 2) * chroma_pitch (I420).  crop = (y, x, h, w) or None: the whole frame.  YV12 is I420 with the two chroma offsets exchanged.
    Nothing is validated here beyond what the derived values need: the library's tdnet_set_input_surface / tdnet_set_output_surface are the judges."""

    def __init__(self, layout, height, width, pitch=0, chroma_pitch=0, crop=None, standard=0, u_offset=None, v_offset=None):
        self.layout = SURF_NAMES[layout.lower()] if isinstance(layout, str) else int(layout)
        if self.layout not in _SURF_FORM:
            raise ValueError("Surface: layout %r is not one of SURF_* (0..5)" % (layout,))
        self.height, self.width, self.pitch, self.chroma_pitch, self.standard = int(height), int(width), int(pitch), int(chroma_pitch), int(standard)
        self.crop = None if crop is None else tuple(int(v) for v in crop)
        if self.crop is not None and len(self.crop) != 4:
            raise ValueError("Surface: crop is (y, x, height, width)")
        self.u_offset = None if u_offset is None else int(u_offset)
        self.v_offset = None if v_offset is None else int(v_offset)

    @property
    def wide(self):
        """16-bit words with the 10-bit sample in bits 15..6."""
        return self.layout == SURF_P010

    @property
    def packed422(self):
        return self.layout in SURF_422

    @property
    def chroma_size(self):
        """(rows, pairs per row) of the chroma samples."""
        return (self.height if self.packed422 else (self.height + 1) // 2), (self.width + 1) // 2

    @property
    def luma_row_bytes(self):
        return 4 * ((self.width + 1) // 2) if self.packed422 else self.width * _SURF_FORM[self.layout][0]

    @property
    def chroma_row_bytes(self):
        return _SURF_FORM[self.layout][2] * ((self.width + 1) // 2)

    @property
    def row_pitch(self):
        return self.pitch if self.pitch else self.luma_row_bytes

    @property
    def cpitch(self):
        if self.packed422:
            return self.row_pitch
        if self.chroma_pitch:
            return self.chroma_pitch
        return (self.row_pitch + 1) // 2 if self.layout == SURF_I420 else self.row_pitch

    @property
    def u_off(self):
        return 0 if self.packed422 else self.u_offset if self.u_offset else self.height * self.row_pitch

    @property
    def v_off(self):
        if self.layout != SURF_I420:
            return self.u_off
        return self.v_offset if self.v_offset else self.u_off + ((self.height + 1) // 2) * self.cpitch

    @property
    def rect(self):
        return (0, 0, self.height, self.width) if self.crop is None or self.crop == (0, 0, 0, 0) else self.crop

    @property
    def size(self):
        return self.rect[2:]

    def key(self):
        return (self.layout, self.height, self.width, self.row_pitch, self.cpitch) + self.rect + (self.standard, self.u_off, self.v_off)

    def __repr__(self):
        return "Surface(layout=%d, %dx%d, pitch=%d, chroma_pitch=%d, u=%d, v=%d, rect=%r)" % (self.layout, self.height, self.width, self.row_pitch, self.cpitch,
                                                                                               self.u_off, self.v_off, self.rect)


def surface_sample_index(surface):
    """(luma [height, width], U [rows, pairs], V [rows, pairs]): the byte index of every sample of the WHOLE frame (of its low byte for P010), by the
    table of include/tdnet.h "surfaces".  Pixel (Y, X) takes chroma sample (Y >> 1, X >> 1) -- 4:2:2: (Y, X >> 1)."""
    s = surface
    ls, lo, cs, uo, vo = _SURF_FORM[s.layout]
    rows, pairs = s.chroma_size
    luma = np.arange(s.height)[:, None] * s.row_pitch + np.arange(s.width)[None, :] * ls + lo
    c = np.arange(rows)[:, None] * s.cpitch + np.arange(pairs)[None, :] * cs
    return luma, s.u_off + c + uo, s.v_off + c + vo


def surface_extent(surface):
    """Bytes from the surface's base to the largest end over its planes (last row's start + row bytes): nothing behind them is ever touched."""
    s = surface
    end = (s.height - 1) * s.row_pitch + s.luma_row_bytes
    if not s.packed422:
        plane = (s.chroma_size[0] - 1) * s.cpitch + s.chroma_row_bytes
        end = max(end, s.u_off + plane, s.v_off + plane)
    return end


def _surface_samples(buf, surface, idx):
    return (buf[idx].astype(np.int64) | (buf[idx + 1].astype(np.int64) << 8)) >> 6 if surface.wide else buf[idx].astype(np.int64)


def surface_to_rgb_u8(buf, surface):
    """The oracle of the library's surface input: the bytes of a frame -> uint8 RGB [h, w, 3] of the surface's rectangle.  Every pixel of the WHOLE frame
    is converted at its absolute coordinates, then the rectangle is sliced: an odd origin shifts the chroma phase.  8 bit: nv12_to_rgb_u8's formulas.
    P010, on the 10-bit samples w16 >> 6, K = rint(c * 2^18):
        yy = max(0, Y10 - 4 yoff) * CY + 2^19;  u = U10 - 512;  v = V10 - 512;  R = clamp8((yy + CVR v) >> 20) ...
    in integers that fit int32 (asserted)."""
    b = np.asarray(buf).reshape(-1)
    s = surface
    assert b.dtype == np.uint8 and b.size >= surface_extent(s), (b.dtype, b.size, surface_extent(s))
    y, x, h, w = s.rect
    assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= s.height and x + w <= s.width
    li, ui, vi = surface_sample_index(s)
    cy_, cx_ = (np.arange(s.height) >> (0 if s.packed422 else 1))[:, None], (np.arange(s.width) >> 1)[None, :]
    Y, U, V = _surface_samples(b, s, li), _surface_samples(b, s, ui)[cy_, cx_], _surface_samples(b, s, vi)[cy_, cx_]
    yoff, dec = NV12_STANDARDS[int(s.standard)]
    bits = 18 if s.wide else 20
    CY, CUB, CUG, CVG, CVR = (int(np.rint(c * float(1 << bits))) for c in dec)
    mid, yoff = (512, 4 * yoff) if s.wide else (128, yoff)
    u, v = U - mid, V - mid
    yy = np.maximum(0, Y - yoff) * CY + (1 << 19)
    sums = np.stack([yy + CVR * v, yy + CVG * v + CUG * u, yy + CUB * u], axis=-1)
    assert np.abs(sums).max() < 2 ** 31 and np.abs(CVG * v).max() < 2 ** 31
    return np.ascontiguousarray(np.clip(sums >> 20, 0, 255).astype(np.uint8)[y:y + h, x:x + w])


def surface_from_samples(Y, U, V, surface, fill=0, low_bits=None):
    """The bytes [0, surface_extent) of the WHOLE frame from its samples: Y [height, width], U and V [chroma rows, pairs] -- bytes, or 10-bit values for
    P010, whose words' low 6 bits take low_bits (an int, or an array of three of the samples' shapes; default 0).  Every other byte holds `fill`."""
    s = surface
    li, ui, vi = surface_sample_index(s)
    out = np.full(surface_extent(s), fill, np.uint8)
    lows = [0, 0, 0] if low_bits is None else [low_bits] * 3 if np.isscalar(low_bits) else list(low_bits)
    for idx, val, low in ((li, Y, lows[0]), (ui, U, lows[1]), (vi, V, lows[2])):
        val = np.asarray(val).astype(np.int64)
        assert val.shape == idx.shape and val.min() >= 0 and val.max() < (1024 if s.wide else 256), (val.shape, idx.shape)
        if s.wide:
            word = (val << 6) | (np.asarray(low).astype(np.int64) & 63)
            out[idx], out[idx + 1] = (word & 255).astype(np.uint8), (word >> 8).astype(np.uint8)
        else:
            out[idx] = val.astype(np.uint8)
    return out


def _surface_forward(pic, surface):
    """(Y [h, w], U, V [ceil(h / 2), ceil(w / 2)]) of a picture [h, w, 3] placed at an EVEN origin, by the forward formulas of "destination views" (8 bit) and
    of "surfaces" (P010): the samples a 4:2:0 destination takes."""
    if not surface.wide:
        Y, UV = nv12_from_rgb_u8(pic, surface.standard, planes=True)
        return Y.astype(np.int64), UV[..., 0].astype(np.int64), UV[..., 1].astype(np.int64)
    H, W = pic.shape[:2]
    hc, wc = (H + 1) // 2, (W + 1) // 2
    yoff, K = nv12_forward_coeffs(surface.standard)
    p = pic.astype(np.int64)
    assert (p @ np.abs(K[0])).max() + (yoff << 20) + (1 << 17) < 2 ** 31
    Y = np.clip((p @ K[0] + (yoff << 20) + (1 << 17)) >> 18, 0, 1023)
    S, cnt = np.zeros((2 * hc, 2 * wc, 3), np.int64), np.zeros((2 * hc, 2 * wc), np.int64)
    S[:H, :W], cnt[:H, :W] = p, 1
    S, n = S.reshape(hc, 2, wc, 2, 3).sum(axis=(1, 3)), cnt.reshape(hc, 2, wc, 2).sum(axis=(1, 3))
    m = (4 // n)[..., None]
    assert (m * (S @ np.abs(K[1:]).T)).max() + (128 << 22) + (1 << 19) < 2 ** 31
    UV = np.clip((m * (S @ K[1:].T) + (128 << 22) + (1 << 19)) >> 20, 0, 1023)
    return Y, UV[..., 0], UV[..., 1]


def pack_surface(rgb_frame, surface, fill=0):
    """A host generator: the bytes [0, surface_extent) of the WHOLE frame rgb_frame [height, width, 3] in the surface's layout; padding and gaps hold
    `fill`.  4:2:0: the forward formulas a destination uses; 4:2:2: their luma, and per pixel pair of a row the chroma of that pair's mean -- it only
    has to be a function, surface_to_rgb_u8 is not its inverse."""
    img = np.asarray(rgb_frame)
    s = surface
    assert img.dtype == np.uint8 and img.shape == (s.height, s.width, 3)
    if not s.packed422:
        return surface_from_samples(*_surface_forward(img, s), s, fill)
    yoff, K = nv12_forward_coeffs(s.standard)
    p = img.astype(np.int64)
    Y = np.clip((p @ K[0] + (yoff << 20) + (1 << 19)) >> 20, 0, 255)
    wc = (s.width + 1) // 2
    pad = np.concatenate([p, p[:, -1:]], axis=1)[:, :2 * wc].reshape(s.height, wc, 2, 3).sum(axis=2)
    UV = np.clip((2 * (pad @ K[1:].T) + (128 << 22) + (1 << 21)) >> 22, 0, 255)
    return surface_from_samples(Y, UV[..., 0], UV[..., 1], s, fill)


def write_surface(frame_bytes, surface, picture_rgb):
    """The host oracle of the library's surface destinations (NV12, NV21, I420, P010; even origin): a COPY of a frame's bytes with picture_rgb [h, w, 3]
    (true r, g, b) written into the surface's rectangle -- its luma samples and the chroma samples covering it, by the forward formulas; P010 stores
    value << 6, little-endian, the low bits zero.  Every other byte keeps its value."""
    s = surface
    b = np.array(np.asarray(frame_bytes).reshape(-1), copy=True)
    pic = np.asarray(picture_rgb)
    y, x, h, w = s.rect
    assert s.layout in SURF_DST, "YUY2 / UYVY are not destination layouts"
    assert b.dtype == np.uint8 and b.size >= surface_extent(s) and pic.dtype == np.uint8 and pic.shape == (h, w, 3), (b.dtype, b.size, pic.shape, s.rect)
    assert 0 <= y and 0 <= x and y + h <= s.height and x + w <= s.width and y % 2 == 0 and x % 2 == 0, "a 4:2:0 destination starts on the chroma grid"
    Y, U, V = _surface_forward(pic, s)
    li, ui, vi = surface_sample_index(s)
    hc, wc = U.shape
    for idx, val in ((li[y:y + h, x:x + w], Y), (ui[y // 2:y // 2 + hc, x // 2:x // 2 + wc], U), (vi[y // 2:y // 2 + hc, x // 2:x // 2 + wc], V)):
        if s.wide:
            b[idx], b[idx + 1] = ((val << 6) & 255).astype(np.uint8), (val >> 2).astype(np.uint8)
        else:
            b[idx] = val.astype(np.uint8)
    return b


def nearest_index(n_src, n_dst):
    """Source index per destination index of the nearest-sample resize of the label map (test.py:64, cv2.INTER_NEAREST): int64 [n_dst] =
    min(int64(o * (n_src / n_dst)), n_src - 1) -- the quotient first, in float64, then the product, then truncation.  This is the project's rule:
    the frame loop (tdnet_amd/test.py) and the library's colour-map kernels (td_handle.h rgb_nearest_index, the same operations in C) share it."""
    return np.minimum((np.arange(n_dst) * (n_src / n_dst)).astype(np.int64), n_src - 1)


def overlay_u8(src_rgb_u8, labels, palette_rgba):
    """The oracle of the library's overlay output (include/tdnet.h "overlay out"): uint8 [Hs, Ws, 3].  src_rgb_u8 [Hs, Ws, 3] is the frame at
    its own size, labels [H, W] the label map at the network size, palette_rgba [n, 4] bytes r, g, b, a.  Source pixel (y, x) takes the label
    at (nearest_index(H, Hs)[y], nearest_index(W, Ws)[x]); a label >= n has weight 0.  Per channel, in int32:
        A = a + (a >> 7);  out = (c * A + s * (256 - A) + 128) >> 8
    so a = 0 returns the source byte and a = 255 the palette's, exactly, and nothing needs a clamp."""
    src, lab, pal = np.asarray(src_rgb_u8), np.asarray(labels), np.asarray(palette_rgba)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3 and lab.ndim == 2
    assert pal.dtype == np.uint8 and pal.ndim == 2 and pal.shape[1] == 4 and 1 <= pal.shape[0] <= 256
    Hs, Ws = src.shape[:2]
    H, W = lab.shape
    l = lab[nearest_index(H, Hs)][:, nearest_index(W, Ws)].astype(np.int64)
    table = np.zeros((max(256, int(l.max()) + 1), 4), np.int32)       # rows >= n stay zero: A = 0
    table[:pal.shape[0]] = pal
    assert l.min() >= 0
    c, a = table[l][..., :3], table[l][..., 3:]
    A = a + (a >> 7)
    out = (c * A + src.astype(np.int32) * (256 - A) + 128) >> 8
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def matte_u8(full_logits, classes):
    """The oracle of the library's matte output (include/tdnet.h "matte out"): uint8 [H, W].  full_logits [C, H, W] are the full-resolution
    logits, classes the ids of the set (duplicates are legal, an empty list is the empty set).  In float64, the maximum subtracted:
        matte = floor(255 * sum_{c in S} exp(v_c - max) / sum_c exp(v_c - max) + 0.5)
    Every class gives 255 and the empty set 0, exactly.  The library evaluates the same in fp32: it may differ by 1 where 255 num / den is within
    rounding of a half (tests/matte_cases.py has the gate)."""
    v = np.asarray(full_logits, dtype=np.float64)
    assert v.ndim == 3
    member = np.zeros(v.shape[0], bool)
    ids = np.asarray(list(classes), dtype=np.int64)
    assert ids.size == 0 or (ids.min() >= 0 and ids.max() < v.shape[0]), "class ids must be below %d" % v.shape[0]
    member[ids] = True
    e = np.exp(v - v.max(axis=0, keepdims=True))
    t = 255.0 * (e[member].sum(axis=0) / e.sum(axis=0))
    return np.floor(t + 0.5).astype(np.uint8)


def composite_u8(src_rgb, matte, H, W, bg=None):
    """The oracle of the library's composite (include/tdnet.h "matte out"): src_rgb [Hs, Ws, 3] is the frame at its own size, matte [H, W] the
    matte bytes at the network size.  Source pixel (y, x) takes M = matte[nearest_index(H, Hs)[y], nearest_index(W, Ws)[x]].
    bg = (r, g, b): uint8 [Hs, Ws, 3], per channel in int32
        A = M + (M >> 7);  out = (s * A + bg * (256 - A) + 128) >> 8
    so M = 255 returns the source byte and M = 0 the background's, exactly.  bg = None (the alpha mode): uint8 [Hs, Ws, 4], the source's three
    bytes unchanged and M as the fourth."""
    src, m = np.asarray(src_rgb), np.asarray(matte)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3 and m.dtype == np.uint8 and m.shape == (H, W)
    Hs, Ws = src.shape[:2]
    M = m[nearest_index(H, Hs)][:, nearest_index(W, Ws)].astype(np.int32)
    if bg is None:
        return np.concatenate([src, M.astype(np.uint8)[..., None]], axis=2)
    b = np.asarray(bg, dtype=np.int32)
    assert b.shape == (3,) and b.min() >= 0 and b.max() <= 255
    A = (M + (M >> 7))[..., None]
    out = (src.astype(np.int32) * A + b * (256 - A) + 128) >> 8
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def luma_u8(rgb):
    """The guide of a frame (include/tdnet.h "refined matte"): uint8 [..., 3] r g b -> uint8 [...], Y = (77 R + 150 G + 29 B + 128) >> 8.
    The weights add up to 256, so grey (v, v, v) gives v and nothing needs a clamp."""
    p = np.asarray(rgb)
    assert p.dtype == np.uint8 and p.shape[-1] == 3
    p = p.astype(np.int32)
    return ((77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8).astype(np.uint8)


REFINE_MAX_RADIUS = 16
REFINE_MIN_EPS, REFINE_MAX_EPS = 4, 65025


def _box_sum(a, r):
    """int64 [h, w]: the sum of `a` over the box of radius r around every pixel, clipped to the map (an integral image: exact)."""
    h, w = a.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r, w - 1) + 1
    return ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]


def refine_matte_u8(guide, matte, radius, eps, want_coeff=False):
    """The oracle of the library's refined matte (include/tdnet.h "refined matte"): He et al.'s guided filter of the matte bytes [h, w] with
    the guide bytes [h, w], restated so that every step is an integer operation or ONE correctly rounded fp32 operation.  The window of a pixel
    is the box of radius `radius` (1..16) clipped to the map, N its pixel count, S_x the sums over it; eps (4..65025) is in squared byte units.
        cov = N S_GM - S_G S_M;   den = N S_GG - S_G^2 + eps N^2 (> 0);   a = f32(cov) / f32(den)
        a_q = clamp(rint(a * 1024), -32767, 32767)                        the slope in Q10
        b_q = rint(f32(1024 S_M - a_q S_G) / f32(16 N))                   the offset in Q6
        A = sum a_q, B = sum b_q over the window;   out = clamp8(rint(f32(A G + 16 B) / f32(1024 N)))
    The integers are int64 here; f32() is the round-to-nearest-even conversion, / the IEEE fp32 division, rint rounds halves to even.
    want_coeff: (out, a_q int16 [h, w], b_q int32 [h, w])."""
    G, M = np.asarray(guide), np.asarray(matte)
    assert G.dtype == np.uint8 and M.dtype == np.uint8 and G.ndim == 2 and G.shape == M.shape and G.size > 0
    r, eps = int(radius), int(eps)
    assert 1 <= r <= REFINE_MAX_RADIUS and REFINE_MIN_EPS <= eps <= REFINE_MAX_EPS, (radius, eps)
    g, m = G.astype(np.int64), M.astype(np.int64)
    N = _box_sum(np.ones_like(g), r)
    SG, SM, SGG, SGM = _box_sum(g, r), _box_sum(m, r), _box_sum(g * g, r), _box_sum(g * m, r)
    cov = N * SGM - SG * SM
    den = N * SGG - SG * SG + eps * N * N
    assert den.min() > 0
    f32 = lambda v: v.astype(np.float32)
    a = f32(cov) / f32(den)
    aq = np.clip(np.rint(a * np.float32(1024.0)), -32767, 32767).astype(np.int64)
    bq = np.rint(f32(1024 * SM - aq * SG) / f32(16 * N)).astype(np.int64)
    A, B = _box_sum(aq, r), _box_sum(bq, r)
    out = np.clip(np.rint(f32(A * g + 16 * B) / f32(1024 * N)), 0, 255).astype(np.uint8)
    return (out, aq.astype(np.int16), bq.astype(np.int32)) if want_coeff else out


# One record of the library's regions table (include/tdnet.h tdnet_region, 48 bytes): the box is inclusive, the centroid is sum / area
REGION_DTYPE = np.dtype([("label", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("first_y", "<i4"), ("first_x", "<i4"),
                         ("sum_x", "<u8"), ("sum_y", "<u8")])
REGIONS_HEADER_DTYPE = np.dtype([("count", "<u4"), ("stored", "<u4"), ("status", "<u4"), ("reserved", "<u4")])
REGIONS_OVERFLOW, REGIONS_BOUND = 1, 2                               # header status bits


def regions_u8(labels, classes, connectivity=8, min_area=1, max_regions=256):
    """The oracle of the library's regions output (include/tdnet.h "regions out"): (ids int32 [H, W], count, table).  labels [H, W] uint8; classes the
    ids of the set.  A region is a maximal set of pixels whose label is in the set, connected (4 or 8 neighbours) through pixels of the SAME label.
    A plain flood fill started at every unvisited member pixel in raster order: the start is the region's first pixel, so the regions come out
    by growing key.  Regions below min_area are dropped, the others numbered from 1; ids holds the number (0: background or dropped), also beyond
    max_regions; table is a REGION_DTYPE array of min(count, max_regions) records, record i for region i + 1."""
    lab = np.asarray(labels)
    assert lab.ndim == 2 and lab.dtype == np.uint8 and connectivity in (4, 8) and min_area >= 1 and max_regions >= 1
    H, W = lab.shape
    member = set(int(c) for c in classes)
    flat = lab.reshape(-1).tolist()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    seen = [False] * (H * W)
    found = []                                                         # (pixels, record) by growing first pixel
    for start in range(H * W):
        l = flat[start]
        if seen[start] or l not in member:
            continue
        seen[start] = True
        stack, pixels = [start], []
        while stack:
            p = stack.pop()
            pixels.append(p)
            y, x = divmod(p, W)
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W:
                    q = yy * W + xx
                    if not seen[q] and flat[q] == l:
                        seen[q] = True
                        stack.append(q)
        if len(pixels) < min_area:
            continue
        ys, xs = [p // W for p in pixels], [p % W for p in pixels]
        found.append((pixels, (l, len(pixels), min(xs), min(ys), max(xs), max(ys), start // W, start % W, sum(xs), sum(ys))))
    ids = np.zeros(H * W, np.int32)
    for k, (pixels, _) in enumerate(found):
        ids[pixels] = k + 1
    table = np.array([rec for _, rec in found[:max_regions]], dtype=REGION_DTYPE) if found else np.zeros(0, REGION_DTYPE)
    return ids.reshape(H, W), len(found), table


class RegionTable(np.ndarray):
    """REGION_DTYPE records of the regions a frame's table holds (record i: region i + 1), with the header's .count (all regions found, which may
    exceed len()) and .status (REGIONS_OVERFLOW: count > max_regions) as attributes."""
    count = 0
    status = 0

    def __array_finalize__(self, obj):
        self.count = getattr(obj, "count", 0)
        self.status = getattr(obj, "status", 0)


def region_table(buf, max_regions):
    """The table the library wrote (16 + 48 * max_regions bytes) as a RegionTable of its `stored` records (a copy)."""
    hdr, recs = regions_unpack(buf, max_regions)
    t = recs[:int(hdr["stored"])].copy().view(RegionTable)
    t.count, t.status = int(hdr["count"]), int(hdr["status"])
    return t


def regions_unpack(buf, max_regions):
    """A regions table as the library writes it (bytes, or a uint8 array of 16 + 48 * max_regions) -> (header record, REGION_DTYPE [max_regions])."""
    raw = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    assert raw.size == 16 + 48 * max_regions, (raw.size, max_regions)
    return raw[:16].view(REGIONS_HEADER_DTYPE)[0], raw[16:].view(REGION_DTYPE)


# One record of the library's tracks table (include/tdnet.h tdnet_track, 24 bytes; record i belongs to region i + 1 of the regions table of the same call)
TRACK_DTYPE = np.dtype([("track", "<u4"), ("age", "<u4"), ("prev_region", "<u4"), ("overlap", "<u4"), ("origin_track", "<u4"), ("reserved", "<u4")])
TRACKS_HEADER_DTYPE = np.dtype([("count", "<u4"), ("matched", "<u4"), ("ended", "<u4"), ("status", "<u4")])
TRACKS_BOUND = 1                                                     # header status bit


class TrackOracle:
    """The oracle of the library's tracks output (include/tdnet.h "tracks out"): a small stateful matcher.  .step(labels) labels the frame with
    regions_u8, counts the overlaps n(p, c) of regions that have a record on both sides with np.unique over the pixel pairs, applies the contract --
    best partners with ties to the smallest number, mutual choice and n >= min_overlap continue a track, every other region is born with the next id --
    and returns (ids, region table, track map, header, records): ids and table as regions_u8 gives them, track map int32 [H, W], header a
    TRACKS_HEADER_DTYPE record, records TRACK_DTYPE [stored].  It remembers ONE frame.  .reset() forgets every track: ids restart at 1."""

    def __init__(self, classes, connectivity=8, min_area=1, max_regions=256, min_overlap=1):
        assert min_overlap >= 1
        self.classes, self.connectivity, self.min_area, self.max_regions, self.min_overlap = list(classes), connectivity, min_area, max_regions, min_overlap
        self.reset()

    def reset(self):
        self.prev_ids = None                                           # ids' with everything beyond stored' zeroed
        self.prev_label = np.zeros(0, np.int64)
        self.prev_track = np.zeros(0, np.int64)
        self.prev_age = np.zeros(0, np.int64)
        self.next = 1

    def step(self, labels):
        ids, count, table = regions_u8(labels, self.classes, self.connectivity, self.min_area, self.max_regions)
        stored, storedp = len(table), len(self.prev_track)
        cur = np.where(ids <= stored, ids, 0).astype(np.int64)
        label = table["label"].astype(np.int64)
        n = {}                                                         # (p, c) -> overlap, equal labels only
        if storedp and stored:
            assert self.prev_ids.shape == cur.shape, "a tracker is for frames of one size"
            both = (self.prev_ids > 0) & (cur > 0)
            pairs, counts = np.unique(np.stack([self.prev_ids[both], cur[both]], 1), axis=0, return_counts=True)
            for (p, c), k in zip(pairs.tolist(), counts.tolist()):
                if self.prev_label[p - 1] == label[c - 1]:
                    n[(p, c)] = k
        bp, bc = {}, {}                                                # best partner: largest n, then the smallest number
        for (p, c), k in sorted(n.items()):
            if c not in bp or k > n[(bp[c], c)]:
                bp[c] = p
        for (p, c), k in sorted(n.items(), key=lambda it: (it[0][1], it[0][0])):
            if p not in bc or k > n[(p, bc[p])]:
                bc[p] = c
        recs = np.zeros(stored, TRACK_DTYPE)
        matched = 0
        for c in range(1, stored + 1):
            p = bp.get(c, 0)
            if p and bc[p] == c and n[(p, c)] >= self.min_overlap:
                t = int(self.prev_track[p - 1])
                recs[c - 1] = (t, int(self.prev_age[p - 1]) + 1, p, n[(p, c)], t, 0)
                matched += 1
            else:
                recs[c - 1] = (self.next, 1, 0, 0, int(self.prev_track[p - 1]) if p else 0, 0)
                self.next += 1
        header = np.zeros(1, TRACKS_HEADER_DTYPE)[0]
        header["count"], header["matched"], header["ended"], header["status"] = stored, matched, storedp - matched, 0
        track_map = np.concatenate([[0], recs["track"].astype(np.int64)])[cur].astype(np.int32)
        self.prev_ids, self.prev_label = cur, label
        self.prev_track, self.prev_age = recs["track"].astype(np.int64), recs["age"].astype(np.int64)
        return ids, table, track_map, header, recs


class TrackTable(np.ndarray):
    """TRACK_DTYPE records of the regions a frame's regions table holds (record i: region i + 1), with the header's .matched, .ended and .status as
    attributes; born = len() - matched."""
    matched = 0
    ended = 0
    status = 0

    def __array_finalize__(self, obj):
        self.matched, self.ended, self.status = getattr(obj, "matched", 0), getattr(obj, "ended", 0), getattr(obj, "status", 0)


def tracks_unpack(buf, max_regions):
    """A tracks table as the library writes it (bytes, or a uint8 array of 16 + 24 * max_regions) -> (header record, TRACK_DTYPE [max_regions])."""
    raw = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    assert raw.size == 16 + 24 * max_regions, (raw.size, max_regions)
    return raw[:16].view(TRACKS_HEADER_DTYPE)[0], raw[16:].view(TRACK_DTYPE)


def track_table(buf, max_regions):
    """The table the library wrote (16 + 24 * max_regions bytes) as a TrackTable of its `count` records (a copy)."""
    hdr, recs = tracks_unpack(buf, max_regions)
    t = recs[:int(hdr["count"])].copy().view(TrackTable)
    t.matched, t.ended, t.status = int(hdr["matched"]), int(hdr["ended"]), int(hdr["status"])
    return t


# The library's runs table (include/tdnet.h "runs out"): a 16-byte header, then 8-byte records; record `stored` is the closing record
RUN_DTYPE = np.dtype([("start", "<u4"), ("value", "<i4")])
RUNS_HEADER_DTYPE = np.dtype([("count", "<u4"), ("stored", "<u4"), ("status", "<u4"), ("reserved", "<u4")])
RUNS_OVERFLOW = 1                                                      # header status bit


def runs_of(m, max_runs=None):
    """The run-length table of a map [H, W] (uint8 labels or int32 ids) as the library defines it: pixel i = Y W + X starts a run iff X == 0 or
    m[i] != m[i - 1].  Returns (RUNS_HEADER_DTYPE record, RUN_DTYPE [stored + 1]): the first min(count, max_runs) runs and the closing record
    {start of the next run, or H W; 0}.  max_runs None: H W, every run."""
    m = np.asarray(m)
    H, W = m.shape
    flag = np.ones((H, W), bool)
    flag[:, 1:] = m[:, 1:] != m[:, :-1]
    starts = np.flatnonzero(flag.reshape(-1))
    count = int(starts.size)
    max_runs = H * W if max_runs is None else int(max_runs)
    stored = min(count, max_runs)
    recs = np.zeros(stored + 1, RUN_DTYPE)
    recs["start"][:stored] = starts[:stored]
    recs["value"][:stored] = m.reshape(-1)[starts[:stored]].astype(np.int64)
    recs["start"][stored] = starts[stored] if stored < count else H * W
    hdr = np.zeros(1, RUNS_HEADER_DTYPE)[0]
    hdr["count"], hdr["stored"], hdr["status"] = count, stored, RUNS_OVERFLOW if count > max_runs else 0
    return hdr, recs


def runs_decode(header, records, H, W, fill, dtype=np.int32):
    """The map a table stands for: every pixel below the closing record's start takes the value of its run (dtype uint8: the low byte), the rest `fill`."""
    stored = int(header["stored"])
    starts = records["start"][:stored + 1].astype(np.int64)
    out = np.full(H * W, fill, np.int64)
    out[:starts[stored]] = np.repeat(records["value"][:stored].astype(np.int64), np.diff(starts))
    return (out & 255).astype(np.uint8).reshape(H, W) if np.dtype(dtype) == np.uint8 else out.astype(np.int32).reshape(H, W)


def run_table(buf):
    """A runs table as the library wrote it (bytes, or an array of 16 + 8 (max_runs + 1) bytes) -> (header record, RUN_DTYPE [stored + 1], copies): the
    stored runs and the closing record.  What lies behind the closing record was never written and is not looked at."""
    raw = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    hdr = raw[:16].view(RUNS_HEADER_DTYPE)[0].copy()
    n = int(hdr["stored"]) + 1
    assert raw.size >= 16 + 8 * n, (raw.size, n)
    return hdr, raw[16:16 + 8 * n].view(RUN_DTYPE).copy()


class cityscapesLoader():
    colors = [[128, 64, 128], [244, 35, 232], [70, 70, 70], [102, 102, 156], [190, 153, 153], [153, 153, 153],
              [250, 170, 30], [220, 220, 0], [107, 142, 35], [152, 251, 152], [0, 130, 180], [220, 20, 60],
              [255, 0, 0], [0, 0, 142], [0, 0, 70], [0, 60, 100], [0, 80, 100], [0, 0, 230], [119, 11, 32]]
    label_colours = dict(zip(range(19), colors))

    def __init__(self, img_path, in_size, pin_memory=False, as_uint8=False, as_nv12=False, nv12_standard=0):
        self.img_path = img_path
        self.as_nv12 = bool(as_nv12)                     # not in the reference: frames become NV12 surfaces [1, Hs + ceil(Hs / 2), pitch] (rgb_to_nv12: what a video decoder hands over), items carry (Hs, Ws) as a fifth element (model.forward_nv12 / forward_labels_nv12 convert, resize and normalise on the device)
        self.nv12_standard = int(nv12_standard)
        self.as_uint8 = bool(as_uint8)                   # not in the reference: frames stay the decoded bytes [1, Hs, Ws, 3] (model.forward_u8 / forward_labels_u8 resize and normalise on the device, bit-identically)
        self.pin_memory = bool(pin_memory)               # not in the reference: frames land in page-locked memory (DevicePrefetcher uploads them without a bounce copy)
        self.n_classes = 19
        self.files = sorted(recursive_glob(rootdir=self.img_path, suffix=".png"))
        self.files_num = len(self.files)
        self.data = []
        self.size = (in_size[1], in_size[0])            # (W, H) as dataloader.py:52
        self.mean = np.array([.485, .456, .406])
        self.std = np.array([.229, .224, .225])

    def normalise(self, img_u8):
        """uint8 HWC (already at self.size) -> fp32 [1,3,H,W], dataloader.py:66-71."""
        img = img_u8 / 255.0
        img = (img - self.mean) / self.std
        img = img.transpose(2, 0, 1)[np.newaxis, :]
        t = torch.from_numpy(img).float()
        return t.pin_memory() if self.pin_memory else t

    def load_frames(self):
        from PIL import Image
        for path in self.files:
            path = path.rstrip()
            img_name = path.split('/')[-1]
            folder = path.split('/')[-2]
            im = np.asarray(Image.open(path).convert("RGB"))
            if self.as_nv12:
                t = torch.from_numpy(rgb_to_nv12(im, standard=self.nv12_standard)[np.newaxis])
                self.data.append([t.pin_memory() if self.pin_memory else t, img_name, folder, self.size, (im.shape[0], im.shape[1])])
                continue
            if self.as_uint8:                                          # no resize, no normalisation: a quarter of the fp32 frame's bytes (at equal size)
                t = torch.from_numpy(np.ascontiguousarray(im)[np.newaxis])
                self.data.append([t.pin_memory() if self.pin_memory else t, img_name, folder, self.size])
                continue
            im = resize_linear_u8(im, self.size)                       # = cv2.resize(img, self.size), dataloader.py:64
            self.data.append([self.normalise(im), img_name, folder, self.size])

    def decode_segmap(self, temp):
        rgb = np.zeros((temp.shape[0], temp.shape[1], 3))
        for l in range(0, self.n_classes):
            rgb[temp == l] = self.label_colours[l]
        # labels outside 0..18 keep their raw value in all three channels, as dataloader.py:75-88 does
        other = (temp < 0) | (temp >= self.n_classes)
        rgb[other] = temp[other][:, None]
        return rgb


class DevicePrefetcher:
    """Iterate `loader.data` items ([img [1,3,H,W] fp32 CPU -- or [1,Hs,Ws,3] uint8 from cityscapesLoader(as_uint8=True), or an NV12 surface
    [1,rows,pitch] uint8 from as_nv12=True: the device buffers take the items' dtype and shape, further elements travel as they are --, name,
    folder, size], dataloader.py:73) with the image ALREADY ON THE DEVICE:
    the host->device copy of item i + 1 runs on a copy stream while the caller's stream computes item i.  Page-locked frames
    (cityscapesLoader(..., pin_memory=True)) upload asynchronously; a pageable frame is staged by the HIP runtime while the host waits (still
    under the device's previous frame; an own bounce copy into pinned memory was measured SLOWER than that: 106 against 149 frames/s).
    The reference's loop (`image = image.to(device)`, test.py:47) is then a no-op and needs no change.  Not in the reference: its loop
    uploads a pageable tensor synchronously (216 frames/s at 1024x2048 on MI355X against 255-270 this way, 274 with a resident clip;
    tools/pcie_inclusive_probe.py).

    `depth` (>= 2, default 3) device buffers, reused round-robin: work enqueued on the yielded tensor BEFORE the next `depth - 1` requests
    is safe (the upload that overwrites it waits for an event recorded at that request); the frame loop's use (forward, then drop) fits,
    clone() to keep a frame longer.  Three rather than two, so that the upload of item i + 1 -- issued when item i is requested -- goes
    into the buffer of item i - 2, whose frame has long finished: a pageable upload then never makes the host wait for frame i - 1.

    STREAM CONTRACT: "the consumer's last use" of a buffer is what the CURRENT stream has enqueued when the next item is requested (the
    `freed` event is recorded there).  A consumer that reads the yielded tensor on ANOTHER stream must order that stream into the current one
    before it asks for the next item (`current.wait_stream(other)`), or the upload `depth - 1` requests later may overwrite a frame still being
    read.  The package's own multi-stream consumers do: a batch joins its side lane before forward() returns (model/_base.py), and
    parallel.FramePipelinedStream's lane 0 -- the caller's stream -- waits for every other lane's encode (the only read of the input) inside
    the round, with or without join."""

    def __init__(self, items, device, depth=3):
        self.items, self.device, self.depth = list(items), torch.device(device), max(2, int(depth))
        if self.device.type != "cuda":
            raise ValueError("DevicePrefetcher stages frames for a GPU: device must be cuda")

    def __len__(self):
        return len(self.items)

    def _device_buffer(self, shape):
        return torch.empty(shape, dtype=getattr(self.items[0][0], "dtype", torch.float32), device=self.device)

    def __iter__(self):
        if not self.items:
            return
        dev, D = self.device, self.depth
        copy_s = torch.cuda.Stream(dev)
        shape = tuple(self.items[0][0].shape)
        on_dev = [self._device_buffer(shape) for _ in range(D)]
        landed = [None] * D                                            # the upload into slot k has arrived (copy stream)
        freed = [None] * D                                             # the consumer's stream has passed its last use of slot k

        def upload(i):
            k = i % D
            img = self.items[i][0]
            if tuple(img.shape) != shape:
                raise RuntimeError("DevicePrefetcher: frame %d has shape %s, the stream's frames are %s" % (i, tuple(img.shape), shape))
            with torch.cuda.stream(copy_s):
                if freed[k] is not None:
                    copy_s.wait_event(freed[k])                        # the DEVICE buffer: the consumer's last use of it is behind that event
                on_dev[k].copy_(img, non_blocking=True)                # page-locked frame: asynchronous; pageable: HIP stages it, the host waits here
                landed[k] = torch.cuda.Event()
                landed[k].record(copy_s)

        upload(0)
        for i in range(len(self.items)):
            if i >= 1:                                                 # the consumer asks for item i: its use of item i - 1 is enqueued
                freed[(i - 1) % D] = torch.cuda.Event()
                freed[(i - 1) % D].record(torch.cuda.current_stream(dev))
            if i + 1 < len(self.items):
                upload(i + 1)                                          # into the slot of item i + 1 - D
            torch.cuda.current_stream(dev).wait_event(landed[i % D])
            yield [on_dev[i % D]] + list(self.items[i][1:])


class LabelDownloader:
    """Device int32 (or uint8: forward_labels_u8) label maps -> host numpy arrays through pinned memory, asynchronously: submit(labels, tag) enqueues the copy on a side
    stream and returns the results that have ARRIVED meanwhile as [(tag, array)], in order; drain() waits for the rest.  The arrays are
    VIEWS of the pinned buffers, valid until the next submit() / drain() call (copy what must live longer).  Replaces the
    synchronous `output.max(1)[1].cpu().numpy()` of test.py:61 (a 16.8 MB int64 round trip per 1024x2048 frame) in a loop that wants the
    device to keep running."""

    def __init__(self, device, depth=3):
        self.device, self.depth = torch.device(device), max(2, int(depth))
        self.stream = torch.cuda.Stream(self.device)
        self._slots, self._inflight, self._handed = [], [], []

    @staticmethod
    def _host_buffer(shape, dtype):
        return torch.empty(shape, dtype=dtype).pin_memory()

    def _collect(self, block):
        self._slots.extend(self._handed)                              # the views handed out by the previous call expire now
        self._handed = []
        out = []
        while self._inflight and (block or self._inflight[0][0].query()):
            ev, buf, tag = self._inflight.pop(0)
            ev.synchronize()
            out.append((tag, buf.numpy()))
            self._handed.append(buf)
        return out

    def submit(self, labels, tag=None):
        done = self._collect(block=len(self._inflight) >= self.depth)
        buf = None
        for j, b in enumerate(self._slots):
            if b.shape == labels.shape and b.dtype == labels.dtype:
                buf = self._slots.pop(j)
                break
        if buf is None:
            buf = self._host_buffer(labels.shape, labels.dtype)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            buf.copy_(labels, non_blocking=True)
            labels.record_stream(self.stream)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._inflight.append((ev, buf, tag))
        return done

    def drain(self):
        return self._collect(block=True)


class RunsDownloader:
    """Device runs tables (include/tdnet.h "runs out": a uint8 tensor of runs_bytes) -> host records through pinned memory, asynchronously, beside
    LabelDownloader: submit(table, tag) enqueues ONE copy on a side stream -- the header and a prefix of the records, sized from the count of the latest
    frame that has arrived plus a quarter (before any has: the whole table) -- and returns what has ARRIVED meanwhile as [(tag, header,
    records[:stored + 1])], in order; drain() waits for the rest.  Where the header says the prefix was short, the remainder is fetched with a second
    copy before the frame is handed out.  The downloader keeps the table tensor until then: do not let a later frame overwrite it earlier (rotate
    depth + 1 tables).  The records are VIEWS of the pinned buffers, valid until the next submit() / drain() call.  .short counts the second copies."""

    def __init__(self, device, depth=3):
        self.device, self.depth = torch.device(device), max(2, int(depth))
        self.stream = torch.cuda.Stream(self.device)
        self._slots, self._inflight, self._handed = [], [], []
        self._last_count = None
        self.short = 0

    def _collect(self, block):
        self._slots.extend(self._handed)
        self._handed = []
        out = []
        while self._inflight and (block or self._inflight[0][0].query()):
            ev, buf, table, nbytes, tag = self._inflight.pop(0)
            ev.synchronize()
            raw = buf.numpy()
            hdr = raw[:16].view(RUNS_HEADER_DTYPE)[0].copy()
            need = 16 + 8 * (int(hdr["stored"]) + 1)
            if need > nbytes:                                          # the prefix was short: the remainder, now
                self.short += 1
                with torch.cuda.stream(self.stream):
                    buf[nbytes:need].copy_(table[nbytes:need], non_blocking=True)
                self.stream.synchronize()
            self._last_count = int(hdr["count"])
            out.append((tag, hdr, raw[16:need].view(RUN_DTYPE)))
            self._handed.append(buf)
        return out

    def submit(self, table, tag=None):
        done = self._collect(block=len(self._inflight) >= self.depth)
        table = table.view(torch.uint8).reshape(-1)
        total = int(table.numel())
        buf = None
        for j, b in enumerate(self._slots):
            if b.numel() == total:
                buf = self._slots.pop(j)
                break
        if buf is None:
            buf = torch.empty(total, dtype=torch.uint8).pin_memory()
        nbytes = total if self._last_count is None else min(total, 16 + 8 * (self._last_count + self._last_count // 4 + 1))
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            buf[:nbytes].copy_(table[:nbytes], non_blocking=True)
            table.record_stream(self.stream)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._inflight.append((ev, buf, table, nbytes, tag))
        return done

    def drain(self):
        return self._collect(block=True)
