"""Thin, torch-free owner of one tdnet handle (one video stream on one GPU).

Pointers are plain integers: the model classes pass `tensor.data_ptr()` of torch-ROCm tensors; PyTorch is plumbing
for device memory and streams only.
"""
import ctypes

import numpy as np

from . import _capi


def _ptr(a):
    """int address of a numpy array / integer pointer / None."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    return a.ctypes.data


def view_struct(view):
    """_capi.TdnetView of a dataloader.SourceView, as the caller stated it (0 / None stay the C ABI's defaults)."""
    t = _capi.TdnetView()
    t.format, t.height, t.width, t.pitch, t.standard = view.format, view.height, view.width, view.pitch, view.standard
    if view.crop is not None:
        t.crop_y, t.crop_x, t.crop_height, t.crop_width = view.crop
    t.uv_offset = 0 if view.uv_offset is None else view.uv_offset
    return t


def surface_struct(surface):
    """_capi.TdnetSurface of a dataloader.Surface, as the caller stated it (0 / None stay the C ABI's defaults)."""
    t = _capi.TdnetSurface()
    t.layout, t.height, t.width, t.pitch, t.chroma_pitch, t.standard = (surface.layout, surface.height, surface.width, surface.pitch, surface.chroma_pitch,
                                                                        surface.standard)
    if surface.crop is not None:
        t.crop_y, t.crop_x, t.crop_height, t.crop_width = surface.crop
    t.u_offset = 0 if surface.u_offset is None else surface.u_offset
    t.v_offset = 0 if surface.v_offset is None else surface.v_offset
    return t


class Engine:
    def __init__(self, model, backbone, nclass, height, width, device=0, lib=None, opts=None, _shared_from=None, arch=None):
        """opts: None (library defaults) or a dict of tdnet_opts fields (winograd=, precision=, pipeline=, ...): per handle.
        arch: None (tdnet_create_opts: the shipped dilated, multi-grid backbone) or a dict {dilated:, multi_grid:} of booleans
        (tdnet_create_arch: any layout the reference constructors accept, and pspnet on ResNet-18 / 34)."""
        self.lib = lib or _capi.lib()
        self.cfg = _capi.TdnetCfg(model, backbone, nclass, height, width, device)
        h = ctypes.c_void_p()
        if _shared_from is not None:                                   # a further handle on the same weight block (tdnet_create_shared)
            self.lib.check(self.lib.tdnet_create_shared(_shared_from.h, None, ctypes.byref(h)))
            self.h = h
            self.finalized = True
            return
        o = self.lib.opts(**(opts or {}))
        if arch is None:
            self.lib.check(self.lib.tdnet_create_opts(ctypes.byref(self.cfg), ctypes.byref(o), ctypes.byref(h)))
        else:
            a = arch if isinstance(arch, _capi.TdnetArch) else self.lib.arch(**arch)
            self.lib.check(self.lib.tdnet_create_arch(ctypes.byref(self.cfg), ctypes.byref(a), ctypes.byref(o), ctypes.byref(h)))
        self.h = h
        self.finalized = False

    def share(self):
        """A new Engine on THIS engine's weights (one copy of the packed weights in HBM): own workspace, own K/Q/V FIFO, own streams.
        The weight block is reference-counted in the library: either engine may be closed first."""
        if not self.finalized:
            raise _capi.TdnetError("share(): load_state_dict() first")
        c = self.cfg
        return Engine(c.model, c.backbone, c.nclass, c.height, c.width, c.device, lib=self.lib, _shared_from=self)

    def warmup(self, stream=None):
        """The one host-synchronising step of a handle (placement of its internal streams against `stream`), done now instead of
        inside the first frame (include/tdnet.h "Conventions")."""
        self.lib.check(self.lib.tdnet_warmup(self.h, stream))

    def memory_bytes(self):
        """(bytes of the shared weight block, bytes of this handle alone, handles sharing the block)."""
        w, m = ctypes.c_size_t(), ctypes.c_size_t()
        n = self.lib.check(self.lib.tdnet_memory_bytes(self.h, ctypes.byref(w), ctypes.byref(m)))
        return w.value, m.value, n

    def last_launch_count(self):
        return self.lib.tdnet_last_launch_count(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tdnet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights: strict, like load_state_dict(strict=True) (td4_psp18.py:236-237)
    def load_state_dict(self, sd):
        for name, v in sd.items():
            a = np.ascontiguousarray(np.asarray(v, dtype=np.float32)).reshape(-1)
            if a.size == 0:
                a = np.zeros(1, np.float32)
            self.lib.check(self.lib.tdnet_set_weight(self.h, name.encode(), a.ctypes.data, a.size))
        self.lib.check(self.lib.tdnet_finalize_weights(self.h))
        self.finalized = True

    def forward(self, img_ptr, pos_id, logits_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward(self.h, _ptr(img_ptr), int(pos_id), _ptr(logits_ptr), stream))

    def forward_labels(self, img_ptr, pos_id, labels_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_labels(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), stream))

    # ---- uint8 frames in, uint8 labels out (include/tdnet.h) ----
    def set_input_u8(self, src_height, src_width, mean=None, std=None):
        """Frames will arrive as uint8 [src_height, src_width, 3]; mean / std: three numbers each, None = the loader's.  A configuration
        call (it may synchronise); repeating it with equal arguments does nothing."""
        key = (int(src_height), int(src_width), None if mean is None else tuple(float(v) for v in mean),
               None if std is None else tuple(float(v) for v in std))
        if getattr(self, "_u8_key", None) == key:
            return
        for v in key[2:]:
            if v is not None and len(v) != 3:
                raise _capi.TdnetError("set_input_u8: mean and std are three numbers each")
        m = None if key[2] is None else (ctypes.c_double * 3)(*key[2])
        sd = None if key[3] is None else (ctypes.c_double * 3)(*key[3])
        self.lib.check(self.lib.tdnet_set_input_u8(self.h, key[0], key[1], m, sd))
        self._u8_key, self._nv12_key, self._view_key = key, None, None   # ONE byte-input configuration per handle

    def set_input_nv12(self, src_height, src_width, pitch, uv_offset=None, standard=0, mean=None, std=None):
        """Frames will arrive as NV12 surfaces (include/tdnet.h "NV12 frames in"): the byte entries (forward_u8, ...) then read their image
        pointer as the surface's base, until set_input_u8 switches back.  uv_offset None: src_height * pitch.  A configuration call (it may
        synchronise); repeating it with equal arguments does nothing."""
        key = (int(src_height), int(src_width), int(pitch), int(src_height) * int(pitch) if uv_offset is None else int(uv_offset), int(standard),
               None if mean is None else tuple(float(v) for v in mean), None if std is None else tuple(float(v) for v in std))
        if getattr(self, "_nv12_key", None) == key:
            return
        for v in key[5:]:
            if v is not None and len(v) != 3:
                raise _capi.TdnetError("set_input_nv12: mean and std are three numbers each")
        if uv_offset is not None and key[3] < 0:
            raise _capi.TdnetError("set_input_nv12: uv_offset must not be negative")
        m = None if key[5] is None else (ctypes.c_double * 3)(*key[5])
        sd = None if key[6] is None else (ctypes.c_double * 3)(*key[6])
        self.lib.check(self.lib.tdnet_set_input_nv12(self.h, key[0], key[1], key[2], key[3], key[4], m, sd))
        self._nv12_key, self._u8_key, self._view_key = key, None, None

    def set_input_view(self, view, mean=None, std=None):
        """Frames will arrive as a source view (include/tdnet.h "source views"; `view`: a dataloader.SourceView): the byte entries then read
        their image pointer as the base of the WHOLE frame and take the view's rectangle of it, until another set_input_* call.  A configuration
        call (it may synchronise); repeating it with equal arguments does nothing."""
        key = (view.key(), None if mean is None else tuple(float(v) for v in mean), None if std is None else tuple(float(v) for v in std))
        if getattr(self, "_view_key", None) == key:
            return
        for v in key[1:]:
            if v is not None and len(v) != 3:
                raise _capi.TdnetError("set_input_view: mean and std are three numbers each")
        if view.uv_offset is not None and view.uv_offset < 0:
            raise _capi.TdnetError("set_input_view: uv_offset must not be negative")
        m = None if key[1] is None else (ctypes.c_double * 3)(*key[1])
        sd = None if key[2] is None else (ctypes.c_double * 3)(*key[2])
        self.lib.check(self.lib.tdnet_set_input_view(self.h, ctypes.byref(view_struct(view)), m, sd))
        self._view_key, self._u8_key, self._nv12_key = key, None, None

    def set_input_surface(self, surface, mean=None, std=None):
        """Frames will arrive as YUV surfaces (include/tdnet.h "surfaces"; `surface`: a dataloader.Surface -- NV12, NV21, I420 / YV12, P010, YUY2, UYVY):
        the byte entries then read their image pointer as the surface's base and take its rectangle, until another set_input_* call.  A configuration
        call (it may synchronise); the library recognises equal arguments itself."""
        for v in (mean, std):
            if v is not None and len(v) != 3:
                raise _capi.TdnetError("set_input_surface: mean and std are three numbers each")
        for name in ("u_offset", "v_offset"):
            if getattr(surface, name) is not None and getattr(surface, name) < 0:
                raise _capi.TdnetError("set_input_surface: %s must not be negative" % name)
        m = None if mean is None else (ctypes.c_double * 3)(*[float(v) for v in mean])
        sd = None if std is None else (ctypes.c_double * 3)(*[float(v) for v in std])
        self.lib.check(self.lib.tdnet_set_input_surface(self.h, ctypes.byref(surface_struct(surface)), m, sd))
        self._u8_key, self._nv12_key, self._view_key = None, None, None   # ONE byte-input configuration per handle

    def forward_u8(self, img_ptr, pos_id, logits_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8(self.h, _ptr(img_ptr), int(pos_id), _ptr(logits_ptr), stream))

    def forward_u8_labels(self, img_ptr, pos_id, labels_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_labels(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), stream))

    def encode_u8(self, img_ptr, pos_id, stream=None):
        self.lib.check(self.lib.tdnet_encode_u8(self.h, _ptr(img_ptr), int(pos_id), stream))

    def propagate_labels_u8(self, labels_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_labels_u8(self.h, _ptr(labels_ptr), stream))

    def argmax_u8(self, logits_ptr, labels_ptr, stream=None):
        self.lib.check(self.lib.tdnet_argmax_u8(self.h, _ptr(logits_ptr), _ptr(labels_ptr), stream))

    # ---- colour map out (include/tdnet.h) ----
    def set_output_rgb(self, out_height, out_width, palette):
        """Frames may be asked for as the colour map uint8 [out_height, out_width, 3]; palette: n_colours x 3 byte values (1..256 rows).  A
        configuration call (it may synchronise); repeating it with equal arguments does nothing."""
        pal = None if palette is None else np.ascontiguousarray(np.asarray(palette, dtype=np.uint8))
        if pal is not None and (pal.ndim != 2 or pal.shape[1] != 3):
            raise _capi.TdnetError("set_output_rgb: the palette is n_colours rows of 3 bytes")
        key = (int(out_height), int(out_width), None if pal is None else pal.tobytes())
        if getattr(self, "_rgb_key", None) == key:
            return
        self.lib.check(self.lib.tdnet_set_output_rgb(self.h, key[0], key[1], None if pal is None else pal.ctypes.data, 0 if pal is None else pal.shape[0]))
        self._rgb_key = key

    def forward_rgb(self, img_ptr, pos_id, rgb_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_rgb(self.h, _ptr(img_ptr), int(pos_id), _ptr(rgb_ptr), stream))

    def forward_u8_rgb(self, img_ptr, pos_id, rgb_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_rgb(self.h, _ptr(img_ptr), int(pos_id), _ptr(rgb_ptr), stream))

    def propagate_rgb(self, rgb_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_rgb(self.h, _ptr(rgb_ptr), stream))

    def labels_rgb(self, labels_ptr, rgb_ptr, stream=None):
        self.lib.check(self.lib.tdnet_labels_rgb(self.h, _ptr(labels_ptr), _ptr(rgb_ptr), stream))

    # ---- overlay out (include/tdnet.h) ----
    def set_output_overlay(self, palette_rgba):
        """Frames may be asked for as the overlay uint8 [Hs, Ws, 3] over their source bytes; palette_rgba: n_colours x 4 byte values r, g, b, a
        (1..256 rows; a = 0 leaves the source, a = 255 replaces it).  A configuration call (it may synchronise); repeating it with equal arguments
        does nothing.  Before or after set_input_u8 / set_input_nv12."""
        pal = None if palette_rgba is None else np.ascontiguousarray(np.asarray(palette_rgba, dtype=np.uint8))
        if pal is not None and (pal.ndim != 2 or pal.shape[1] != 4):
            raise _capi.TdnetError("set_output_overlay: the palette is n_colours rows of 4 bytes (r, g, b, a)")
        key = (None if pal is None else pal.tobytes(),)
        if getattr(self, "_overlay_key", None) == key:
            return
        self.lib.check(self.lib.tdnet_set_output_overlay(self.h, None if pal is None else pal.ctypes.data, 0 if pal is None else pal.shape[0]))
        self._overlay_key = key

    def forward_u8_overlay(self, img_ptr, pos_id, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_overlay(self.h, _ptr(img_ptr), int(pos_id), _ptr(out_ptr), stream))

    def propagate_overlay(self, img_ptr, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_overlay(self.h, _ptr(img_ptr), _ptr(out_ptr), stream))

    def labels_overlay(self, labels_ptr, img_ptr, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_labels_overlay(self.h, _ptr(labels_ptr), _ptr(img_ptr), _ptr(out_ptr), stream))

    # ---- destination views (include/tdnet.h) ----
    def set_output_surface(self, surface):
        """The picture entries write into `surface`'s rectangle of a 4:2:0 frame (a dataloader.Surface: NV12, NV21, I420 / YV12 or P010; their picture
        pointer is then the surface's base); None: the contiguous block again.  Replaces a destination view, and is replaced by one."""
        for name in ("u_offset", "v_offset"):
            if surface is not None and getattr(surface, name) is not None and getattr(surface, name) < 0:
                raise _capi.TdnetError("set_output_surface: %s must not be negative" % name)
        self.lib.check(self.lib.tdnet_set_output_surface(self.h, None if surface is None else ctypes.byref(surface_struct(surface))))

    def set_output_view(self, view):
        """The picture entries (forward_rgb, forward_u8_rgb, propagate_rgb, labels_rgb, forward_u8_overlay, propagate_overlay, labels_overlay) will
        write into `view`'s rectangle of a pitched frame (a dataloader.SourceView; their picture pointer is then the frame's base); None: the
        contiguous [h, w, 3] block again.  The rectangle must be the picture's size: the frame entries check that.  A configuration call."""
        if view is not None and view.uv_offset is not None and view.uv_offset < 0:
            raise _capi.TdnetError("set_output_view: uv_offset must not be negative")
        self.lib.check(self.lib.tdnet_set_output_view(self.h, None if view is None else ctypes.byref(view_struct(view))))

    # ---- score out (include/tdnet.h) ----
    def set_score(self, gt_map=None):
        """Frames may be scored against ground truth: allocates this handle's zeroed confusion matrix.  gt_map: 256 byte values (ground-truth byte ->
        class, anything >= nclass = ignore), None = identity.  A configuration call (it may synchronise); repeating it with an equal map does nothing."""
        m = None if gt_map is None else np.ascontiguousarray(np.asarray(gt_map).astype(np.uint8, casting="unsafe"))
        if m is not None and (m.shape != (256,) or not np.array_equal(m, np.asarray(gt_map))):
            raise _capi.TdnetError("set_score: gt_map is 256 values in 0..255")
        key = (None if m is None else m.tobytes(),)
        if getattr(self, "_score_key", None) == key:
            return
        self.lib.check(self.lib.tdnet_set_score(self.h, None if m is None else m.ctypes.data))
        self._score_key = key

    def forward_score(self, img_ptr, pos_id, gt_ptr, labels_ptr=None, stream=None):
        self.lib.check(self.lib.tdnet_forward_score(self.h, _ptr(img_ptr), int(pos_id), _ptr(gt_ptr), _ptr(labels_ptr), stream))

    def forward_u8_score(self, img_ptr, pos_id, gt_ptr, labels_ptr=None, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_score(self.h, _ptr(img_ptr), int(pos_id), _ptr(gt_ptr), _ptr(labels_ptr), stream))

    def propagate_score(self, gt_ptr, labels_ptr=None, stream=None):
        self.lib.check(self.lib.tdnet_propagate_score(self.h, _ptr(gt_ptr), _ptr(labels_ptr), stream))

    def labels_score(self, labels_ptr, gt_ptr, stream=None):
        self.lib.check(self.lib.tdnet_labels_score(self.h, _ptr(labels_ptr), _ptr(gt_ptr), stream))

    def score_reset(self, stream=None):
        self.lib.check(self.lib.tdnet_score_reset(self.h, stream))

    def score_export(self, cm_ptr, stream=None):
        """Enqueue a copy of the nclass x nclass uint64 counts into a device buffer of the caller's."""
        self.lib.check(self.lib.tdnet_score_export(self.h, _ptr(cm_ptr), stream))

    def score_read(self, stream=None):
        """The counts as uint64 [nclass, nclass] on the host (synchronises `stream`)."""
        n = self.cfg.nclass
        out = np.zeros((n, n), np.uint64)
        got = self.lib.check(self.lib.tdnet_score_read(self.h, out.ctypes.data, out.size, stream))
        assert got == out.size, (got, out.size)
        return out

    # ---- confidence out (include/tdnet.h) ----
    def set_confidence(self, min_conf=0, reject_label=255):
        """Labels whose confidence byte is below min_conf (0..255; 0 rejects nothing) are written as reject_label (0..255) by the *_conf entries.
        Plain host state of this handle: no allocation, no synchronisation."""
        self.lib.check(self.lib.tdnet_set_confidence(self.h, int(min_conf), int(reject_label)))

    def forward_labels_conf(self, img_ptr, pos_id, labels_ptr, conf_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_labels_conf(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(conf_ptr), stream))

    def forward_u8_labels_conf(self, img_ptr, pos_id, labels_ptr, conf_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_labels_conf(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(conf_ptr), stream))

    def propagate_labels_conf(self, labels_ptr, conf_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_labels_conf(self.h, _ptr(labels_ptr), _ptr(conf_ptr), stream))

    def logits_conf(self, logits_ptr, labels_ptr, conf_ptr, stream=None):
        self.lib.check(self.lib.tdnet_logits_conf(self.h, _ptr(logits_ptr), _ptr(labels_ptr), _ptr(conf_ptr), stream))

    # ---- matte out (include/tdnet.h) ----
    def set_matte(self, classes):
        """The *_matte entries will write the softmax mass of this class set (ids below nclass; duplicates are legal, an empty list is the empty
        set) as a byte per pixel.  Plain host state of this handle: no allocation, no synchronisation."""
        ids = [int(c) for c in classes]
        if len(ids) > 256 or any(c < 0 or c > 255 for c in ids):
            raise _capi.TdnetError("set_matte: at most 256 class ids in 0..255")
        buf = (ctypes.c_uint8 * max(1, len(ids)))(*ids)
        self.lib.check(self.lib.tdnet_set_matte(self.h, buf if ids else None, len(ids)))

    def forward_matte(self, img_ptr, pos_id, labels_ptr, matte_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_matte(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(matte_ptr), stream))

    def forward_u8_matte(self, img_ptr, pos_id, labels_ptr, matte_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_matte(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(matte_ptr), stream))

    def propagate_matte(self, labels_ptr, matte_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_matte(self.h, _ptr(labels_ptr), _ptr(matte_ptr), stream))

    def logits_matte(self, logits_ptr, labels_ptr, matte_ptr, stream=None):
        self.lib.check(self.lib.tdnet_logits_matte(self.h, _ptr(logits_ptr), _ptr(labels_ptr), _ptr(matte_ptr), stream))

    def set_output_composite(self, background=None):
        """Frames may be asked for as the composite (include/tdnet.h "matte out"): the source frame through the matte at the source's size.
        background (r, g, b): the colour mode, blended over it; None: the alpha mode -- the source's colour bytes and the matte as the x byte of a
        32-bit destination view (set_output_view).  A configuration call; before or after the byte-input configuration."""
        if background is None:
            self.lib.check(self.lib.tdnet_set_output_composite(self.h, 1, None))
            return
        bg = [int(v) for v in background]
        if len(bg) != 3 or any(v < 0 or v > 255 for v in bg):
            raise _capi.TdnetError("set_output_composite: the background is three byte values r, g, b")
        self.lib.check(self.lib.tdnet_set_output_composite(self.h, 0, (ctypes.c_uint8 * 3)(*bg)))

    def forward_u8_composite(self, img_ptr, pos_id, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_composite(self.h, _ptr(img_ptr), int(pos_id), _ptr(out_ptr), stream))

    def propagate_composite(self, img_ptr, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_composite(self.h, _ptr(img_ptr), _ptr(out_ptr), stream))

    def matte_composite(self, matte_ptr, img_ptr, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_matte_composite(self.h, _ptr(matte_ptr), _ptr(img_ptr), _ptr(out_ptr), stream))

    # ---- refined matte (include/tdnet.h) ----
    def set_matte_refine(self, radius, eps=65):
        """radius 1..16 and eps 4..65025 (squared byte units): the composite entries composite through the guided-filtered matte, and the *_matte_refined
        entries write it at the source's size.  radius 0: off (the default).  A configuration call; before or after the byte-input configuration."""
        self.lib.check(self.lib.tdnet_set_matte_refine(self.h, int(radius), int(eps)))

    def forward_u8_matte_refined(self, img_ptr, pos_id, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_matte_refined(self.h, _ptr(img_ptr), int(pos_id), _ptr(out_ptr), stream))

    def propagate_matte_refined(self, img_ptr, out_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_matte_refined(self.h, _ptr(img_ptr), _ptr(out_ptr), stream))

    def refine_scratch_bytes(self, rows, cols):
        """bytes of the scratch refine_matte needs for a map of rows x cols (6 per pixel; 4-byte aligned device memory of the caller's)"""
        return int(self.lib.tdnet_refine_scratch_bytes(int(rows), int(cols)))

    def refine_matte(self, guide_ptr, guide_pitch, matte_ptr, matte_pitch, out_ptr, out_pitch, rows, cols, radius, eps, scratch_ptr, stream=None):
        """The guided filter of the matte bytes [rows, cols] with the guide bytes, rows `pitch` bytes apart at any byte addresses -> out.  Needs no
        configuration; only enqueues (two launches)."""
        self.lib.check(self.lib.tdnet_refine_matte(self.h, _ptr(guide_ptr), int(guide_pitch), _ptr(matte_ptr), int(matte_pitch), _ptr(out_ptr), int(out_pitch),
                                                   int(rows), int(cols), int(radius), int(eps), _ptr(scratch_ptr), stream))

    # ---- regions out (include/tdnet.h) ----
    def set_regions(self, classes, connectivity=8, max_regions=256, min_area=1):
        """The *_regions entries will label the connected components (4 or 8 neighbours, same label) of this class set, drop those below min_area and
        describe the first max_regions in their table.  A configuration call: allocates this handle's workspace once."""
        ids = [int(c) for c in classes]
        if len(ids) > 256 or any(c < 0 or c > 255 for c in ids):
            raise _capi.TdnetError("set_regions: at most 256 class ids in 0..255")
        buf = (ctypes.c_uint8 * max(1, len(ids)))(*ids)
        self.lib.check(self.lib.tdnet_set_regions(self.h, buf if ids else None, len(ids), int(connectivity), int(max_regions), int(min_area)))

    def regions_bytes(self):
        """bytes of the table the regions entries write (16 + 48 * max_regions; 8-byte aligned device memory of the caller's); 0 before set_regions"""
        return int(self.lib.tdnet_regions_bytes(self.h))

    def forward_regions(self, img_ptr, pos_id, labels_ptr, ids_ptr, regions_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_regions(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), stream))

    def forward_u8_regions(self, img_ptr, pos_id, labels_ptr, ids_ptr, regions_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_regions(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), stream))

    def propagate_regions(self, labels_ptr, ids_ptr, regions_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_regions(self.h, _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), stream))

    def labels_regions(self, labels_ptr, ids_ptr, regions_ptr, stream=None):
        self.lib.check(self.lib.tdnet_labels_regions(self.h, _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), stream))

    # ---- tracks out (include/tdnet.h) ----
    def set_tracks(self, min_overlap=1):
        """The *_tracks entries will match each frame's regions against those of the previous tracked frame by pixel overlap (a match needs at least
        min_overlap pixels).  A configuration call: allocates this handle's track state once; a second call keeps the tracks."""
        self.lib.check(self.lib.tdnet_set_tracks(self.h, int(min_overlap)))

    def tracks_bytes(self):
        """bytes of the table the tracks entries write (16 + 24 * max_regions; 8-byte aligned device memory of the caller's); 0 until both set_regions and set_tracks"""
        return int(self.lib.tdnet_tracks_bytes(self.h))

    def forward_tracks(self, img_ptr, pos_id, labels_ptr, ids_ptr, regions_ptr, track_ids_ptr, tracks_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_tracks(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), _ptr(track_ids_ptr),
                                                     _ptr(tracks_ptr), stream))

    def forward_u8_tracks(self, img_ptr, pos_id, labels_ptr, ids_ptr, regions_ptr, track_ids_ptr, tracks_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_tracks(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), _ptr(track_ids_ptr),
                                                        _ptr(tracks_ptr), stream))

    def propagate_tracks(self, labels_ptr, ids_ptr, regions_ptr, track_ids_ptr, tracks_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_tracks(self.h, _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), _ptr(track_ids_ptr), _ptr(tracks_ptr), stream))

    def labels_tracks(self, labels_ptr, ids_ptr, regions_ptr, track_ids_ptr, tracks_ptr, stream=None):
        self.lib.check(self.lib.tdnet_labels_tracks(self.h, _ptr(labels_ptr), _ptr(ids_ptr), _ptr(regions_ptr), _ptr(track_ids_ptr), _ptr(tracks_ptr), stream))

    def tracks_reset(self, stream=None):
        """forget every track (enqueued on the stream): the next tracked frame's regions are all born, from track 1"""
        self.lib.check(self.lib.tdnet_tracks_reset(self.h, stream))

    # ---- runs out (include/tdnet.h) ----
    def set_runs(self, max_runs):
        """The *_runs entries will code a map as a table of at most max_runs (1 .. H W) horizontal runs.  A configuration call: allocates this handle's
        workspace once."""
        self.lib.check(self.lib.tdnet_set_runs(self.h, int(max_runs)))

    def runs_bytes(self):
        """bytes of the table the runs entries write (16 + 8 * (max_runs + 1); 8-byte aligned device memory of the caller's); 0 before set_runs"""
        return int(self.lib.tdnet_runs_bytes(self.h))

    def forward_runs(self, img_ptr, pos_id, labels_ptr, runs_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_runs(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(runs_ptr), stream))

    def forward_u8_runs(self, img_ptr, pos_id, labels_ptr, runs_ptr, stream=None):
        self.lib.check(self.lib.tdnet_forward_u8_runs(self.h, _ptr(img_ptr), int(pos_id), _ptr(labels_ptr), _ptr(runs_ptr), stream))

    def propagate_runs(self, labels_ptr, runs_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_runs(self.h, _ptr(labels_ptr), _ptr(runs_ptr), stream))

    def labels_runs(self, labels_ptr, runs_ptr, stream=None):
        """the unfused form on a uint8 map [H, W] at any byte address"""
        self.lib.check(self.lib.tdnet_labels_runs(self.h, _ptr(labels_ptr), _ptr(runs_ptr), stream))

    def ids_runs(self, ids_ptr, runs_ptr, stream=None):
        """the unfused form on an int32 map [H, W] (an id map or a track map), 4-byte aligned"""
        self.lib.check(self.lib.tdnet_ids_runs(self.h, _ptr(ids_ptr), _ptr(runs_ptr), stream))

    def runs_labels(self, runs_ptr, fill, labels_ptr, stream=None):
        """a table back into a uint8 map [H, W]; pixels the table does not cover get `fill`"""
        self.lib.check(self.lib.tdnet_runs_labels(self.h, _ptr(runs_ptr), int(fill), _ptr(labels_ptr), stream))

    def runs_ids(self, runs_ptr, fill, ids_ptr, stream=None):
        """a table back into an int32 map [H, W]; pixels the table does not cover get `fill`"""
        self.lib.check(self.lib.tdnet_runs_ids(self.h, _ptr(runs_ptr), int(fill), _ptr(ids_ptr), stream))

    # ---- split frame + cache transport (path-parallel single stream; include/tdnet.h) ----
    def encode(self, img_ptr, pos_id, stream=None):
        self.lib.check(self.lib.tdnet_encode(self.h, _ptr(img_ptr), int(pos_id), stream))

    def propagate(self, logits_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate(self.h, _ptr(logits_ptr), stream))

    def propagate_labels(self, labels_ptr, stream=None):
        self.lib.check(self.lib.tdnet_propagate_labels(self.h, _ptr(labels_ptr), stream))

    def cache_dims(self):
        import ctypes
        lk, dk, dv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.lib.check(self.lib.tdnet_cache_dims(self.h, ctypes.byref(lk), ctypes.byref(dk), ctypes.byref(dv)))
        return lk.value, dk.value, dv.value

    def cache_export(self, q_ptr, k_ptr, v_ptr, stream=None):
        self.lib.check(self.lib.tdnet_cache_export(self.h, _ptr(q_ptr), _ptr(k_ptr), _ptr(v_ptr), stream))

    def cache_push(self, q_ptr, k_ptr, v_ptr, stream=None):
        self.lib.check(self.lib.tdnet_cache_push(self.h, _ptr(q_ptr), _ptr(k_ptr), _ptr(v_ptr), stream))

    def argmax(self, logits_ptr, labels_ptr, stream=None):
        self.lib.check(self.lib.tdnet_argmax(self.h, _ptr(logits_ptr), _ptr(labels_ptr), stream))

    def reset(self):
        self.lib.check(self.lib.tdnet_reset(self.h))

    def fifo_len(self):
        return self.lib.tdnet_fifo_len(self.h)

    def stage(self, name, shape):
        out = np.empty(int(np.prod(shape)), np.float32)
        n = self.lib.check(self.lib.tdnet_get_stage(self.h, name.encode(), out.ctypes.data, out.size))
        assert n == out.size, (name, n, out.size)
        return out.reshape(shape)

    def opts(self):
        o = _capi.TdnetOpts()
        self.lib.check(self.lib.tdnet_get_opts(self.h, ctypes.byref(o)))
        return o.as_dict()

    def arch(self):
        a = _capi.TdnetArch()
        self.lib.check(self.lib.tdnet_get_arch(self.h, ctypes.byref(a)))
        return a.as_dict()

    def feature_dims(self):
        """(h, w) of the backbone's output map: the library's stride rule, not restated here."""
        h, w = ctypes.c_int(), ctypes.c_int()
        self.lib.check(self.lib.tdnet_feature_dims(self.h, ctypes.byref(h), ctypes.byref(w)))
        return h.value, w.value

    def flops_per_frame(self):
        return self.lib.tdnet_flops_per_frame(self.h)

    def set_profiling(self, on):
        self.lib.check(self.lib.tdnet_set_profiling(self.h, int(on)))

    def last(self, which):
        """(ms, algorithmic flop, launches) of a kernel family in the last forward; see include/tdnet.h."""
        return (self.lib.tdnet_last_ms(self.h, which), self.lib.tdnet_last_flops(self.h, which),
                self.lib.tdnet_last_launches(self.h, which))
