"""ctypes binding of include/tdnet.h (libtdnet_hip.so) and, for tests / tools only, of include/tdnet_test.h (libtdnet_hip_test.so).

The HIP library is the product: importing a model fails loudly when it is missing -- there is no CPU or
torch fallback anywhere in this package.  The product library exports the C ABI of include/tdnet.h and nothing else; the single-operator entry
points and probes the tests use live in a second library built from the same sources (tdnet_amd/build.py), loaded by `test_lib()`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libtdnet_hip.so")
TEST_LIB = os.path.join(_HERE, "lib", "libtdnet_hip_test.so")

c_float_p = ctypes.POINTER(ctypes.c_float)
c_void_p = ctypes.c_void_p


class TdnetCfg(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("backbone", ctypes.c_int32), ("nclass", ctypes.c_int32),
                ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("device", ctypes.c_int32)]


class TdnetOpts(ctypes.Structure):
    """include/tdnet.h tdnet_opts: per-handle kernel configuration (nothing in the library is process-wide)."""
    _fields_ = [("winograd", ctypes.c_int32), ("precision", ctypes.c_int32), ("pipeline", ctypes.c_int32),
                ("gemm_persistent", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("attention", ctypes.c_int32),
                ("fusion", ctypes.c_int32), ("overlap", ctypes.c_int32), ("reserved", ctypes.c_int32 * 8)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class TdnetArch(ctypes.Structure):
    """include/tdnet.h tdnet_arch: the backbone layout (the reference constructors' dilated / multi_grid)."""
    _fields_ = [("dilated", ctypes.c_int32), ("multi_grid", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]

    def as_dict(self):
        return {"dilated": self.dilated, "multi_grid": self.multi_grid}


class TdnetView(ctypes.Structure):
    """include/tdnet.h tdnet_view: a rectangle of a pitched frame in one of the TDNET_PIX_* formats."""
    _fields_ = [("format", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("pitch", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_x", ctypes.c_int32), ("crop_height", ctypes.c_int32), ("crop_width", ctypes.c_int32),
                ("standard", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5), ("uv_offset", ctypes.c_uint64)]


class TdnetSurface(ctypes.Structure):
    """include/tdnet.h tdnet_surface: a rectangle of a YUV frame in one of the TDNET_SURF_* layouts, its planes in one allocation."""
    _fields_ = [("layout", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("pitch", ctypes.c_int32), ("chroma_pitch", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_x", ctypes.c_int32), ("crop_height", ctypes.c_int32), ("crop_width", ctypes.c_int32),
                ("standard", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4), ("u_offset", ctypes.c_uint64), ("v_offset", ctypes.c_uint64)]


class TdnetError(RuntimeError):
    pass


# name -> (restype, argtypes); every symbol include/tdnet.h declares
WINOGRAD_DEFAULT = 3          # include/tdnet.h TDNET_WINOGRAD_DEFAULT: F(4x4,3x3) for the wide stride-1 3x3 convs
c_opts_p = ctypes.POINTER(TdnetOpts)
c_arch_p = ctypes.POINTER(TdnetArch)
c_view_p = ctypes.POINTER(TdnetView)
c_surface_p = ctypes.POINTER(TdnetSurface)

SYMBOLS = {
    "tdnet_opts_default": (None, [c_opts_p]),
    "tdnet_arch_default": (None, [c_arch_p]),
    "tdnet_create": (ctypes.c_int, [ctypes.POINTER(TdnetCfg), ctypes.POINTER(c_void_p)]),
    "tdnet_create_opts": (ctypes.c_int, [ctypes.POINTER(TdnetCfg), c_opts_p, ctypes.POINTER(c_void_p)]),
    "tdnet_create_arch": (ctypes.c_int, [ctypes.POINTER(TdnetCfg), c_arch_p, c_opts_p, ctypes.POINTER(c_void_p)]),
    "tdnet_get_opts": (ctypes.c_int, [c_void_p, c_opts_p]),
    "tdnet_get_arch": (ctypes.c_int, [c_void_p, c_arch_p]),
    "tdnet_feature_dims": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "tdnet_destroy": (None, [c_void_p]),
    "tdnet_set_weight": (ctypes.c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "tdnet_finalize_weights": (ctypes.c_int, [c_void_p]),
    "tdnet_create_shared": (ctypes.c_int, [c_void_p, c_opts_p, ctypes.POINTER(c_void_p)]),
    "tdnet_warmup": (ctypes.c_int, [c_void_p, c_void_p]),
    "tdnet_memory_bytes": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "tdnet_last_launch_count": (ctypes.c_int, [c_void_p]),
    "tdnet_streams_share_queue": (ctypes.c_int, [c_void_p, c_void_p, ctypes.POINTER(ctypes.c_int)]),
    "tdnet_forward": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_argmax": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_forward_labels": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_set_input_u8": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "tdnet_set_input_nv12": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "tdnet_set_input_view": (ctypes.c_int, [c_void_p, c_view_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "tdnet_set_input_surface": (ctypes.c_int, [c_void_p, c_surface_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "tdnet_set_output_surface": (ctypes.c_int, [c_void_p, c_surface_p]),
    "tdnet_forward_u8": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_forward_u8_labels": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_argmax_u8": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_encode_u8": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p]),
    "tdnet_propagate_labels_u8": (ctypes.c_int, [c_void_p, c_void_p, c_void_p]),
    "tdnet_set_output_rgb": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int]),
    "tdnet_forward_rgb": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_forward_u8_rgb": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_labels_rgb": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_rgb": (ctypes.c_int, [c_void_p, c_void_p, c_void_p]),
    "tdnet_set_output_overlay": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int]),
    "tdnet_forward_u8_overlay": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_labels_overlay": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_overlay": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_set_output_view": (ctypes.c_int, [c_void_p, c_view_p]),
    "tdnet_set_score": (ctypes.c_int, [c_void_p, c_void_p]),
    "tdnet_forward_score": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_forward_u8_score": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_score": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_labels_score": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_score_reset": (ctypes.c_int, [c_void_p, c_void_p]),
    "tdnet_score_export": (ctypes.c_int, [c_void_p, c_void_p, c_void_p]),
    "tdnet_score_read": (ctypes.c_long, [c_void_p, c_void_p, ctypes.c_size_t, c_void_p]),
    "tdnet_set_confidence": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int]),
    "tdnet_forward_labels_conf": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_forward_u8_labels_conf": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_labels_conf": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_logits_conf": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_set_matte": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int]),
    "tdnet_forward_matte": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_forward_u8_matte": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_matte": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_logits_matte": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_set_output_composite": (ctypes.c_int, [c_void_p, ctypes.c_int, c_void_p]),
    "tdnet_forward_u8_composite": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_propagate_composite": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_matte_composite": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_set_matte_refine": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int]),
    "tdnet_forward_u8_matte_refined": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_propagate_matte_refined": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_refine_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "tdnet_refine_matte": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t] + [ctypes.c_int] * 4 + [c_void_p, c_void_p]),
    "tdnet_set_regions": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "tdnet_regions_bytes": (ctypes.c_size_t, [c_void_p]),
    "tdnet_forward_regions": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_forward_u8_regions": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_regions": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_labels_regions": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_set_tracks": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "tdnet_tracks_bytes": (ctypes.c_size_t, [c_void_p]),
    "tdnet_forward_tracks": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int] + [c_void_p] * 6),
    "tdnet_forward_u8_tracks": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int] + [c_void_p] * 6),
    "tdnet_propagate_tracks": (ctypes.c_int, [c_void_p] * 7),
    "tdnet_labels_tracks": (ctypes.c_int, [c_void_p] * 7),
    "tdnet_tracks_reset": (ctypes.c_int, [c_void_p, c_void_p]),
    "tdnet_set_runs": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "tdnet_runs_bytes": (ctypes.c_size_t, [c_void_p]),
    "tdnet_forward_runs": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_forward_u8_runs": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_runs": (ctypes.c_int, [c_void_p] * 4),
    "tdnet_labels_runs": (ctypes.c_int, [c_void_p] * 4),
    "tdnet_ids_runs": (ctypes.c_int, [c_void_p] * 4),
    "tdnet_runs_labels": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_runs_ids": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_reset": (ctypes.c_int, [c_void_p]),
    "tdnet_fifo_len": (ctypes.c_int, [c_void_p]),
    "tdnet_encode": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p]),
    "tdnet_propagate": (ctypes.c_int, [c_void_p, c_void_p, c_void_p]),
    "tdnet_propagate_labels": (ctypes.c_int, [c_void_p, c_void_p, c_void_p]),
    "tdnet_cache_dims": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "tdnet_cache_export": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_cache_push": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_get_stage": (ctypes.c_long, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t]),
    "tdnet_flops_per_frame": (ctypes.c_double, [c_void_p]),
    "tdnet_set_profiling": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "tdnet_last_ms": (ctypes.c_double, [c_void_p, ctypes.c_int]),
    "tdnet_last_flops": (ctypes.c_double, [c_void_p, ctypes.c_int]),
    "tdnet_last_launches": (ctypes.c_double, [c_void_p, ctypes.c_int]),
    "tdnet_last_error": (ctypes.c_char_p, []),
    "tdnet_version": (ctypes.c_char_p, []),
}


# include/tdnet_test.h: libtdnet_hip_test.so (and the emulator library) only
TEST_SYMBOLS = {
    "tdnet_bench_mfma_peak": (ctypes.c_double, [ctypes.c_int, ctypes.c_int, c_void_p]),
    "tdnet_bench_conv": (ctypes.c_double, [ctypes.c_int] * 9 + [c_opts_p, c_void_p]),
    "tdnet_op_conv2d": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int, c_opts_p, ctypes.c_int,
                                       c_void_p, c_void_p]),
    "tdnet_op_conv_wino_f64": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_conv2d_f16io": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int, ctypes.c_int,
                                             c_void_p, c_void_p]),
    "tdnet_op_conv2d_f16mix": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_conv_group_f16": (ctypes.c_int, [ctypes.c_int] + [c_void_p] * 12 + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int), c_void_p]),
    "tdnet_op_cache_subsample": (ctypes.c_int, [c_void_p, c_void_p] + [ctypes.c_int] * 4 + [c_void_p, c_void_p, c_void_p]),
    "tdnet_op_conv1x1_rows": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                             c_opts_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_maxpool": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_stem_f16": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_stem": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_opts_p, c_void_p, c_void_p]),
    "tdnet_op_attention": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_op_layernorm_hw": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_op_layernorm_hw_f16": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdnet_op_ppm": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                    c_void_p, c_void_p]),
    "tdnet_op_upsample": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         c_void_p, c_void_p]),
    "tdnet_op_stem_image": (ctypes.c_long, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), ctypes.c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "tdnet_op_stem_image_nv12": (ctypes.c_long, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "tdnet_op_stem_image_view": (ctypes.c_long, [c_void_p, c_view_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                 ctypes.c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "tdnet_op_stem_image_surface": (ctypes.c_long, [c_void_p, c_surface_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                    ctypes.c_int, c_void_p, ctypes.c_size_t, c_void_p]),
    "tdnet_op_overlay_surface": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, c_surface_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_picture_surface": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_surface_p, c_view_p, ctypes.c_int, ctypes.c_int,
                                                c_void_p, c_surface_p, c_view_p, c_void_p]),
    "tdnet_op_overlay_view": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, c_view_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_picture_view": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_view_p, ctypes.c_int, ctypes.c_int,
                                             c_void_p, c_view_p, c_void_p]),
    "tdnet_op_upsample_argmax": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_op_upsample_argmax_rgb": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 7 + [c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p]),
    "tdnet_op_overlay": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_size_t, ctypes.c_int, c_void_p, ctypes.c_int,
                                        c_void_p, c_void_p]),
    "tdnet_op_upsample_argmax_score": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p] * 6),
    "tdnet_op_upsample_argmax_conf": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_upsample_argmax_matte": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_composite": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, ctypes.c_int] + [c_void_p] * 6 + [ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_refine_coeff": (ctypes.c_int, [c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t] + [ctypes.c_int] * 4 + [c_void_p, c_void_p, c_void_p]),
    "tdnet_op_refine_gather": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, ctypes.c_int] + [c_void_p] * 7),
    "tdnet_op_refine_tile": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 3),
    "tdnet_op_regions": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, c_void_p] + [ctypes.c_int] * 4 + [c_void_p, c_void_p, c_void_p]),
    "tdnet_op_regions_tile": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "tdnet_op_tracks_state_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "tdnet_op_tracks": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 3 + [c_void_p] + [ctypes.c_int] * 5 + [c_void_p] * 6),
    "tdnet_op_tracks_capacity": (ctypes.c_long, [ctypes.c_int, ctypes.c_int]),
    "tdnet_op_runs": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 5 + [c_void_p, c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_runs_decode": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 4 + [c_void_p, c_void_p, c_void_p]),
    "tdnet_op_runs_block": (ctypes.c_int, []),
    "tdnet_op_nearest_index": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_void_p]),
    "tdnet_op_enc_first": (ctypes.c_int, [c_void_p] + [ctypes.c_int] * 4 + [c_void_p] * 4 + [ctypes.c_int] + [c_void_p] * 4 + [ctypes.c_int] + [c_void_p] * 5),
    "tdnet_op_conv1x1_src2_null": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                                  c_void_p, ctypes.c_int, c_opts_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_classifier": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "tdnet_op_head_cls": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                         c_void_p, c_void_p, ctypes.c_int, c_opts_p, ctypes.c_int, c_void_p, c_void_p]),
}


class Lib:
    """A loaded libtdnet shared object with typed entry points; `check()` turns return codes into TdnetError.  test_symbols: also bind the
    entry points of include/tdnet_test.h (the tests' library and the emulator build carry them, the product library does not)."""

    def __init__(self, path=DEFAULT_LIB, test_symbols=False):
        if not os.path.exists(path):
            raise TdnetError("HIP library not found: %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        self.path = path
        if path in (DEFAULT_LIB, TEST_LIB):
            # PyTorch-ROCm bundles its own HIP runtime under the same SONAME; it must be the one already loaded when this
            # library's libamdhip64 dependency is resolved, or the process ends up with two runtimes and hipSetDevice reports
            # "no ROCm-capable device" (seen on the GPU box when the library was loaded before `import torch`).
            import torch  # noqa: F401
        self.dll = ctypes.CDLL(path)
        for name, (res, args) in list(SYMBOLS.items()) + (list(TEST_SYMBOLS.items()) if test_symbols else []):
            fn = getattr(self.dll, name)              # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def opts(self, **kw):
        """tdnet_opts with the library defaults, overridden by keyword (winograd=0, precision=1, ...)."""
        o = TdnetOpts()
        self.tdnet_opts_default(ctypes.byref(o))
        for k, v in kw.items():
            if k not in dict(TdnetOpts._fields_) or k.startswith("reserved"):
                raise TypeError("unknown tdnet_opts field %r" % k)
            if v is not None:
                setattr(o, k, int(v))
        return o

    def arch(self, dilated=True, multi_grid=True):
        """tdnet_arch from the reference constructors' booleans."""
        a = TdnetArch()
        self.tdnet_arch_default(ctypes.byref(a))
        a.dilated, a.multi_grid = int(bool(dilated)), int(bool(multi_grid))
        return a

    def check(self, rc):
        if rc is not None and rc < 0:
            raise TdnetError(self.tdnet_last_error().decode())
        return rc


_default = None
_test = None


def lib():
    """The product library (in-tree libtdnet_hip.so), loaded once."""
    global _default
    if _default is None:
        _default = Lib(DEFAULT_LIB)
    return _default


def test_lib():
    """tests / tools only: the superset library with the single-operator entry points and probes of include/tdnet_test.h."""
    global _test
    if _test is None:
        _test = Lib(TEST_LIB, test_symbols=True)
    return _test
