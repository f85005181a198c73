"""Shared host-side mirror of the reference's stateful TDNet modules (Testing/model/pspnet/td4_psp18.py, td2_psp50.py).

Same constructor arguments, same `forward(img, pos_id)` contract, same failure behaviour (AssertionError on bad
path_num/backbone, RuntimeError on strict-load mismatches and on a LayerNorm/input-size mismatch), but the arithmetic
runs in libtdnet_hip.so (hand-written gfx950 kernels) through the C ABI of include/tdnet.h.  PyTorch supplies device
memory and the current HIP stream only.  There is no CPU path here: a CPU tensor raises.

Differences from the reference, on purpose:
  * a missing checkpoint file is an ERROR unless `synthetic_seed` is given (the reference prints and silently keeps
    random init, td4_psp18.py:239-240);
  * `reset()` empties the K/Q/V FIFO so a second clip can be fed (the reference has no reset);
  * a batch of N > 1 frames is N independent video streams in the reference too (every cached tensor, LayerNorm plane and softmax is
    per sample; td4_psp18.py:123-154 with [N, Lk, 64] queue entries): here sample i runs on its own handle (own FIFO), created the
    first time a batch that large arrives, and the odd samples on a second HIP stream beside the caller's, joined before
    forward() returns: frames of small maps leave CUs idle that another sample's kernels fill (720x960 fp16, two samples: 1445
    frames/s instead of 1100; 1024x2048: no change -- profiles/r04z_multi_clip_*).  Like the reference's queues, the batch size
    must not change while frames are cached;
  * `load_state_dict(strict=False)` drops unexpected keys and reports missing ones like nn.Module does, but a missing tensor has no
    "constructor initialisation" to fall back on here: it is taken from the seeded synthetic generator when `synthetic_seed` is given
    and is an error at the first frame otherwise;
  * td4 accepts all three backbones the reference's constructor accepts (td4_psp18.py:52-66), including the never-shipped
    resnet50 (d_model = d_v = 2048): its attention runs as four 512-channel launches.

Constructor arguments taken as the reference takes them: `dilated` / `multi_grid` select the backbone layout (resnet.py:138-158;
dilated=False is output stride 32: the feature map, the LayerNorm plane and the logits before the x32 upsample are five halvings of the
input), `nclass` is 1..256 (NYUD-v2: 40).  `norm_layer` and `aux` are accepted and ignored.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import arch, weights
from ..engine import Engine
from .._capi import TdnetError


class _TDNetBase(nn.Module):
    _model_id = None       # 4 or 2
    _spec_name = None      # "td4" / "td2"

    def __init__(self, nclass=21, norm_layer=None, backbone="resnet18", dilated=True, aux=True, multi_grid=True,
                 path_num=None, model_path=None, synthetic_seed=None, kernel_opts=None):
        """kernel_opts (not in the reference): dict of include/tdnet.h tdnet_opts fields for THIS instance's handle, e.g.
        {"winograd": 0} for all-direct convs or {"precision": 1} for the fp16-MFMA mode; None = library defaults."""
        super().__init__()
        assert backbone == "resnet50" or backbone == "resnet34" or backbone == "resnet18"
        assert path_num == self._model_id
        self.psp_path = model_path
        self.path_num = path_num
        self.nclass = nclass
        self.backbone = backbone
        self.dilated, self.multi_grid = bool(dilated), bool(multi_grid)
        self.synthetic_seed = synthetic_seed
        self.kernel_opts = dict(kernel_opts or {})
        self._pending_shape = None
        self.spec = arch.model_spec(self._spec_name, nclass, backbone, self.dilated, self.multi_grid)
        self._state = None
        self._engine = None
        self._engine_key = None
        self._init_batch_state()
        self.pretrained_mp_load()

    def _init_batch_state(self):
        self._extra_engines = []                                       # handles of the batch samples 1 .. N-1 (own FIFO each)
        self._extra_streams = []                                       # ... and the HIP streams their frames are enqueued on
        self._extra_streams_for = None                                 # the caller's stream they were placed against
        self._missing_keys = []
        self._batch = None                                             # batch size of the frames currently cached

    # ---- weights ---------------------------------------------------------------------------------------------
    def pretrained_mp_load(self):
        """td4_psp18.py:232-240, except that a missing file raises (see module docstring)."""
        if self.psp_path is not None:
            if os.path.isfile(self.psp_path):
                print("Loading pretrained model from '{}'".format(self.psp_path))
                self.load_state_dict(torch.load(self.psp_path, map_location="cpu"), strict=True)
            elif self.synthetic_seed is None:
                raise FileNotFoundError("No pretrained found at '{}' (pass synthetic_seed=... to run on seeded "
                                        "synthetic weights)".format(self.psp_path))

    def load_state_dict(self, state_dict, strict=True):
        """strict=True (td4_psp18.py:237): the key/shape check against the reference inventory happens in the C library at finalize
        time and raises RuntimeError.  strict=False: unexpected keys are dropped and missing ones recorded, as nn.Module does; the
        result is nn.Module's (missing_keys, unexpected_keys) tuple.  Tensors of the wrong size raise in both modes, like torch."""
        from torch.nn.modules.module import _IncompatibleKeys
        st = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in state_dict.items()}
        missing, unexpected = [], []
        if not strict:
            known = arch.state_dict_shapes(self.spec, 1, 1)                # the key inventory does not depend on the feature size
            unexpected = [k for k in st if k not in known]
            missing = [k for k in known if k not in st and not k.endswith("num_batches_tracked")
                       and not (k.startswith("pretrained") and (k.endswith(".fc.weight") or k.endswith(".fc.bias")))]
            st = {k: v for k, v in st.items() if k in known}
        self._state = st
        self._missing_keys = missing
        self._close_engines()
        return _IncompatibleKeys(missing, unexpected)

    def _close_engines(self):
        for e in [self._engine] + list(getattr(self, "_extra_engines", [])):
            if e is not None:
                e.close()
        self._engine, self._engine_key, self._extra_engines, self._batch = None, None, [], None

    def state_dict(self, *a, **k):
        """{name: CPU tensor} with the reference's keys, so torch.save(model.state_dict()) round-trips like the reference's
        checkpoints (td4_psp18.py:236-237); num_batches_tracked entries are int64 scalars as nn.BatchNorm2d registers them."""
        from collections import OrderedDict
        out = OrderedDict()
        for name, v in (self._state or {}).items():
            a_ = np.asarray(v)
            out[name] = torch.from_numpy(np.array(a_, dtype=np.int64 if name.endswith("num_batches_tracked") else np.float32))
        return out

    # ---- engine ----------------------------------------------------------------------------------------------
    def _get_engine(self, img):
        n, c, H, W = img.shape
        return self._engine_for(H, W, img.device.index or 0, n)

    def _engines_for_batch(self, img, size=None):
        """One handle per batch sample: sample 0 on the model's own handle, sample i > 0 on its own (same weights, own FIFO).
        size: the network's (H, W) where the tensor does not carry it (uint8 frames at their source size)."""
        n = img.shape[0]
        H, W = size if size is not None else img.shape[2:]
        first = self._engine_for(H, W, img.device.index or 0, n)
        if self._batch is not None and n != self._batch and first.fifo_len() > 0:
            # the reference's queues hold [N, Lk, .] tensors: a frame with another N fails in torch.bmm (transformer.py:133)
            raise RuntimeError("Expected batch size %d (the batch size of the cached frames), got %d: reset() the model before feeding "
                               "streams of another batch size" % (self._batch, n))
        self._batch = n
        while len(self._extra_engines) < n - 1:
            # the samples of a batch share one nn.Module's parameters in the reference (td4_psp18.py:216-229): the extra handles share
            # sample 0's weight block (include/tdnet.h tdnet_create_shared) -- own workspace + FIFO + streams, no second copy of the weights
            self._extra_engines.append(first.share())
        return [first] + self._extra_engines[:n - 1]

    def ensure_engine(self, H, W, device):
        """Build the handle (weights, workspace, FIFO) from the stream geometry alone, before any frame is seen.  A path-parallel rank
        that owns no frame of a short first round never calls encode(), yet it must accept its peers' cache entries
        (parallel.PathParallelStream calls this before the first exchange)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise TdnetError("tdnet_amd runs on MI355X only: got device %s (no CPU fallback)" % device)
        return self._engine_for(int(H), int(W), device.index or 0)

    def _engine_for(self, H, W, dev, n=1):
        key = (H, W, dev)
        if self._engine is not None and self._engine_key == key:
            return self._engine
        if self._engine is not None:
            raise RuntimeError("input size/device changed from %s to %s: one model instance serves one stream geometry"
                               % (self._engine_key, key))
        self._engine, self._engine_key = self._build_engine(H, W, dev, n), key
        return self._engine

    def _build_engine(self, H, W, dev, n=1):
        h, w = arch.spec_feat_size(self.spec, H), arch.spec_feat_size(self.spec, W)
        sd = self._state
        if sd is None:
            if self.synthetic_seed is None:
                raise RuntimeError("no weights loaded: give model_path or synthetic_seed (the HIP path never runs on "
                                   "unspecified random init)")
            sd = weights.synth_state_dict(self.spec, h, w, self.synthetic_seed)
        if self._missing_keys:                                           # load_state_dict(strict=False) left these without values
            if self.synthetic_seed is None:
                raise RuntimeError("load_state_dict(strict=False) left %d tensor(s) without values (first: %s); the reference would run them at "
                                   "their random initialisation, which this path refuses -- pass synthetic_seed=... to fill them from the "
                                   "seeded generator" % (len(self._missing_keys), self._missing_keys[0]))
            fill = weights.synth_state_dict(self.spec, h, w, self.synthetic_seed)
            sd = dict(sd)
            for k in self._missing_keys:
                sd[k] = fill[k]
        ln = sd.get("layer_norm1.ln.weight")
        if ln is not None and tuple(ln.shape) != (h, w):
            # same failure the reference raises from nn.LayerNorm (td4_psp18.py:107-110 hard-codes [97,193])
            raise RuntimeError("Given normalized_shape=%s, expected input with shape [*, %d, %d], but got input of size"
                               "[%d, %d, %d, %d]" % (list(ln.shape), ln.shape[0], ln.shape[1], n, self.spec.d_v, h, w))
        try:
            eng = Engine(self._model_id, int(self.backbone[6:]), self.nclass, H, W, dev, opts=self.kernel_opts,
                         arch={"dilated": self.dilated, "multi_grid": self.multi_grid})
            if eng.feature_dims() != (h, w):
                raise TdnetError("internal: feature size %s (library) != %s (arch.py)" % (eng.feature_dims(), (h, w)))
            eng.load_state_dict(sd)
        except TdnetError as e:
            raise RuntimeError("Error(s) in loading state_dict for %s:\n\t%s" % (type(self).__name__, e))
        return eng

    def share_weights_with(self, owner):
        """Serve another stream of the SAME geometry from `owner`'s weight block instead of loading this instance's own copy: this
        model's handle becomes a tdnet_create_shared handle of owner's (own workspace, FIFO and streams; include/tdnet.h).  Used for
        the second lane of parallel.FramePipelinedStream and for clips sharing a GPU (bench.py --clips-per-gpu).  `owner` must have its
        handle (ensure_engine / a first frame); either model may be closed first (the block is reference-counted)."""
        if owner._engine is None:
            raise RuntimeError("share_weights_with(): the owner has no handle yet -- call owner.ensure_engine(H, W, device) first")
        self._close_engines()
        self._state = owner._state
        self._missing_keys = list(owner._missing_keys)
        self._engine, self._engine_key = owner._engine.share(), owner._engine_key
        return self

    # ---- nn.Module surface used by Testing/test.py:40-41,53 ------------------------------------------------------
    def _check_frame(self, img, pos_id):
        if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3:
            raise RuntimeError("expected an image tensor [1,3,H,W]")
        if img.device.type != "cuda":
            raise TdnetError("tdnet_amd runs on MI355X only: got a %s tensor (no CPU fallback)" % img.device.type)
        if img.shape[0] < 1:
            raise RuntimeError("expected an image tensor [N,3,H,W] with N >= 1")
        if pos_id not in range(self.path_num):
            raise RuntimeError("pos_id must be t mod %d" % self.path_num)

    def _for_each_sample(self, img, call, size=None):
        """call(i, engine, raw_stream) for every batch sample: even samples on the caller's stream, odd ones on a second stream, which
        waits for the caller's (the input is ready) and is joined again before this returns -- so the caller's stream stays the only
        one the caller has to order against, as with a single handle.  N = 1 (test.py:46-53): one handle, one call, no events."""
        engines = self._engines_for_batch(img) if size is None else self._engines_for_batch(img, size)
        cur = torch.cuda.current_stream(img.device)
        if len(engines) == 1:
            call(0, engines[0], cur.cuda_stream)
            return
        if self._extra_streams_for != cur.cuda_stream:                 # placed against the caller's stream: another caller stream, again
            self._extra_streams, self._extra_streams_for = [], cur.cuda_stream
        # TWO lanes whatever N: even samples on the caller's stream, odd ones on one extra stream.  A third concurrent frame gains
        # nothing and can cost a lot (720x960 fp16, frames/s in total: 1 sample 1100, 2: 1445, 3 on three streams: 1280 with two
        # hardware queues, 850 with three -- the process then owns more busy queues than stay resident; profiles/r04z_*batched*)
        if not self._extra_streams:
            self._extra_streams.append(self._stream_beside([cur], img.device, engines[0].lib))
        side = self._extra_streams[0]
        ready = torch.cuda.Event()
        ready.record(cur)
        side.wait_event(ready)
        try:
            for i, eng in enumerate(engines):
                call(i, eng, (side if i & 1 else cur).cuda_stream)
        except BaseException:
            # a sample failed (TdnetError from the C library): the samples before it have committed their frame, the ones after it
            # have not -- the per-sample FIFOs are out of step.  Like FramePipelinedStream.process: every stream starts over.
            for eng in engines:
                eng.reset()
            self._batch = None
            raise
        finally:
            cur.wait_stream(side)                                      # whatever happened, the caller's stream is ordered behind the side lane:
                                                                       # `out` and the temporary input were allocated on it and may be freed now

    @staticmethod
    def _stream_beside(taken, device, lib):
        """A stream whose kernels really run BESIDE those of `taken`: HIP deals streams onto a small pool of hardware queues and two
        streams on one queue serialise (which pair collides depends on how many streams the process has created -- with three queues
        the second sample's first candidate lands on the caller's queue: 1066 instead of 1430 frames/s for two 720x960 clips,
        profiles/r04z_hw_queues_*).  Candidates from torch's pool are tried against every taken stream with the library's spin-pair test
        (include/tdnet.h tdnet_streams_share_queue); with more samples than queues the last candidate is used as it is."""
        import ctypes
        s = None
        for _ in range(8):
            s = torch.cuda.Stream(device)
            shared = ctypes.c_int(0)
            for t in taken:
                lib.check(lib.tdnet_streams_share_queue(t.cuda_stream, s.cuda_stream, ctypes.byref(shared)))
                if shared.value:
                    break
            if not shared.value:
                break
        return s

    def forward(self, img, pos_id=0):
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        N = img.shape[0]
        out = torch.empty((N, self.nclass, img.shape[2], img.shape[3]), device=img.device, dtype=torch.float32)
        self._for_each_sample(img, lambda i, eng, s: eng.forward(img[i].data_ptr(), pos_id, out[i].data_ptr(), s))
        return out

    def forward_labels(self, img, pos_id=0):
        """model(img,pos_id).max(1)[1] without materialising the full-resolution logits; int32 [1,H,W]."""
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        N = img.shape[0]
        out = torch.empty((N, img.shape[2], img.shape[3]), device=img.device, dtype=torch.int32)
        self._for_each_sample(img, lambda i, eng, s: eng.forward_labels(img[i].data_ptr(), pos_id, out[i].data_ptr(), s))
        return out

    # ---- uint8 frames in, uint8 labels out (not in the reference; include/tdnet.h "uint8 frames in") ---------------------------------
    # img_u8: torch.uint8 CUDA tensor [N, Hs, Ws, 3] -- the decoded frames as they are (RGB, HWC, any source size).  The library resizes to
    # the network size and normalises on the device, bit-identically to cityscapesLoader (resize_linear_u8 + normalise), so
    # forward_u8(frame_bytes) == forward(loader_tensor).  The NETWORK size is the one the handle was built for: by ensure_engine(H, W, device)
    # or an earlier frame; a model without a handle takes it from in_size=(H, W) (as cityscapesLoader does).
    # view: a dataloader.SourceView (include/tdnet.h "source views") -- img_u8 is then a contiguous uint8 tensor [N, nbytes], nbytes >= view_extent(view):
    # N WHOLE frames in the view's format and pitch, of which the library reads the view's rectangle (b g r or 4-byte pixels, a crop, an NV12 surface
    # with a display rectangle), bit-identically to forward_u8(dataloader.view_to_rgb_u8(frame, view)).
    # surface: a dataloader.Surface (include/tdnet.h "surfaces") in place of view -- img_u8 is then N WHOLE YUV frames [N, nbytes], nbytes >=
    # surface_extent(surface), in one of the layouts NV12 / NV21 / I420 (YV12) / P010 / YUY2 / UYVY, bit-identically to
    # forward_u8(dataloader.surface_to_rgb_u8(frame, surface)).  out_surface: a 4:2:0 Surface in place of out_view.  Giving both of a pair is an error.
    @staticmethod
    def _one_of(a, b, name_a, name_b):
        """view= and surface= (out_view= and out_surface=) describe the same thing two ways: at most one of them."""
        if a is not None and b is not None:
            raise RuntimeError("give %s or %s, not both" % (name_a, name_b))
        return a if b is None else b

    @staticmethod
    def _is_surface(x):
        from ..dataloader import Surface
        return isinstance(x, Surface)

    def _set_in(self, eng, view, mean, std):
        (eng.set_input_surface if self._is_surface(view) else eng.set_input_view)(view, mean, std)

    def _set_out(self, eng, out_view):
        """The destination of the picture entries: a view, a surface, or None (either call restores the contiguous block)."""
        (eng.set_output_surface if self._is_surface(out_view) else eng.set_output_view)(out_view)

    @classmethod
    def _frame_extent(cls, x):
        from ..dataloader import surface_extent, view_extent
        return surface_extent(x) if cls._is_surface(x) else view_extent(x)

    @staticmethod
    def _check_surface(s, what, dst=False):
        """What the derived values of a Surface need, before an engine exists; the library judges the rest."""
        from ..dataloader import SURF_DST
        y, x, h, w = s.rect
        if s.height < 1 or s.width < 1 or h < 1 or w < 1 or y < 0 or x < 0 or y + h > s.height or x + w > s.width:
            raise RuntimeError("%s's rectangle (y, x, h, w) = %r is not inside its %d x %d frame" % (what, s.rect, s.height, s.width))
        if s.row_pitch < s.luma_row_bytes:
            raise RuntimeError("%s's pitch %d is below the %d bytes a row of %d pixels holds" % (what, s.row_pitch, s.luma_row_bytes, s.width))
        if not s.packed422 and s.cpitch < s.chroma_row_bytes:
            raise RuntimeError("%s's chroma pitch %d is below the %d bytes a chroma row of %d pixels holds" % (what, s.cpitch, s.chroma_row_bytes, s.width))
        if dst and s.layout not in SURF_DST:
            raise RuntimeError("%s: YUY2 / UYVY are not destination layouts (NV12, NV21, I420 and P010 are)" % what)
        if dst and (y % 2 or x % 2):
            raise RuntimeError("%s's origin (%d, %d) must be even for a 4:2:0 destination" % (what, y, x))

    def _check_frame_view(self, img, view):
        """The error classes of _check_frame_u8 for a batch of whole frames read through `view`; nothing is built before it passes."""
        from ..dataloader import SourceView, Surface, view_extent
        if not isinstance(view, (SourceView, Surface)):
            raise RuntimeError("view must be a dataloader.SourceView (surface: a dataloader.Surface), got %s" % type(view).__name__)
        if isinstance(view, Surface):
            if not torch.is_tensor(img) or img.dtype != torch.uint8:
                raise RuntimeError("expected a torch.uint8 frame tensor [N,nbytes], got %s" % (img.dtype if torch.is_tensor(img) else type(img).__name__))
            if img.dim() != 2 or img.shape[0] < 1:
                raise RuntimeError("expected a uint8 frame tensor [N,nbytes] (whole surfaces) with N >= 1, got shape %s" % (tuple(img.shape),))
            if not img.is_contiguous():
                raise RuntimeError("expected a CONTIGUOUS uint8 frame tensor [N,nbytes]: the surface's pitches describe the rows")
            self._check_surface(view, "the surface")
            if int(img.shape[1]) < self._frame_extent(view):
                raise RuntimeError("a frame tensor of %d bytes per sample is below the %d bytes the surface needs" % (img.shape[1], self._frame_extent(view)))
            return
        if not torch.is_tensor(img) or img.dtype != torch.uint8:
            raise RuntimeError("expected a torch.uint8 frame tensor [N,nbytes], got %s" % (img.dtype if torch.is_tensor(img) else type(img).__name__))
        if img.dim() != 2 or img.shape[0] < 1:
            raise RuntimeError("expected a uint8 frame tensor [N,nbytes] (whole frames read through the view) with N >= 1, got shape %s" % (tuple(img.shape),))
        if not img.is_contiguous():
            raise RuntimeError("expected a CONTIGUOUS uint8 frame tensor [N,nbytes]: the view's pitch describes the rows")
        y, x, h, w = view.rect
        if view.height < 1 or view.width < 1 or h < 1 or w < 1 or y < 0 or x < 0 or y + h > view.height or x + w > view.width:
            raise RuntimeError("the view's rectangle (y, x, h, w) = %r is not inside its %d x %d frame" % (view.rect, view.height, view.width))
        row = 2 * ((view.width + 1) // 2) if view.nv12 else view.width * view.bpp
        if view.row_pitch < row:
            raise RuntimeError("the view's pitch %d is below the %d bytes a row of %d pixels holds" % (view.row_pitch, row, view.width))
        if view.nv12 and view.uv < view.height * view.row_pitch:
            raise RuntimeError("the view's uv_offset %d is inside the Y plane (%d rows of pitch %d)" % (view.uv, view.height, view.row_pitch))
        if int(img.shape[1]) < view_extent(view):
            raise RuntimeError("a frame tensor of %d bytes per sample is below the %d bytes the view's frame needs" % (img.shape[1], view_extent(view)))

    def _check_frame_u8(self, img, pos_id, in_size, view=None):
        if view is not None:
            self._check_frame_view(img, view)
        elif not torch.is_tensor(img) or img.dtype != torch.uint8:
            raise RuntimeError("expected a torch.uint8 image tensor [N,Hs,Ws,3], got %s" % (img.dtype if torch.is_tensor(img) else type(img).__name__))
        if view is None and (img.dim() != 4 or img.shape[3] != 3):
            raise RuntimeError("expected a uint8 image tensor [N,Hs,Ws,3] (HWC, RGB), got shape %s" % (tuple(img.shape),))
        if img.device.type != "cuda":
            raise TdnetError("tdnet_amd runs on MI355X only: got a %s tensor (no CPU fallback)" % img.device.type)
        if view is None and (img.shape[0] < 1 or img.shape[1] < 1 or img.shape[2] < 1):
            raise RuntimeError("expected a uint8 image tensor [N,Hs,Ws,3] with N, Hs, Ws >= 1")
        if pos_id not in range(self.path_num):
            raise RuntimeError("pos_id must be t mod %d" % self.path_num)
        if in_size is not None:
            return int(in_size[0]), int(in_size[1])
        if self._engine_key is None:
            raise RuntimeError("the network size is not known yet: pass in_size=(H, W), or call ensure_engine(H, W, device) first")
        return self._engine_key[0], self._engine_key[1]

    def _u8_call(self, img, size, call, mean, std, nv12=None, view=None):
        """nv12: None, or (Hs, Ws, pitch, uv_offset, standard) -- img is then a batch of NV12 surfaces and the handles are configured for those.
        view: None, or a SourceView -- img is then a batch of whole frames [N, nbytes] read through it."""
        Hs, Ws = (0, 0) if view is not None else (int(img.shape[1]), int(img.shape[2]))

        def one(i, eng, s):
            if view is not None:
                self._set_in(eng, view, mean, std)
            elif nv12 is None:
                eng.set_input_u8(Hs, Ws, mean, std)                    # (re)configured when the source size changes; a no-op otherwise
            else:
                eng.set_input_nv12(*nv12, mean=mean, std=std)
            call(i, eng, s)
        self._for_each_sample(img, one, size)

    def forward_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None):
        """forward() on the decoded bytes: logits [N, nclass, H, W] at the network size."""
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        out = torch.empty((img.shape[0], self.nclass, H, W), device=img.device, dtype=torch.float32)
        self._u8_call(img, (H, W), lambda i, eng, s: eng.forward_u8(img[i].data_ptr(), pos_id, out[i].data_ptr(), s), mean, std, view=view)
        return out

    def forward_labels_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None):
        """forward_labels() on the decoded bytes, labels as uint8 [N, H, W] (the same labels: nclass <= 256)."""
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        out = torch.empty((img.shape[0], H, W), device=img.device, dtype=torch.uint8)
        self._u8_call(img, (H, W), lambda i, eng, s: eng.forward_u8_labels(img[i].data_ptr(), pos_id, out[i].data_ptr(), s), mean, std, view=view)
        return out

    def encode_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None):
        """encode() on the decoded bytes."""
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        if img_u8.shape[0] != 1:
            raise RuntimeError("encode_u8(): the split frame serves ONE stream (batch size 1)")
        img = img_u8.contiguous()
        eng = self._engine_for(H, W, img.device.index or 0, 1)
        if view is not None:
            self._set_in(eng, view, mean, std)
        else:
            eng.set_input_u8(int(img.shape[1]), int(img.shape[2]), mean, std)
        self._pending_shape = (H, W, img.device)
        eng.encode_u8(img.data_ptr(), pos_id, torch.cuda.current_stream(img.device).cuda_stream)

    def argmax_u8(self, logits):
        """logits [N, nclass, H, W] (fp32, CUDA) of this model -> uint8 labels [N, H, W] = logits.max(1)[1]."""
        if self._engine is None:
            raise RuntimeError("argmax_u8(): no handle yet")
        logits = logits.contiguous().float()
        out = torch.empty((logits.shape[0],) + tuple(logits.shape[2:]), device=logits.device, dtype=torch.uint8)
        s = torch.cuda.current_stream(logits.device).cuda_stream
        for i in range(logits.shape[0]):
            self._engine.argmax_u8(logits[i].data_ptr(), out[i].data_ptr(), s)
        return out

    # ---- NV12 frames in (not in the reference; include/tdnet.h "NV12 frames in") ---------------------------------------------------------
    # surf: torch.uint8 CUDA tensor [N, rows, pitch] -- N decoder surfaces as they are: the Y plane's rows from byte 0, the interleaved UV
    # plane's from uv_offset (None: Hs * pitch), both with the row pitch.  src_size = (Hs, Ws) is the picture's size.  The library converts
    # (standard: 0 BT.601 limited, 1 BT.709 limited, 2 BT.601 full, 3 BT.709 full), resizes and normalises in the frame's first launch,
    # bit-identically to forward_u8(dataloader.nv12_to_rgb_u8(surface)).
    def _check_frame_nv12(self, surf, pos_id, src_size, in_size, uv_offset, standard):
        """-> ((H, W), (Hs, Ws, pitch, uv_offset, standard)).  The error classes of _check_frame_u8; nothing is built before it passes."""
        if not torch.is_tensor(surf) or surf.dtype != torch.uint8:
            raise RuntimeError("expected a torch.uint8 surface tensor [N,rows,pitch], got %s" % (surf.dtype if torch.is_tensor(surf) else type(surf).__name__))
        if surf.dim() != 3 or surf.shape[0] < 1:
            raise RuntimeError("expected a uint8 surface tensor [N,rows,pitch] (NV12: Y rows, then UV rows) with N >= 1, got shape %s" % (tuple(surf.shape),))
        if src_size is None or len(src_size) != 2 or int(src_size[0]) < 1 or int(src_size[1]) < 1:
            raise RuntimeError("src_size must be (Hs, Ws), at least (1, 1), got %r" % (src_size,))
        Hs, Ws, pitch = int(src_size[0]), int(src_size[1]), int(surf.shape[2])
        off = Hs * pitch if uv_offset is None else int(uv_offset)
        if standard not in (0, 1, 2, 3):
            raise RuntimeError("standard must be 0 (BT.601 limited), 1 (BT.709 limited), 2 (BT.601 full) or 3 (BT.709 full), got %r" % (standard,))
        if pitch < 2 * ((Ws + 1) // 2):
            raise RuntimeError("the surface's pitch %d is below the %d bytes a row of %d columns holds" % (pitch, 2 * ((Ws + 1) // 2), Ws))
        if off < Hs * pitch:
            raise RuntimeError("uv_offset %d is inside the Y plane (%d rows of pitch %d)" % (off, Hs, pitch))
        extent = off + ((Hs + 1) // 2 - 1) * pitch + 2 * ((Ws + 1) // 2)
        if int(surf.shape[1]) * pitch < extent:
            raise RuntimeError("a surface of %d rows x pitch %d holds %d bytes, a %d x %d picture with uv_offset %d needs %d"
                               % (surf.shape[1], pitch, int(surf.shape[1]) * pitch, Hs, Ws, off, extent))
        if surf.device.type != "cuda":
            raise TdnetError("tdnet_amd runs on MI355X only: got a %s tensor (no CPU fallback)" % surf.device.type)
        if pos_id not in range(self.path_num):
            raise RuntimeError("pos_id must be t mod %d" % self.path_num)
        if in_size is not None:
            return (int(in_size[0]), int(in_size[1])), (Hs, Ws, pitch, off, int(standard))
        if self._engine_key is None:
            raise RuntimeError("the network size is not known yet: pass in_size=(H, W), or call ensure_engine(H, W, device) first")
        return (self._engine_key[0], self._engine_key[1]), (Hs, Ws, pitch, off, int(standard))

    def forward_nv12(self, surf, pos_id=0, src_size=None, in_size=None, uv_offset=None, standard=0, mean=None, std=None):
        """forward() on decoder surfaces: logits [N, nclass, H, W] at the network size."""
        (H, W), nv = self._check_frame_nv12(surf, pos_id, src_size, in_size, uv_offset, standard)
        img = surf.contiguous()
        out = torch.empty((img.shape[0], self.nclass, H, W), device=img.device, dtype=torch.float32)
        self._u8_call(img, (H, W), lambda i, eng, s: eng.forward_u8(img[i].data_ptr(), pos_id, out[i].data_ptr(), s), mean, std, nv)
        return out

    def forward_labels_nv12(self, surf, pos_id=0, src_size=None, in_size=None, uv_offset=None, standard=0, mean=None, std=None):
        """forward_labels() on decoder surfaces, labels as uint8 [N, H, W]."""
        (H, W), nv = self._check_frame_nv12(surf, pos_id, src_size, in_size, uv_offset, standard)
        img = surf.contiguous()
        out = torch.empty((img.shape[0], H, W), device=img.device, dtype=torch.uint8)
        self._u8_call(img, (H, W), lambda i, eng, s: eng.forward_u8_labels(img[i].data_ptr(), pos_id, out[i].data_ptr(), s), mean, std, nv)
        return out

    def encode_nv12(self, surf, pos_id=0, src_size=None, in_size=None, uv_offset=None, standard=0, mean=None, std=None):
        """encode() on a decoder surface."""
        (H, W), nv = self._check_frame_nv12(surf, pos_id, src_size, in_size, uv_offset, standard)
        if surf.shape[0] != 1:
            raise RuntimeError("encode_nv12(): the split frame serves ONE stream (batch size 1)")
        img = surf.contiguous()
        eng = self._engine_for(H, W, img.device.index or 0, 1)
        eng.set_input_nv12(*nv, mean=mean, std=std)
        self._pending_shape = (H, W, img.device)
        eng.encode_u8(img.data_ptr(), pos_id, torch.cuda.current_stream(img.device).cuda_stream)

    def forward_rgb_nv12(self, surf, pos_id, src_size, in_size, out_size, palette=None, uv_offset=None, standard=0, mean=None, std=None):
        """forward_labels_nv12() with the colour map [N, oh, ow, 3] uint8 in place of the label map: a decoder surface in, a picture out."""
        self._rgb_size(out_size)
        (H, W), nv = self._check_frame_nv12(surf, pos_id, src_size, in_size, uv_offset, standard)
        img = surf.contiguous()
        out, pal = self._rgb_out(img.shape[0], out_size, img.device), self._palette(palette)

        def one(i, eng, s):
            eng.set_output_rgb(out.shape[1], out.shape[2], pal)
            eng.set_output_view(None)
            eng.forward_u8_rgb(img[i].data_ptr(), pos_id, out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, nv)
        return out

    def forward_score_nv12(self, surf, gt_u8, pos_id=0, src_size=None, in_size=None, gt_map=None, return_labels=False, uv_offset=None, standard=0,
                           mean=None, std=None):
        """forward_labels_nv12() with the frame scored on the device (see forward_score_u8)."""
        self._check_gt_type(gt_u8)
        (H, W), nv = self._check_frame_nv12(surf, pos_id, src_size, in_size, uv_offset, standard)
        img = surf.contiguous()
        gt = self._check_gt(gt_u8, img.shape[0], H, W, img.device)
        out = torch.empty((img.shape[0], H, W), device=img.device, dtype=torch.uint8) if return_labels else None

        def one(i, eng, s):
            eng.set_score(gt_map)
            eng.forward_u8_score(img[i].data_ptr(), pos_id, gt[i].data_ptr(), None if out is None else out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, nv)
        return out

    def forward_labels_conf_nv12(self, surf, pos_id=0, src_size=None, in_size=None, uv_offset=None, standard=0, mean=None, std=None):
        """forward_labels_nv12() with the confidence map: (labels uint8 [N, H, W], conf uint8 [N, H, W])."""
        (H, W), nv = self._check_frame_nv12(surf, pos_id, src_size, in_size, uv_offset, standard)
        img = surf.contiguous()
        shape = (img.shape[0], H, W)
        out, conf = torch.empty(shape, device=img.device, dtype=torch.uint8), torch.empty(shape, device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_confidence(*self._confidence)
            eng.forward_u8_labels_conf(img[i].data_ptr(), pos_id, out[i].data_ptr(), conf[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, nv)
        return out, conf

    # ---- colour map out (not in the reference's model; its loop makes the picture on the host, test.py:61-71) -------------------------
    # The frame's last kernel writes decode_segmap(labels[ys][:, xs]) directly: uint8 [N, oh, ow, 3], ys / xs = dataloader.nearest_index.
    # out_size = (oh, ow); palette: n_colours x 3 byte values, None = cityscapesLoader.label_colours.
    @staticmethod
    def _palette(palette):
        if palette is None:
            from ..dataloader import cityscapesLoader
            palette = cityscapesLoader.colors
        return np.ascontiguousarray(np.asarray(palette, dtype=np.uint8))

    @staticmethod
    def _rgb_size(out_size):
        if out_size is None or len(out_size) != 2 or int(out_size[0]) < 1 or int(out_size[1]) < 1:
            raise RuntimeError("out_size must be (oh, ow), at least (1, 1), got %r" % (out_size,))
        return int(out_size[0]), int(out_size[1])

    # out_view: a dataloader.SourceView (include/tdnet.h "destination views") -- the picture is then written into the view's rectangle of a pitched RGB /
    # BGR / RGBA / BGRA / NV12 frame and the method returns a uint8 tensor [N, nbytes], nbytes >= view_extent(out_view): N whole destination frames.
    # out: that tensor supplied by the caller (only the rectangle's bytes are written: the rest of a frame the caller composed stays); None: zeros.  The
    # rectangle must be the picture's size; the source's colour order no longer decides the picture's, the destination format does.
    def _dst_out(self, out_view, out, size, n, device):
        """The tensor [N, nbytes] the entries write into: the caller's, checked, or zeros."""
        from ..dataloader import view_extent
        self._dst_check(out_view, out, size, n)
        if out is None:
            return torch.zeros((n, self._frame_extent(out_view)), device=device, dtype=torch.uint8)
        if out.device != device:
            raise RuntimeError("out must be on the frames' device %s, got %s" % (device, out.device))
        return out

    @classmethod
    def _dst_check(cls, out_view, out, size, n):
        """The checks of a destination view (or surface) and tensor, made before an engine exists (and before the frames' device is looked at, like view=)."""
        from ..dataloader import SourceView, Surface, view_extent
        if not isinstance(out_view, (SourceView, Surface)):
            raise RuntimeError("out_view must be a dataloader.SourceView (out_surface: a dataloader.Surface), got %s" % type(out_view).__name__)
        if isinstance(out_view, Surface):
            cls._check_surface(out_view, "out_surface", dst=True)
            if tuple(out_view.size) != tuple(int(v) for v in size):
                raise RuntimeError("out_surface's rectangle is %d x %d but the picture is %d x %d: nothing is resized" % (tuple(out_view.size) + (size[0], size[1])))
            cls._dst_tensor_check(out, n, cls._frame_extent(out_view), "out_surface")
            return
        y, x, h, w = out_view.rect
        if out_view.height < 1 or out_view.width < 1 or h < 1 or w < 1 or y < 0 or x < 0 or y + h > out_view.height or x + w > out_view.width:
            raise RuntimeError("out_view's rectangle (y, x, h, w) = %r is not inside its %d x %d frame" % (out_view.rect, out_view.height, out_view.width))
        if (h, w) != tuple(int(v) for v in size):
            raise RuntimeError("out_view's rectangle is %d x %d but the picture is %d x %d: nothing is resized" % (h, w, size[0], size[1]))
        row = 2 * ((out_view.width + 1) // 2) if out_view.nv12 else out_view.width * out_view.bpp
        if out_view.row_pitch < row:
            raise RuntimeError("out_view's pitch %d is below the %d bytes a row of %d pixels holds" % (out_view.row_pitch, row, out_view.width))
        if out_view.nv12 and out_view.uv < out_view.height * out_view.row_pitch:
            raise RuntimeError("out_view's uv_offset %d is inside the Y plane (%d rows of pitch %d)" % (out_view.uv, out_view.height, out_view.row_pitch))
        if out_view.nv12 and (y % 2 or x % 2):
            raise RuntimeError("out_view's origin (%d, %d) must be even for an NV12 destination" % (y, x))
        cls._dst_tensor_check(out, n, view_extent(out_view), "out_view")

    @staticmethod
    def _dst_tensor_check(out, n, need, what):
        if out is None:
            return
        if not torch.is_tensor(out) or out.dtype != torch.uint8:
            raise RuntimeError("out must be a torch.uint8 tensor, got %s" % (out.dtype if torch.is_tensor(out) else type(out).__name__))
        if out.dim() != 2 or out.shape[0] != n:
            raise RuntimeError("out must be a uint8 tensor [N,nbytes] with N = %d (whole destination frames), got shape %s" % (n, tuple(out.shape)))
        if not out.is_contiguous():
            raise RuntimeError("out must be a CONTIGUOUS uint8 tensor [N,nbytes]: %s's pitch describes the rows" % what)
        if int(out.shape[1]) < need:
            raise RuntimeError("out holds %d bytes per sample, below the %d bytes %s's frame needs" % (out.shape[1], need, what))

    def _rgb_out(self, n, out_size, device):
        oh, ow = self._rgb_size(out_size)
        return torch.empty((n, oh, ow, 3), device=device, dtype=torch.uint8)

    def forward_rgb(self, img, pos_id, out_size, palette=None, out_view=None, out=None, out_surface=None):
        """forward_labels() with the colour map [N, oh, ow, 3] uint8 in place of the label map (out_view: see _dst_out)."""
        out_view = self._one_of(out_view, out_surface, "out_view", "out_surface")
        oh, ow = self._rgb_size(out_size)
        self._check_frame(img, pos_id)
        out = self._dst_out(out_view, out, (oh, ow), img.shape[0], img.device) if out_view is not None else self._rgb_out(img.shape[0], out_size, img.device)
        img = img.contiguous().float()
        pal = self._palette(palette)

        def one(i, eng, s):
            eng.set_output_rgb(oh, ow, pal)
            self._set_out(eng, out_view)
            eng.forward_rgb(img[i].data_ptr(), pos_id, out[i].data_ptr(), s)
        self._for_each_sample(img, one)
        return out

    def forward_rgb_u8(self, img_u8, pos_id, in_size, out_size, palette=None, mean=None, std=None, view=None, out_view=None, out=None, surface=None, out_surface=None):
        """forward_labels_u8() with the colour map [N, oh, ow, 3] uint8 in place of the label map: bytes in, picture out (out_view: see _dst_out)."""
        view = self._one_of(view, surface, "view", "surface")
        out_view = self._one_of(out_view, out_surface, "out_view", "out_surface")
        oh, ow = self._rgb_size(out_size)
        if out_view is not None and torch.is_tensor(img_u8) and img_u8.dim() >= 1:
            self._dst_check(out_view, out, (oh, ow), img_u8.shape[0])
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        out = self._dst_out(out_view, out, (oh, ow), img.shape[0], img.device) if out_view is not None else self._rgb_out(img.shape[0], out_size, img.device)
        pal = self._palette(palette)

        def one(i, eng, s):
            eng.set_output_rgb(oh, ow, pal)
            self._set_out(eng, out_view)
            eng.forward_u8_rgb(img[i].data_ptr(), pos_id, out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out

    def labels_rgb(self, labels_u8, out_size, palette=None, out_view=None, out=None, out_surface=None):
        """uint8 labels [N, H, W] (CUDA) of this model -> their colour maps [N, oh, ow, 3] (out_view: see _dst_out)."""
        out_view = self._one_of(out_view, out_surface, "out_view", "out_surface")
        if self._engine is None:
            raise RuntimeError("labels_rgb(): no handle yet")
        if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3 or tuple(labels_u8.shape[1:]) != tuple(self._engine_key[:2]):
            raise RuntimeError("labels_rgb(): expected uint8 labels [N, %d, %d]" % tuple(self._engine_key[:2]))
        labels = labels_u8.contiguous()
        oh, ow = self._rgb_size(out_size)
        out = self._dst_out(out_view, out, (oh, ow), labels.shape[0], labels.device) if out_view is not None else self._rgb_out(labels.shape[0], out_size, labels.device)
        self._engine.set_output_rgb(oh, ow, self._palette(palette))
        self._set_out(self._engine, out_view)
        s = torch.cuda.current_stream(labels.device).cuda_stream
        for i in range(labels.shape[0]):
            self._engine.labels_rgb(labels[i].data_ptr(), out[i].data_ptr(), s)
        return out

    # ---- overlay out (not in the reference; include/tdnet.h "overlay out") ---------------------------------------------------------------
    # The frame's last kernel blends the class colours over the SOURCE bytes, at the source's size: uint8 [N, Hs, Ws, 3].  palette: [n, 3] byte
    # values (None = cityscapesLoader.label_colours) with `alpha` in 0..1 -- a scalar or one per class -- giving the opacity byte rint(255 alpha);
    # or [n, 4] bytes r, g, b, a taken as they are (alpha is then ignored).  a = 0 leaves the frame, a = 255 replaces it; labels >= n show the frame.
    @classmethod
    def _palette_rgba(cls, palette, alpha):
        if palette is not None:
            p = np.asarray(palette)
            if p.ndim != 2 or p.shape[1] not in (3, 4) or not 1 <= p.shape[0] <= 256:
                raise RuntimeError("palette must be [n, 3] colours or [n, 4] bytes r, g, b, a with n in 1..256, got shape %s" % (p.shape,))
            if p.shape[1] == 4:
                return np.ascontiguousarray(p.astype(np.uint8))
        pal = cls._palette(palette)
        a = np.asarray(alpha, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != pal.shape[0]) or not np.isfinite(a).all() or (a < 0).any() or (a > 1).any():
            raise RuntimeError("alpha must be a number in 0..1 or one per palette row (%d), got %r" % (pal.shape[0], alpha))
        out = np.empty((pal.shape[0], 4), np.uint8)
        out[:, :3] = pal
        out[:, 3] = np.rint(255.0 * a).astype(np.uint8)
        return out

    def forward_overlay_u8(self, img_u8, pos_id, in_size, palette=None, alpha=0.5, mean=None, std=None, view=None, out_view=None, out=None, surface=None, out_surface=None):
        """forward_labels_u8() with the overlay [N, Hs, Ws, 3] uint8 in place of the label map: the frame's bytes in, the tinted frame out
        (out_view: see _dst_out)."""
        view = self._one_of(view, surface, "view", "surface")
        out_view = self._one_of(out_view, out_surface, "out_view", "out_surface")
        pal = self._palette_rgba(palette, alpha)
        if view is not None:
            self._check_frame_view(img_u8, view)
        if out_view is not None and torch.is_tensor(img_u8) and (view is not None or img_u8.dim() == 4):
            self._dst_check(out_view, out, tuple(view.size) if view is not None else tuple(img_u8.shape[1:3]), img_u8.shape[0])
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        if out_view is not None:
            out = self._dst_out(out_view, out, tuple(view.size) if view is not None else (int(img.shape[1]), int(img.shape[2])), img.shape[0], img.device)
        else:
            out = torch.empty(tuple(img.shape) if view is None else (img.shape[0],) + tuple(view.size) + (3,), device=img.device, dtype=torch.uint8)   # a view: [N, h, w, 3] in the source's colour order

        def one(i, eng, s):
            eng.set_output_overlay(pal)
            self._set_out(eng, out_view)
            eng.forward_u8_overlay(img[i].data_ptr(), pos_id, out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out

    def forward_overlay_nv12(self, surf, pos_id, src_size, in_size, palette=None, alpha=0.5, uv_offset=None, standard=0, mean=None, std=None):
        """forward_labels_nv12() with the overlay [N, Hs, Ws, 3] uint8 RGB in place of the label map: a decoder surface in, the tinted frame out."""
        pal = self._palette_rgba(palette, alpha)
        (H, W), nv = self._check_frame_nv12(surf, pos_id, src_size, in_size, uv_offset, standard)
        img = surf.contiguous()
        out = torch.empty((img.shape[0], nv[0], nv[1], 3), device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_output_overlay(pal)
            eng.set_output_view(None)
            eng.forward_u8_overlay(img[i].data_ptr(), pos_id, out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, nv)
        return out

    def _overlay_source(self, who, src, n, src_size, uv_offset, standard):
        """The source of an unfused / split overlay -> (contiguous tensor, (Hs, Ws), nv12 arguments or None): uint8 [N, Hs, Ws, 3] packed RGB, or
        with src_size=(Hs, Ws) NV12 surfaces [N, rows, pitch]."""
        if not torch.is_tensor(src) or src.dtype != torch.uint8:
            raise RuntimeError("%s: expected the source frames as a torch.uint8 tensor, got %s" % (who, src.dtype if torch.is_tensor(src) else type(src).__name__))
        if src_size is None:
            if src.dim() != 4 or src.shape[3] != 3 or src.shape[0] != n or src.shape[1] < 1 or src.shape[2] < 1:
                raise RuntimeError("%s: expected uint8 source frames [%d, Hs, Ws, 3], got shape %s" % (who, n, tuple(src.shape)))
            return src.contiguous(), (int(src.shape[1]), int(src.shape[2])), None
        _, nv = self._check_frame_nv12(src, 0, src_size, self._engine_key[:2], uv_offset, standard)
        if src.shape[0] != n:
            raise RuntimeError("%s: expected %d surfaces, got %d" % (who, n, src.shape[0]))
        return src.contiguous(), (nv[0], nv[1]), nv

    def labels_overlay(self, labels_u8, src, palette=None, alpha=0.5, src_size=None, uv_offset=None, standard=0, mean=None, std=None, view=None,
                       out_view=None, out=None, surface=None, out_surface=None):
        """uint8 labels [N, H, W] (CUDA) of this model blended over their source frames -> [N, Hs, Ws, 3]; src: uint8 [N, Hs, Ws, 3], or with
        src_size=(Hs, Ws) NV12 surfaces [N, rows, pitch].  After forward_labels_conf_u8 with a reject_label outside the palette: the overlay over
        the accepted pixels only (out_view: see _dst_out)."""
        view = self._one_of(view, surface, "view", "surface")
        out_view = self._one_of(out_view, out_surface, "out_view", "out_surface")
        if self._engine is None:
            raise RuntimeError("labels_overlay(): no handle yet")
        if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3 or tuple(labels_u8.shape[1:]) != tuple(self._engine_key[:2]):
            raise RuntimeError("labels_overlay(): expected uint8 labels [N, %d, %d]" % tuple(self._engine_key[:2]))
        labels = labels_u8.contiguous()
        if view is not None:                                           # src: whole frames [N, nbytes] read through the view; the overlay of its rectangle
            self._check_frame_view(src, view)
            if src.shape[0] != labels.shape[0]:
                raise RuntimeError("labels_overlay(): expected %d frames, got %d" % (labels.shape[0], src.shape[0]))
            img, (Hs, Ws), nv = src, view.size, None
        else:
            img, (Hs, Ws), nv = self._overlay_source("labels_overlay()", src, labels.shape[0], src_size, uv_offset, standard)
        pal = self._palette_rgba(palette, alpha)
        if out_view is not None:
            out = self._dst_out(out_view, out, (Hs, Ws), labels.shape[0], labels.device)
        else:
            out = torch.empty((labels.shape[0], Hs, Ws, 3), device=labels.device, dtype=torch.uint8)
        eng = self._engine
        if view is not None:
            self._set_in(eng, view, mean, std)
        elif nv is None:
            eng.set_input_u8(Hs, Ws, mean, std)
        else:
            eng.set_input_nv12(*nv, mean=mean, std=std)
        eng.set_output_overlay(pal)
        self._set_out(eng, out_view)
        s = torch.cuda.current_stream(labels.device).cuda_stream
        for i in range(labels.shape[0]):
            eng.labels_overlay(labels[i].data_ptr(), img[i].data_ptr(), out[i].data_ptr(), s)
        return out

    # ---- score out (not in the reference's model; its validation loop counts on the host, Training/validate.py:59-70) -----------------------
    # The frame's last kernel adds the frame's confusion counts against gt_u8 -- uint8 [N, H, W] at the NETWORK size, CUDA -- to a matrix each
    # handle owns (a batch is N handles: confusion_matrix() sums them).  gt_map: 256 values (ground-truth byte -> class id, >= nclass = ignore),
    # None = identity.  return_labels: also return the uint8 label map [N, H, W] (the labels forward_labels_u8 gives).
    @staticmethod
    def _check_gt_type(gt):
        if not torch.is_tensor(gt) or gt.dtype != torch.uint8 or gt.dim() != 3:
            raise RuntimeError("expected the ground truth gt as a torch.uint8 tensor [N, H, W], got %s"
                               % ("%s %s" % (gt.dtype, tuple(gt.shape)) if torch.is_tensor(gt) else type(gt).__name__))

    def _check_gt(self, gt, n, H, W, device):
        self._check_gt_type(gt)
        if tuple(gt.shape) != (n, H, W):
            raise RuntimeError("expected the ground truth gt as a torch.uint8 tensor [%d, %d, %d] at the network size, got %s"
                               % (n, H, W, tuple(gt.shape)))
        if gt.device != device:
            raise RuntimeError("the ground truth gt must be on the frame's device %s, got %s" % (device, gt.device))
        return gt.contiguous()

    def forward_score(self, img, gt_u8, pos_id=0, gt_map=None, return_labels=False):
        """forward_labels() with the frame scored on the device: returns the uint8 labels [N, H, W] if return_labels, else None."""
        self._check_gt_type(gt_u8)
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        gt = self._check_gt(gt_u8, img.shape[0], img.shape[2], img.shape[3], img.device)
        out = torch.empty((img.shape[0], img.shape[2], img.shape[3]), device=img.device, dtype=torch.uint8) if return_labels else None

        def one(i, eng, s):
            eng.set_score(gt_map)
            eng.forward_score(img[i].data_ptr(), pos_id, gt[i].data_ptr(), None if out is None else out[i].data_ptr(), s)
        self._for_each_sample(img, one)
        return out

    def forward_score_u8(self, img_u8, gt_u8, pos_id=0, in_size=None, gt_map=None, return_labels=False, mean=None, std=None, view=None, surface=None):
        """forward_labels_u8() with the frame scored on the device: bytes in, counts added; the uint8 labels [N, H, W] if return_labels."""
        view = self._one_of(view, surface, "view", "surface")
        self._check_gt_type(gt_u8)
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        gt = self._check_gt(gt_u8, img.shape[0], H, W, img.device)
        out = torch.empty((img.shape[0], H, W), device=img.device, dtype=torch.uint8) if return_labels else None

        def one(i, eng, s):
            eng.set_score(gt_map)
            eng.forward_u8_score(img[i].data_ptr(), pos_id, gt[i].data_ptr(), None if out is None else out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out

    def score_labels(self, labels_u8, gt_u8, gt_map=None):
        """The unfused form: uint8 labels [N, H, W] (CUDA) of this model counted against gt_u8, sample i on handle i."""
        if self._engine is None:
            raise RuntimeError("score_labels(): no handle yet")
        H, W = self._engine_key[:2]
        if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3 or tuple(labels_u8.shape[1:]) != (H, W):
            raise RuntimeError("score_labels(): expected uint8 labels [N, %d, %d]" % (H, W))
        labels = labels_u8.contiguous()
        gt = self._check_gt(gt_u8, labels.shape[0], H, W, labels.device)
        engines = [self._engine] + list(self._extra_engines)
        if labels.shape[0] > len(engines):
            raise RuntimeError("score_labels(): %d label maps but %d handle(s)" % (labels.shape[0], len(engines)))
        s = torch.cuda.current_stream(labels.device).cuda_stream
        for i in range(labels.shape[0]):
            engines[i].set_score(gt_map)
            engines[i].labels_score(labels[i].data_ptr(), gt[i].data_ptr(), s)

    def _score_engines(self, who):
        if self._engine is None:
            raise RuntimeError("%s(): no handle yet" % who)
        return [e for e in [self._engine] + list(self._extra_engines) if getattr(e, "_score_key", None) is not None]

    def confusion_matrix(self):
        """int64 numpy [nclass, nclass]: the counts of every frame scored since the last reset_score(), summed over the batch's handles
        (synchronises the current stream)."""
        total = np.zeros((self.nclass, self.nclass), np.int64)
        for e in self._score_engines("confusion_matrix"):
            total += e.score_read(torch.cuda.current_stream(self._engine_key[2]).cuda_stream).astype(np.int64)
        return total

    def get_scores(self):
        """The reference's runningScore.get_scores() of confusion_matrix(): ({overall / mean / frequency-weighted accuracy, mean IoU}, {class: IoU})."""
        from ..metrics import runningScore
        rs = runningScore(self.nclass)
        rs.add_counts(self.confusion_matrix())
        return rs.get_scores()

    def reset_score(self):
        """Zero the matrices (enqueued on the current stream)."""
        for e in self._score_engines("reset_score"):
            e.score_reset(torch.cuda.current_stream(self._engine_key[2]).cuda_stream)

    # ---- confidence out (not in the reference's model; a caller of the reference runs softmax over the full-resolution logits itself) -------
    # The frame's last kernel also writes, per pixel, the softmax probability of the label as a byte (255 = certain; include/tdnet.h
    # "confidence out"), and writes reject_label in place of a label whose byte is below the threshold.
    _confidence = (0, 255)

    def set_confidence(self, threshold=0.0, reject_label=255):
        """Labels with a softmax probability below `threshold` (0..1) come out as reject_label (0..255) from the *_conf methods.  The comparison is
        made on the confidence BYTE: min_conf = ceil(255 threshold) clamped to 0..255 (a threshold that is k / 255 up to the rounding of the
        division gives k); 0 rejects nothing.  Applies to every handle of a batch, the ones created later included."""
        import math
        min_conf = min(255, max(0, int(math.ceil(255.0 * float(threshold) - 1e-9))))
        if int(reject_label) != reject_label or not 0 <= int(reject_label) <= 255:
            raise RuntimeError("set_confidence(): reject_label must be an integer in 0..255, got %r" % (reject_label,))
        self._confidence = (min_conf, int(reject_label))
        return self._confidence

    def forward_labels_conf(self, img, pos_id=0):
        """forward_labels() with the confidence map: (labels uint8 [N, H, W], conf uint8 [N, H, W])."""
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        shape = (img.shape[0], img.shape[2], img.shape[3])
        out, conf = torch.empty(shape, device=img.device, dtype=torch.uint8), torch.empty(shape, device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_confidence(*self._confidence)
            eng.forward_labels_conf(img[i].data_ptr(), pos_id, out[i].data_ptr(), conf[i].data_ptr(), s)
        self._for_each_sample(img, one)
        return out, conf

    def forward_labels_conf_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None):
        """forward_labels_u8() with the confidence map: bytes in, (labels uint8 [N, H, W], conf uint8 [N, H, W]) out."""
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        shape = (img.shape[0], H, W)
        out, conf = torch.empty(shape, device=img.device, dtype=torch.uint8), torch.empty(shape, device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_confidence(*self._confidence)
            eng.forward_u8_labels_conf(img[i].data_ptr(), pos_id, out[i].data_ptr(), conf[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out, conf

    def logits_conf(self, logits):
        """The unfused form: logits [N, nclass, H, W] (fp32, CUDA) of this model -> (labels uint8 [N, H, W], conf uint8 [N, H, W])."""
        if self._engine is None:
            raise RuntimeError("logits_conf(): no handle yet")
        H, W = self._engine_key[:2]
        if not torch.is_tensor(logits) or logits.dim() != 4 or tuple(logits.shape[1:]) != (self.nclass, H, W):
            raise RuntimeError("logits_conf(): expected logits [N, %d, %d, %d]" % (self.nclass, H, W))
        logits = logits.contiguous().float()
        shape = (logits.shape[0], H, W)
        out, conf = torch.empty(shape, device=logits.device, dtype=torch.uint8), torch.empty(shape, device=logits.device, dtype=torch.uint8)
        s = torch.cuda.current_stream(logits.device).cuda_stream
        self._engine.set_confidence(*self._confidence)
        for i in range(logits.shape[0]):
            self._engine.logits_conf(logits[i].data_ptr(), out[i].data_ptr(), conf[i].data_ptr(), s)
        return out, conf

    # ---- matte out (not in the reference's model; a caller of the reference runs softmax, a class sum, a resize and a blend over the logits) ----
    # The frame's last kernel writes, per pixel, the softmax mass of a class set as a byte (255 = certainly one of them; include/tdnet.h
    # "matte out"), or the source frame composited by it at the source's size.
    _matte = None

    def set_matte(self, classes):
        """The class set of the *_matte / *_composite methods: an iterable of class ids below nclass (duplicates are legal, empty = the empty
        set).  Applies to every handle of a batch, the ones created later included.  Returns the sorted ids."""
        try:
            ids = [c for c in classes]
        except TypeError:
            raise RuntimeError("set_matte(): classes must be an iterable of class ids, got %r" % (classes,))
        for c in ids:
            try:
                ok = not isinstance(c, bool) and int(c) == c and 0 <= int(c) < self.nclass
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise RuntimeError("set_matte(): %r is not a class id (0..%d)" % (c, self.nclass - 1))
        self._matte = tuple(sorted(set(int(c) for c in ids)))
        return self._matte

    def _need_matte(self, who):
        if self._matte is None:
            raise RuntimeError("%s(): no class set (call set_matte(classes) first)" % who)
        return self._matte

    def forward_matte(self, img, pos_id=0):
        """forward_labels() with the matte: (labels uint8 [N, H, W], matte uint8 [N, H, W])."""
        ids = self._need_matte("forward_matte")
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        shape = (img.shape[0], img.shape[2], img.shape[3])
        out, matte = torch.empty(shape, device=img.device, dtype=torch.uint8), torch.empty(shape, device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_matte(ids)
            eng.forward_matte(img[i].data_ptr(), pos_id, out[i].data_ptr(), matte[i].data_ptr(), s)
        self._for_each_sample(img, one)
        return out, matte

    def forward_matte_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None):
        """forward_labels_u8() with the matte: bytes in, (labels uint8 [N, H, W], matte uint8 [N, H, W]) out."""
        ids = self._need_matte("forward_matte_u8")
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        shape = (img.shape[0], H, W)
        out, matte = torch.empty(shape, device=img.device, dtype=torch.uint8), torch.empty(shape, device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_matte(ids)
            eng.forward_u8_matte(img[i].data_ptr(), pos_id, out[i].data_ptr(), matte[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out, matte

    _refine = (0, 65)

    def set_matte_refine(self, radius, eps=65):
        """The refined matte (include/tdnet.h "refined matte"): radius 1..16 and eps 4..65025 (squared byte units; 65 ~ 1e-3 * 255^2) -- the composite methods
        then composite through the matte guided-filtered by the frame's luma at the frame's own size, and forward_matte_refined_u8 / propagate(matte_refined=True)
        return that matte.  radius 0: off, the default.  Host state of the model; every handle is told when it runs.  Returns (radius, eps)."""
        if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= 16:
            raise RuntimeError("set_matte_refine(): radius must be 0 (off) or in 1..16, got %r" % (radius,))
        if int(radius) and (isinstance(eps, bool) or int(eps) != eps or not 4 <= int(eps) <= 65025):
            raise RuntimeError("set_matte_refine(): eps must be in 4..65025 (squared byte units), got %r" % (eps,))
        self._refine = (int(radius), int(eps) if int(radius) else 0)
        return self._refine

    def forward_matte_refined_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None):
        """forward_labels_u8() with the refined matte in place of the label map: bytes in, uint8 [N, Hs, Ws] out -- the matte of set_matte()'s class set at the
        frame's own (a view's rectangle's) size, guided-filtered by the frame's luma with set_matte_refine()'s radius and eps."""
        ids = self._need_matte("forward_matte_refined_u8")
        if not self._refine[0]:
            raise RuntimeError("forward_matte_refined_u8(): no refinement (call set_matte_refine(radius, eps) with a radius of 1..16 first)")
        view = self._one_of(view, surface, "view", "surface")
        if view is not None:
            self._check_frame_view(img_u8, view)
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        size = tuple(view.size) if view is not None else (int(img.shape[1]), int(img.shape[2]))
        out = torch.empty((img.shape[0],) + size, device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_matte(ids)
            eng.set_matte_refine(*self._refine)
            eng.forward_u8_matte_refined(img[i].data_ptr(), pos_id, out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out

    def logits_matte(self, logits):
        """The unfused form: logits [N, nclass, H, W] (fp32, CUDA) of this model -> (labels uint8 [N, H, W], matte uint8 [N, H, W])."""
        ids = self._need_matte("logits_matte")
        if self._engine is None:
            raise RuntimeError("logits_matte(): no handle yet")
        H, W = self._engine_key[:2]
        if not torch.is_tensor(logits) or logits.dim() != 4 or tuple(logits.shape[1:]) != (self.nclass, H, W):
            raise RuntimeError("logits_matte(): expected logits [N, %d, %d, %d]" % (self.nclass, H, W))
        logits = logits.contiguous().float()
        shape = (logits.shape[0], H, W)
        out, matte = torch.empty(shape, device=logits.device, dtype=torch.uint8), torch.empty(shape, device=logits.device, dtype=torch.uint8)
        s = torch.cuda.current_stream(logits.device).cuda_stream
        self._engine.set_matte(ids)
        for i in range(logits.shape[0]):
            self._engine.logits_matte(logits[i].data_ptr(), out[i].data_ptr(), matte[i].data_ptr(), s)
        return out, matte

    def refine_matte(self, guide, matte, radius, eps=65):
        """The refined matte (include/tdnet.h "refined matte"): the guided filter of matte uint8 [N, h, w] (or [h, w]) with guide uint8 of the same shape,
        both CUDA, any size -> uint8 of that shape.  radius 1..16; eps 4..65025 in squared byte units (65 ~ 1e-3 * 255^2).  The rows of either input may
        be a strided view (stride(-1) == 1); needs no configuration, only a handle for its device.  dataloader.luma_u8 is the guide of a frame."""
        if self._engine is None:
            raise RuntimeError("refine_matte(): no handle yet")
        for name, t in (("guide", guide), ("matte", matte)):
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() not in (2, 3) or t.numel() == 0:
                raise RuntimeError("refine_matte(): %s must be a non-empty uint8 CUDA tensor [N, h, w] or [h, w]" % name)
        if guide.shape != matte.shape:
            raise RuntimeError("refine_matte(): guide %s and matte %s differ in shape" % (tuple(guide.shape), tuple(matte.shape)))
        g3, m3 = (guide, matte) if guide.dim() == 3 else (guide[None], matte[None])
        rows = lambda t: t if t.stride(-1) == 1 and t.stride(-2) >= t.shape[-1] else t.contiguous()
        g3, m3 = rows(g3), rows(m3)
        n, h, w = g3.shape
        out = torch.empty((n, h, w), device=g3.device, dtype=torch.uint8)
        scratch = torch.empty(((self._engine.refine_scratch_bytes(h, w) + 3) // 4,), device=g3.device, dtype=torch.int32)
        s = torch.cuda.current_stream(g3.device).cuda_stream
        for i in range(n):
            self._engine.refine_matte(g3[i].data_ptr(), g3.stride(1), m3[i].data_ptr(), m3.stride(1), out[i].data_ptr(), w, h, w, radius, eps, scratch.data_ptr(), s)
        return out if guide.dim() == 3 else out[0]

    # ---- regions out (not in the reference's model; a caller of the reference downloads the labels and runs a connected-components pass on the host) ----
    # The connected components of a class set of the frame's labels, numbered by their first pixel, with area, box and coordinate sums (include/tdnet.h
    # "regions out").  Every method returns (labels uint8 [N, H, W], ids int32 [N, H, W] or None, [dataloader.RegionTable per sample]); reading the tables
    # synchronises with the device.
    _regions = None

    def set_regions(self, classes, connectivity=8, max_regions=256, min_area=1):
        """The configuration of the *_regions methods: an iterable of class ids below nclass (duplicates are legal, empty = no region at all), 4 or 8
        neighbours, the number of records of the table (1..65536; more regions than that are still counted and numbered in the id map) and the area below
        which a region is dropped.  Host state of the model; every handle is told when it runs."""
        try:
            ids = list(classes)
        except TypeError:
            raise RuntimeError("set_regions(): classes must be an iterable of class ids, got %r" % (classes,))
        for c in ids:
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < self.nclass:
                raise RuntimeError("set_regions(): %r is not a class id (0..%d)" % (c, self.nclass - 1))
        if connectivity not in (4, 8):
            raise RuntimeError("set_regions(): connectivity must be 4 or 8, got %r" % (connectivity,))
        if not 1 <= int(max_regions) <= 65536 or int(min_area) < 1:
            raise RuntimeError("set_regions(): max_regions must be in 1..65536 and min_area at least 1, got %r and %r" % (max_regions, min_area))
        self._regions = (tuple(sorted(set(int(c) for c in ids))), int(connectivity), int(max_regions), int(min_area))
        return self._regions

    def _need_regions(self, who):
        if self._regions is None:
            raise RuntimeError("%s(): no configuration (call set_regions(classes) first)" % who)
        return self._regions

    def _regions_out(self, n, H, W, device, return_ids):
        max_regions = self._regions[2]
        out = torch.empty((n, H, W), device=device, dtype=torch.uint8)
        ids = torch.empty((n, H, W), device=device, dtype=torch.int32) if return_ids else None
        table = torch.empty((n, 2 + 6 * max_regions), device=device, dtype=torch.int64)   # 16 + 48 * max_regions bytes per sample, 8-byte aligned
        return out, ids, table

    def _regions_tables(self, table):
        from ..dataloader import region_table
        host = table.cpu().numpy()
        return [region_table(host[i], self._regions[2]) for i in range(host.shape[0])]

    def forward_regions(self, img, pos_id=0, return_ids=True):
        """forward_labels() with the regions of set_regions()'s class set behind the labels."""
        cfg = self._need_regions("forward_regions")
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        out, ids, table = self._regions_out(img.shape[0], img.shape[2], img.shape[3], img.device, return_ids)

        def one(i, eng, s):
            eng.set_regions(*cfg)
            eng.forward_regions(img[i].data_ptr(), pos_id, out[i].data_ptr(), None if ids is None else ids[i].data_ptr(), table[i].data_ptr(), s)
        self._for_each_sample(img, one)
        return out, ids, self._regions_tables(table)

    def forward_regions_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None, return_ids=True):
        """forward_labels_u8() with the regions behind the labels: bytes in (any byte-input configuration: view= / surface= as there)."""
        cfg = self._need_regions("forward_regions_u8")
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        out, ids, table = self._regions_out(img.shape[0], H, W, img.device, return_ids)

        def one(i, eng, s):
            eng.set_regions(*cfg)
            eng.forward_u8_regions(img[i].data_ptr(), pos_id, out[i].data_ptr(), None if ids is None else ids[i].data_ptr(), table[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out, ids, self._regions_tables(table)

    def regions_labels(self, labels_u8, return_ids=True):
        """The unfused form: uint8 labels [N, H, W] (CUDA) of this model's size -- the label entries', or the confidence entries' with rejected pixels,
        which are background -- sample i on handle i.  Returns the labels as given."""
        cfg = self._need_regions("regions_labels")
        if self._engine is None:
            raise RuntimeError("regions_labels(): no handle yet")
        H, W = self._engine_key[:2]
        if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3 or tuple(labels_u8.shape[1:]) != (H, W):
            raise RuntimeError("regions_labels(): expected uint8 labels [N, %d, %d]" % (H, W))
        labels = labels_u8.contiguous()
        engines = [self._engine] + list(self._extra_engines)
        if labels.shape[0] > len(engines):
            raise RuntimeError("regions_labels(): %d label maps but %d handle(s)" % (labels.shape[0], len(engines)))
        _, ids, table = self._regions_out(labels.shape[0], H, W, labels.device, return_ids)
        s = torch.cuda.current_stream(labels.device).cuda_stream
        for i in range(labels.shape[0]):
            engines[i].set_regions(*cfg)
            engines[i].labels_regions(labels[i].data_ptr(), None if ids is None else ids[i].data_ptr(), table[i].data_ptr(), s)
        return labels, ids, self._regions_tables(table)

    def propagate_regions(self, return_ids=True):
        """propagate() with the regions behind the labels, for the frame encode() / encode_u8() left pending."""
        cfg = self._need_regions("propagate_regions")
        if self._engine is None or self._pending_shape is None:
            raise RuntimeError("propagate_regions(): no encoded frame is pending (call encode(img, pos_id) first)")
        H, W, dev = self._pending_shape
        out, ids, table = self._regions_out(1, H, W, dev, return_ids)
        self._engine.set_regions(*cfg)
        self._pending_shape = None
        self._engine.propagate_regions(out.data_ptr(), None if ids is None else ids.data_ptr(), table.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return out, ids, self._regions_tables(table)

    # ---- tracks out (not in the reference's model; a caller of the reference downloads two id maps per frame and counts their overlaps on the host) ----
    # The regions methods plus region identity across frames (include/tdnet.h "tracks out"): every method returns what its regions method returns plus
    # (track map int32 [N, H, W] or None, [dataloader.TrackTable per sample]).  The track state lives on the device, per handle (sample i of a batch is a
    # stream of its own); it remembers ONE frame, and only the tracked methods advance it.
    _tracks = None

    def set_tracks(self, min_overlap=1):
        """The configuration of the *_tracks methods: a region continues a track only if the two overlap in at least min_overlap pixels."""
        if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, np.integer)) or int(min_overlap) < 1:
            raise RuntimeError("set_tracks(): min_overlap must be an integer >= 1, got %r" % (min_overlap,))
        self._tracks = int(min_overlap)
        return self._tracks

    def _need_tracks(self, who):
        cfg = self._need_regions(who)
        if self._tracks is None:
            raise RuntimeError("%s(): no configuration (call set_tracks() first)" % who)
        return cfg

    def _tracks_out(self, n, H, W, device, return_track_ids):
        tmap = torch.empty((n, H, W), device=device, dtype=torch.int32) if return_track_ids else None
        return tmap, torch.empty((n, 2 + 3 * self._regions[2]), device=device, dtype=torch.int64)   # 16 + 24 * max_regions bytes per sample, 8-byte aligned

    def _tracks_tables(self, table):
        from ..dataloader import track_table
        host = table.cpu().numpy()
        return [track_table(host[i], self._regions[2]) for i in range(host.shape[0])]

    def _tracks_config(self, eng, cfg):
        eng.set_regions(*cfg)
        eng.set_tracks(self._tracks)

    def forward_tracks(self, img, pos_id=0, return_ids=True, return_track_ids=True):
        """forward_regions() with the tracks behind the regions."""
        cfg = self._need_tracks("forward_tracks")
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        out, ids, table = self._regions_out(img.shape[0], img.shape[2], img.shape[3], img.device, return_ids)
        tmap, ttable = self._tracks_out(img.shape[0], img.shape[2], img.shape[3], img.device, return_track_ids)

        def one(i, eng, s):
            self._tracks_config(eng, cfg)
            eng.forward_tracks(img[i].data_ptr(), pos_id, out[i].data_ptr(), None if ids is None else ids[i].data_ptr(), table[i].data_ptr(),
                               None if tmap is None else tmap[i].data_ptr(), ttable[i].data_ptr(), s)
        self._for_each_sample(img, one)
        return out, ids, self._regions_tables(table), tmap, self._tracks_tables(ttable)

    def forward_tracks_u8(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None, return_ids=True, return_track_ids=True):
        """forward_regions_u8() with the tracks behind the regions: bytes in (any byte-input configuration: view= / surface= as there)."""
        cfg = self._need_tracks("forward_tracks_u8")
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        out, ids, table = self._regions_out(img.shape[0], H, W, img.device, return_ids)
        tmap, ttable = self._tracks_out(img.shape[0], H, W, img.device, return_track_ids)

        def one(i, eng, s):
            self._tracks_config(eng, cfg)
            eng.forward_u8_tracks(img[i].data_ptr(), pos_id, out[i].data_ptr(), None if ids is None else ids[i].data_ptr(), table[i].data_ptr(),
                                  None if tmap is None else tmap[i].data_ptr(), ttable[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out, ids, self._regions_tables(table), tmap, self._tracks_tables(ttable)

    def labels_tracks(self, labels_u8, return_ids=True, return_track_ids=True):
        """The unfused form: uint8 labels [N, H, W] (CUDA) of this model's size, sample i on handle i (and on handle i's tracks).  Returns the labels as given."""
        cfg = self._need_tracks("labels_tracks")
        if self._engine is None:
            raise RuntimeError("labels_tracks(): no handle yet")
        H, W = self._engine_key[:2]
        if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3 or tuple(labels_u8.shape[1:]) != (H, W):
            raise RuntimeError("labels_tracks(): expected uint8 labels [N, %d, %d]" % (H, W))
        labels = labels_u8.contiguous()
        engines = [self._engine] + list(self._extra_engines)
        if labels.shape[0] > len(engines):
            raise RuntimeError("labels_tracks(): %d label maps but %d handle(s)" % (labels.shape[0], len(engines)))
        _, ids, table = self._regions_out(labels.shape[0], H, W, labels.device, return_ids)
        tmap, ttable = self._tracks_out(labels.shape[0], H, W, labels.device, return_track_ids)
        s = torch.cuda.current_stream(labels.device).cuda_stream
        for i in range(labels.shape[0]):
            self._tracks_config(engines[i], cfg)
            engines[i].labels_tracks(labels[i].data_ptr(), None if ids is None else ids[i].data_ptr(), table[i].data_ptr(),
                                     None if tmap is None else tmap[i].data_ptr(), ttable[i].data_ptr(), s)
        return labels, ids, self._regions_tables(table), tmap, self._tracks_tables(ttable)

    def propagate_tracks(self, return_ids=True, return_track_ids=True):
        """propagate_regions() with the tracks behind the regions, for the frame encode() / encode_u8() left pending."""
        cfg = self._need_tracks("propagate_tracks")
        if self._engine is None or self._pending_shape is None:
            raise RuntimeError("propagate_tracks(): no encoded frame is pending (call encode(img, pos_id) first)")
        H, W, dev = self._pending_shape
        out, ids, table = self._regions_out(1, H, W, dev, return_ids)
        tmap, ttable = self._tracks_out(1, H, W, dev, return_track_ids)
        self._tracks_config(self._engine, cfg)
        self._pending_shape = None
        self._engine.propagate_tracks(out.data_ptr(), None if ids is None else ids.data_ptr(), table.data_ptr(), None if tmap is None else tmap.data_ptr(),
                                      ttable.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return out, ids, self._regions_tables(table), tmap, self._tracks_tables(ttable)

    def reset_tracks(self):
        """Forget every track on every handle that has tracks (enqueued on the current stream): the next tracked frame's regions are all born, from id 1."""
        if self._engine is None or self._tracks is None:
            return
        for eng in [self._engine] + list(self._extra_engines):
            eng.set_tracks(self._tracks)                               # idempotent; a handle that never ran a tracked frame gets its (zeroed) state here
            eng.tracks_reset(torch.cuda.current_stream().cuda_stream)

    # ---- runs out (not in the reference's model; a caller of the reference downloads the map itself) ----
    # A label map or an id / track map as a run-length table (include/tdnet.h "runs out").  The coding methods return (..., table int64 [N, 2 + max_runs + 1]
    # on the device, [(header, records[:stored + 1]) per sample]); reading the records synchronises with the device and copies the header and the stored
    # prefix only.  dataloader.RunsDownloader takes table[i] for a loop that must not wait.
    _runs = None

    def set_runs(self, max_runs=None):
        """The configuration of the *_runs methods: the number of runs a table holds (1 .. H W; None: H W, every map fits).  Host state of the model; every
        handle is told when it runs."""
        if max_runs is not None and (isinstance(max_runs, bool) or not isinstance(max_runs, (int, np.integer)) or int(max_runs) < 1):
            raise RuntimeError("set_runs(): max_runs must be an integer >= 1 or None, got %r" % (max_runs,))
        self._runs = (None if max_runs is None else int(max_runs),)
        return self._runs

    def _need_runs(self, who, H, W):
        if self._runs is None:
            raise RuntimeError("%s(): no configuration (call set_runs() first)" % who)
        max_runs = H * W if self._runs[0] is None else self._runs[0]
        if max_runs > H * W:
            raise RuntimeError("%s(): max_runs = %d is more than the %d pixels of a %d x %d map" % (who, max_runs, H * W, H, W))
        return max_runs

    @staticmethod
    def _runs_tables(table):
        from ..dataloader import RUN_DTYPE, RUNS_HEADER_DTYPE
        out = []
        for i in range(table.shape[0]):
            hdr = table[i, :2].cpu().numpy().view(RUNS_HEADER_DTYPE)[0]
            out.append((hdr, table[i, 2:2 + int(hdr["stored"]) + 1].cpu().numpy().view(RUN_DTYPE)))
        return out

    def forward_runs(self, img, pos_id=0):
        """forward_labels() with the run-length table of the labels behind them: (labels uint8 [N, H, W], table, [(header, records)])."""
        self._check_frame(img, pos_id)
        img = img.contiguous().float()
        n, H, W = img.shape[0], img.shape[2], img.shape[3]
        max_runs = self._need_runs("forward_runs", H, W)
        out = torch.empty((n, H, W), device=img.device, dtype=torch.uint8)
        table = torch.empty((n, 2 + max_runs + 1), device=img.device, dtype=torch.int64)

        def one(i, eng, s):
            eng.set_runs(max_runs)
            eng.forward_runs(img[i].data_ptr(), pos_id, out[i].data_ptr(), table[i].data_ptr(), s)
        self._for_each_sample(img, one)
        return out, table, self._runs_tables(table)

    def forward_u8_runs(self, img_u8, pos_id=0, in_size=None, mean=None, std=None, view=None, surface=None):
        """forward_labels_u8() with the run-length table behind the labels: bytes in (any byte-input configuration: view= / surface= as there)."""
        view = self._one_of(view, surface, "view", "surface")
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        max_runs = self._need_runs("forward_u8_runs", H, W)
        img = img_u8.contiguous()
        out = torch.empty((img.shape[0], H, W), device=img.device, dtype=torch.uint8)
        table = torch.empty((img.shape[0], 2 + max_runs + 1), device=img.device, dtype=torch.int64)

        def one(i, eng, s):
            eng.set_runs(max_runs)
            eng.forward_u8_runs(img[i].data_ptr(), pos_id, out[i].data_ptr(), table[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out, table, self._runs_tables(table)

    def propagate_runs(self):
        """propagate() with the run-length table behind the labels, for the frame encode() / encode_u8() left pending."""
        if self._engine is None or self._pending_shape is None:
            raise RuntimeError("propagate_runs(): no encoded frame is pending (call encode(img, pos_id) first)")
        H, W, dev = self._pending_shape
        max_runs = self._need_runs("propagate_runs", H, W)
        out = torch.empty((1, H, W), device=dev, dtype=torch.uint8)
        table = torch.empty((1, 2 + max_runs + 1), device=dev, dtype=torch.int64)
        self._engine.set_runs(max_runs)
        self._pending_shape = None
        self._engine.propagate_runs(out.data_ptr(), table.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return out, table, self._runs_tables(table)

    def _runs_maps(self, who, maps, dtype):
        if self._engine is None:
            raise RuntimeError("%s(): no handle yet" % who)
        H, W = self._engine_key[:2]
        if not torch.is_tensor(maps) or maps.dtype != dtype or maps.dim() != 3 or tuple(maps.shape[1:]) != (H, W) or not maps.is_cuda:
            raise RuntimeError("%s(): expected %s maps [N, %d, %d] on the device" % (who, str(dtype).replace("torch.", ""), H, W))
        engines = [self._engine] + list(self._extra_engines)
        if maps.shape[0] > len(engines):
            raise RuntimeError("%s(): %d maps but %d handle(s)" % (who, maps.shape[0], len(engines)))
        return H, W, engines

    def _runs_code(self, who, maps, dtype):
        H, W, engines = self._runs_maps(who, maps, dtype)
        max_runs = self._need_runs(who, H, W)
        maps = maps.contiguous()
        table = torch.empty((maps.shape[0], 2 + max_runs + 1), device=maps.device, dtype=torch.int64)
        s = torch.cuda.current_stream(maps.device).cuda_stream
        for i in range(maps.shape[0]):
            engines[i].set_runs(max_runs)
            (engines[i].labels_runs if dtype == torch.uint8 else engines[i].ids_runs)(maps[i].data_ptr(), table[i].data_ptr(), s)
        return table, self._runs_tables(table)

    def labels_runs(self, labels_u8):
        """The unfused form: uint8 maps [N, H, W] (CUDA) of this model's size, sample i on handle i.  Returns (table, [(header, records)])."""
        return self._runs_code("labels_runs", labels_u8, torch.uint8)

    def ids_runs(self, ids_i32):
        """The unfused form on int32 maps [N, H, W] (CUDA): the id maps or track maps of the regions / tracks methods, or any int32 values."""
        return self._runs_code("ids_runs", ids_i32, torch.int32)

    def _runs_decode(self, who, table, fill, dtype):
        if self._engine is None:
            raise RuntimeError("%s(): no handle yet" % who)
        H, W = self._engine_key[:2]
        max_runs = self._need_runs(who, H, W)
        if not torch.is_tensor(table) or table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 2 + max_runs + 1 or not table.is_cuda:
            raise RuntimeError("%s(): expected int64 tables [N, %d] on the device (max_runs = %d)" % (who, 2 + max_runs + 1, max_runs))
        engines = [self._engine] + list(self._extra_engines)
        if table.shape[0] > len(engines):
            raise RuntimeError("%s(): %d tables but %d handle(s)" % (who, table.shape[0], len(engines)))
        table = table.contiguous()
        out = torch.empty((table.shape[0], H, W), device=table.device, dtype=dtype)
        s = torch.cuda.current_stream(table.device).cuda_stream
        for i in range(table.shape[0]):
            engines[i].set_runs(max_runs)
            (engines[i].runs_labels if dtype == torch.uint8 else engines[i].runs_ids)(table[i].data_ptr(), int(fill), out[i].data_ptr(), s)
        return out

    def runs_labels(self, table, fill=0):
        """Tables back into uint8 maps [N, H, W] on the device; pixels a table does not cover (an overflowed one) get `fill`."""
        return self._runs_decode("runs_labels", table, fill, torch.uint8)

    def runs_ids(self, table, fill=0):
        """Tables back into int32 maps [N, H, W] on the device; pixels a table does not cover get `fill`."""
        return self._runs_decode("runs_ids", table, fill, torch.int32)

    @staticmethod
    def _background(background):
        if background is None:
            return None
        try:
            bg = tuple(int(v) for v in background)
        except (TypeError, ValueError):
            bg = ()
        if len(bg) != 3 or any(v < 0 or v > 255 for v in bg) or any(int(v) != v for v in background):
            raise RuntimeError("background must be three byte values (r, g, b) or None (the alpha mode), got %r" % (background,))
        return bg

    def forward_composite_u8(self, img_u8, pos_id, in_size, background=(0, 0, 0), mean=None, std=None, view=None, out_view=None, out=None, surface=None):
        """forward_labels_u8() with the composite in place of the label map: the frame's bytes in, the frame through the matte of set_matte()'s
        class set out -- blended over background (r, g, b) -> uint8 [N, Hs, Ws, 3] (out_view: see _dst_out), or with background=None the source's
        colour bytes and the matte as the x byte of a 32-bit out_view (required then)."""
        ids = self._need_matte("forward_composite_u8")
        bg = self._background(background)
        view = self._one_of(view, surface, "view", "surface")
        if bg is None and (out_view is None or getattr(out_view, "bpp", 0) != 4):
            raise RuntimeError("forward_composite_u8(background=None): the alpha mode needs a 32-bit out_view (RGBA32 / BGRA32)")
        if out_view is not None and getattr(out_view, "nv12", True):
            raise RuntimeError("forward_composite_u8(): composite into 4:2:0 is not built; out_view must be a packed dataloader.SourceView")
        if view is not None:
            self._check_frame_view(img_u8, view)
        if out_view is not None and torch.is_tensor(img_u8) and (view is not None or img_u8.dim() == 4):
            self._dst_check(out_view, out, tuple(view.size) if view is not None else tuple(img_u8.shape[1:3]), img_u8.shape[0])
        H, W = self._check_frame_u8(img_u8, pos_id, in_size, view)
        img = img_u8.contiguous()
        if out_view is not None:
            out = self._dst_out(out_view, out, tuple(view.size) if view is not None else (int(img.shape[1]), int(img.shape[2])), img.shape[0], img.device)
        else:
            out = torch.empty(tuple(img.shape) if view is None else (img.shape[0],) + tuple(view.size) + (3,), device=img.device, dtype=torch.uint8)

        def one(i, eng, s):
            eng.set_matte(ids)
            eng.set_output_composite(bg)
            eng.set_matte_refine(*self._refine)
            self._set_out(eng, out_view)
            eng.forward_u8_composite(img[i].data_ptr(), pos_id, out[i].data_ptr(), s)
        self._u8_call(img, (H, W), one, mean, std, view=view)
        return out

    # ---- split frame + cache transport (path-parallel single stream: parallel.PathParallelStream) ------------------
    def encode(self, img, pos_id=0):
        """First half of forward(): backbone + pyramid slice + Encoding; the frame's cache entry is left pending."""
        self._check_frame(img, pos_id)
        if img.shape[0] != 1:
            raise RuntimeError("encode(): the split frame serves ONE stream (batch size 1)")
        img = img.contiguous().float()
        eng = self._get_engine(img)
        self._pending_shape = (img.shape[2], img.shape[3], img.device)
        eng.encode(img.data_ptr(), pos_id, torch.cuda.current_stream(img.device).cuda_stream)

    def propagate(self, labels=False, out_size=None, palette=None, gt=None, gt_map=None, conf=False, src=None, alpha=0.5, src_size=None,
                  uv_offset=None, standard=0, matte=False, composite=False, background=(0, 0, 0), matte_refined=False):
        """Second half of forward() for the pending frame, against the FIFO as it stands; returns logits, int32 labels (labels=True),
        uint8 labels (labels="u8"), the colour map [1, oh, ow, 3] (labels="rgb", with out_size=(oh, ow) and a palette as forward_rgb) or, with
        labels="score" and gt=uint8 [1, H, W], the uint8 labels of a frame whose counts were added to the handle's matrix (forward_score).
        conf=True: (uint8 labels, uint8 confidence), both [1, H, W], as forward_labels_conf gives them (labels must be left False, True or "u8").
        labels="overlay" with src = the frame that was encoded (uint8 [1, Hs, Ws, 3], or with src_size=(Hs, Ws) the NV12 surface [1, rows, pitch]):
        the overlay [1, Hs, Ws, 3] as forward_overlay_u8 / forward_overlay_nv12 give it (palette, alpha as there); the source is passed again
        because the library does not remember pointers across calls.
        matte=True: (uint8 labels, uint8 matte), both [1, H, W], as forward_matte gives them.  composite=True with src = the packed RGB frame that
        was encoded (uint8 [1, Hs, Ws, 3]): the composite [1, Hs, Ws, 3] over `background` as forward_composite_u8 gives it -- into the contiguous block: like
        every picture method called without out_view it sets the handle's destination view to none (the model classes name the destination per call; a
        view set on the engine by hand does not survive it).  matte_refined=True with the same src: the refined matte [1, Hs, Ws] as
        forward_matte_refined_u8 gives it."""
        if self._engine is None or self._pending_shape is None:
            raise RuntimeError("propagate(): no encoded frame is pending (call encode(img, pos_id) first)")
        if matte_refined:
            who = "propagate(matte_refined=True)"
            if matte or composite or conf or labels:
                raise RuntimeError("%s: asks for one last kernel; conf, matte, composite or labels=%r ask for another" % (who, labels))
            ids = self._need_matte("propagate")
            if not self._refine[0]:
                raise RuntimeError("%s: no refinement (call set_matte_refine(radius, eps) with a radius of 1..16 first)" % who)
            H, W, dev = self._pending_shape
            key = getattr(self._engine, "_u8_key", None)
            if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() != 4 or src.shape[0] != 1 or src.shape[3] != 3 or key is None or \
                    tuple(src.shape[1:3]) != tuple(key[:2]) or src.device != dev:
                raise RuntimeError("%s: src must be the packed RGB frame that was encoded with encode_u8, uint8 [1, Hs, Ws, 3] on %s" % (who, dev))
            img = src.contiguous()
            out = torch.empty(tuple(img.shape[:3]), device=dev, dtype=torch.uint8)
            self._engine.set_matte(ids)
            self._engine.set_matte_refine(*self._refine)
            self._pending_shape = None
            self._engine.propagate_matte_refined(img.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out
        if matte or composite:
            who = "propagate(matte=True)" if matte else "propagate(composite=True)"
            if (matte and composite) or conf or labels in ("rgb", "score", "overlay"):
                raise RuntimeError("%s: asks for one last kernel; conf, another of matte / composite or labels=%r ask for another" % (who, labels))
            ids = self._need_matte("propagate")
            H, W, dev = self._pending_shape
            s = torch.cuda.current_stream(dev).cuda_stream
            if matte:
                out, mm = torch.empty((1, H, W), device=dev, dtype=torch.uint8), torch.empty((1, H, W), device=dev, dtype=torch.uint8)
                self._engine.set_matte(ids)
                self._pending_shape = None
                self._engine.propagate_matte(out.data_ptr(), mm.data_ptr(), s)
                return out, mm
            bg = self._background(background)
            if bg is None:
                raise RuntimeError("propagate(composite=True): the alpha mode needs a destination view; use forward_composite_u8(out_view=...)")
            key = getattr(self._engine, "_u8_key", None)
            if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() != 4 or src.shape[0] != 1 or src.shape[3] != 3 or key is None or \
                    tuple(src.shape[1:3]) != tuple(key[:2]) or src.device != dev:
                raise RuntimeError("propagate(composite=True): src must be the packed RGB frame that was encoded with encode_u8, uint8 [1, Hs, Ws, 3] on %s" % (dev,))
            img = src.contiguous()
            out = torch.empty(tuple(img.shape), device=dev, dtype=torch.uint8)
            self._engine.set_matte(ids)
            self._engine.set_output_composite(bg)
            self._engine.set_matte_refine(*self._refine)
            self._engine.set_output_view(None)
            self._pending_shape = None
            self._engine.propagate_composite(img.data_ptr(), out.data_ptr(), s)
            return out
        if conf:
            if labels in ("rgb", "score", "overlay"):
                raise RuntimeError("propagate(conf=True): gives uint8 labels and confidence; labels=%r asks for another last kernel" % (labels,))
            H, W, dev = self._pending_shape
            out, cmap = torch.empty((1, H, W), device=dev, dtype=torch.uint8), torch.empty((1, H, W), device=dev, dtype=torch.uint8)
            self._engine.set_confidence(*self._confidence)
            self._pending_shape = None
            self._engine.propagate_labels_conf(out.data_ptr(), cmap.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out, cmap
        if isinstance(labels, str) and labels not in ("u8", "rgb", "score", "overlay"):
            raise RuntimeError("propagate(): labels must be False, True, \"u8\", \"rgb\", \"score\" or \"overlay\"")
        if labels == "overlay":
            H, W, dev = self._pending_shape
            pal = self._palette_rgba(palette, alpha)
            img, (Hs, Ws), nv = self._overlay_source("propagate(labels=\"overlay\")", src, 1, src_size, uv_offset, standard)
            if img.device != dev:
                raise RuntimeError("propagate(labels=\"overlay\"): src must be on the frame's device %s, got %s" % (dev, img.device))
            key = getattr(self._engine, "_u8_key", None) or getattr(self._engine, "_nv12_key", None)   # encode_u8 / encode_nv12 configured the input
            if key is None or (Hs, Ws) != tuple(key[:2]) or (nv is None) != (getattr(self._engine, "_u8_key", None) is not None):
                raise RuntimeError("propagate(labels=\"overlay\"): src is not of the size and format of the frame that was encoded (encode_u8 / encode_nv12)")
            out = torch.empty((1, Hs, Ws, 3), device=dev, dtype=torch.uint8)
            self._engine.set_output_overlay(pal)
            self._engine.set_output_view(None)
            self._pending_shape = None
            self._engine.propagate_overlay(img.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out
        if labels == "score":
            H, W, dev = self._pending_shape
            gt = self._check_gt(gt, 1, H, W, dev)
            out = torch.empty((1, H, W), device=dev, dtype=torch.uint8)
            self._engine.set_score(gt_map)
            self._pending_shape = None
            self._engine.propagate_score(gt.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out
        if labels == "rgb" and out_size is None:
            raise RuntimeError("propagate(labels=\"rgb\"): out_size=(oh, ow) is required")
        H, W, dev = self._pending_shape
        s = torch.cuda.current_stream(dev).cuda_stream
        if labels == "rgb":
            out = self._rgb_out(1, out_size, dev)
            self._engine.set_output_rgb(out.shape[1], out.shape[2], self._palette(palette))
            self._engine.set_output_view(None)
            self._pending_shape = None
            self._engine.propagate_rgb(out.data_ptr(), s)
            return out
        self._pending_shape = None
        if isinstance(labels, str):
            out = torch.empty((1, H, W), device=dev, dtype=torch.uint8)
            self._engine.propagate_labels_u8(out.data_ptr(), s)
        elif labels:
            out = torch.empty((1, H, W), device=dev, dtype=torch.int32)
            self._engine.propagate_labels(out.data_ptr(), s)
        else:
            out = torch.empty((1, self.nclass, H, W), device=dev, dtype=torch.float32)
            self._engine.propagate(out.data_ptr(), s)
        return out

    def cache_entry_numel(self):
        """(q, k, v) element counts of one cache entry: [Lk,64], [Lk,64], [Lk,d_v]."""
        if self._engine is None:
            raise RuntimeError("cache_entry_numel(): the geometry is known once a frame has been encoded; use cache_entry_numel_for(H, W) before")
        lk, dk, dv = self._engine.cache_dims()
        return lk * dk, lk * dk, lk * dv

    def cache_entry_numel_for(self, H, W):
        """The same from the input size alone (arch): lets every rank of a path-parallel group size its buffers before any frame."""
        lk = arch.key_size(arch.spec_feat_size(self.spec, H)) * arch.key_size(arch.spec_feat_size(self.spec, W))
        return lk * self.spec.d_k, lk * self.spec.d_k, lk * self.spec.d_v

    def cache_export(self, q, k, v):
        """Copy the pending frame's cache entry into the given contiguous fp32 CUDA tensors."""
        self._engine.cache_export(q.data_ptr(), k.data_ptr(), v.data_ptr(), torch.cuda.current_stream(q.device).cuda_stream)

    def cache_push(self, q, k, v):
        """Append a peer's cache entry to the FIFO (contiguous fp32 CUDA tensors)."""
        if self._engine is None:
            raise RuntimeError("cache_push(): no handle yet -- call ensure_engine(H, W, device) (or encode a frame) first")
        self._engine.cache_push(q.data_ptr(), k.data_ptr(), v.data_ptr(), torch.cuda.current_stream(q.device).cuda_stream)

    def reset(self):
        for e in [self._engine] + list(self._extra_engines):
            if e is not None:
                e.reset()
        self._batch = None
        self._pending_shape = None                                     # a frame encoded but not propagated is dropped with the FIFO (tdnet_reset)

    @property
    def engine(self):
        return self._engine
