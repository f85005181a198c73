// td_model.hip -- the translation unit of libtdnet_hip.so: the C ABI of include/tdnet.h, and nothing else.  The host code behind it lives in the
// headers this file pulls in (td_frame.h -> td_launch.h -> td_weights.h -> td_handle.h -> the kernel headers).  The single-operator entry points and
// probes of the tests (include/tdnet_test.h, td_ops_test.h) are a SECOND library, libtdnet_hip_test.so = td_model_test.hip = this file + td_ops_test.h.
//
// Reference behaviour mirrored here (paths relative to /root/reference/Testing/model/pspnet):
//   forward / path dispatch ........ td4_psp18.py:216-229, td2_psp50.py:146-155
//   per-path graph ................. td4_psp18.py:137-212, td2_psp50.py:112-143      (td_frame.h)
//   FIFO ........................... td4_psp18.py:123-134 (depth 3), td2_psp50.py:98-109 (depth 1)
//   strict state_dict loading ...... td4_psp18.py:232-240                            (td_weights.h)
#include "td_frame.h"

extern "C" const char* tdnet_last_error(void) { return g_err; }
// The build stamps the library with a hash of its sources (tdnet_amd/build.py: -DTDNET_SRC_HASH): tests and smoke() compare it with
// the sources that were shipped, so a stale prebuilt .so cannot pass for HEAD's kernels.
#ifndef TDNET_SRC_HASH
#define TDNET_SRC_HASH "unstamped"
#endif
extern "C" const char* tdnet_version(void) { return "tdnet_amd 0.3 (gfx950, fp32 MFMA) tdnet-src-hash:" TDNET_SRC_HASH; }
// Per-handle kernel configuration (include/tdnet.h tdnet_opts); nothing here is process-wide: two handles in one process may differ.
extern "C" void tdnet_opts_default(tdnet_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->winograd = TDNET_WINOGRAD_DEFAULT;   // F(4x4,3x3) for the stride-1 3x3 convs with Cin, Cout >= 128
    o->precision = 0;                       // fp32 MFMA: the only mode the 1e-3 logits gate applies to
    o->pipeline = 1;                        // two-stage conv prefetch
    o->gemm_persistent = 1;                 // stride-1 1x1 convs and the Winograd GEMMs on the persistent multi-tile GEMM kernel
    o->attention = TDNET_ATTENTION_DEFAULT;
    o->fusion = TDNET_FUSION_DEFAULT;
    o->overlap = TDNET_OVERLAP_DEFAULT;
}
extern "C" void tdnet_arch_default(tdnet_arch* a) {
    if (!a) return;
    memset(a, 0, sizeof(*a));
    a->dilated = 1;                         // output stride 8 (resnet.py:140-149)
    a->multi_grid = 1;                      // layer-4 dilations 4, 8, 16
}
extern "C" int tdnet_create(const tdnet_cfg* cfg, tdnet_t** out) { return tdnet_create_opts(cfg, nullptr, out); }

// geometry of a handle from its configuration and block list (the same for every handle of a weight block)
static void set_geometry(tdnet* n, const tdnet_cfg* cfg) {
    n->cfg = *cfg;
    n->P = cfg->model;
    const int exp = cfg->backbone >= 50 ? 4 : 1;                       // Bottleneck expansion (td2_psp50.py:63-66)
    n->deep = cfg->backbone >= 50;
    n->C = 512 * exp;
    n->SC = n->deep ? 128 : 64;
    n->DV = cfg->model == 4 ? 512 * exp : 128 * exp;                   // td4_psp18.py:85 (512*expansion) / td2_psp50.py:79 (512*exp//4)
    n->MID = cfg->model == 4 ? n->DV / 4 : n->DV / 2;                  // FCNHead chn_down 4 / 2
    if (cfg->model == 1) { n->DV = 2 * n->C; n->MID = n->C / 4; }      // PSPHead: conv3x3 on the 2C-channel concat -> C/4 (pspnet.py:105-109)
    n->FIFO = cfg->model == 4 ? 3 : cfg->model == 2 ? 1 : 0;
    n->H = cfg->height; n->W = cfg->width;
    n->H1 = (n->H - 1) / 2 + 1; n->W1 = (n->W - 1) / 2 + 1;
    n->H2 = (n->H1 - 1) / 2 + 1; n->W2 = (n->W1 - 1) / 2 + 1;
    n->h = feature_size(n->H, n->bspec); n->w = feature_size(n->W, n->bspec);   // output stride 8 or 32, from the block list
    n->hk = key_size(n->h); n->wk = key_size(n->w);
    n->Lq = n->h * n->w; n->Lk = n->hk * n->wk;
}

extern "C" int tdnet_create_arch(const tdnet_cfg* cfg, const tdnet_arch* arch, const tdnet_opts* opts, tdnet_t** out) {
    if (!cfg || !out) return td_fail("tdnet_create: null argument");
    tdnet_arch a;
    tdnet_arch_default(&a);
    if (arch) {
        if ((arch->dilated != 0 && arch->dilated != 1) || (arch->multi_grid != 0 && arch->multi_grid != 1))
            return td_fail("tdnet_create: tdnet_arch.dilated / multi_grid must be 0 or 1, got %d / %d", arch->dilated, arch->multi_grid);
        for (int r : arch->reserved)
            if (r != 0) return td_fail("tdnet_create: tdnet_arch.reserved must be 0");
        a = *arch;
    }
    if (cfg->model != 4 && cfg->model != 2 && cfg->model != 1)
        return td_fail("tdnet_create: model must be 4 (td4), 2 (td2) or 1 (single-frame PSPNet), got %d", cfg->model);
    if (cfg->backbone != 18 && cfg->backbone != 34 && cfg->backbone != 50 && cfg->backbone != 101)
        return td_fail("tdnet_create: backbone must be 18, 34, 50 or 101, got %d", cfg->backbone);
    if (cfg->backbone == 101 && cfg->model != 1)
        return td_fail("tdnet_create: resnet101 is the PSPNet baseline's backbone (pspnet.py:36); td4 / td2 accept 18, 34 or 50");
    if (cfg->nclass < 1 || cfg->nclass > 256) return td_fail("tdnet_create: nclass must be in 1..256, got %d", cfg->nclass);
    if (cfg->height < 9 || cfg->width < 9) return td_fail("tdnet_create: input too small");
    {
        int ndev = 0;
        TD_HIP(hipGetDeviceCount(&ndev));
        if (cfg->device < 0 || cfg->device >= ndev) return td_fail("tdnet_create: device %d out of range (%d visible)", cfg->device, ndev);
    }
    TdWeights* wt = new TdWeights();
    wt->device = cfg->device;
    wt->arch = a;
    tdnet* n = new tdnet(wt);
    n->bspec = backbone_blocks(cfg->backbone, a.dilated != 0, a.multi_grid != 0);
    set_geometry(n, cfg);
    n->opts = opts_or_default(opts);
    build_expected(n);
    *out = n;
    return 0;
}

extern "C" int tdnet_create_opts(const tdnet_cfg* cfg, const tdnet_opts* opts, tdnet_t** out) {
    if (cfg && cfg->model == 1 && (cfg->backbone == 18 || cfg->backbone == 34))
        return td_fail("tdnet_create: pspnet on resnet%d is created with tdnet_create_arch; tdnet_create_opts keeps accepting 50 or 101 only", cfg->backbone);
    return tdnet_create_arch(cfg, nullptr, opts, out);
}

extern "C" int tdnet_get_arch(const tdnet_t* n, tdnet_arch* out) {
    if (!n || !out) return td_fail("tdnet_get_arch: null argument");
    *out = n->wt->arch;
    return 0;
}
extern "C" int tdnet_feature_dims(const tdnet_t* n, int* height, int* width) {
    if (!n) return td_fail("tdnet_feature_dims: null handle");
    if (height) *height = n->h;
    if (width) *width = n->w;
    return 0;
}

// A second (third, ...) handle on the SAME weights: its own workspace, K/Q/V FIFO, streams and events -- one more video stream, or one
// more frame of the same stream in flight -- while the folded, packed weights stay one copy in HBM.  The reference's batch of N samples
// shares one nn.Module's parameters the same way (td4_psp18.py:216-229).
extern "C" int tdnet_create_shared(const tdnet_t* weights_of, const tdnet_opts* opts, tdnet_t** out) {
    if (!weights_of || !out) return td_fail("tdnet_create_shared: null argument");
    if (!weights_of->finalized) return td_fail("tdnet_create_shared: the handle whose weights are to be shared is not finalized");
    if (opts) {                                                        // the packing depends on the options: a shared block has ONE set
        const tdnet_opts o = opts_or_default(opts);
        if (memcmp(&o, &weights_of->opts, sizeof(o)) != 0)
            return td_fail("tdnet_create_shared: tdnet_opts differ from those the weights were packed for (pass NULL to inherit them)");
    }
    TD_ON_DEVICE(weights_of, -1);
    tdnet* n = new tdnet(weights_of->wt);
    n->wt->refs.fetch_add(1, std::memory_order_relaxed);
    set_geometry(n, &weights_of->cfg);
    n->opts = weights_of->opts;
    if (init_handle(n)) { tdnet_destroy(n); return -1; }
    *out = n;
    return 0;
}

extern "C" void tdnet_destroy(tdnet_t* n) {
    if (!n) return;
    TD_ON_DEVICE(n);
    for (float* q : {n->img4, n->s1, n->s1b, n->bx, n->bt, n->br, n->bu, n->rowpart, n->pooled, n->ppmfeat, n->z, n->v_cur, n->q1, n->q_cur,
                     n->k1, n->vp, n->chain_a, n->chain_b, n->feat, n->ln_part, n->ln_mean, n->ln_rstd, n->ln, n->headmid,
                     n->lowres, n->stage_tmp, n->logits_tmp, n->wino_v, n->wino_m, n->ppm_basis, n->fold_g[0], n->fold_g[1], n->fold_g[2]})
        if (q) hipFree(q);
    for (auto& s : n->slots) { if (s.q) hipFree(s.q); if (s.k) hipFree(s.k); if (s.v) hipFree(s.v); }
    for (auto& r : n->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    if (n->vt16) hipFree(n->vt16);
    u8_free(n->u8);
    rgb_free(n->rgb);
    overlay_free(n->overlay);
    score_free(n->score);
    regions_free(n->regions);
    tracks_free(n->tracks);
    runs_free(n->runs);
    refine_free(n->refine);
    for (float* q : {n->wino_v2, n->wino_m2}) if (q) hipFree(q);
    for (auto* v : {&n->seg_t, &n->seg_r, &n->seg_x}) for (float* q : *v) if (q) hipFree(q);
    if (n->chain2) hipStreamDestroy(n->chain2);
    for (hipStream_t x : n->probe_streams) hipStreamDestroy(x);
    for (hipStream_t x : n->retired_streams) hipStreamDestroy(x);
    if (n->ev_cfork) hipEventDestroy(n->ev_cfork);
    if (n->ev_cjoin) hipEventDestroy(n->ev_cjoin);
    if (n->side) hipStreamDestroy(n->side);
    if (n->ev_fork) hipEventDestroy(n->ev_fork);
    if (n->ev_join) hipEventDestroy(n->ev_join);
    TdWeights* wt = n->wt;
    delete n;
    if (wt->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) {                                             // the last handle of the block, whichever it is (the owner may go first)
        for (auto& p : wt->paths) free_path(p);
        delete wt;
    }
}

extern "C" int tdnet_set_weight(tdnet_t* n, const char* name, const float* host, size_t count) {
    if (!n || !name || !host) return td_fail("tdnet_set_weight: null argument");
    if (n->finalized) return td_fail("tdnet_set_weight: weights already finalized");
    auto it = n->expected.find(name);
    if (it == n->expected.end()) return td_fail("Unexpected key in state_dict: \"%s\"", name);
    if (it->second != count) return td_fail("size mismatch for %s: expected %zu elements, got %zu", name, it->second, count);
    const std::string s = name;
    if (s.find(".fc.weight") != std::string::npos && s.compare(0, 10, "pretrained") == 0) return 0;   // unused classifier
    if (s.find(".fc.bias") != std::string::npos && s.compare(0, 10, "pretrained") == 0) return 0;
    if (s.size() > 19 && s.compare(s.size() - 19, 19, "num_batches_tracked") == 0) { n->sd[s] = {0.f}; return 0; }
    n->sd[s].assign(host, host + count);
    return 0;
}
extern "C" int tdnet_finalize_weights(tdnet_t* n) {
    if (!n) return td_fail("tdnet_finalize_weights: null handle");
    if (n->finalized) return td_fail("tdnet_finalize_weights: already finalized");
    TD_ON_DEVICE(n, -1);
    TD_TRY(finalize_block(n));
    return init_handle(n);
}
extern "C" int tdnet_warmup(tdnet_t* n, void* stream) {
    if (!n) return td_fail("tdnet_warmup: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_warmup: weights not finalized");
    TD_ON_DEVICE(n, -1);
    return place_chain_stream(n, (hipStream_t)stream, true);
}
extern "C" int tdnet_memory_bytes(const tdnet_t* n, size_t* weights, size_t* handle) {
    if (!n) return td_fail("tdnet_memory_bytes: null handle");
    if (weights) *weights = n->wt->device_bytes;
    if (handle) *handle = n->ws_bytes;
    return n->wt->refs.load(std::memory_order_relaxed);
}
extern "C" int tdnet_last_launch_count(const tdnet_t* n) { return n ? n->launches : -1; }
extern "C" int tdnet_streams_share_queue(void* stream_a, void* stream_b, int* shared) {
    if (!shared) return td_fail("tdnet_streams_share_queue: shared is NULL");
    *shared = 0;
    if (stream_a == stream_b) { *shared = 1; return 0; }
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventCreate(&e2) != hipSuccess) {
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
        return td_fail("tdnet_streams_share_queue: hipEventCreate failed");
    }
    bool sh = false;
    const int rc = streams_share_a_queue((hipStream_t)stream_a, (hipStream_t)stream_b, e0, e1, e2, &sh);
    hipEventDestroy(e0); hipEventDestroy(e1); hipEventDestroy(e2);
    *shared = sh ? 1 : 0;
    return rc;
}

// tdnet_last_launch_count: everything a frame entry enqueued, the final upsample / argmax kernel included (counted in TD_LAUNCH itself)
struct LaunchCount {
    tdnet* n; long l0;
    explicit LaunchCount(tdnet* n_) : n(n_), l0(td_launch_count) {}
    ~LaunchCount() { n->launches = (int)(td_launch_count - l0); }
};
// The frame entries differ in how the image arrives -- FrameInput: fp32 NCHW, or uint8 HWC through tdnet_set_input_u8; or not at all: the frame
// tdnet_encode left pending -- and in what leaves (td_launch.h FrameOutput); everything between is one frame, and ONE tail: frame_out.  fp32 and
// uint8 entries may be mixed frame by frame on one handle.
struct FrameSource { const FrameInput* img; int pos_id; };            // img == nullptr: the pending encoded frame (the tdnet_propagate* entries)
static int propagate_lowres(tdnet* n, hipStream_t s);
// `who` names the entry in the messages of the frame's checks.  The forward route's last launch is a family-2 profile record; the propagate
// route stays outside the records (tdnet_last_ms / tdnet_last_launches of a split frame are those of its tdnet_encode half).  A form that
// is not configured is refused before the frame starts: the FIFO and a pending frame stay as they are.
// With a destination view in force (tdnet_set_output_view) the picture must be the view's rectangle.  The configurations are independent of each other's
// order, so it is the frame entry that checks, on the host, before anything is enqueued; `kind`'s own configuration exists (output_configured).
static int picture_dst_check(const tdnet* n, OutKind kind, const char* who) {
    if (!n->dst.set || (kind != OUT_RGB && kind != OUT_OVERLAY)) return 0;
    const bool rgb = kind == OUT_RGB;
    const int ph = rgb ? n->rgb.oh : n->u8.Hs, pw = rgb ? n->rgb.ow : n->u8.Ws;
    if (ph != n->dst.h || pw != n->dst.w)
        return td_fail("%s: the %s is %d x %d but the destination view's rectangle is %d x %d (tdnet_set_output_view: nothing is resized)", who,
                       rgb ? "colour map" : "overlay", ph, pw, n->dst.h, n->dst.w);
    return 0;
}
static int frame_out(tdnet* n, const FrameSource& src, const FrameOutput& out, void* stream, const char* who) {
    TD_ON_DEVICE(n, -1);
    TD_TRY(output_configured(n, out.kind, who));
    TD_TRY(picture_dst_check(n, out.kind, who));
    LaunchCount count_(n);
    hipStream_t s = (hipStream_t)stream;
    if (src.img ? forward_lowres(n, *src.img, src.pos_id, s, who) : propagate_lowres(n, s)) return -1;
    if (src.img) prof_begin(n, 2, false, 0, s);
    const int rc = emit_output(n, out, s, who);
    if (src.img) prof_end(n, s);
    TD_HIP(hipGetLastError());
    return rc;
}
static int frame_out(tdnet* n, const FrameInput& img, int pos_id, const FrameOutput& out, void* stream, const char* who) {
    return frame_out(n, FrameSource{&img, pos_id}, out, stream, who);
}
static inline FrameInput frame_input_u8(const tdnet* n, const uint8_t* img) { return FrameInput{img, TD_IMG_U8, &n->u8}; }
extern "C" int tdnet_forward(tdnet_t* n, const float* img, int pos_id, float* logits, void* stream) {
    if (!n || !img || !logits) return td_fail("tdnet_forward: null argument");
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_LOGITS, logits}, stream, "tdnet_forward");
}
extern "C" int tdnet_forward_u8(tdnet_t* n, const uint8_t* img, int pos_id, float* logits, void* stream) {
    if (!n || !img || !logits) return td_fail("tdnet_forward_u8: null argument");
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_LOGITS, logits}, stream, "tdnet_forward_u8");
}
extern "C" int tdnet_argmax(tdnet_t* n, const float* logits, int32_t* labels, void* stream) {
    if (!n || !logits || !labels) return td_fail("tdnet_argmax: null argument");
    TD_ON_DEVICE(n, -1);
    launch_argmax(logits, n->cfg.nclass, (long)n->H * n->W, labels, (hipStream_t)stream);
    TD_HIP(hipGetLastError());
    return 0;
}
extern "C" int tdnet_argmax_u8(tdnet_t* n, const float* logits, uint8_t* labels, void* stream) {
    if (!n || !logits || !labels) return td_fail("tdnet_argmax_u8: null argument");
    TD_ON_DEVICE(n, -1);
    TD_TRY(launch_argmax_u8(logits, n->cfg.nclass, (long)n->H * n->W, labels, (hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
extern "C" int tdnet_forward_labels(tdnet_t* n, const float* img, int pos_id, int32_t* labels, void* stream) {
    if (!n || !img || !labels) return td_fail("tdnet_forward_labels: null argument");
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_LABELS_I32, labels}, stream, "tdnet_forward");   // its frame checks have always reported as tdnet_forward
}
extern "C" int tdnet_forward_u8_labels(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* labels, void* stream) {
    if (!n || !img || !labels) return td_fail("tdnet_forward_u8_labels: null argument");
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_LABELS_U8, labels}, stream, "tdnet_forward_u8_labels");
}
// The overlay's index tables belong to the pair (network size, source size): a byte-input configuration that changed the source size rebuilds them
// (the caller has synchronised: the previous tables existed only beside a previous input configuration).  Nothing to do without an overlay.
static int overlay_follow_input(tdnet* n, const char* who) {
    if (!n->overlay.set && !n->comp.set && !n->refine.radius) return 0;   // the composite and the refined matte sample through the same tables
    const size_t before = n->overlay.bytes;
    int rc = overlay_tables(n->overlay, n->H, n->W, n->u8.Hs, n->u8.Ws, who);
    n->ws_bytes += n->overlay.bytes - before;
    if (!rc) rc = overlay_set_swap(n->overlay, n->u8.swap, who);       // the picture's colour order is the source's
    if (!rc && n->refine.radius) {                                     // the refined matte's workspace is the source's size
        const size_t rb = n->refine.bytes;
        rc = refine_alloc(n->refine, n->u8.Hs, n->u8.Ws, who);
        n->ws_bytes += n->refine.bytes - rb;
    }
    return rc;
}
// The handle's ONE byte-input configuration, whichever entry describes it (not a frame call: it may synchronise; idempotent for equal arguments).  The
// tables live in memory this handle owns; a tdnet_create_shared handle has its own configuration.  A failed call leaves the previous one in force.
static int set_input(tdnet* n, const SrcView& sv, int Hs, int Ws, const double* mean, const double* std_, const char* who) {
    TD_ON_DEVICE(n, -1);
    static const double mean0[3] = {.485, .456, .406}, std0[3] = {.229, .224, .225};   // dataloader.py:52-53
    const double* m = mean ? mean : mean0;
    const double* sd = std_ ? std_ : std0;
    if (u8_same(n->u8, sv, Hs, Ws, m, sd)) return 0;
    if (n->u8.set) TD_HIP(hipDeviceSynchronize());                    // a frame in flight may still read the tables that are about to go
    const size_t before = n->u8.bytes;
    TD_TRY(u8_build(n->u8, sv, Hs, Ws, n->H, n->W, m, sd, who));
    n->ws_bytes += n->u8.bytes - before;                               // tdnet_memory_bytes: the tables belong to this handle
    return overlay_follow_input(n, who);
}
// packed RGB [src_height][src_width][3]: the whole, tight RGB24 view
extern "C" int tdnet_set_input_u8(tdnet_t* n, int src_height, int src_width, const double* mean, const double* std_) {
    if (!n) return td_fail("tdnet_set_input_u8: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_input_u8: weights not finalized");
    return set_input(n, src_view_rgb(src_height, src_width), src_height, src_width, mean, std_, "tdnet_set_input_u8");
}
// an NV12 surface of this layout (td_ingest.h IngestYuv with YuvFormNv12): the whole NV12 view
extern "C" int tdnet_set_input_nv12(tdnet_t* n, int src_height, int src_width, int pitch, size_t uv_offset, int standard, const double* mean, const double* std_) {
    if (!n) return td_fail("tdnet_set_input_nv12: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_input_nv12: weights not finalized");
    const Nv12Layout nv = {pitch, uv_offset, standard};
    return set_input(n, src_view_nv12(src_height, src_width, nv), src_height, src_width, mean, std_, "tdnet_set_input_nv12");
}
// a rectangle of a pitched frame in one of the five pixel formats (include/tdnet.h "source views")
extern "C" int tdnet_set_input_view(tdnet_t* n, const tdnet_view* v, const double* mean, const double* std_) {
    if (!n) return td_fail("tdnet_set_input_view: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_input_view: weights not finalized");
    SrcView sv;
    int Hs = 0, Ws = 0;
    TD_TRY(view_resolve(v, sv, Hs, Ws, "tdnet_set_input_view"));
    return set_input(n, sv, Hs, Ws, mean, std_, "tdnet_set_input_view");
}
// a rectangle of a YUV surface in one of the six layouts (include/tdnet.h "surfaces")
extern "C" int tdnet_set_input_surface(tdnet_t* n, const tdnet_surface* t, const double* mean, const double* std_) {
    if (!n) return td_fail("tdnet_set_input_surface: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_input_surface: weights not finalized");
    SrcView sv;
    int Hs = 0, Ws = 0;
    TD_TRY(surface_resolve(t, sv, Hs, Ws, "tdnet_set_input_surface"));
    return set_input(n, sv, Hs, Ws, mean, std_, "tdnet_set_input_surface");
}
// ---- colour map out ----------------------------------------------------------------------------------------------------------------
// Configuration of the colour-map output (not a frame call: it may synchronise; idempotent for equal arguments).  Tables and palette live in
// memory this handle owns; a tdnet_create_shared handle has its own configuration.
extern "C" int tdnet_set_output_rgb(tdnet_t* n, int out_height, int out_width, const uint8_t* palette_rgb, int n_colours) {
    if (!n) return td_fail("tdnet_set_output_rgb: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_output_rgb: weights not finalized");
    TD_ON_DEVICE(n, -1);
    if (rgb_same(n->rgb, out_height, out_width, palette_rgb, n_colours)) return 0;
    if (n->rgb.set) TD_HIP(hipDeviceSynchronize());                   // a frame in flight may still read the tables that are about to go
    const size_t before = n->rgb.bytes;
    TD_TRY(rgb_build(n->rgb, n->H, n->W, out_height, out_width, palette_rgb, n_colours, "tdnet_set_output_rgb"));
    n->ws_bytes += n->rgb.bytes - before;
    return 0;
}
// The labels entries with another last launch: the picture instead of the label map.  Same frame, same FIFO step, same number of launches.
extern "C" int tdnet_forward_rgb(tdnet_t* n, const float* img, int pos_id, uint8_t* rgb, void* stream) {
    if (!n || !img || !rgb) return td_fail("tdnet_forward_rgb: null argument");
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_RGB, rgb}, stream, "tdnet_forward_rgb");
}
extern "C" int tdnet_forward_u8_rgb(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* rgb, void* stream) {
    if (!n || !img || !rgb) return td_fail("tdnet_forward_u8_rgb: null argument");
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_RGB, rgb}, stream, "tdnet_forward_u8_rgb");
}
extern "C" int tdnet_labels_rgb(tdnet_t* n, const uint8_t* labels, uint8_t* rgb, void* stream) {
    if (!n || !labels || !rgb) return td_fail("tdnet_labels_rgb: null argument");
    TD_ON_DEVICE(n, -1);
    TD_TRY(output_configured(n, OUT_RGB, "tdnet_labels_rgb"));
    TD_TRY(picture_dst_check(n, OUT_RGB, "tdnet_labels_rgb"));
    if (n->dst.set) TD_TRY(launch_picture_dst(nullptr, 0, 0, 0, labels, &n->rgb, nullptr, nullptr, nullptr, n->dst, rgb, (hipStream_t)stream));
    else
    TD_TRY(launch_labels_rgb(labels, n->rgb, rgb, (hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
// ---- overlay out -----------------------------------------------------------------------------------------------------------------------
// Configuration of the overlay output (not a frame call: it may synchronise; idempotent for equal arguments).  Independent of the order of the
// byte-input configuration: the index tables are built here if the handle has one, by tdnet_set_input_u8 / tdnet_set_input_nv12 otherwise.
extern "C" int tdnet_set_output_overlay(tdnet_t* n, const uint8_t* palette_rgba, int n_colours) {
    if (!n) return td_fail("tdnet_set_output_overlay: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_output_overlay: weights not finalized");
    TD_ON_DEVICE(n, -1);
    if (overlay_same(n->overlay, palette_rgba, n_colours)) return 0;
    if (n->overlay.set) TD_HIP(hipDeviceSynchronize());               // a frame in flight may still read the table that is about to go
    const size_t before = n->overlay.bytes;
    TD_TRY(overlay_build(n->overlay, palette_rgba, n_colours, "tdnet_set_output_overlay"));
    int rc = n->u8.set ? overlay_tables(n->overlay, n->H, n->W, n->u8.Hs, n->u8.Ws, "tdnet_set_output_overlay") : 0;
    n->ws_bytes += n->overlay.bytes - before;
    if (!rc && n->u8.set) rc = overlay_set_swap(n->overlay, n->u8.swap, "tdnet_set_output_overlay");
    return rc;
}
// What every overlay entry checks on the host before anything is enqueued: both configurations exist, and `out` [Hs][Ws][3] does not overlap the
// source extent (the WHOLE frame's, whatever rectangle of it the view is) -- the kernel reads the source while it writes the picture.
static int overlay_args(const tdnet* n, const uint8_t* src, const uint8_t* out, const char* who) {
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    TD_TRY(output_configured(n, OUT_OVERLAY, who));
    TD_TRY(picture_dst_check(n, OUT_OVERLAY, who));
    const U8Input& u = n->u8;
    const size_t nout = n->dst.set ? n->dst.extent : (size_t)3 * u.Hs * u.Ws, nsrc = u.extent;   // a destination view: the WHOLE destination frame's extent
    const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out;
    if (s0 < o0 + nout && o0 < s0 + nsrc) return td_fail("%s: out overlaps the source frame (%zu bytes at %p against %zu bytes at %p)", who, nout, (const void*)out, nsrc, (const void*)src);
    return 0;
}
// The labels entries with another last launch: the overlay instead of the label map; the image pointer is the frame's image (first launch) AND the
// overlay's source (last launch).  Same frame, same FIFO step, same number of launches.
extern "C" int tdnet_forward_u8_overlay(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* out, void* stream) {
    if (!n || !img || !out) return td_fail("tdnet_forward_u8_overlay: null argument");
    TD_TRY(overlay_args(n, img, out, "tdnet_forward_u8_overlay"));
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_OVERLAY, out, nullptr, nullptr, img}, stream, "tdnet_forward_u8_overlay");
}
extern "C" int tdnet_labels_overlay(tdnet_t* n, const uint8_t* labels, const uint8_t* img, uint8_t* out, void* stream) {
    if (!n || !labels || !img || !out) return td_fail("tdnet_labels_overlay: null argument");
    TD_TRY(overlay_args(n, img, out, "tdnet_labels_overlay"));
    TD_ON_DEVICE(n, -1);
    if (n->dst.set) TD_TRY(launch_picture_dst(nullptr, 0, 0, 0, labels, nullptr, &n->overlay, &n->u8, img, n->dst, out, (hipStream_t)stream));
    else
    TD_TRY(launch_labels_overlay(labels, n->overlay, n->u8, img, out, (hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
// ---- destination views -----------------------------------------------------------------------------------------------------------------
// Configuration of where the picture entries write (include/tdnet.h "destination views"): plain host state of the handle -- the kernels take it as
// arguments when an entry enqueues, so nothing is allocated and nothing in flight reads it; idempotent; per handle.  NULL: contiguous [h][w][3] again.  A
// failed call leaves the previous configuration in force.
extern "C" int tdnet_set_output_view(tdnet_t* n, const tdnet_view* v) {
    if (!n) return td_fail("tdnet_set_output_view: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_output_view: weights not finalized");
    if (!v) { n->dst = DstOutput(); return 0; }
    return dst_build(n->dst, v, "tdnet_set_output_view");
}
// The same for a rectangle of a 4:2:0 surface (include/tdnet.h "surfaces"); the view and the surface replace each other: ONE destination at a time
extern "C" int tdnet_set_output_surface(tdnet_t* n, const tdnet_surface* t) {
    if (!n) return td_fail("tdnet_set_output_surface: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_output_surface: weights not finalized");
    if (!t) { n->dst = DstOutput(); return 0; }
    return dst_surface_build(n->dst, t, "tdnet_set_output_surface");
}
// ---- score out -------------------------------------------------------------------------------------------------------------------------
// Configuration of the score output (not a frame call: it may synchronise; idempotent for an equal map).  The matrix and the map live in memory
// this handle owns; a tdnet_create_shared handle has its own.  A DIFFERENT map starts a new, zeroed matrix: counts folded two ways do not mix.
extern "C" int tdnet_set_score(tdnet_t* n, const uint8_t* gt_map) {
    if (!n) return td_fail("tdnet_set_score: null handle");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_set_score: weights not finalized");
    TD_ON_DEVICE(n, -1);
    unsigned char m[256];
    score_map_or_identity(gt_map, m);
    if (n->score.set && memcmp(n->score.map, m, 256) == 0) return 0;
    if (n->score.set) TD_HIP(hipDeviceSynchronize());                 // a frame in flight may still add into the matrix that is about to go
    const size_t before = n->score.bytes;
    TD_TRY(score_build(n->score, n->cfg.nclass, gt_map, "tdnet_set_score"));
    n->ws_bytes += n->score.bytes - before;
    return 0;
}
#define TD_NEED_SCORE(n, who) TD_TRY(output_configured(n, OUT_SCORE, who))
// The labels entries with another last launch: the frame's counts added to the handle's matrix, the label map written too if asked for.  Same
// frame, same FIFO step, same number of launches.
extern "C" int tdnet_forward_score(tdnet_t* n, const float* img, int pos_id, const uint8_t* gt, uint8_t* labels, void* stream) {
    if (!n || !img || !gt) return td_fail("tdnet_forward_score: null argument");
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_SCORE, labels, gt}, stream, "tdnet_forward_score");
}
extern "C" int tdnet_forward_u8_score(tdnet_t* n, const uint8_t* img, int pos_id, const uint8_t* gt, uint8_t* labels, void* stream) {
    if (!n || !img || !gt) return td_fail("tdnet_forward_u8_score: null argument");
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_SCORE, labels, gt}, stream, "tdnet_forward_u8_score");
}
extern "C" int tdnet_labels_score(tdnet_t* n, const uint8_t* labels, const uint8_t* gt, void* stream) {
    if (!n || !labels || !gt) return td_fail("tdnet_labels_score: null argument");
    TD_ON_DEVICE(n, -1);
    TD_NEED_SCORE(n, "tdnet_labels_score");
    TD_TRY(launch_labels_score(labels, n->cfg.nclass, n->H, n->W, gt, n->score.dmap, n->score.cm, (hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
extern "C" int tdnet_score_reset(tdnet_t* n, void* stream) {
    if (!n) return td_fail("tdnet_score_reset: null handle");
    TD_ON_DEVICE(n, -1);
    TD_NEED_SCORE(n, "tdnet_score_reset");
    TD_HIP(hipMemsetAsync(n->score.cm, 0, (size_t)n->score.nclass * n->score.nclass * sizeof(unsigned long long), (hipStream_t)stream));
    return 0;
}
extern "C" int tdnet_score_export(tdnet_t* n, uint64_t* cm_dev, void* stream) {
    if (!n || !cm_dev) return td_fail("tdnet_score_export: null argument");
    TD_ON_DEVICE(n, -1);
    TD_NEED_SCORE(n, "tdnet_score_export");
    TD_HIP(hipMemcpyAsync(cm_dev, n->score.cm, (size_t)n->score.nclass * n->score.nclass * sizeof(unsigned long long), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
extern "C" long tdnet_score_read(tdnet_t* n, uint64_t* cm_host, size_t capacity, void* stream) {
    if (!n || !cm_host) return td_fail("tdnet_score_read: null argument");
    TD_ON_DEVICE(n, -1);
    TD_NEED_SCORE(n, "tdnet_score_read");
    const size_t count = (size_t)n->score.nclass * n->score.nclass;
    if (capacity < count) return td_fail("tdnet_score_read: capacity %zu < %zu", capacity, count);
    TD_HIP(hipStreamSynchronize((hipStream_t)stream));
    TD_HIP(hipMemcpy(cm_host, n->score.cm, count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return (long)count;
}
// ---- confidence out --------------------------------------------------------------------------------------------------------------------
// Plain host state of the handle (no allocation, no synchronisation): the threshold and the label that replaces a rejected one.  A *_conf entry
// passes the values in force when it ENQUEUES its last launch (kernel arguments: a captured graph replays the ones it was captured with).
extern "C" int tdnet_set_confidence(tdnet_t* n, int min_conf, int reject_label) {
    if (!n) return td_fail("tdnet_set_confidence: null handle");
    if (min_conf < 0 || min_conf > 255) return td_fail("tdnet_set_confidence: min_conf = %d must be in 0..255", min_conf);
    if (reject_label < 0 || reject_label > 255) return td_fail("tdnet_set_confidence: reject_label = %d must be in 0..255", reject_label);
    n->min_conf = min_conf;
    n->reject_label = reject_label;
    return 0;
}
// The labels entries with another last launch: the confidence map beside (or, labels == NULL, instead of) the label map.  Same frame, same FIFO
// step, same number of launches.
extern "C" int tdnet_forward_labels_conf(tdnet_t* n, const float* img, int pos_id, uint8_t* labels, uint8_t* conf, void* stream) {
    if (!n || !img || !conf) return td_fail("tdnet_forward_labels_conf: null argument");
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_CONF, labels, nullptr, conf}, stream, "tdnet_forward_labels_conf");
}
extern "C" int tdnet_forward_u8_labels_conf(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* labels, uint8_t* conf, void* stream) {
    if (!n || !img || !conf) return td_fail("tdnet_forward_u8_labels_conf: null argument");
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_CONF, labels, nullptr, conf}, stream, "tdnet_forward_u8_labels_conf");
}
extern "C" int tdnet_logits_conf(tdnet_t* n, const float* logits, uint8_t* labels, uint8_t* conf, void* stream) {
    if (!n || !logits || !conf) return td_fail("tdnet_logits_conf: null argument");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_logits_conf: weights not finalized");
    TD_ON_DEVICE(n, -1);
    TD_TRY(launch_logits_conf_u8(logits, n->cfg.nclass, (long)n->H * n->W, labels, conf, n->min_conf, n->reject_label, (hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
// ---- matte out -------------------------------------------------------------------------------------------------------------------------
// Plain host state of the handle (no allocation, no synchronisation, no weights needed: only cfg.nclass): the class set as 256 membership bits.  A
// *_matte entry passes the words in force when it ENQUEUES its last launch (kernel arguments: a captured graph replays the set it was captured with).
extern "C" int tdnet_set_matte(tdnet_t* n, const uint8_t* classes, int count) {
    if (!n) return td_fail("tdnet_set_matte: null handle");
    if (count < 0 || count > 256) return td_fail("tdnet_set_matte: n = %d must be in 0..256", count);
    if (count > 0 && !classes) return td_fail("tdnet_set_matte: classes is NULL with n = %d", count);
    MatteSet set = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < count; ++i) {
        if (classes[i] >= n->cfg.nclass) return td_fail("tdnet_set_matte: classes[%d] = %d is not a class id (nclass = %d)", i, (int)classes[i], n->cfg.nclass);
        set.w[classes[i] >> 5] |= 1u << (classes[i] & 31);              // duplicates are legal
    }
    n->matte = set;
    n->matte_set = true;
    return 0;
}
// The labels entries with another last launch: the matte beside (or, labels == NULL, instead of) the label map.  Same frame, same FIFO step, same
// number of launches.
extern "C" int tdnet_forward_matte(tdnet_t* n, const float* img, int pos_id, uint8_t* labels, uint8_t* matte, void* stream) {
    if (!n || !img || !matte) return td_fail("tdnet_forward_matte: null argument");
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_MATTE, labels, nullptr, matte}, stream, "tdnet_forward_matte");
}
extern "C" int tdnet_forward_u8_matte(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* labels, uint8_t* matte, void* stream) {
    if (!n || !img || !matte) return td_fail("tdnet_forward_u8_matte: null argument");
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_MATTE, labels, nullptr, matte}, stream, "tdnet_forward_u8_matte");
}
extern "C" int tdnet_logits_matte(tdnet_t* n, const float* logits, uint8_t* labels, uint8_t* matte, void* stream) {
    if (!n || !logits || !matte) return td_fail("tdnet_logits_matte: null argument");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_logits_matte: weights not finalized");
    TD_ON_DEVICE(n, -1);
    TD_TRY(output_configured(n, OUT_MATTE, "tdnet_logits_matte"));
    TD_TRY(launch_logits_matte_u8(logits, n->cfg.nclass, (long)n->H * n->W, labels, matte, n->matte, (hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
// Configuration of the composite output (not a frame call: it may synchronise; idempotent for equal arguments).  Mode and background are plain host state
// (kernel arguments); the index tables are the overlay's, built here if the handle has a byte input, by the byte-input configuration otherwise.
extern "C" int tdnet_set_output_composite(tdnet_t* n, int mode, const uint8_t* bg_rgb) {
    const char* who = "tdnet_set_output_composite";
    if (!n) return td_fail("%s: null handle", who);
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    if (mode != TDNET_COMPOSITE_COLOUR && mode != TDNET_COMPOSITE_ALPHA) return td_fail("%s: mode = %d must be 0 (TDNET_COMPOSITE_COLOUR) or 1 (TDNET_COMPOSITE_ALPHA)", who, mode);
    if (mode == TDNET_COMPOSITE_COLOUR && !bg_rgb) return td_fail("%s: bg_rgb is NULL (the colour mode blends over a background)", who);
    if (mode == TDNET_COMPOSITE_ALPHA && bg_rgb) return td_fail("%s: bg_rgb must be NULL in the alpha mode (nothing is blended)", who);
    TD_ON_DEVICE(n, -1);
    CompositeOutput c;
    c.set = true; c.mode = mode;
    if (bg_rgb) memcpy(c.bg, bg_rgb, 3);
    if (n->u8.set) {
        const size_t before = n->overlay.bytes;
        const int rc = overlay_tables(n->overlay, n->H, n->W, n->u8.Hs, n->u8.Ws, who);
        n->ws_bytes += n->overlay.bytes - before;
        TD_TRY(rc);
    }
    n->comp = c;
    return 0;
}
// What every composite entry checks on the host before anything is enqueued: the configurations exist, the destination in force can take this mode, and
// `out` (or the destination frame's extent) does not overlap the source extent -- the kernel reads the source while it writes the picture.
static int composite_args(const tdnet* n, bool fused, const uint8_t* src, const uint8_t* out, const char* who) {
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    if (fused) TD_TRY(output_configured(n, OUT_COMPOSITE, who));
    else {
        if (!n->comp.set) return td_fail("%s: the composite output is not configured (call tdnet_set_output_composite first)", who);
        if (!n->u8.set) return td_fail("%s: the byte input is not configured (call tdnet_set_input_u8 or one of its siblings first): the composite is written at its source size", who);
    }
    const U8Input& u = n->u8;
    const DstOutput& d = n->dst;
    TD_TRY(composite_dst_check(u, n->comp, d, who));
    if (n->refine.radius) TD_TRY(refine_ready(n->refine, u, who));
    const size_t nout = d.set ? d.extent : (size_t)3 * u.Hs * u.Ws, nsrc = u.extent;
    const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out;
    if (s0 < o0 + nout && o0 < s0 + nsrc) return td_fail("%s: out overlaps the source frame (%zu bytes at %p against %zu bytes at %p)", who, nout, (const void*)out, nsrc, (const void*)src);
    return 0;
}
// The labels entries with another last launch: the composite instead of the label map; the image pointer is the frame's image (first launch) AND the
// composite's source (last launch).  Same frame, same FIFO step, same number of launches.
extern "C" int tdnet_forward_u8_composite(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* out, void* stream) {
    if (!n || !img || !out) return td_fail("tdnet_forward_u8_composite: null argument");
    TD_TRY(composite_args(n, true, img, out, "tdnet_forward_u8_composite"));
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_COMPOSITE, out, nullptr, nullptr, img}, stream, "tdnet_forward_u8_composite");
}
// the unfused form: from a matte map [H][W] the caller holds; needs no class set
extern "C" int tdnet_matte_composite(tdnet_t* n, const uint8_t* matte, const uint8_t* img, uint8_t* out, void* stream) {
    if (!n || !matte || !img || !out) return td_fail("tdnet_matte_composite: null argument");
    TD_TRY(composite_args(n, false, img, out, "tdnet_matte_composite"));
    TD_ON_DEVICE(n, -1);
    if (n->refine.radius) TD_TRY(run_refined_composite(nullptr, 0, 0, 0, matte, n->matte, n->overlay, n->u8, img, n->comp, n->dst, n->refine, out, (hipStream_t)stream, "tdnet_matte_composite"));
    else
    TD_TRY(launch_composite(nullptr, 0, 0, 0, matte, n->matte, n->overlay, n->u8, img, n->comp, n->dst, out, (hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
// ---- refined matte ---------------------------------------------------------------------------------------------------------------------
// Configuration (not a frame call: it may allocate and synchronise; idempotent for equal arguments; per handle; either order with the byte-input
// configuration: the workspace follows the source size and is allocated here if the handle has a byte input, by that configuration otherwise).  radius 0 = off,
// the default: the composite entries are then what they are without this call.  A failed call leaves the previous state in force.
extern "C" int tdnet_set_matte_refine(tdnet_t* n, int radius, int eps) {
    const char* who = "tdnet_set_matte_refine";
    if (!n) return td_fail("%s: null handle", who);
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    if (radius != 0) TD_TRY(refine_range_check(radius, eps, who));
    TD_ON_DEVICE(n, -1);
    if (radius == 0) {
        if (n->refine.luma) { TD_HIP(hipDeviceSynchronize()); n->ws_bytes -= n->refine.bytes; refine_free(n->refine); }
        n->refine.radius = n->refine.eps = 0;
        return 0;
    }
    if (n->u8.set) {
        RefineState& r = n->refine;
        if (r.luma && (r.Hs != n->u8.Hs || r.Ws != n->u8.Ws)) TD_HIP(hipDeviceSynchronize());
        const size_t ob = n->overlay.bytes, rb = r.bytes;
        int rc = overlay_tables(n->overlay, n->H, n->W, n->u8.Hs, n->u8.Ws, who);
        n->ws_bytes += n->overlay.bytes - ob;
        if (!rc) rc = overlay_set_swap(n->overlay, n->u8.swap, who);
        if (!rc) rc = refine_alloc(r, n->u8.Hs, n->u8.Ws, who);
        n->ws_bytes += r.bytes - rb;
        TD_TRY(rc);
    }
    n->refine.radius = radius;
    n->refine.eps = eps;
    return 0;
}
// What the two refined-matte frame entries check on the host before anything is enqueued
static int refined_args(const tdnet* n, const uint8_t* src, const uint8_t* out, const char* who) {
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    TD_TRY(output_configured(n, OUT_MATTE_REFINED, who));
    const size_t nout = (size_t)n->u8.Hs * n->u8.Ws, nsrc = n->u8.extent;
    const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out;
    if (s0 < o0 + nout && o0 < s0 + nsrc) return td_fail("%s: out overlaps the source frame (%zu bytes at %p against %zu bytes at %p)", who, nout, (const void*)out, nsrc, (const void*)src);
    return 0;
}
// The labels entries with the other end: the refined matte [Hs][Ws] at the source's size; tdnet_last_launch_count = the label entry's + 2
extern "C" int tdnet_forward_u8_matte_refined(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* out, void* stream) {
    if (!n || !img || !out) return td_fail("tdnet_forward_u8_matte_refined: null argument");
    TD_TRY(refined_args(n, img, out, "tdnet_forward_u8_matte_refined"));
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_MATTE_REFINED, out, nullptr, nullptr, img}, stream, "tdnet_forward_u8_matte_refined");
}
// The operator on maps the caller holds (td_refine.h): the handle gives the device, nothing else -- no configuration, no weights.  Every check is made
// before the first launch; the two launches only enqueue.
extern "C" size_t tdnet_refine_scratch_bytes(int rows, int cols) { return refine_scratch_bytes(rows, cols); }
extern "C" int tdnet_refine_matte(tdnet_t* n, const uint8_t* guide, size_t guide_pitch, const uint8_t* matte, size_t matte_pitch, uint8_t* out, size_t out_pitch,
                                  int rows, int cols, int radius, int eps, void* scratch, void* stream) {
    const char* who = "tdnet_refine_matte";
    if (!n) return td_fail("%s: null handle", who);
    TD_TRY(refine_args_check(guide, guide_pitch, matte, matte_pitch, out, out_pitch, true, rows, cols, radius, eps, scratch, who));
    TD_ON_DEVICE(n, -1);
    launch_refine_coeff(guide, guide_pitch, matte, matte_pitch, rows, cols, radius, eps, scratch, (hipStream_t)stream);
    launch_refine_apply(guide, guide_pitch, out, out_pitch, rows, cols, radius, scratch, (hipStream_t)stream);
    TD_HIP(hipGetLastError());
    return 0;
}
// ---- split frame + cache transport (path-parallel single stream) ------------------------------------
// Rank g of a path-parallel group serves the frames t = g (mod W): it encodes its frame as soon as the image is there, publishes
// the resulting cache entry, receives the entries of the frames in between from its peers (in frame order) and only then
// propagates.  The FIFO of every rank therefore holds exactly what the sequential td4_psp18.py:123-154 would hold.
static int encode_impl(tdnet* n, const FrameInput& img, int pos_id, void* stream, const char* who) {
    TD_ON_DEVICE(n, -1);
    if (frame_checks(n, pos_id, who, &img)) return -1;
    if (n->cfg.model == 1) return td_fail("%s: pspnet has no temporal state; use tdnet_forward", who);
    if (n->pending_slot >= 0) return td_fail("%s: the previous encoded frame has not been propagated", who);
    n->nrec = 0;
    n->failed = false;
    TD_TRY(place_chain_stream(n, (hipStream_t)stream));
    LaunchCount count_(n);
    if (encode_frame(n, n->paths[pos_id], img, (hipStream_t)stream)) {  // a failed frame is dropped (as in tdnet_forward): no entry stays pending
        rejoin_streams(n, (hipStream_t)stream);
        n->pending_slot = n->pending_pos = -1;
        return -1;
    }
    n->pending_pos = pos_id;
    TD_HIP(hipGetLastError());
    return 0;
}
extern "C" int tdnet_encode(tdnet_t* n, const float* img, int pos_id, void* stream) {
    if (!n || !img) return td_fail("tdnet_encode: null argument");
    return encode_impl(n, frame_input_f32(img), pos_id, stream, "tdnet_encode");
}
extern "C" int tdnet_encode_u8(tdnet_t* n, const uint8_t* img, int pos_id, void* stream) {
    if (!n || !img) return td_fail("tdnet_encode_u8: null argument");
    return encode_impl(n, frame_input_u8(n, img), pos_id, stream, "tdnet_encode_u8");
}
static int propagate_lowres(tdnet* n, hipStream_t s) {
    if (n->pending_slot < 0) return td_fail("tdnet_propagate: no encoded frame (call tdnet_encode first)");
    PathLayers& L = n->paths[n->pending_pos];
    const bool steady = (int)n->fifo.size() >= n->FIFO;
    if ((steady && launch_chain_now(n, L, s)) || finish_frame(n, L, steady, s)) { rejoin_streams(n, s); n->pending_slot = n->pending_pos = -1; return -1; }
    return 0;
}
static const FrameSource pending_frame = {nullptr, -1};
extern "C" int tdnet_propagate(tdnet_t* n, float* logits, void* stream) {
    if (!n || !logits) return td_fail("tdnet_propagate: null argument");
    return frame_out(n, pending_frame, FrameOutput{OUT_LOGITS, logits}, stream, "tdnet_propagate");
}
extern "C" int tdnet_propagate_labels(tdnet_t* n, int32_t* labels, void* stream) {
    if (!n || !labels) return td_fail("tdnet_propagate_labels: null argument");
    return frame_out(n, pending_frame, FrameOutput{OUT_LABELS_I32, labels}, stream, "tdnet_propagate_labels");
}
extern "C" int tdnet_propagate_labels_u8(tdnet_t* n, uint8_t* labels, void* stream) {
    if (!n || !labels) return td_fail("tdnet_propagate_labels_u8: null argument");
    return frame_out(n, pending_frame, FrameOutput{OUT_LABELS_U8, labels}, stream, "tdnet_propagate_labels_u8");
}
extern "C" int tdnet_propagate_rgb(tdnet_t* n, uint8_t* rgb, void* stream) {
    if (!n || !rgb) return td_fail("tdnet_propagate_rgb: null argument");
    return frame_out(n, pending_frame, FrameOutput{OUT_RGB, rgb}, stream, "tdnet_propagate_rgb");
}
extern "C" int tdnet_propagate_overlay(tdnet_t* n, const uint8_t* img, uint8_t* out, void* stream) {
    if (!n || !img || !out) return td_fail("tdnet_propagate_overlay: null argument");
    TD_TRY(overlay_args(n, img, out, "tdnet_propagate_overlay"));
    return frame_out(n, pending_frame, FrameOutput{OUT_OVERLAY, out, nullptr, nullptr, img}, stream, "tdnet_propagate_overlay");
}
extern "C" int tdnet_propagate_score(tdnet_t* n, const uint8_t* gt, uint8_t* labels, void* stream) {
    if (!n || !gt) return td_fail("tdnet_propagate_score: null argument");
    return frame_out(n, pending_frame, FrameOutput{OUT_SCORE, labels, gt}, stream, "tdnet_propagate_score");
}
extern "C" int tdnet_propagate_labels_conf(tdnet_t* n, uint8_t* labels, uint8_t* conf, void* stream) {
    if (!n || !conf) return td_fail("tdnet_propagate_labels_conf: null argument");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_propagate_labels_conf: weights not finalized");   // (its siblings leave this to "no encoded frame")
    return frame_out(n, pending_frame, FrameOutput{OUT_CONF, labels, nullptr, conf}, stream, "tdnet_propagate_labels_conf");
}
extern "C" int tdnet_propagate_matte(tdnet_t* n, uint8_t* labels, uint8_t* matte, void* stream) {
    if (!n || !matte) return td_fail("tdnet_propagate_matte: null argument");
    if (!n->finalized || !n->ws_ready) return td_fail("tdnet_propagate_matte: weights not finalized");
    return frame_out(n, pending_frame, FrameOutput{OUT_MATTE, labels, nullptr, matte}, stream, "tdnet_propagate_matte");
}
extern "C" int tdnet_propagate_matte_refined(tdnet_t* n, const uint8_t* img, uint8_t* out, void* stream) {
    if (!n || !img || !out) return td_fail("tdnet_propagate_matte_refined: null argument");
    TD_TRY(refined_args(n, img, out, "tdnet_propagate_matte_refined"));
    return frame_out(n, pending_frame, FrameOutput{OUT_MATTE_REFINED, out, nullptr, nullptr, img}, stream, "tdnet_propagate_matte_refined");
}
extern "C" int tdnet_propagate_composite(tdnet_t* n, const uint8_t* img, uint8_t* out, void* stream) {
    if (!n || !img || !out) return td_fail("tdnet_propagate_composite: null argument");
    TD_TRY(composite_args(n, true, img, out, "tdnet_propagate_composite"));
    return frame_out(n, pending_frame, FrameOutput{OUT_COMPOSITE, out, nullptr, nullptr, img}, stream, "tdnet_propagate_composite");
}
// ---- regions out -----------------------------------------------------------------------------------------------------------------------
// Configuration of the regions output (not a frame call: it may synchronise; idempotent for equal arguments; per handle).  The class set, the connectivity
// and the two limits are plain host state, passed as kernel arguments when an entry ENQUEUES; the workspace (three int32 maps, a byte map, the block
// counts) lives in memory this handle owns.  A failed call changes nothing.
extern "C" int tdnet_set_regions(tdnet_t* n, const uint8_t* classes, int count, int connectivity, int max_regions, int min_area) {
    const char* who = "tdnet_set_regions";
    if (!n) return td_fail("%s: null handle", who);
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    if (count < 0 || count > 256) return td_fail("%s: n = %d must be in 0..256", who, count);
    if (count > 0 && !classes) return td_fail("%s: classes is NULL with n = %d", who, count);
    if (connectivity != 4 && connectivity != 8) return td_fail("%s: connectivity = %d must be 4 or 8", who, connectivity);
    if (max_regions < 1 || max_regions > 65536) return td_fail("%s: max_regions = %d must be in 1..65536", who, max_regions);
    if (min_area < 1) return td_fail("%s: min_area = %d must be at least 1", who, min_area);
    MatteSet set = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < count; ++i) {
        if (classes[i] >= n->cfg.nclass) return td_fail("%s: classes[%d] = %d is not a class id (nclass = %d)", who, i, (int)classes[i], n->cfg.nclass);
        set.w[classes[i] >> 5] |= 1u << (classes[i] & 31);              // duplicates are legal
    }
    TD_ON_DEVICE(n, -1);
    if (!n->regions.parent) {                                          // the workspace depends on the handle's size alone: allocated once
        const size_t before = n->regions.bytes;
        TD_TRY(regions_alloc(n->regions, n->H, n->W, who));
        n->ws_bytes += n->regions.bytes - before;
    }
    RegionsOutput& r = n->regions;
    r.classes = set; r.conn = connectivity; r.max_regions = max_regions; r.min_area = min_area;
    r.set = true;
    return 0;
}
extern "C" size_t tdnet_regions_bytes(const tdnet_t* n) { return n && n->regions.set ? regions_table_bytes(n->regions.max_regions) : 0; }
// What every regions entry checks on the host before anything is enqueued: the configuration exists and the table can be addressed
static int regions_args(const tdnet* n, const void* table, const char* who) {
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    TD_TRY(output_configured(n, OUT_REGIONS, who));
    return regions_table_check(table, who);
}
// The labels entries with another tail: the frame's label launch is the first of the TDNET_REGIONS_LAUNCHES region launches.  Same frame, same FIFO step;
// labels and ids may each be NULL.
extern "C" int tdnet_forward_regions(tdnet_t* n, const float* img, int pos_id, uint8_t* labels, int32_t* ids, void* regions_dev, void* stream) {
    if (!n || !img) return td_fail("tdnet_forward_regions: null argument");
    TD_TRY(regions_args(n, regions_dev, "tdnet_forward_regions"));
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_REGIONS, labels, nullptr, nullptr, nullptr, ids, regions_dev}, stream, "tdnet_forward_regions");
}
extern "C" int tdnet_forward_u8_regions(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* labels, int32_t* ids, void* regions_dev, void* stream) {
    if (!n || !img) return td_fail("tdnet_forward_u8_regions: null argument");
    TD_TRY(regions_args(n, regions_dev, "tdnet_forward_u8_regions"));
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_REGIONS, labels, nullptr, nullptr, nullptr, ids, regions_dev}, stream, "tdnet_forward_u8_regions");
}
extern "C" int tdnet_propagate_regions(tdnet_t* n, uint8_t* labels, int32_t* ids, void* regions_dev, void* stream) {
    if (!n) return td_fail("tdnet_propagate_regions: null argument");
    TD_TRY(regions_args(n, regions_dev, "tdnet_propagate_regions"));
    return frame_out(n, pending_frame, FrameOutput{OUT_REGIONS, labels, nullptr, nullptr, nullptr, ids, regions_dev}, stream, "tdnet_propagate_regions");
}
// the unfused form: from a uint8 label map [H][W] the caller holds (at any byte address); needs no frame state beyond the configuration
extern "C" int tdnet_labels_regions(tdnet_t* n, const uint8_t* labels, int32_t* ids, void* regions_dev, void* stream) {
    if (!n || !labels) return td_fail("tdnet_labels_regions: null argument");
    TD_TRY(regions_args(n, regions_dev, "tdnet_labels_regions"));
    TD_ON_DEVICE(n, -1);
    TD_TRY(run_regions(nullptr, n->cfg.nclass, 0, 0, n->H, n->W, labels, nullptr, ids, regions_dev, n->regions, (hipStream_t)stream, "tdnet_labels_regions"));
    TD_HIP(hipGetLastError());
    return 0;
}
// ---- tracks out --------------------------------------------------------------------------------------------------------------------------
// Configuration of the tracks output (not a frame call: it may synchronise; idempotent; per handle; independent of the order of the other tdnet_set_*
// calls).  The state blob is sized from the handle alone (H, W and the ceiling of 65536 regions) and allocated, zeroed, ONCE: a second call only
// changes min_overlap and leaves the tracks as they are.  A failed call changes nothing.
extern "C" int tdnet_set_tracks(tdnet_t* n, int min_overlap) {
    const char* who = "tdnet_set_tracks";
    if (!n) return td_fail("%s: null handle", who);
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    if (min_overlap < 1) return td_fail("%s: min_overlap = %d must be at least 1", who, min_overlap);
    TD_ON_DEVICE(n, -1);
    if (!n->tracks.blob) {
        const size_t before = n->tracks.bytes;
        TD_TRY(tracks_alloc(n->tracks, n->H, n->W, who));
        n->ws_bytes += n->tracks.bytes - before;
    }
    n->tracks.min_overlap = min_overlap;
    n->tracks.set = true;
    return 0;
}
extern "C" size_t tdnet_tracks_bytes(const tdnet_t* n) { return n && n->regions.set && n->tracks.set ? tracks_table_bytes(n->regions.max_regions) : 0; }
// What every tracks entry checks on the host before anything is enqueued: both configurations exist and both tables can be addressed
static int tracks_args(const tdnet* n, const void* regions_dev, const void* tracks_dev, const char* who) {
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    TD_TRY(output_configured(n, OUT_TRACKS, who));
    TD_TRY(regions_table_check(regions_dev, who));
    return tracks_table_check(tracks_dev, who);
}
// The regions entries with the tracking launches behind them.  Same frame, same FIFO step, same labels, ids and regions table; labels, ids and track_ids
// may each be NULL.
extern "C" int tdnet_forward_tracks(tdnet_t* n, const float* img, int pos_id, uint8_t* labels, int32_t* ids, void* regions_dev, int32_t* track_ids, void* tracks_dev,
                                    void* stream) {
    if (!n || !img) return td_fail("tdnet_forward_tracks: null argument");
    TD_TRY(tracks_args(n, regions_dev, tracks_dev, "tdnet_forward_tracks"));
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_TRACKS, labels, nullptr, nullptr, nullptr, ids, regions_dev, track_ids, tracks_dev}, stream,
                     "tdnet_forward_tracks");
}
extern "C" int tdnet_forward_u8_tracks(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* labels, int32_t* ids, void* regions_dev, int32_t* track_ids, void* tracks_dev,
                                       void* stream) {
    if (!n || !img) return td_fail("tdnet_forward_u8_tracks: null argument");
    TD_TRY(tracks_args(n, regions_dev, tracks_dev, "tdnet_forward_u8_tracks"));
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_TRACKS, labels, nullptr, nullptr, nullptr, ids, regions_dev, track_ids, tracks_dev}, stream,
                     "tdnet_forward_u8_tracks");
}
extern "C" int tdnet_propagate_tracks(tdnet_t* n, uint8_t* labels, int32_t* ids, void* regions_dev, int32_t* track_ids, void* tracks_dev, void* stream) {
    if (!n) return td_fail("tdnet_propagate_tracks: null argument");
    TD_TRY(tracks_args(n, regions_dev, tracks_dev, "tdnet_propagate_tracks"));
    return frame_out(n, pending_frame, FrameOutput{OUT_TRACKS, labels, nullptr, nullptr, nullptr, ids, regions_dev, track_ids, tracks_dev}, stream, "tdnet_propagate_tracks");
}
// the unfused form: from a uint8 label map [H][W] the caller holds (at any byte address)
extern "C" int tdnet_labels_tracks(tdnet_t* n, const uint8_t* labels, int32_t* ids, void* regions_dev, int32_t* track_ids, void* tracks_dev, void* stream) {
    const char* who = "tdnet_labels_tracks";
    if (!n || !labels) return td_fail("%s: null argument", who);
    TD_TRY(tracks_args(n, regions_dev, tracks_dev, who));
    TD_ON_DEVICE(n, -1);
    int32_t* cur = ids ? ids : n->tracks.st.cur;
    TD_TRY(run_regions(nullptr, n->cfg.nclass, 0, 0, n->H, n->W, labels, nullptr, cur, regions_dev, n->regions, (hipStream_t)stream, who));
    TD_TRY(run_tracks(n->H, n->W, cur, regions_dev, track_ids, tracks_dev, n->tracks.st, n->regions.max_regions, n->tracks.min_overlap, (hipStream_t)stream, who));
    TD_HIP(hipGetLastError());
    return 0;
}
// Forget every track: enqueued on `stream` (one launch), ordered like a frame entry.  The next tracked frame's regions are all born, from track 1.
extern "C" int tdnet_tracks_reset(tdnet_t* n, void* stream) {
    if (!n) return td_fail("tdnet_tracks_reset: null handle");
    if (!n->tracks.set) return td_fail("tdnet_tracks_reset: the tracks output is not configured (call tdnet_set_tracks first)");
    TD_ON_DEVICE(n, -1);
    TD_LAUNCH(k_tracks_reset, dim3(1), dim3(64), 0, (hipStream_t)stream, n->tracks.st);
    TD_HIP(hipGetLastError());
    return 0;
}
// ---- runs out ----------------------------------------------------------------------------------------------------------------------------
// Configuration of the runs output (not a frame call: it may synchronise; idempotent for equal arguments; per handle).  max_runs is plain host state, passed
// as a kernel argument when an entry ENQUEUES; the workspace (a byte map, the block counts) depends on the handle's size alone and is allocated once.  A
// failed call changes nothing.
extern "C" int tdnet_set_runs(tdnet_t* n, int max_runs) {
    const char* who = "tdnet_set_runs";
    if (!n) return td_fail("%s: null handle", who);
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    TD_TRY(regions_size_check(n->H, n->W, who));
    if (max_runs < 1 || (long)max_runs > (long)n->H * n->W) return td_fail("%s: max_runs = %d must be in 1..%ld (H W)", who, max_runs, (long)n->H * n->W);
    TD_ON_DEVICE(n, -1);
    if (!n->runs.blk) {
        const size_t before = n->runs.bytes;
        TD_TRY(runs_alloc(n->runs, n->H, n->W, true, who));
        n->ws_bytes += n->runs.bytes - before;
    }
    n->runs.max_runs = max_runs;
    n->runs.set = true;
    return 0;
}
extern "C" size_t tdnet_runs_bytes(const tdnet_t* n) { return n && n->runs.set ? runs_table_bytes(n->runs.max_runs) : 0; }
// What every runs entry checks on the host before anything is enqueued: the configuration exists and the table can be addressed
static int runs_args(const tdnet* n, const void* table, const char* who) {
    if (!n->finalized || !n->ws_ready) return td_fail("%s: weights not finalized", who);
    TD_TRY(output_configured(n, OUT_RUNS, who));
    return runs_table_check(table, who);
}
// The labels entries with the coding launches behind the label launch.  Same frame, same FIFO step, same labels; labels may be NULL.
extern "C" int tdnet_forward_runs(tdnet_t* n, const float* img, int pos_id, uint8_t* labels, void* runs_dev, void* stream) {
    if (!n || !img) return td_fail("tdnet_forward_runs: null argument");
    TD_TRY(runs_args(n, runs_dev, "tdnet_forward_runs"));
    return frame_out(n, frame_input_f32(img), pos_id, FrameOutput{OUT_RUNS, labels, nullptr, nullptr, nullptr, nullptr, runs_dev}, stream, "tdnet_forward_runs");
}
extern "C" int tdnet_forward_u8_runs(tdnet_t* n, const uint8_t* img, int pos_id, uint8_t* labels, void* runs_dev, void* stream) {
    if (!n || !img) return td_fail("tdnet_forward_u8_runs: null argument");
    TD_TRY(runs_args(n, runs_dev, "tdnet_forward_u8_runs"));
    return frame_out(n, frame_input_u8(n, img), pos_id, FrameOutput{OUT_RUNS, labels, nullptr, nullptr, nullptr, nullptr, runs_dev}, stream, "tdnet_forward_u8_runs");
}
extern "C" int tdnet_propagate_runs(tdnet_t* n, uint8_t* labels, void* runs_dev, void* stream) {
    if (!n) return td_fail("tdnet_propagate_runs: null argument");
    TD_TRY(runs_args(n, runs_dev, "tdnet_propagate_runs"));
    return frame_out(n, pending_frame, FrameOutput{OUT_RUNS, labels, nullptr, nullptr, nullptr, nullptr, runs_dev}, stream, "tdnet_propagate_runs");
}
// the unfused forms: from a uint8 map at any byte address, or an int32 map (the id map or the track map a regions / tracks entry wrote on the same stream)
static int runs_unfused(tdnet* n, const void* map, bool i32, void* runs_dev, void* stream, const char* who) {
    if (!n || !map) return td_fail("%s: null argument", who);
    TD_TRY(runs_args(n, runs_dev, who));
    TD_ON_DEVICE(n, -1);
    TD_TRY(run_runs(n->H, n->W, map, i32, runs_dev, n->runs, n->runs.max_runs, (hipStream_t)stream, who));
    TD_HIP(hipGetLastError());
    return 0;
}
extern "C" int tdnet_labels_runs(tdnet_t* n, const uint8_t* labels, void* runs_dev, void* stream) { return runs_unfused(n, labels, false, runs_dev, stream, "tdnet_labels_runs"); }
extern "C" int tdnet_ids_runs(tdnet_t* n, const int32_t* ids, void* runs_dev, void* stream) { return runs_unfused(n, ids, true, runs_dev, stream, "tdnet_ids_runs"); }
// the way back: one launch
static int runs_decode(tdnet* n, const void* runs_dev, int fill, void* out, bool i32, void* stream, const char* who) {
    if (!n || !out) return td_fail("%s: null argument", who);
    TD_TRY(runs_args(n, runs_dev, who));
    TD_ON_DEVICE(n, -1);
    TD_TRY(run_runs_decode(n->H, n->W, runs_dev, fill, out, i32, n->runs, n->runs.max_runs, (hipStream_t)stream, who));
    TD_HIP(hipGetLastError());
    return 0;
}
extern "C" int tdnet_runs_labels(tdnet_t* n, const void* runs_dev, int fill, uint8_t* labels, void* stream) { return runs_decode(n, runs_dev, fill, labels, false, stream, "tdnet_runs_labels"); }
extern "C" int tdnet_runs_ids(tdnet_t* n, const void* runs_dev, int fill, int32_t* ids, void* stream) { return runs_decode(n, runs_dev, fill, ids, true, stream, "tdnet_runs_ids"); }
extern "C" int tdnet_cache_dims(const tdnet_t* n, int* Lk, int* dk, int* dv) {
    if (!n) return td_fail("tdnet_cache_dims: null handle");
    if (n->cfg.model == 1) return td_fail("tdnet_cache_dims: pspnet has no cache");
    if (Lk) *Lk = n->Lk;
    if (dk) *dk = 64;
    if (dv) *dv = n->DV;
    return 0;
}
extern "C" int tdnet_cache_export(tdnet_t* n, float* q, float* k, float* v, void* stream) {
    if (!n || !q || !k || !v) return td_fail("tdnet_cache_export: null argument");
    if (n->pending_slot < 0) return td_fail("tdnet_cache_export: no encoded frame (call tdnet_encode first)");
    TD_ON_DEVICE(n, -1);
    const CacheSlot& c = n->slots[n->pending_slot];
    hipStream_t s = (hipStream_t)stream;
    TD_HIP(hipMemcpyAsync(q, c.q, (size_t)n->Lk * 64 * sizeof(float), hipMemcpyDeviceToDevice, s));
    TD_HIP(hipMemcpyAsync(k, c.k, (size_t)n->Lk * 64 * sizeof(float), hipMemcpyDeviceToDevice, s));
    TD_HIP(hipMemcpyAsync(v, c.v, (size_t)n->Lk * n->DV * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
extern "C" int tdnet_cache_push(tdnet_t* n, const float* q, const float* k, const float* v, void* stream) {
    if (!n || !q || !k || !v) return td_fail("tdnet_cache_push: null argument");
    if (n->cfg.model == 1) return td_fail("tdnet_cache_push: pspnet has no cache");
    TD_ON_DEVICE(n, -1);
    const int slot = free_slot(n);
    if (slot < 0) return td_fail("internal: no free cache slot");
    const CacheSlot& c = n->slots[slot];
    hipStream_t s = (hipStream_t)stream;
    TD_HIP(hipMemcpyAsync(c.q, q, (size_t)n->Lk * 64 * sizeof(float), hipMemcpyDeviceToDevice, s));
    TD_HIP(hipMemcpyAsync(c.k, k, (size_t)n->Lk * 64 * sizeof(float), hipMemcpyDeviceToDevice, s));
    TD_HIP(hipMemcpyAsync(c.v, v, (size_t)n->Lk * n->DV * sizeof(float), hipMemcpyDeviceToDevice, s));
    fifo_commit(n, slot);
    return 0;
}
extern "C" int tdnet_reset(tdnet_t* n) {
    if (!n) return td_fail("tdnet_reset: null handle");
    n->fifo.clear();
    n->last_slot = -1;
    n->pending_slot = n->pending_pos = -1;
    return 0;
}
extern "C" int tdnet_fifo_len(const tdnet_t* n) { return n ? (int)n->fifo.size() : -1; }

// ---------------------------------------------------------------------------------------------------------------
// introspection
// ---------------------------------------------------------------------------------------------------------------
extern "C" long tdnet_get_stage(tdnet_t* n, const char* name, float* host, size_t capacity) {
    if (!n || !name || !host) return td_fail("tdnet_get_stage: null argument");
    TD_ON_DEVICE(n, -1);
    const std::string s = name;
    const float* src = nullptr;
    long rows = n->Lq, C = 0;
    bool nhwc_map = true, planar = false;
    if (s == "c4") { src = n->c4 ? n->c4 : n->bx; C = n->C; }
    else if (s == "z") { src = n->z; C = n->cfg.model == 1 ? 2 * n->C : n->C; }
    else if (s == "lowres") { src = n->lowres; C = n->cfg.nclass; planar = true; }
    else if (n->cfg.model == 1) return td_fail("tdnet_get_stage: stage \"%s\" does not exist in the single-frame PSPNet", name);
    else if (s == "v_cur") { src = n->v_cur; C = n->DV; }
    else if (s == "feat") { src = n->feat_is_vcur ? n->v_cur : n->feat; C = n->DV; }   // warm-up: feat = v_cur (td4_psp18.py:142-143)
    else if (s == "ln") { src = n->ln; C = n->DV; }
    else if (s == "q_cur") { src = n->q_cur; C = 64; nhwc_map = false; }
    else if (s == "cache_q" || s == "cache_k" || s == "cache_v") {
        if (n->last_slot < 0) return td_fail("tdnet_get_stage: no frame cached yet");
        const CacheSlot& c = n->slots[n->last_slot];
        src = s == "cache_q" ? c.q : s == "cache_k" ? c.k : c.v;
        C = s == "cache_v" ? n->DV : 64; rows = n->Lk; nhwc_map = false;
    } else return td_fail("tdnet_get_stage: unknown stage \"%s\"", name);
    const size_t count = (size_t)rows * C;
    if (capacity < count) return td_fail("tdnet_get_stage: capacity %zu < %zu", capacity, count);
    TD_HIP(hipDeviceSynchronize());
    if (s == "ln" && n->ln_pending) {                                  // fusion bit 4 skipped this map: materialise it now, same arithmetic
        const PathLayers& PL = n->paths[n->ln_path];
        TD_LAUNCH(k_ln_apply, dim3(td_grid_for((long)n->Lq * (n->DV / 4))), dim3(256), 0, (hipStream_t)0, (const float*)(n->feat_is_vcur ? n->v_cur : n->feat),
                  (const float*)n->ln_mean, (const float*)n->ln_rstd, (const float*)PL.d_ln_g, (const float*)PL.d_ln_b, n->ln, n->Lq, n->DV);
        TD_HIP(hipDeviceSynchronize());
        n->ln_pending = false;
    }
    if (s == "z" && n->z_pending) {                                    // fusion bit 2097152 skipped this map: assemble it now from c4 and the pooled features, same kernel
        launch_ppm_assemble(n->c4, n->ppmfeat, n->z, n->h, n->w, n->C, n->paths[n->z_path].pid * (n->C / 2), n->C / 2, n->C / 8, (hipStream_t)0);
        TD_HIP(hipDeviceSynchronize());
        n->z_pending = false;
    }
    if (nhwc_map && !planar) {                                         // [HW][C] -> [C][HW] like the reference's NCHW maps
        TD_LAUNCH(k_nhwc_to_nchw, dim3(td_grid_for((long)count)), dim3(256), 0, (hipStream_t)0, src, n->stage_tmp, rows, (int)C);
        TD_HIP(hipDeviceSynchronize());
        TD_HIP(hipMemcpy(host, n->stage_tmp, count * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        TD_HIP(hipMemcpy(host, src, count * sizeof(float), hipMemcpyDeviceToHost));
    }
    return (long)count;
}
extern "C" double tdnet_flops_per_frame(const tdnet_t* n) { return n && n->finalized ? n->flops_frame : -1.0; }

extern "C" int tdnet_get_opts(const tdnet_t* n, tdnet_opts* out) {
    if (!n || !out) return td_fail("tdnet_get_opts: null argument");
    *out = n->opts;
    return 0;
}

extern "C" int tdnet_set_profiling(tdnet_t* n, int on) {
    if (!n) return td_fail("tdnet_set_profiling: null handle");
    n->prof = on != 0;
    n->nrec = 0;
    return 0;
}
// which: 0 conv/GEMM kernels, 1 attention kernels, 2 everything else, 3 the dominant kernel only (128x128-tile 3x3 igemm / LDS-DMA conv /
// Winograd GEMM), 4 every 3x3 conv that reads an fp16 map (the fp16 mode's fixed roofline set).
// mode : 0 -> summed device ms, 1 -> summed algorithmic FLOP, 2 -> launch count
static double prof_query(const tdnet* n, int which, int mode) {
    if (!n || !n->prof || n->nrec == 0) return -1.0;
    double ms = 0.0, fl = 0.0, cnt = 0.0;
    int domkind = 1;                                                   // the Winograd GEMM is the dominant kernel whenever it runs
    for (size_t i = 0; i < n->nrec; ++i) if ((n->recs[i].dominant & 3) == 2) domkind = 2;
    for (size_t i = 0; i < n->nrec; ++i) {
        const ProfRec& r = n->recs[i];
        const bool take = which == 3 ? (r.family == 0 && (r.dominant & 3) == domkind) : which == 4 ? (r.family == 0 && (r.dominant & 4) != 0) : r.family == which;
        if (!take) continue;
        if (mode == 0) {
            hipEventSynchronize(r.e1);
            float t = 0.f;
            hipEventElapsedTime(&t, r.e0, r.e1);
            ms += t;
        }
        fl += r.flops; cnt += 1.0;
    }
    return mode == 0 ? ms : mode == 1 ? fl : cnt;
}
extern "C" double tdnet_last_ms(const tdnet_t* n, int which) { return prof_query(n, which, 0); }
extern "C" double tdnet_last_flops(const tdnet_t* n, int which) { return prof_query(n, which, 1); }
extern "C" double tdnet_last_launches(const tdnet_t* n, int which) { return prof_query(n, which, 2); }

