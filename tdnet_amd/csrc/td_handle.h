// td_handle.h -- host-side types of libtdnet_hip.so: error reporting, the architecture description, a device conv layer, the WEIGHT BLOCK
// (folded + packed weights of all paths, shared by every handle created from it) and the HANDLE (workspace, K/Q/V FIFO, streams).
//
// Split of the former td_model.hip monolith (round 5):
//   td_handle.h    this file
//   td_weights.h   strict state_dict inventory, BN folding (fp64), plan_conv (which kernel each conv runs on, decided once), packing, upload,
//                  the row-parity plan, workspace allocation
//   td_launch.h    one launch helper per operator (conv / Winograd conv / attention / LayerNorm / pyramid / stem / classifier): a switch on
//                  the layer's planned route; one per output form, and emit_output, a frame's last launch
//   td_frame.h     the per-frame kernel sequence: FIFO, cache-only attention chain, row-parity chains, encode / finish, stream placement
//   td_ingest.h    (kernels) uint8 image in; the host side of its tables is at the end of this file
//   td_out.h       (kernels) the output stage behind the low-resolution logits: upsample, argmax, int32 / uint8 labels, colour map out (the
//                  host side of its tables is at the end of this file), and the one class loop td_score.h and td_conf.h share with them
//   td_score.h     (kernels) score out: the confusion matrix against ground truth; its host side is at the end of this file too
//   td_conf.h      (kernels) confidence out: the softmax probability of the label as a byte, rejection of low-confidence labels
//   td_matte.h     (kernels) matte out: the softmax mass of a class set as a byte
//   td_regions.h   (kernels) regions out: connected components of a class set with boxes; its workspace's host side is at the end of this file
//   td_tracks.h    (kernels) tracks out: region identity across frames by pixel overlap; its state's host side is at the end of this file
//   td_runs.h      (kernels) runs out: a label or id map as a run-length table, and back; its workspace's host side is at the end of this file
//   td_ops_test.h  single-operator entry points for the tests + roofline / tuning probes (not on the product path)
//   td_model.hip   the translation unit: the C ABI of include/tdnet.h
#pragma once
#include "../../include/tdnet.h"
#include "td_device.h"
#include "td_conv.h"
#include "td_conv_h.h"
#include "td_conv_hd.h"
#include "td_conv_ad.h"
#include "td_wino.h"
#include "td_wino_f64.h"
#include "td_gemm.h"
#include "td_gemm_dma.h"
#include "td_gemm_b3.h"
#include "td_conv_ad_b3.h"
#include "td_attn.h"
#include "td_attn_h.h"
#include "td_attn_b3.h"
#include "td_misc.h"
#include "td_ingest.h"
#include "td_out.h"
#include "td_score.h"
#include "td_conf.h"
#include "td_matte.h"
#include "td_regions.h"
#include "td_runs.h"
#include "td_tracks.h"
#include "td_refine.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
static int td_fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}
#define TD_HIP(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return td_fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define TD_TRY(expr) do { if ((expr) != 0) return -1; } while (0)

// Every C-ABI entry that touches the device runs under the HANDLE's device and restores the caller's current device on exit:
// PyTorch tracks its own current device, and a library that changed it behind torch's back would misplace later allocations;
// a handle on cuda:1 used while the current device is 0 would otherwise launch its kernels and side stream on the wrong GPU.
struct DevGuard {
    int prev = -1;
    bool switched = false, ok = true;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev) { ok = hipSetDevice(dev) == hipSuccess; switched = ok; }
    }
    ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define TD_ON_DEVICE(n, ...)                                                                      \
    DevGuard dev_guard_((n)->cfg.device);                                                         \
    if (!dev_guard_.ok) { td_fail("cannot select HIP device %d", (n)->cfg.device); return __VA_ARGS__; }

// ---------------------------------------------------------------------------------------------------------------
// architecture description (same rules as tdnet_amd/arch.py; resnet.py:114-202)
// ---------------------------------------------------------------------------------------------------------------
// bott: conv1x1(cin->planes) conv3x3(planes->planes, stride, dil1) conv1x1(planes->cout); Bottleneck ignores dil2 (resnet.py:62-111)
struct BlockSpec { std::string name; int cin, cout, stride, dil1, dil2; bool ds; bool bott; int planes; };

// dilated (tdnet_arch.dilated): layers 3-4 at stride 1 with dilation 2 / 4 (output stride 8, resnet.py:140-149); otherwise at stride 2 with
// dilation 1 (output stride 32, resnet.py:150-158; `for_seg` is never passed by the Testing constructors).  multi_grid: layer 4's conv1
// dilations 4, 8, 16 (resnet.py:181,196); without it 2, 4, 4 (:188,199).  Ignored when not dilated.
static std::vector<BlockSpec> backbone_blocks(int backbone, bool dilated = true, bool multi_grid = true) {
    const int nb18[4] = {2, 2, 2, 2}, nb34[4] = {3, 4, 6, 3};
    const int nb101[4] = {3, 4, 23, 3};
    const int* nb = backbone == 18 ? nb18 : backbone == 101 ? nb101 : nb34;   // ResNet-50 has the ResNet-34 block counts
    const bool bott = backbone == 50 || backbone == 101;
    const int exp = bott ? 4 : 1;
    const int planes[4] = {64, 128, 256, 512};
    const int strides[4] = {1, 2, dilated ? 1 : 2, dilated ? 1 : 2}, dils[4] = {1, 1, dilated ? 2 : 1, dilated ? 4 : 1};
    std::vector<BlockSpec> out;
    int inpl = bott ? 128 : 64;                                      // deep_base stem ends in 128 channels (resnet.py:117)
    for (int li = 0; li < 4; ++li) {
        for (int b = 0; b < nb[li]; ++b) {
            const bool first = b == 0, mg = li == 3 && dilated && multi_grid;
            int d1;
            if (mg) d1 = b == 0 ? 4 : b == 1 ? 8 : 16;            // multi-grid (4,8,16): resnet.py:181,196-198
            else if (first) d1 = (dils[li] == 1 || dils[li] == 2) ? 1 : 2;
            else d1 = dils[li];
            BlockSpec s;
            char nm[32];
            snprintf(nm, sizeof(nm), "layer%d.%d", li + 1, b);
            s.name = nm;
            s.cin = first ? inpl : planes[li] * exp;
            s.cout = planes[li] * exp;
            s.bott = bott;
            s.planes = planes[li];
            s.stride = first ? strides[li] : 1;
            s.dil1 = d1;
            s.dil2 = dils[li];
            s.ds = first && (strides[li] != 1 || inpl != planes[li] * exp);
            out.push_back(s);
        }
        inpl = planes[li] * exp;
    }
    return out;
}
static int key_size(int n) { return (n - 1) / 4 + 1; }
static int out_size(int n, int KS, int stride, int dil, int pad) { return (n + 2 * pad - dil * (KS - 1) - 1) / stride + 1; }
// Feature size of an input axis from the strides themselves: the stem conv (stride 2, "same" padding), the 3x3 stride-2 max-pool, then every
// block's strided conv (3x3 with padding = dilation; the 1x1 downsample beside it gives the same size).  Output stride 8 or 32 follows from the list.
static int feature_size(int n, const std::vector<BlockSpec>& blocks) {
    n = (n - 1) / 2 + 1;
    n = (n - 1) / 2 + 1;
    for (const BlockSpec& s : blocks) n = out_size(n, 3, s.stride, s.dil1, s.dil1);
    return n;
}

// ---------------------------------------------------------------------------------------------------------------
// device conv layer
// ---------------------------------------------------------------------------------------------------------------
// The launch path of a conv layer and, where that path is a GEMM, its kernel.  plan_conv (td_weights.h) fixes both; nothing changes them
// afterwards, and the launch helpers (td_launch.h) switch on them without looking at the options again.
enum ConvRoute {
    CR_IGEMM,                                                          // fp32 implicit GEMM (td_conv.h conv_launch)
    CR_ADIRECT,                                                        // fp32, Cout <= 64: A operand straight from global (td_conv_ad.h, fusion bit 32); stem: NHWC4 taps
    CR_ADIRECT_ROWS,                                                   // ... the 7x7 stem on the packed-row image (td_conv_ad.h STEM = 2; fusion bit 65536)
    CR_ADIRECT_B3,                                                     // precision 2: the narrow direct convs on the split bf16 MFMA (td_conv_ad_b3.h; fusion bit 524288)
    CR_ADIRECT_ROWS_B3,                                                // ... the packed-row stem (td_conv_ad_b3.h STEM = 2)
    CR_GEMM1X1,                                                        // a stride-1 1x1 conv as one persistent GEMM (`gemm`: GK_PERSISTENT or GK_B3)
    CR_STEM_H,                                                         // precision 1: the 7x7 stem on the fp16 MFMA (td_conv_h.h)
    CR_CONV_H,                                                         // precision 1: fp16-MFMA operands, register-staged (td_conv_h.h)
    CR_CONV_DMA,                                                       // precision 1, fp16 map in: the LDS-DMA kernel, tile form `rh` (td_conv_hd.h)
    CR_WINO,                                                           // Winograd F(4x4,3x3): d_wp = 36 packed 1x1 weight sets, `gemm` runs them (td_wino.h)
    CR_WINO_F64                                                        // fp32, 64 -> 64 3x3 on a large map: the fused F(4x4,3x3) kernel, one launch (td_wino_f64.h; fusion bit 4194304)
};
enum GemmKernel {
    GK_CONV,                                                           // one tile per workgroup on the conv kernel (gemm_persistent = 0, or K % 64 != 0)
    GK_PERSISTENT,                                                     // k_gemm_persistent (td_gemm.h)
    GK_DMA,                                                            // the LDS-DMA-fed kernel (td_gemm_dma.h; tdnet_opts.overlap bit 8)
    GK_B3                                                              // k_gemm_b3: d_wp holds the three bf16 parts of the weights (td_gemm_b3.h gemm_b3_pack; tdnet_opts.precision = 2)
};
struct ConvLayer {
    int Cin = 0, Cout = 0, KS = 1, stride = 1, dil = 1, pad = 0, act = 0;
    bool stem = false;
    ConvRoute route = CR_IGEMM;
    GemmKernel gemm = GK_CONV;                                         // CR_WINO, CR_GEMM1X1 only
    bool in16 = false, out16 = false;                                  // fp16 routes only: the input (+ residual) / output map is stored as fp16 in HBM
    int rh = 0;                                                        // CR_CONV_DMA: the ConvDmaCode of its tile (64 rh rows for the plain forms; td_conv_hd.h)
    bool rowimg_off = false;                                           // test hook (tdnet_op_conv2d_f16io tile + 32): keep the tap-by-tap LDS-DMA kernel
    int pers = 1;                                                      // tdnet_opts.gemm_persistent of the owning handle (> 1: the forced grid of the persistent GEMMs)
    int chunks = 1;                                                    // > 1: run as that many row-parity chunks (tdnet_opts.overlap bit 1); the GEMM tile is picked for T / chunks rows
    int vw = 0;                                                        // != 0: the low-register F(4x4) transform kernels with vw channels per lane (td_wino.h k_wino4_*_c)
    int wino = 0;                                                      // CR_WINO: the output tile edge m = 4, otherwise 0
    float* d_zero = nullptr;                                           // zero bias for the batched GEMM pass
    ConvTile tile = CT_128x128;
    int CoutPad = 0, nsteps = 0;
    float* d_wp = nullptr;
    float* d_bias = nullptr;
    bool h16() const { return route == CR_STEM_H || route == CR_CONV_H || route == CR_CONV_DMA; }   // fp16-MFMA operands
    bool stem_rows() const { return route == CR_ADIRECT_ROWS || route == CR_ADIRECT_ROWS_B3; }      // reads the packed-row image
    double flops_per_pixel() const { return 2.0 * Cout * (stem ? 3.0 * KS * KS : (double)Cin * KS * KS); }
};

// Per-handle kernel configuration (include/tdnet.h tdnet_opts); nothing here is process-wide: two handles in one process may differ.
static_assert(TDNET_FUSION_DEFAULT == 8364070 && TDNET_FUSION_MASK == 8364070 && TDNET_OVERLAP_DEFAULT == 41 && TDNET_OVERLAP_MASK == 0x3f,
              "the named option bits of include/tdnet.h must add up to the documented values");
static tdnet_opts opts_or_default(const tdnet_opts* o) {
    tdnet_opts d;
    tdnet_opts_default(&d);
    if (!o) return d;
    d = *o;
    d.winograd = d.winograd <= 0 ? 0 : (d.winograd == 2 || d.winograd >= 4) ? 4 : 3;   // 1 / 2 were F(2x2,3x3) (removed in round 5): the F(4x4) forms of the same scope
    d.precision = d.precision < 0 ? 0 : d.precision > 3 ? 1 : d.precision;   // 0 fp32 MFMA, 1 fp16 MFMA, 2 fp32-accurate GEMMs on the bf16 MFMA (td_gemm_b3.h), 3 = 2 at any GEMM size (tests)
    d.pipeline = d.pipeline ? 1 : 0;
    d.gemm_persistent = d.gemm_persistent < 0 ? 0 : d.gemm_persistent;
    d.attention = d.attention < 0 ? 0 : d.attention > 2 ? 2 : d.attention;
    d.fusion &= TDNET_FUSION_MASK;                                    // retired bits are ignored: opts report only what is in effect
    d.overlap = d.overlap < 0 ? 0 : d.overlap & TDNET_OVERLAP_MASK;
    if ((d.overlap & TDNET_OVERLAP_VW_MASK) == TDNET_OVERLAP_VW_MASK) d.overlap &= ~TDNET_OVERLAP_VW_MASK;
    d.reserved0 = 0;
    for (int& r : d.reserved) r = 0;
    return d;
}

// ---------------------------------------------------------------------------------------------------------------
// weight block + handle
// ---------------------------------------------------------------------------------------------------------------
struct BlockLayers { ConvLayer c1, c2, c3, ds; bool has_ds = false, bott = false; };
struct AtnLayer { ConvLayer fc; float* d_bias = nullptr; };          // fc applied to the value matrix (no bias), bias added after P V'
struct PathLayers {
    ConvLayer stem, stem2, stem3;                                      // stem2/3: deep_base only (resnet.py:122-131)
    std::vector<BlockLayers> blocks;
    float* d_ppm_w = nullptr; float* d_ppm_b = nullptr;                // [4][FS][512], [4][FS]
    ConvLayer enc_v, enc_q0, enc_q1, enc_k0, enc_k1;
    std::vector<AtnLayer> atn;                                         // in the order the path applies them
    float* d_ln_g = nullptr; float* d_ln_b = nullptr;                  // [h*w]
    ConvLayer head3;
    float* d_cls_w = nullptr; float* d_cls_b = nullptr;                // [nclass][mid], [nclass]
    int pid = 0;
};
struct CacheSlot { float* q = nullptr; float* k = nullptr; float* v = nullptr; };
// The uint8 image input of a handle (tdnet_set_input_u8 / tdnet_set_input_nv12 / tdnet_set_input_view: ONE configuration at a time): source size, normalisation and
// the device tables k_ingest (td_ingest.h) reads.  Per handle: tdnet_create_shared handles configure their own.
struct Nv12Layout { int pitch; size_t uv_offset; int standard; };      // tdnet_set_input_nv12's surface arguments
// What the byte entries' image pointer is the base of (include/tdnet.h "source views"): a frame fh x fw of `format` with rows `pitch` bytes apart
// (0: tight), of which the image is the rectangle Hs x Ws at (oy, ox).  tdnet_set_input_u8 and tdnet_set_input_nv12 are the two obvious views.
struct SrcView {
    int format = 0;                                                    // TDNET_PIX_*
    int fh = 0, fw = 0, pitch = 0, oy = 0, ox = 0;
    size_t uv_offset = 0;                                              // NV12
    int standard = 0;                                                  // NV12
    // a YUV surface (include/tdnet.h "surfaces"; surface_resolve): `format` is then TDNET_PIX_NV12 for the readers that only ask "packed or not"
    bool surf = false;
    int layout = 0, cpitch = 0;                                        // TDNET_SURF_*; bytes per chroma row (pitch for 4:2:2)
    size_t u_off = 0, v_off = 0, extent = 0;                           // resolved plane offsets (4:2:2: 0); the surface's extent
};
static SrcView src_view_rgb(int Hs, int Ws) { SrcView v; v.fh = Hs; v.fw = Ws; return v; }
static SrcView src_view_nv12(int Hs, int Ws, const Nv12Layout& nv) {
    SrcView v; v.format = TDNET_PIX_NV12; v.fh = Hs; v.fw = Ws; v.pitch = nv.pitch; v.uv_offset = nv.uv_offset; v.standard = nv.standard; return v;
}
static int src_view_bpp(int format) { return format == TDNET_PIX_NV12 ? 1 : format >= TDNET_PIX_RGBA32 ? 4 : 3; }
struct U8Input {
    bool set = false;
    bool nv12 = false;                                                 // false: packed pixels; true: an NV12 surface
    bool surf = false;                                                 // a YUV surface (tdnet_set_input_surface): the layout reaches the kernels as arguments; nv12 is false then
    int layout = 0, cpitch = 0;                                        // surf: TDNET_SURF_*; bytes per chroma row
    size_t u_off = 0, v_off = 0;                                       // surf: the resolved plane offsets
    int format = 0, bpp = 3;                                           // TDNET_PIX_*; bytes per packed pixel
    bool swap = false;                                                 // packed: the colour bytes are b g r
    int fh = 0, fw = 0, oy = 0, ox = 0;                                // the whole frame; the origin of the rectangle Hs x Ws the image is
    int pitch = 0, standard = 0, span_c = 0;                           // bytes per frame row; NV12: TDNET_YUV_*, LDS bytes per staged chroma span
    size_t uv_offset = 0, extent = 0;                                  // NV12: the UV plane's offset; the bytes [base, base + extent) of the whole frame: nothing else is read
    int coef[6] = {0, 0, 0, 0, 0, 0};                                  // NV12: yoff, CY, CUB, CUG, CVG, CVR (nv12_coeffs)
    int Hs = 0, Ws = 0, H = 0, W = 0, Wt = 0;                          // Wt: W rounded up to a multiple of 4 (the x tables' row length)
    double mean[3] = {0, 0, 0}, std[3] = {1, 1, 1};
    bool resize = false;                                               // false: source size == network size, lookup only
    int span = 0, threads = 256;                                       // LDS bytes per staged source row; workgroup size (a strip = 4 * threads columns)
    float* lut = nullptr;                                              // [3][256]
    int* xt = nullptr;                                                 // [4][Wt]
    int* yt = nullptr;                                                 // [H][4]
    size_t bytes = 0;                                                  // HBM held by the three tables
};
// The colour-map output of a handle (tdnet_set_output_rgb): picture size, palette and the device tables the picture kernels (td_out.h k_picture_rows / k_picture_420)
// read.  Per handle, like U8Input.
struct RgbOutput {
    bool set = false;
    int H = 0, W = 0, oh = 0, ow = 0, n_colours = 0;
    unsigned char palette[768] = {0};                                  // the caller's, kept to recognise an equal call
    int* ys = nullptr;                                                 // [oh]: nearest_index(H, oh)
    int* xs = nullptr;                                                 // [ow]: nearest_index(W, ow)
    unsigned* lut = nullptr;                                           // [256]: r | g << 8 | b << 16
    size_t bytes = 0;
};
// The overlay output of a handle (tdnet_set_output_overlay): palette with opacity, the colour table the picture kernels read,
// and the index tables of the pair (network size, source size) -- the source size is the byte input's, so the tables follow U8Input (overlay_tables).
// Per handle, like U8Input.
struct OverlayOutput {
    bool set = false;
    int n_colours = 0;
    unsigned char palette[1024] = {0};                                 // the caller's r, g, b, a rows, kept to recognise an equal call
    unsigned* lut = nullptr;                                           // [256]: r | g << 8 | b << 16 | a << 24; 0 for a label >= n_colours
    bool swap = false;                                                 // the table holds b | g << 8 | r << 16 | a << 24: the source's bytes are b g r, and so is the picture
    int H = 0, W = 0, Hs = 0, Ws = 0;                                  // the pair ys / xs were built for (Hs == 0: not built yet)
    int* ys = nullptr;                                                 // [Hs]: nearest_index(H, Hs)
    int* xs = nullptr;                                                 // [Ws]: nearest_index(W, Ws)
    size_t bytes = 0;
};
// The destination view of a handle (tdnet_set_output_view): where the picture entries write -- the rectangle h x w at (oy, ox) of a frame fh x fw of
// `format` whose rows are `pitch` bytes apart.  Plain host state (the kernels take it as arguments): nothing is allocated.  Per handle, like U8Input.
struct DstOutput {
    bool set = false;
    int format = 0, bpp = 3;                                           // TDNET_PIX_*; bytes per packed pixel
    bool swap = false;                                                 // packed: the colour bytes are b g r
    int fh = 0, fw = 0, oy = 0, ox = 0, h = 0, w = 0, pitch = 0, standard = 0;
    size_t uv_offset = 0, extent = 0;                                  // NV12; the bytes [base, base + extent) of the whole frame: nothing else is written
    int yoff = 0, ky[3] = {0, 0, 0}, ku[3] = {0, 0, 0}, kv[3] = {0, 0, 0};   // NV12: nv12_forward_coeffs, rows over r, g, b
    // a 4:2:0 surface (tdnet_set_output_surface; dst_surface_build): format is TDNET_PIX_NV12, uv_offset = u_off; the view and the surface replace each other
    bool surf = false;
    int layout = 0, cpitch = 0;                                        // TDNET_SURF_* (NV12, NV21, I420, P010); bytes per chroma row
    size_t u_off = 0, v_off = 0;
};
// The composite output of a handle (tdnet_set_output_composite): the mode and the background.  Plain host state -- both travel as kernel arguments; the
// index tables of the pair (network size, source size) are the overlay's (OverlayOutput ys / xs: overlay_tables builds them for either configuration).
struct CompositeOutput {
    bool set = false;
    int mode = 0;                                                      // TDNET_COMPOSITE_COLOUR / TDNET_COMPOSITE_ALPHA
    unsigned char bg[3] = {0, 0, 0};                                   // colour mode: true r, g, b
};
// The score output of a handle (tdnet_set_score): the device confusion matrix the score kernels add into and the 256-byte ground-truth map they
// read.  Per handle, like U8Input.
struct ScoreOutput {
    bool set = false;
    int nclass = 0;
    unsigned char map[256] = {0};                                      // the caller's (identity for NULL), kept to recognise an equal call
    unsigned long long* cm = nullptr;                                  // [nclass][nclass] counts
    unsigned char* dmap = nullptr;                                     // [256]
    size_t bytes = 0;
};
// The regions output of a handle (tdnet_set_regions): the configuration -- plain host state, read when an entry enqueues -- and the workspace the seven
// launches of td_regions.h pass their maps through.  Per handle, like U8Input.
struct RegionsOutput {
    bool set = false;
    MatteSet classes = {{0, 0, 0, 0, 0, 0, 0, 0}};
    int conn = 8, max_regions = 0, min_area = 1;
    int H = 0, W = 0;
    int *parent = nullptr, *root = nullptr, *area = nullptr, *blk = nullptr;   // three int32 [H][W]; the block counts
    unsigned* flag = nullptr;                                          // one word, zero between runs
    unsigned char* lab = nullptr;                                      // [H][W]: where a frame's labels go when the caller asks for none
    size_t bytes = 0;
};
// The tracks output of a handle (tdnet_set_tracks): min_overlap -- plain host state, a kernel argument read when an entry enqueues -- and ONE device
// blob that holds everything that lives between frames (td_tracks.h TracksState) at fixed addresses: nothing on the host changes per frame.
struct TracksOutput {
    bool set = false;
    int min_overlap = 1;
    void* blob = nullptr;
    TracksState st = TracksState();
    size_t bytes = 0;
};
// The runs output of a handle (tdnet_set_runs): max_runs -- plain host state, a kernel argument read when an entry enqueues -- and the workspace of
// td_runs.h: the block counts, and a byte map for the frame entries that are asked for no labels.
struct RunsState {
    bool set = false;
    int max_runs = 0;
    int H = 0, W = 0;
    int* blk = nullptr;                                                // [runs_blocks(H, W)]
    unsigned char* lab = nullptr;                                      // [H][W]
    size_t bytes = 0;
};
// The refined matte of a handle (tdnet_set_matte_refine): radius (0 = off) and eps -- plain host state, kernel arguments read when an entry enqueues -- and the
// workspace at the SOURCE's size (it follows the byte input like the overlay's tables): luma and M_src (2 bytes per source pixel), the coefficient planes (6), the
// refined map (1), and the identity index tables the existing composite kernel reads the refined map through.
struct RefineState {
    int radius = 0, eps = 0;
    int Hs = 0, Ws = 0;                                                // the source size the workspace was allocated for (0: none yet)
    unsigned char *luma = nullptr, *msrc = nullptr, *refined = nullptr;   // [Hs][Ws] each
    int* scratch = nullptr;                                            // 6 Hs Ws bytes: b_q int32, then a_q int16
    int *idy = nullptr, *idx = nullptr;                                // [Hs], [Ws]: 0, 1, 2, ...
    size_t bytes = 0;
};
struct ProfRec { int family; int dominant; hipEvent_t e0, e1; double flops; };   // dominant: 0 no, 1 direct 3x3 128x128, 2 Winograd batched GEMM

// Everything a model owns that does NOT change from frame to frame: the host state_dict until it is finalized, then the BN-folded,
// packed, uploaded layers of every path.  One block serves any number of handles (tdnet_create_shared: the samples of a batch, the
// two lanes of a frame-pipelined clip, clips sharing a GPU) -- the reference's batch shares ONE nn.Module's parameters the same way
// (td4_psp18.py:216-229).  Reference-counted; freed with the last handle, whatever the destroy order.
struct TdWeights {
    std::atomic<int> refs{1};                                          // handles on this block; tdnet_create_shared / tdnet_destroy may run on different host threads
    int device = 0;
    tdnet_arch arch = {1, 1, {0, 0, 0, 0, 0, 0}};                     // the backbone's layout (tdnet_create_arch); bspec is built from it
    std::vector<BlockSpec> bspec;
    std::map<std::string, std::vector<float>> sd;                      // host state_dict until finalize
    std::map<std::string, size_t> expected;                            // name -> element count
    bool finalized = false;
    std::vector<PathLayers> paths;
    // Row-parity chains (tdnet_opts.overlap bit 1): the trailing run of even-dilation convs of the backbone starts at conv seg_conv
    // (0: conv1, 1: conv2) of block seg_block (-1: off) -- td_weights.h plan_chains
    int seg_block = -1, seg_conv = 0;
    bool act16 = false;                                                // precision = 1: the maps between the backbone's convs are fp16 in HBM
    double flops_frame = 0.0;
    size_t device_bytes = 0;                                           // HBM held by the block (packed weights, biases, affine maps)
};

struct tdnet {
    TdWeights* const wt;                                               // never null; shared between handles (ref-counted)
    tdnet_cfg cfg;
    tdnet_opts opts;                                                   // per-handle kernel configuration (never process-wide); handles of one block share it
    int P = 0, DV = 0, MID = 0, FIFO = 0, C = 512, SC = 64;            // C = backbone output channels, SC = stem output channels
    bool deep = false;
    int H = 0, W = 0, H1 = 0, W1 = 0, H2 = 0, W2 = 0, h = 0, w = 0, hk = 0, wk = 0, Lq = 0, Lk = 0;
    // views of the weight block under the names the frame code uses
    std::vector<BlockSpec>& bspec;
    std::map<std::string, std::vector<float>>& sd;
    std::map<std::string, size_t>& expected;
    bool& finalized;
    std::vector<PathLayers>& paths;
    int& seg_block; int& seg_conv;
    bool& act16;
    double& flops_frame;
    bool ws_ready = false;                                             // workspace, FIFO slots, streams and events of THIS handle exist
    size_t ws_bytes = 0;                                               // HBM held by this handle alone (workspace + FIFO)
    // workspace
    float *img4 = nullptr, *s1 = nullptr, *s1b = nullptr, *bx = nullptr, *bt = nullptr, *br = nullptr, *bu = nullptr;
    float *rowpart = nullptr, *pooled = nullptr, *ppmfeat = nullptr, *z = nullptr;
    float *v_cur = nullptr, *q1 = nullptr, *q_cur = nullptr, *k1 = nullptr;
    float *vp = nullptr, *chain_a = nullptr, *chain_b = nullptr, *feat = nullptr;
    float *ln_part = nullptr, *ln_mean = nullptr, *ln_rstd = nullptr, *ln = nullptr;
    float *headmid = nullptr, *lowres = nullptr, *stage_tmp = nullptr, *logits_tmp = nullptr;
    float *wino_v = nullptr, *wino_m = nullptr;                        // Winograd workspaces [36][T][Cin] / [36][T][Cout]
    size_t wino_v_floats = 0, wino_m_floats = 0;
    size_t stage_tmp_floats = 0;
    std::vector<CacheSlot> slots;
    std::vector<int> fifo;                                             // slot ids, oldest first
    int last_slot = -1;
    int pending_slot = -1;                                             // cache entry of an encoded, not yet propagated frame
    int pending_pos = -1;
    // cache-only work (V' GEMMs + the two cached-frame attention steps) runs on a side stream under the backbone
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Row-parity chains: chain 0 runs on the forward's stream with wino_v / wino_m, chain 1 on `chain2` with wino_v2 / wino_m2.  The
    // chains may drift apart by more than a block and the channel count changes inside the run, so no map of the run is written in
    // place or shared between blocks: block b owns seg_t[b] (conv1 output), seg_r[b] (downsample output) and seg_x[b] (block output).
    hipStream_t chain2 = nullptr;
    hipEvent_t ev_cfork = nullptr, ev_cjoin = nullptr;
    float *wino_v2 = nullptr, *wino_m2 = nullptr;
    std::vector<float*> seg_t, seg_r, seg_x;
    std::vector<hipStream_t> probe_streams;                            // TDNET_PROBE_EXTRA_STREAMS (-DTDNET_TIMING_PROBES builds only)
    std::vector<hipStream_t> retired_streams;                          // chain2 candidates that shared the caller's hardware queue (place_chain_stream)
    std::vector<void*> placed_for;                                     // the caller streams chain2 has been checked against (place_chain_stream): once per stream
    int chain_replaced = 0;
    float* c4 = nullptr;                                              // backbone output of the last frame (bx, or br in the fp16-activation mode)
    _Float16* vt16 = nullptr;                                         // fp16 attention: V' re-tiled [LkPad / 8][DV][8]; precision 2: its three bf16 parts (3x that, td_attn_b3.h)
    bool ln_pending = false;                                          // the `ln` map of the last frame was not materialised (fusion bit 4)
    // The pyramid folded through the Encoding's first 1x1 convs (fusion bit 2097152; td_weights.h plan_enc_fold, td_misc.h k_ppm_fold_g).  All of it is
    // this handle's: the weight block is shared (tdnet_create_shared) and only read.
    bool enc_fold = false;                                            // this handle's frames take the fold
    float* ppm_basis = nullptr;                                       // [h w][64] bilinear coefficients of the 50 bins (+ 14 zero columns): a function of (h, w) alone
    float* fold_g[3] = {nullptr, nullptr, nullptr};                   // G of enc_v / enc_q0 / enc_k0 as two packed K steps [2][8][CoutPad][4]; rows 50 .. 63 stay zero
    bool z_pending = false;                                           // the `z` map of the last frame was not assembled
    int z_path = 0;
    int ln_path = 0;
    bool feat_is_vcur = false;                                        // warm-up frame (td4_psp18.py:142-143): the "feat" stage IS v_cur (no copy is made)
    bool failed = false;                                              // a launch helper reported an error during the current forward
    bool prof = false;
    std::vector<ProfRec> recs;
    size_t nrec = 0;
    U8Input u8;                                                        // tdnet_set_input_u8 / tdnet_set_input_nv12
    RgbOutput rgb;                                                     // tdnet_set_output_rgb
    OverlayOutput overlay;                                             // tdnet_set_output_overlay
    DstOutput dst;                                                     // tdnet_set_output_view
    ScoreOutput score;                                                // tdnet_set_score
    RegionsOutput regions;                                            // tdnet_set_regions
    TracksOutput tracks;                                              // tdnet_set_tracks
    RunsState runs;                                                   // tdnet_set_runs
    RefineState refine;                                                // tdnet_set_matte_refine
    int min_conf = 0, reject_label = 255;                              // tdnet_set_confidence: plain host state, read when a *_conf entry enqueues its last launch
    CompositeOutput comp;                                              // tdnet_set_output_composite
    bool matte_set = false;                                            // tdnet_set_matte: plain host state like min_conf; the *_matte entries pass the words as kernel arguments
    MatteSet matte = {{0, 0, 0, 0, 0, 0, 0, 0}};                       // 256 membership bits: bit c & 31 of word c >> 5
    int launches = 0;                                                  // kernel launches + device copies enqueued by the current frame (td_launch.h TD_COUNTED)

    explicit tdnet(TdWeights* w)
        : wt(w), bspec(w->bspec), sd(w->sd), expected(w->expected), finalized(w->finalized), paths(w->paths), seg_block(w->seg_block),
          seg_conv(w->seg_conv), act16(w->act16), flops_frame(w->flops_frame) {}
    tdnet(const tdnet&) = delete;
    tdnet& operator=(const tdnet&) = delete;
};

// device allocations of a handle / of a weight block are counted (bytes), so that the cost of an extra lane is a number (tdnet_memory_bytes)
static thread_local size_t* g_alloc_counter = nullptr;
template <typename T>
static int dev_alloc(T** p, size_t count) {
    TD_HIP(hipMalloc((void**)p, count * sizeof(T)));
    if (g_alloc_counter) *g_alloc_counter += count * sizeof(T);
    return 0;
}
static int upload(float** d, const std::vector<float>& v) {
    TD_TRY(dev_alloc(d, v.size()));
    TD_HIP(hipMemcpy(*d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
struct AllocScope {                                                   // RAII: allocations inside the scope are added to *counter
    size_t* prev;
    explicit AllocScope(size_t* counter) : prev(g_alloc_counter) { g_alloc_counter = counter; }
    ~AllocScope() { g_alloc_counter = prev; }
};

// ---------------------------------------------------------------------------------------------------------------
// uint8 image input: the host side of td_ingest.h
// ---------------------------------------------------------------------------------------------------------------
// tdnet_amd/dataloader.py _linear_coeffs (OpenCV's INTER_LINEAR tables) with the same operations in the same types: a double scale,
// fx = (float)((d + 0.5) * scale - 0.5), s = floor(fx), fx -= s in float, clamped at both borders, weights = rint to even of (1 - fx, fx) * 2048
// in float.  (The library is built with -ffp-contract=off: no product here is fused into a later sum.)
static void u8_linear_coeffs(int n_src, int n_dst, std::vector<int>& s0, std::vector<int>& s1, std::vector<int>& w0, std::vector<int>& w1) {
    const double scale = (double)n_src / (double)n_dst;
    s0.resize(n_dst); s1.resize(n_dst); w0.resize(n_dst); w1.resize(n_dst);
    for (int d = 0; d < n_dst; ++d) {
        float fx = (float)(((double)d + 0.5) * scale - 0.5);
        long s = (long)floorf(fx);
        fx = fx - (float)s;
        if (s < 0) { fx = 0.f; s = 0; }
        if (s >= n_src - 1) { fx = 0.f; s = n_src - 1; }
        const float f1 = fx * 2048.0f, om = 1.0f - fx, f0 = om * 2048.0f;
        w1[d] = (int)nearbyintf(f1);
        w0[d] = (int)nearbyintf(f0);
        s0[d] = (int)s;
        s1[d] = (int)std::min<long>(s + 1, n_src - 1);
    }
}
static void u8_free(U8Input& u) {
    if (u.lut) hipFree(u.lut);
    if (u.xt) hipFree(u.xt);
    if (u.yt) hipFree(u.yt);
    u = U8Input();
}
constexpr int TD_INGEST_LDS_MAX = 64 * 1024;
// include/tdnet.h "NV12 frames in": yoff and rint(c 2^20) of the decimal coefficients (CY, CUB, CUG, CVG, CVR) of TDNET_YUV_* 0..3.  Row 0
// reproduces OpenCV's published integers (1220542, 2116026, -409993, -852492, 1673527).
static void nv12_coeffs(int standard, int coef[6]) {
    static const double dec[4][5] = {{1.164, 2.018, -0.391, -0.813, 1.596}, {1.164, 2.112, -0.213, -0.533, 1.793},
                                     {1.0, 1.772, -0.344136, -0.714136, 1.402}, {1.0, 1.8556, -0.187324, -0.468124, 1.5748}};
    coef[0] = standard < 2 ? 16 : 0;
    for (int i = 0; i < 5; ++i) coef[1 + i] = (int)nearbyint(dec[standard][i] * 1048576.0);
}
// What a frame of a view must satisfy as a surface, source or destination alike: tdnet_set_input_nv12's pitch / uv_offset / standard conditions, and an
// extent [base, base + extent) below 2^31 bytes.  pitch: the one in force.
static int view_surface_check(const SrcView& sv, int pitch, const char* who, double* extent_out) {
    double extent = 0.0;
    if (sv.format == TDNET_PIX_NV12) {
        const int cw = (sv.fw - 1) / 2 + 1, chh = (sv.fh - 1) / 2 + 1;  // chroma pairs per row, chroma rows
        if (pitch < 2 * cw) return td_fail("%s: pitch %d is below the %d bytes a row of %d columns holds", who, pitch, 2 * cw, sv.fw);
        if ((double)sv.uv_offset < (double)sv.fh * pitch) return td_fail("%s: uv_offset %zu is inside the Y plane (%d rows of pitch %d)", who, sv.uv_offset, sv.fh, pitch);
        extent = (double)sv.uv_offset + (double)(chh - 1) * pitch + 2.0 * cw;
        if (extent >= 2147483648.0) return td_fail("%s: the surface's extent (uv_offset %zu, pitch %d, %d rows) is 2^31 bytes or more", who, sv.uv_offset, pitch, sv.fh);
        if (sv.standard < 0 || sv.standard > 3) return td_fail("%s: standard %d is not one of TDNET_YUV_* (0..3)", who, sv.standard);
    } else {
        extent = (double)(sv.fh - 1) * pitch + (double)sv.fw * src_view_bpp(sv.format);
        if (extent >= 2147483648.0) return td_fail("%s: the frame's extent (pitch %d, %d rows) is 2^31 bytes or more", who, pitch, sv.fh);
    }
    *extent_out = extent;
    return 0;
}
// include/tdnet.h "destination views": yoff and rint(c 2^20) of the forward matrix's decimals, rows Y, U, V over r, g, b, of TDNET_YUV_* 0..3
static void nv12_forward_coeffs(int standard, int* yoff, int ky[3], int ku[3], int kv[3]) {
    static const double dec[4][9] = {{.257, .504, .098, -.148, -.291, .439, .439, -.368, -.071}, {.183, .614, .062, -.101, -.339, .439, .439, -.399, -.040},
                                     {.299, .587, .114, -.168736, -.331264, .5, .5, -.418688, -.081312}, {.2126, .7152, .0722, -.114572, -.385428, .5, .5, -.454153, -.045847}};
    *yoff = standard < 2 ? 16 : 0;
    for (int i = 0; i < 3; ++i) {
        ky[i] = (int)nearbyint(dec[standard][i] * 1048576.0);
        ku[i] = (int)nearbyint(dec[standard][3 + i] * 1048576.0);
        kv[i] = (int)nearbyint(dec[standard][6 + i] * 1048576.0);
    }
}
// ---- YUV surfaces (include/tdnet.h "surfaces"): the host side of td_ingest.h IngestYuv / td_out.h td_src_px4 ----
// What a layout is to the kernels (td_ingest.h SrcLayout has the table): bytes between luma samples, the luma sample's offset, the vertical chroma
// shift, bytes between chroma pairs, the offsets of U and V within a pair, the chroma spans staged per source row, 16-bit samples.
struct SurfForm { int lstride = 1, loff = 0, cshift = 1, cstep = 2, uo = 0, vo = 1, planes = 1; bool wide = false; };
static SurfForm surf_form(int layout) {
    SurfForm f;
    switch (layout) {
    case TDNET_SURF_NV21: f.uo = 1; f.vo = 0; break;
    case TDNET_SURF_I420: f.cstep = 1; f.uo = f.vo = 0; f.planes = 2; break;
    case TDNET_SURF_P010: f.lstride = 2; f.cstep = 4; f.vo = 2; f.wide = true; break;
    case TDNET_SURF_YUY2: f.lstride = 2; f.cshift = 0; f.cstep = 4; f.uo = 1; f.vo = 3; f.planes = 0; break;
    case TDNET_SURF_UYVY: f.lstride = 2; f.loff = 1; f.cshift = 0; f.cstep = 4; f.uo = 0; f.vo = 2; f.planes = 0; break;
    default: break;                                                    // TDNET_SURF_NV12
    }
    return f;
}
// yoff and rint(c 2^20) of nv12_coeffs' decimals; 10-bit samples: 4 yoff and rint(c 2^18) -- the sum is shifted by 20 either way
static void surf_coeffs(int standard, bool wide, int coef[6]) {
    nv12_coeffs(standard, coef);
    if (!wide) return;
    static const double dec[4][5] = {{1.164, 2.018, -0.391, -0.813, 1.596}, {1.164, 2.112, -0.213, -0.533, 1.793},
                                     {1.0, 1.772, -0.344136, -0.714136, 1.402}, {1.0, 1.8556, -0.187324, -0.468124, 1.5748}};
    coef[0] *= 4;
    for (int i = 0; i < 5; ++i) coef[1 + i] = (int)nearbyint(dec[standard][i] * 262144.0);
}
// tdnet_surface -> (SrcView, Hs x Ws) with every default resolved and the planes checked, or the failure that names the offending field.  mean / std
// and the staged span are u8_build's to check.
static int surface_resolve(const tdnet_surface* t, SrcView& sv, int& Hs, int& Ws, const char* who) {
    if (!t) return td_fail("%s: surface is NULL", who);
    if (t->layout < 0 || t->layout > TDNET_SURF_UYVY) return td_fail("%s: layout %d is not one of TDNET_SURF_* (0..5)", who, t->layout);
    for (int i = 0; i < 4; ++i)
        if (t->reserved[i]) return td_fail("%s: reserved[%d] = %d must be 0", who, i, t->reserved[i]);
    if (t->height < 1 || t->width < 1) return td_fail("%s: height x width = %d x %d must be at least 1 x 1", who, t->height, t->width);
    const bool whole = !t->crop_y && !t->crop_x && !t->crop_height && !t->crop_width;
    const int oy = t->crop_y, ox = t->crop_x, h = whole ? t->height : t->crop_height, w = whole ? t->width : t->crop_width;
    if (oy < 0 || ox < 0) return td_fail("%s: crop_y, crop_x = %d, %d: the origin must not be negative", who, oy, ox);
    if (h < 1 || w < 1) return td_fail("%s: crop_height x crop_width = %d x %d must be at least 1 x 1", who, h, w);
    if (h > t->height || oy > t->height - h) return td_fail("%s: crop_y + crop_height = %d + %d is not inside the frame's height %d", who, oy, h, t->height);
    if (w > t->width || ox > t->width - w) return td_fail("%s: crop_x + crop_width = %d + %d is not inside the frame's width %d", who, ox, w, t->width);
    if (t->standard < 0 || t->standard > 3) return td_fail("%s: standard %d is not one of TDNET_YUV_* (0..3)", who, t->standard);
    const SurfForm f = surf_form(t->layout);
    const double cw = (double)((t->width - 1) / 2 + 1), chh = (double)((t->height - 1) / 2 + 1);
    const double lrow = f.planes ? (double)t->width * f.lstride : 4.0 * cw, crow = f.cstep * cw;   // bytes of a luma (packed) row / of a chroma row
    if (lrow >= 2147483648.0) return td_fail("%s: the surface's extent (a row of %d pixels) is 2^31 bytes or more", who, t->width);
    if (t->pitch < 0) return td_fail("%s: pitch %d is negative", who, t->pitch);
    if (t->pitch && t->pitch < lrow) return td_fail("%s: pitch %d is below the %.0f bytes a row of %d pixels holds", who, t->pitch, lrow, t->width);
    const double pitch = t->pitch ? t->pitch : lrow;
    double ext = (t->height - 1) * pitch + lrow;                       // the luma (packed) plane: [0, ext)
    sv = SrcView();
    sv.surf = true; sv.layout = t->layout; sv.format = TDNET_PIX_NV12; sv.fh = t->height; sv.fw = t->width; sv.oy = oy; sv.ox = ox; sv.standard = t->standard;
    if (!f.planes) {
        if (t->chroma_pitch) return td_fail("%s: chroma_pitch = %d must be 0 for a 4:2:2 layout (the chroma lies in the packed rows)", who, t->chroma_pitch);
        if (t->u_offset) return td_fail("%s: u_offset = %llu must be 0 for a 4:2:2 layout", who, (unsigned long long)t->u_offset);
        if (t->v_offset) return td_fail("%s: v_offset = %llu must be 0 for a 4:2:2 layout", who, (unsigned long long)t->v_offset);
        if (ext >= 2147483648.0) return td_fail("%s: the surface's extent (pitch %.0f, %d rows) is 2^31 bytes or more", who, pitch, t->height);
        sv.pitch = sv.cpitch = (int)pitch;
    } else {
        if (f.planes != 2 && t->v_offset) return td_fail("%s: v_offset = %llu must be 0 for a layout with one chroma plane", who, (unsigned long long)t->v_offset);
        if (t->chroma_pitch < 0) return td_fail("%s: chroma_pitch %d is negative", who, t->chroma_pitch);
        if (t->chroma_pitch && t->chroma_pitch < crow) return td_fail("%s: chroma_pitch %d is below the %.0f bytes a chroma row of %d columns holds", who, t->chroma_pitch, crow, t->width);
        const double cpitch = t->chroma_pitch ? t->chroma_pitch : f.planes == 2 ? floor((pitch + 1) / 2) : pitch;
        if (cpitch < crow) return td_fail("%s: chroma_pitch 0 resolves to %.0f, below the %.0f bytes a chroma row of %d columns holds (pitch %.0f)", who, cpitch, crow, t->width, pitch);
        if ((double)t->u_offset >= 2147483648.0 || (double)t->v_offset >= 2147483648.0 || t->height * pitch >= 2147483648.0)
            return td_fail("%s: the surface's extent (u_offset %llu, v_offset %llu, pitch %.0f, %d rows) is 2^31 bytes or more", who, (unsigned long long)t->u_offset,
                           (unsigned long long)t->v_offset, pitch, t->height);
        const double plane = (chh - 1) * cpitch + crow;                // bytes from a chroma plane's start to its end
        const double u0 = t->u_offset ? (double)t->u_offset : t->height * pitch;
        const double v0 = f.planes != 2 ? u0 : t->v_offset ? (double)t->v_offset : u0 + chh * cpitch;
        if (u0 < ext) return td_fail("%s: u_offset %.0f is inside the luma plane (%d rows of pitch %.0f: %.0f bytes)", who, u0, t->height, pitch, ext);
        if (f.planes == 2) {
            if (v0 < ext) return td_fail("%s: v_offset %.0f is inside the luma plane (%d rows of pitch %.0f: %.0f bytes)", who, v0, t->height, pitch, ext);
            if (u0 < v0 + plane && v0 < u0 + plane) return td_fail("%s: the chroma planes at u_offset %.0f and v_offset %.0f (%.0f bytes each) overlap", who, u0, v0, plane);
        }
        ext = std::max(u0, v0) + plane;
        if (ext >= 2147483648.0) return td_fail("%s: the surface's extent (u_offset %.0f, v_offset %.0f, chroma_pitch %.0f) is 2^31 bytes or more", who, u0, v0, cpitch);
        sv.pitch = (int)pitch; sv.cpitch = (int)cpitch; sv.u_off = (size_t)u0; sv.v_off = (size_t)v0;
    }
    sv.extent = (size_t)ext;
    Hs = h; Ws = w;
    return 0;
}
// Validate, build the tables on the host and upload them into memory `u` owns.  NULL mean / std: the loader's (dataloader.py:52-53).
// sv: what the image pointer is the base of -- the tables are those of the rectangle Hs x Ws whatever the format.  On failure `u` is left as it was.
static int u8_build(U8Input& u, const SrcView& sv, int Hs, int Ws, int H, int W, const double* mean, const double* std_, const char* who) {
    static const double mean0[3] = {.485, .456, .406}, std0[3] = {.229, .224, .225};
    if (!mean) mean = mean0;
    if (!std_) std_ = std0;
    const bool nv = sv.format == TDNET_PIX_NV12 && !sv.surf;
    const int bpp = src_view_bpp(sv.format);
    if (Hs < 1 || Ws < 1) return td_fail("%s: source size %d x %d must be at least 1 x 1", who, Hs, Ws);
    if (H < 1 || W < 1 || H > 65535) return td_fail("%s: network size %d x %d out of range", who, H, W);
    if (!nv && !sv.surf && (double)Hs * Ws * 3 >= 2147483648.0) return td_fail("%s: source size %d x %d is too large", who, Hs, Ws);
    const int pitch = nv || sv.pitch ? sv.pitch : sv.fw * bpp;         // packed, 0: tight (a row that overflows was refused above or by view_resolve)
    double extent = (double)sv.extent;                                 // a surface: surface_resolve has checked it
    if (!sv.surf) TD_TRY(view_surface_check(sv, pitch, who, &extent));
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c])) return td_fail("%s: mean[%d] is not finite", who, c);
        if (!std::isfinite(std_[c]) || std_[c] == 0.0) return td_fail("%s: std[%d] must be finite and non-zero", who, c);
    }
    U8Input v;
    v.Hs = Hs; v.Ws = Ws; v.H = H; v.W = W; v.Wt = (W + 3) / 4 * 4;
    v.format = sv.format; v.bpp = bpp; v.swap = sv.format == TDNET_PIX_BGR24 || sv.format == TDNET_PIX_BGRA32;
    v.fh = sv.fh; v.fw = sv.fw; v.oy = sv.oy; v.ox = sv.ox; v.pitch = pitch; v.extent = (size_t)extent;
    if (nv) {
        v.nv12 = true; v.uv_offset = sv.uv_offset; v.standard = sv.standard;
        nv12_coeffs(sv.standard, v.coef);
    }
    const SurfForm sf = sv.surf ? surf_form(sv.layout) : SurfForm();
    if (sv.surf) {
        v.surf = true; v.layout = sv.layout; v.cpitch = sv.cpitch; v.u_off = sv.u_off; v.v_off = sv.v_off; v.standard = sv.standard;
        surf_coeffs(sv.standard, sf.wide, v.coef);
    }
    for (int c = 0; c < 3; ++c) { v.mean[c] = mean[c]; v.std[c] = std_[c]; }
    v.resize = !(Hs == H && Ws == W);
    std::vector<float> lut(768);
    for (int c = 0; c < 3; ++c)
        for (int b = 0; b < 256; ++b) lut[c * 256 + b] = (float)(((double)b / 255.0 - mean[c]) / std_[c]);
    std::vector<int> xt, yt, x0, x1, a0, a1;
    if (v.resize) {
        std::vector<int> y0, y1, b0, b1;
        u8_linear_coeffs(Ws, W, x0, x1, a0, a1);
        u8_linear_coeffs(Hs, H, y0, y1, b0, b1);
        xt.resize((size_t)4 * v.Wt);
        for (int x = 0; x < v.Wt; ++x) {
            const int k = x < W ? x : W - 1;                           // the padding repeats the last column: every table entry indexes the staged span
            xt[x] = x0[k]; xt[v.Wt + x] = x1[k]; xt[2 * v.Wt + x] = a0[k]; xt[3 * v.Wt + x] = a1[k];
        }
        yt.resize((size_t)4 * H);
        for (int y = 0; y < H; ++y) { yt[4 * y] = y0[y]; yt[4 * y + 1] = y1[y]; yt[4 * y + 2] = b0[y]; yt[4 * y + 3] = b1[y]; }
    }
    // the workgroup size: the largest whose two staged spans (+ up to 15 bytes in front of the first, rounded to 16) fit beside the table;
    // NV12: two Y spans of a byte per column and two chroma spans of a byte pair per two columns OF THE FRAME (the origin's parity counts)
    bool fits = false;
    for (int threads = 256; threads >= 64 && !fits; threads >>= 1) {
        long span = 0, span_c = 0;
        for (int xs = 0; xs < W; xs += 4 * threads) {
            const int xe = std::min(xs + 4 * threads, W);
            const int cl = v.resize ? x0[xs] : xs, ch = v.resize ? x1[xe - 1] : xe - 1;
            const long cols = (long)ch - cl + 1;
            const long pairs = (long)((sv.ox + ch) >> 1) - ((sv.ox + cl) >> 1) + 1;
            if (sv.surf) {                                             // IngestYuv: 4:2:2 stages whole pixel pairs, chroma included
                span = std::max(span, ((sf.planes ? cols * sf.lstride : 4 * pairs) + 15 + 15) / 16 * 16);
                if (sf.planes) span_c = std::max(span_c, (pairs * sf.cstep + 15 + 15) / 16 * 16);
                continue;
            }
            span = std::max(span, (cols * bpp + 15 + 15) / 16 * 16);
            if (nv) span_c = std::max(span_c, (((long)((sv.ox + ch) >> 1) - ((sv.ox + cl) >> 1) + 1) * 2 + 15 + 15) / 16 * 16);
        }
        if (TD_INGEST_LUT_BYTES + 2 * span + 2 * (sv.surf ? sf.planes : 1) * span_c <= TD_INGEST_LDS_MAX) { fits = true; v.threads = threads; v.span = (int)span; v.span_c = (int)span_c; }
    }
    if (!fits && sv.surf)
        return td_fail("%s: a %d -> %d column downscale is beyond what the ingest kernel stages (%d bytes per column%s)", who, Ws, W, sf.lstride,
                       sf.planes == 2 ? " and two chroma planes" : "");
    if (!fits) return td_fail("%s: a %d -> %d column downscale is beyond what the ingest kernel stages (about %s)", who, Ws, W, nv ? "60x" : bpp == 4 ? "30x: 4 bytes per staged column" : "20x");
    if (upload(&v.lut, lut)) return -1;
    if (v.resize) {
        if (dev_alloc(&v.xt, xt.size()) || dev_alloc(&v.yt, yt.size())) { u8_free(v); return -1; }
        if (hipMemcpy(v.xt, xt.data(), xt.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(v.yt, yt.data(), yt.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { u8_free(v); return td_fail("%s: table upload failed", who); }
    }
    v.bytes = lut.size() * sizeof(float) + (xt.size() + yt.size()) * sizeof(int);
    v.set = true;
    u8_free(u);
    u = v;
    return 0;
}

// tdnet_view -> (SrcView, Hs x Ws) with every default resolved, or the failure that names the offending field.  What is a property of the
// surface or of the tables (the NV12 conditions, the extent, mean / std, the staged span) is u8_build's to check.
static int view_resolve(const tdnet_view* t, SrcView& sv, int& Hs, int& Ws, const char* who) {
    if (!t) return td_fail("%s: view is NULL", who);
    if (t->format < 0 || t->format > TDNET_PIX_NV12) return td_fail("%s: format %d is not one of TDNET_PIX_* (0..4)", who, t->format);
    for (int i = 0; i < 5; ++i)
        if (t->reserved[i]) return td_fail("%s: reserved[%d] = %d must be 0", who, i, t->reserved[i]);
    if (t->height < 1 || t->width < 1) return td_fail("%s: height x width = %d x %d must be at least 1 x 1", who, t->height, t->width);
    const bool whole = !t->crop_y && !t->crop_x && !t->crop_height && !t->crop_width;
    const int oy = t->crop_y, ox = t->crop_x, h = whole ? t->height : t->crop_height, w = whole ? t->width : t->crop_width;
    if (oy < 0 || ox < 0) return td_fail("%s: crop_y, crop_x = %d, %d: the origin must not be negative", who, oy, ox);
    if (h < 1 || w < 1) return td_fail("%s: crop_height x crop_width = %d x %d must be at least 1 x 1", who, h, w);
    if (h > t->height || oy > t->height - h) return td_fail("%s: crop_y + crop_height = %d + %d is not inside the frame's height %d", who, oy, h, t->height);
    if (w > t->width || ox > t->width - w) return td_fail("%s: crop_x + crop_width = %d + %d is not inside the frame's width %d", who, ox, w, t->width);
    const bool nv = t->format == TDNET_PIX_NV12;
    const int bpp = src_view_bpp(t->format);
    if (t->pitch < 0) return td_fail("%s: pitch %d is negative", who, t->pitch);
    sv = SrcView();
    sv.format = t->format; sv.fh = t->height; sv.fw = t->width; sv.oy = oy; sv.ox = ox;
    if (nv) {
        sv.pitch = t->pitch ? t->pitch : 2 * ((t->width - 1) / 2 + 1);
        if (!t->uv_offset && (double)t->height * sv.pitch >= 2147483648.0)
            return td_fail("%s: the surface's extent (height %d, pitch %d) is 2^31 bytes or more", who, t->height, sv.pitch);
        sv.uv_offset = t->uv_offset ? (size_t)t->uv_offset : (size_t)t->height * sv.pitch;
        sv.standard = t->standard;
    } else {
        if (t->standard) return td_fail("%s: standard = %d must be 0 for a packed format", who, t->standard);
        if (t->uv_offset) return td_fail("%s: uv_offset = %llu must be 0 for a packed format", who, (unsigned long long)t->uv_offset);
        const double row = (double)t->width * bpp;
        if (row >= 2147483648.0) return td_fail("%s: the frame's extent (a row of %d pixels) is 2^31 bytes or more", who, t->width);
        if (t->pitch && t->pitch < (int)row) return td_fail("%s: pitch %d is below the %d bytes a row of %d pixels holds", who, t->pitch, (int)row, t->width);
        sv.pitch = t->pitch ? t->pitch : (int)row;
        if ((double)(t->height - 1) * sv.pitch + row >= 2147483648.0)
            return td_fail("%s: the frame's extent (pitch %d, %d rows) is 2^31 bytes or more", who, sv.pitch, t->height);
    }
    Hs = h; Ws = w;
    return 0;
}
// the configuration in force is the one these arguments would build (a packed pitch of 0 as u8_build resolves it)
static bool u8_same(const U8Input& u, const SrcView& sv, int Hs, int Ws, const double* m, const double* sd) {
    if (u.surf != sv.surf) return false;
    if (sv.surf && (u.layout != sv.layout || u.cpitch != sv.cpitch || u.u_off != sv.u_off || u.v_off != sv.v_off || u.standard != sv.standard)) return false;
    if (!u.set || u.format != sv.format || u.Hs != Hs || u.Ws != Ws || u.fh != sv.fh || u.fw != sv.fw || u.oy != sv.oy || u.ox != sv.ox) return false;
    const bool nv = sv.format == TDNET_PIX_NV12 && !sv.surf;
    const long pitch = nv || sv.pitch ? sv.pitch : (long)sv.fw * src_view_bpp(sv.format);
    if (u.pitch != pitch || (nv && (u.uv_offset != sv.uv_offset || u.standard != sv.standard))) return false;
    return memcmp(u.mean, m, sizeof(u.mean)) == 0 && memcmp(u.std, sd, sizeof(u.std)) == 0;
}

// tdnet_view -> the destination view it describes, or the failure that names the offending field.  On failure `d` is left as it was.
static int dst_build(DstOutput& d, const tdnet_view* t, const char* who) {
    SrcView sv;
    int h = 0, w = 0;
    TD_TRY(view_resolve(t, sv, h, w, who));
    double extent = 0.0;
    TD_TRY(view_surface_check(sv, sv.pitch, who, &extent));
    if (h > 65535) return td_fail("%s: the rectangle's height %d is above the grid's 65535 rows", who, h);
    const bool nv = sv.format == TDNET_PIX_NV12;
    if (nv && (sv.oy & 1)) return td_fail("%s: crop_y = %d must be even for an NV12 destination (the rectangle starts on the chroma grid)", who, sv.oy);
    if (nv && (sv.ox & 1)) return td_fail("%s: crop_x = %d must be even for an NV12 destination (the rectangle starts on the chroma grid)", who, sv.ox);
    DstOutput v;
    v.set = true;
    v.format = sv.format; v.bpp = src_view_bpp(sv.format); v.swap = sv.format == TDNET_PIX_BGR24 || sv.format == TDNET_PIX_BGRA32;
    v.fh = sv.fh; v.fw = sv.fw; v.oy = sv.oy; v.ox = sv.ox; v.h = h; v.w = w; v.pitch = sv.pitch; v.extent = (size_t)extent;
    if (nv) {
        v.uv_offset = sv.uv_offset; v.standard = sv.standard;
        nv12_forward_coeffs(sv.standard, &v.yoff, v.ky, v.ku, v.kv);
    }
    d = v;
    return 0;
}

// tdnet_surface -> the destination surface it describes, or the failure that names the offending field.  On failure `d` is left as it was.
static int dst_surface_build(DstOutput& d, const tdnet_surface* t, const char* who) {
    if (t && (t->layout == TDNET_SURF_YUY2 || t->layout == TDNET_SURF_UYVY))
        return td_fail("%s: layout %d (%s) is not a destination layout: no encoder takes packed 4:2:2 (NV12, NV21, I420 and P010 are)", who, t->layout,
                       t->layout == TDNET_SURF_YUY2 ? "YUY2" : "UYVY");
    SrcView sv;
    int h = 0, w = 0;
    TD_TRY(surface_resolve(t, sv, h, w, who));
    if (h > 65535) return td_fail("%s: the rectangle's height %d is above the grid's 65535 rows", who, h);
    if (sv.oy & 1) return td_fail("%s: crop_y = %d must be even for a 4:2:0 destination (the rectangle starts on the chroma grid)", who, sv.oy);
    if (sv.ox & 1) return td_fail("%s: crop_x = %d must be even for a 4:2:0 destination (the rectangle starts on the chroma grid)", who, sv.ox);
    DstOutput v;
    v.set = true; v.surf = true;
    v.format = TDNET_PIX_NV12; v.bpp = 1; v.layout = sv.layout;
    v.fh = sv.fh; v.fw = sv.fw; v.oy = sv.oy; v.ox = sv.ox; v.h = h; v.w = w; v.pitch = sv.pitch; v.cpitch = sv.cpitch; v.extent = sv.extent;
    v.u_off = sv.u_off; v.v_off = sv.v_off; v.uv_offset = sv.u_off; v.standard = sv.standard;
    nv12_forward_coeffs(sv.standard, &v.yoff, v.ky, v.ku, v.kv);
    d = v;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// colour-map output: the host side of td_out.h's colour map (TD_SRC_NONE)
// ---------------------------------------------------------------------------------------------------------------
// tdnet_amd/dataloader.py nearest_index with the same operations in the same types: the quotient first, in double, then the product, then
// truncation, then the clamp.  This is the project's rule (tdnet_amd/test.py's resize of the label map since its first version), not cv2's text.
static void rgb_nearest_index(int n_src, int n_dst, std::vector<int>& idx) {
    const double scale = (double)n_src / (double)n_dst;
    idx.resize(n_dst);
    for (int o = 0; o < n_dst; ++o) idx[o] = (int)std::min<long>((long)((double)o * scale), (long)n_src - 1);
}
static void rgb_free(RgbOutput& r) {
    if (r.ys) hipFree(r.ys);
    if (r.xs) hipFree(r.xs);
    if (r.lut) hipFree(r.lut);
    r = RgbOutput();
}
static bool rgb_same(const RgbOutput& r, int oh, int ow, const unsigned char* palette, int n_colours) {
    return r.set && r.oh == oh && r.ow == ow && r.n_colours == n_colours && palette && n_colours >= 1 && n_colours <= 256 &&
           memcmp(r.palette, palette, (size_t)3 * n_colours) == 0;
}
// Validate, build the two index tables and the 256-entry colour table on the host and upload them into memory `r` owns.  On failure `r` is
// left as it was.
static int rgb_build(RgbOutput& r, int H, int W, int oh, int ow, const unsigned char* palette, int n_colours, const char* who) {
    if (oh < 1 || ow < 1) return td_fail("%s: output size %d x %d must be at least 1 x 1", who, oh, ow);
    if (oh > 65535) return td_fail("%s: out_height = %d is above the grid's 65535 rows", who, oh);
    if ((double)oh * ow * 3 >= 2147483648.0) return td_fail("%s: output size %d x %d is too large", who, oh, ow);
    if (n_colours < 1 || n_colours > 256) return td_fail("%s: n_colours = %d must be in 1..256", who, n_colours);
    if (!palette) return td_fail("%s: palette_rgb is NULL (the library carries no colour table of its own)", who);
    if (H < 1 || W < 1) return td_fail("%s: network size %d x %d out of range", who, H, W);
    RgbOutput v;
    v.H = H; v.W = W; v.oh = oh; v.ow = ow; v.n_colours = n_colours;
    memcpy(v.palette, palette, (size_t)3 * n_colours);
    std::vector<int> ys, xs;
    rgb_nearest_index(H, oh, ys);
    rgb_nearest_index(W, ow, xs);
    std::vector<unsigned> lut(256);
    for (unsigned l = 0; l < 256; ++l)                                 // decode_segmap: a label outside the table keeps its value in all three channels
        lut[l] = (int)l < n_colours ? (unsigned)palette[3 * l] | ((unsigned)palette[3 * l + 1] << 8) | ((unsigned)palette[3 * l + 2] << 16) : l * 0x010101u;
    if (dev_alloc(&v.ys, ys.size()) || dev_alloc(&v.xs, xs.size()) || dev_alloc(&v.lut, lut.size())) { rgb_free(v); return -1; }
    if (hipMemcpy(v.ys, ys.data(), ys.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v.xs, xs.data(), xs.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v.lut, lut.data(), lut.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess) { rgb_free(v); return td_fail("%s: table upload failed", who); }
    v.bytes = (ys.size() + xs.size()) * sizeof(int) + lut.size() * sizeof(unsigned);
    v.set = true;
    rgb_free(r);
    r = v;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// overlay output: the host side of td_out.h's overlay (td_src_px4, td_overlay_blend)
// ---------------------------------------------------------------------------------------------------------------
static void overlay_free_tables(OverlayOutput& o) {
    if (o.ys) hipFree(o.ys);
    if (o.xs) hipFree(o.xs);
    o.bytes -= ((size_t)o.Hs + (size_t)o.Ws) * sizeof(int);
    o.ys = o.xs = nullptr;
    o.H = o.W = o.Hs = o.Ws = 0;
}
static void overlay_free(OverlayOutput& o) {
    if (o.Hs) overlay_free_tables(o);
    if (o.lut) hipFree(o.lut);
    o = OverlayOutput();
}
static bool overlay_same(const OverlayOutput& o, const unsigned char* palette, int n_colours) {
    return o.set && o.n_colours == n_colours && palette && n_colours >= 1 && n_colours <= 256 && memcmp(o.palette, palette, (size_t)4 * n_colours) == 0;
}
// Validate and upload the 256-word colour + opacity table.  The index tables are not its business (overlay_tables).  On failure `o` is left as it was.
static void overlay_lut_words(const unsigned char* palette, int n_colours, bool swap, std::vector<unsigned>& lut) {
    lut.assign(256, 0u);                                               // a label outside the table has a = 0: the source pixel shows through
    for (int l = 0; l < n_colours; ++l)
        lut[l] = (unsigned)palette[4 * l + (swap ? 2 : 0)] | ((unsigned)palette[4 * l + 1] << 8) | ((unsigned)palette[4 * l + (swap ? 0 : 2)] << 16) | ((unsigned)palette[4 * l + 3] << 24);
}
// The colour order follows the source's (include/tdnet.h "source views"): the blend is per channel, so a b g r source is the r g b path with the
// table's r and b exchanged.  The caller has synchronised (a byte-input configuration call).
static int overlay_set_swap(OverlayOutput& o, bool swap, const char* who) {
    if (!o.set || o.swap == swap) return 0;
    std::vector<unsigned> lut;
    overlay_lut_words(o.palette, o.n_colours, swap, lut);
    if (hipMemcpy(o.lut, lut.data(), lut.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess) return td_fail("%s: overlay: table upload failed", who);
    o.swap = swap;
    return 0;
}
static int overlay_build(OverlayOutput& o, const unsigned char* palette, int n_colours, const char* who, bool swap = false) {
    if (n_colours < 1 || n_colours > 256) return td_fail("%s: n_colours = %d must be in 1..256", who, n_colours);
    if (!palette) return td_fail("%s: palette_rgba is NULL (the library carries no colour table of its own)", who);
    std::vector<unsigned> lut;
    overlay_lut_words(palette, n_colours, swap, lut);
    unsigned* d = nullptr;
    if (dev_alloc(&d, lut.size())) return -1;
    if (hipMemcpy(d, lut.data(), lut.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return td_fail("%s: table upload failed", who); }
    if (o.lut) hipFree(o.lut);
    else o.bytes += lut.size() * sizeof(unsigned);
    o.lut = d;
    o.n_colours = n_colours;
    o.swap = swap;
    memset(o.palette, 0, sizeof(o.palette));
    memcpy(o.palette, palette, (size_t)4 * n_colours);
    o.set = true;
    return 0;
}
// The index tables of the pair (network H x W, source Hs x Ws): built when the overlay is configured on a handle that has a byte input, and again
// when a later byte-input configuration changes the source size.  On failure the tables are gone (a frame entry then says so).
static int overlay_tables(OverlayOutput& o, int H, int W, int Hs, int Ws, const char* who) {
    if (o.Hs == Hs && o.Ws == Ws && o.H == H && o.W == W) return 0;
    if (o.Hs) overlay_free_tables(o);
    if (Hs < 1 || Ws < 1 || H < 1 || W < 1) return td_fail("%s: overlay: sizes must be at least 1 x 1", who);
    if (Hs > 65535) return td_fail("%s: overlay: src_height = %d is above the grid's 65535 rows", who, Hs);
    if ((double)Hs * Ws * 3 >= 2147483648.0) return td_fail("%s: overlay: a %d x %d picture is too large", who, Hs, Ws);
    std::vector<int> ys, xs;
    rgb_nearest_index(H, Hs, ys);
    rgb_nearest_index(W, Ws, xs);
    int *dy = nullptr, *dx = nullptr;
    if (dev_alloc(&dy, ys.size()) || dev_alloc(&dx, xs.size())) { if (dy) hipFree(dy); return -1; }
    if (hipMemcpy(dy, ys.data(), ys.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dx, xs.data(), xs.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { hipFree(dy); hipFree(dx); return td_fail("%s: overlay: table upload failed", who); }
    o.ys = dy; o.xs = dx;
    o.H = H; o.W = W; o.Hs = Hs; o.Ws = Ws;
    o.bytes += (ys.size() + xs.size()) * sizeof(int);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// score output: the host side of td_score.h's k_upsample_argmax_score / k_labels_score
// ---------------------------------------------------------------------------------------------------------------
static void score_free(ScoreOutput& c) {
    if (c.cm) hipFree(c.cm);
    if (c.dmap) hipFree(c.dmap);
    c = ScoreOutput();
}
static void score_map_or_identity(const unsigned char* gt_map, unsigned char* out) {
    for (int i = 0; i < 256; ++i) out[i] = gt_map ? gt_map[i] : (unsigned char)i;
}
// Allocate the zeroed matrix and upload the 256-byte map (gt_map == NULL: identity) into memory `c` owns.  On failure `c` is left as it was.
static int score_build(ScoreOutput& c, int nclass, const unsigned char* gt_map, const char* who) {
    if (nclass < 1 || nclass > 256) return td_fail("%s: nclass = %d must be in 1..256", who, nclass);
    ScoreOutput v;
    v.nclass = nclass;
    score_map_or_identity(gt_map, v.map);
    const size_t bins = (size_t)nclass * nclass;
    if (dev_alloc(&v.cm, bins) || dev_alloc(&v.dmap, 256)) { score_free(v); return -1; }
    if (hipMemset(v.cm, 0, bins * sizeof(unsigned long long)) != hipSuccess ||
        hipMemcpy(v.dmap, v.map, 256, hipMemcpyHostToDevice) != hipSuccess) { score_free(v); return td_fail("%s: matrix / map upload failed", who); }
    v.bytes = bins * sizeof(unsigned long long) + 256;
    v.set = true;
    score_free(c);
    c = v;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// regions output: the host side of td_regions.h's workspace
// ---------------------------------------------------------------------------------------------------------------
static void regions_free(RegionsOutput& r) {
    for (int* q : {r.parent, r.root, r.area, r.blk}) if (q) hipFree(q);
    if (r.flag) hipFree(r.flag);
    if (r.lab) hipFree(r.lab);
    r = RegionsOutput();
}
static long regions_blocks(int H, int W) { return ((long)H * W + TD_RG_BLOCK - 1) / TD_RG_BLOCK; }
static size_t regions_table_bytes(int max_regions) { return sizeof(TdRegionsHeader) + (size_t)max_regions * sizeof(TdRegion); }
// What the kernels can address: a raster index is an int, a wave's coordinate sum 32 bits
static int regions_size_check(int H, int W, const char* who) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (long)H * W > TD_RG_MAX_PIXELS) return td_fail("%s: a map of %d x %d is outside 1..65535 per side and 2^30 - 16 pixels", who, H, W);
    return 0;
}
// Allocate the workspace of an H x W map (the flag word zeroed) into memory `r` owns; the configuration fields are the caller's.  On failure `r` is left as it was.
static int regions_alloc(RegionsOutput& r, int H, int W, const char* who) {
    TD_TRY(regions_size_check(H, W, who));
    RegionsOutput v;
    const size_t HW = (size_t)H * W, nblk = (size_t)regions_blocks(H, W);
    if (dev_alloc(&v.parent, HW) || dev_alloc(&v.root, HW) || dev_alloc(&v.area, HW) || dev_alloc(&v.blk, nblk) || dev_alloc(&v.flag, 1) || dev_alloc(&v.lab, HW)) {
        regions_free(v);
        return -1;
    }
    if (hipMemset(v.flag, 0, sizeof(unsigned)) != hipSuccess) { regions_free(v); return td_fail("%s: clearing the workspace failed", who); }
    v.H = H; v.W = W;
    v.bytes = 3 * HW * sizeof(int) + nblk * sizeof(int) + sizeof(unsigned) + HW;
    regions_free(r);
    r = v;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// tracks output: the host side of td_tracks.h's state
// ---------------------------------------------------------------------------------------------------------------
// The pair table's size: the power of two >= 2 H W slots (at least 2), so that the H W distinct pairs a frame can have never fill it beyond half
static int tracks_hash_lg(int H, int W) {
    int lg = 1;
    while ((1l << lg) < 2 * (long)H * W) ++lg;
    return lg;
}
static size_t tracks_table_bytes(int max_regions) { return sizeof(TdTracksHeader) + (size_t)max_regions * sizeof(TdTrack); }
// Where the parts of an H x W state lie inside a blob at `base` (16-byte aligned; NULL: only the size is wanted); every part starts on a 16-byte boundary.
// The layout depends on H and W alone: the ceiling of 65536 regions, not the max_regions in force.
static size_t tracks_layout(void* base, int H, int W, TracksState* st) {
    const size_t HW = (size_t)H * W, R = TD_TK_MAX_REGIONS;
    const int lg = tracks_hash_lg(H, W);
    size_t off = 0;
    char* b = (char*)base;
    auto take = [&](size_t bytes) { char* q = b ? b + off : nullptr; off += (bytes + 15) & ~(size_t)15; return q; };
    TracksState v = TracksState();
    v.words = (unsigned*)take(4 * sizeof(unsigned));
    v.prev = (int*)take(HW * sizeof(int));
    v.cur = (int*)take(HW * sizeof(int));
    v.hash = (td_u64*)take(((size_t)1 << lg) * sizeof(td_u64));
    v.best_prev = (td_u64*)take(R * sizeof(td_u64));
    v.best_cur = (td_u64*)take(R * sizeof(td_u64));
    v.lab = (int*)take(R * sizeof(int));
    v.track = (unsigned*)take(R * sizeof(unsigned));
    v.age = (unsigned*)take(R * sizeof(unsigned));
    v.lg = lg;
    if (st) *st = v;
    return off;
}
static void tracks_free(TracksOutput& t) {
    if (t.blob) hipFree(t.blob);
    t = TracksOutput();
}
// Allocate and zero (the reset state) the state of an H x W map into memory `t` owns.  On failure `t` is left as it was.
static int tracks_alloc(TracksOutput& t, int H, int W, const char* who) {
    TD_TRY(regions_size_check(H, W, who));
    TracksOutput v;
    v.bytes = tracks_layout(nullptr, H, W, nullptr);
    unsigned char* blob = nullptr;
    if (dev_alloc(&blob, v.bytes)) return -1;
    v.blob = blob;
    if (hipMemset(v.blob, 0, v.bytes) != hipSuccess) { tracks_free(v); return td_fail("%s: clearing the track state failed", who); }
    tracks_layout(v.blob, H, W, &v.st);
    tracks_free(t);
    t = v;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// runs output: the host side of td_runs.h's workspace
// ---------------------------------------------------------------------------------------------------------------
static void runs_free(RunsState& r) {
    if (r.blk) hipFree(r.blk);
    if (r.lab) hipFree(r.lab);
    r = RunsState();
}
// refined matte: the workspace of RefineState for a source of Hs x Ws.  On failure `r` is left as it was; radius and eps are the caller's.
static void refine_free(RefineState& r) {
    if (r.luma) hipFree(r.luma);
    if (r.msrc) hipFree(r.msrc);
    if (r.refined) hipFree(r.refined);
    if (r.scratch) hipFree(r.scratch);
    if (r.idy) hipFree(r.idy);
    if (r.idx) hipFree(r.idx);
    const int radius = r.radius, eps = r.eps;
    r = RefineState();
    r.radius = radius; r.eps = eps;
}
static int refine_alloc(RefineState& r, int Hs, int Ws, const char* who) {
    if (r.luma && r.Hs == Hs && r.Ws == Ws) return 0;
    if (Hs < 1 || Ws < 1 || Hs > 65535 || Ws > 65535 || (long)Hs * Ws > TD_RG_MAX_PIXELS)
        return td_fail("%s: a source of %d x %d is outside 1..65535 per side and 2^30 - 16 pixels", who, Hs, Ws);
    RefineState v;
    const size_t n = (size_t)Hs * Ws;
    std::vector<int> id((size_t)(Hs > Ws ? Hs : Ws));
    for (size_t i = 0; i < id.size(); ++i) id[i] = (int)i;
    if (dev_alloc(&v.luma, n) || dev_alloc(&v.msrc, n) || dev_alloc(&v.refined, n) || dev_alloc(&v.scratch, (6 * n + 3) / 4) || dev_alloc(&v.idy, (size_t)Hs) ||
        dev_alloc(&v.idx, (size_t)Ws) || hipMemcpy(v.idy, id.data(), (size_t)Hs * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v.idx, id.data(), (size_t)Ws * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        refine_free(v);
        return td_fail("%s: allocating the refined matte's workspace for a %d x %d source failed", who, Hs, Ws);
    }
    v.Hs = Hs; v.Ws = Ws;
    v.bytes = 9 * n + ((size_t)Hs + Ws) * sizeof(int);
    v.radius = r.radius; v.eps = r.eps;
    refine_free(r);
    r = v;
    return 0;
}
// the flat launches' grid: H W / 4 aligned groups, the head lane and a tail lane (td_out.h out_grid_run's count)
static long runs_blocks(int H, int W) { return ((long)H * W / 4 + 2 + TD_RN_LANES - 1) / TD_RN_LANES; }
static size_t runs_table_bytes(int max_runs) { return sizeof(TdRunsHeader) + ((size_t)max_runs + 1) * sizeof(TdRun); }
// Allocate the workspace of an H x W map into memory `r` owns (with_map: the byte map too); max_runs is the caller's.  On failure `r` is left as it was.
static int runs_alloc(RunsState& r, int H, int W, bool with_map, const char* who) {
    TD_TRY(regions_size_check(H, W, who));
    RunsState v;
    const size_t HW = (size_t)H * W, nblk = (size_t)runs_blocks(H, W);
    if (dev_alloc(&v.blk, nblk) || (with_map && dev_alloc(&v.lab, HW))) { runs_free(v); return -1; }
    v.H = H; v.W = W;
    v.bytes = nblk * sizeof(int) + (with_map ? HW : 0);
    runs_free(r);
    r = v;
    return 0;
}
