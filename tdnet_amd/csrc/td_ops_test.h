// td_ops_test.h -- single-operator entry points (tests/ check each kernel family against torch fp32 through them) and the roofline /
// tuning probes of include/tdnet_test.h.  NOT in the product library: libtdnet_hip.so (td_model.hip) is built without this file; the
// tests' libtdnet_hip_test.so (td_model_test.hip = td_model.hip + this file) and the emulator library carry it.
#pragma once
#include "td_frame.h"

// ---------------------------------------------------------------------------------------------------------------
// single-operator entry points (tests)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int tdnet_op_conv2d(const float* in, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout, int KS,
                               int stride, int dil, const float* resid, int act, const tdnet_opts* opts, int tile, float* out,
                               void* stream) {
    // tile < 0: the heuristic's tile for this shape; 0..CT_COUNT-1: forced (0: 128x128, 1: 64x128, 2: 128x64, 3..5: the same on the
    // two-stage pipeline) -- lets tests cover every variant
    if (KS != 1 && KS != 3) return td_fail("tdnet_op_conv2d: KS must be 1 or 3");
    if (tile >= CT_COUNT) return td_fail("tdnet_op_conv2d: tile must be < %d", CT_COUNT);
    const tdnet_opts o = opts_or_default(opts);
    ConvLayer L;
    std::vector<float> w(w_host, w_host + (size_t)Cout * Cin * KS * KS), b;
    if (bias_host) b.assign(bias_host, bias_host + Cout);
    const int pad = dil * (KS / 2);
    const long M = (long)out_size(H, KS, stride, dil, pad) * out_size(W, KS, stride, dil, pad);
    // tdnet_opts.overlap bit 1: an even-dilation Winograd conv runs as its two row-parity chunks (here one after the other)
    if (plan_conv(L, Cout, Cin, KS, stride, dil, act, false, M, o, tile < 0 ? -1 : tile, (o.overlap & TDNET_OVERLAP_CHAINS) ? 2 : 1) || upload_conv(L, w, b)) return -1;
    int rc = run_conv(nullptr, L, in, H, W, resid, out, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_conv2d: device error");
    free_conv_layer(L);
    return rc;
}
// The plan of tdnet_op_conv_wino_f64 (and tdnet_bench_conv's tile -2): the fused 64-channel Winograd route (fusion bit 4194304, td_wino_f64.h) whatever the
// map size -- plan_conv's own rule with the size it asks for.  An error, nothing allocated, for a conv the route does not take.
static int op_plan_wino_f64(const char* who, ConvLayer& L, int H, int W, int Cin, int Cout, int KS, int stride, int dil, int act) {
    tdnet_opts o = opts_or_default(nullptr);
    o.fusion |= TDNET_FUSION_WINO_F64;
    if (H < 1 || W < 1) return td_fail("%s: empty input", who);
    if (!plan_wino_f64(o, Cout, Cin, KS, stride, dil, act, false, false, 1))
        return td_fail("%s: the fused Winograd kernel takes a 3x3 stride-1 dilation-1 conv from 64 to 64 channels with act 0 or 1 (got %d -> %d, KS %d, stride %d, dil %d, act %d)",
                       who, Cin, Cout, KS, stride, dil, act);
    if (!wino_f64_size_ok(H, W))
        return td_fail("%s: the fused Winograd kernel addresses a map of at most %ld pixels with its 32-bit byte offsets (got %d x %d)", who, TD_WINO_F64_MAX_PIXELS, H, W);
    TD_TRY(plan_conv(L, Cout, Cin, KS, stride, dil, act, false, std::max<long>((long)H * W, TD_WINO_F64_MIN_PIXELS), o));
    if (L.route != CR_WINO_F64) return td_fail("%s: internal: the conv was not planned on the fused Winograd kernel", who);
    return 0;
}
// A conv on the fused 64-channel Winograd F(4x4) kernel (k_wino4_f64) at ANY map size -- a frame takes the route from TD_WINO_F64_MIN_PIXELS output pixels on.
// Arguments as tdnet_op_conv2d's (resid may be NULL).
extern "C" int tdnet_op_conv_wino_f64(const float* in, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout, int KS,
                                      int stride, int dil, const float* resid, int act, float* out, void* stream) {
    const char* who = "tdnet_op_conv_wino_f64";
    if (!in || !w_host || !out) return td_fail("%s: in, weight and out expected", who);
    ConvLayer L;
    TD_TRY(op_plan_wino_f64(who, L, H, W, Cin, Cout, KS, stride, dil, act));
    std::vector<float> w(w_host, w_host + (size_t)Cout * Cin * KS * KS), b;
    if (bias_host) b.assign(bias_host, bias_host + Cout);
    int rc = upload_conv(L, w, b);
    if (!rc) rc = run_conv(nullptr, L, in, H, W, resid, out, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    free_conv_layer(L);
    return rc;
}
// The plan of a conv of tdnet_op_conv2d_f16io / _f16mix: tile code -> forced tile / LDS-DMA form, then plan_conv with precision = 1.  Shared by the single-conv entries and
// tdnet_op_conv_group_f16, so that a group's member is the layer the single entry runs.  Nothing is allocated.
static int op_plan_conv_h(const char* who, ConvLayer& L, int H, int W, int Cin, int Cout, int KS, int stride, int dil, int act, int tile, bool in16, bool out16) {
    if (KS != 1 && KS != 3) return td_fail("%s: KS must be 1 or 3", who);
    if (H < 1 || W < 1 || Cout < 1 || stride < 1 || dil < 1) return td_fail("%s: empty input", who);
    if (Cin < 64 || Cin % 64) return td_fail("%s: Cin must be a multiple of 64", who);
    // tile 16 / 17 / 18 / 19: the LDS-DMA kernel with 128 / 192 / 256-row tiles, 256 x 256 (td_conv_hd.h); 21: 128 rows on two LDS buffers
    // whatever the grid (16 chooses by the grid); 22: 128 rows, eight waves; 25 / 26: 192 / 128 rows on row images with one barrier per K
    // step; 27 / 28: 256 / 192 rows in the early-landing form only; -1: the heuristic (DMA kernel where it applies)
    const bool no_rowimg = tile >= 48 && tile <= 61;                   // 48 + code: the same tile, tap-by-tap staging (k_conv_dma_h) instead of row images
    if (no_rowimg) tile -= 32;
    static const int code_of_tile[14] = {CD_128, CD_192, CD_256, CD_256x256, CD_NONE, CD_128_2BUF, CD_128_8W,            // 16 .. 22
                                         CD_NONE, CD_NONE, CD_192_STEP, CD_128_STEP, CD_256_EARLY, CD_192_EARLY, CD_NONE};   // 23 .. 29
    static const int code_of_tile_p[6] = {CD_128_P, CD_192_P, CD_NONE,         // 31 / 32: row images with four dedicated loader waves (k_conv_dma_h3p)
                                          CD_128_N, CD_192_N, CD_NONE};        // 34 / 35: narrow tiles, rows x 64 channels (k_conv_dma_h3n)
    if (tile == 30) return td_fail("%s: tile 30 (the weights-resident 64 -> 64 kernel) was removed in round 5", who);
    const int force_rh = tile >= 16 && tile <= 29 ? code_of_tile[tile - 16] : tile >= 31 && tile <= 36 ? code_of_tile_p[tile - 31] : 0;
    if (((tile >= 16 && tile <= 29) || (tile >= 31 && tile <= 36)) && !force_rh)
        return td_fail("%s: tile %d names an LDS-DMA form that was removed (no frame launches it)", who, tile);
    if (force_rh && !in16) return td_fail("%s: tile %d is an LDS-DMA form, which reads an fp16 map (in16)", who, tile);
    if (force_rh) tile = CT_128x128_DEEP;
    if (tile >= CT_COUNT) return td_fail("%s: tile must be < %d or 16..36 (+ 32 for 16..29)", who, CT_COUNT);
    tdnet_opts o = opts_or_default(nullptr);
    o.precision = 1;
    const int pad = dil * (KS / 2);
    const int Ho = out_size(H, KS, stride, dil, pad), Wo = out_size(W, KS, stride, dil, pad);
    // the LDS-DMA form of an fp16 input map: the forced one, or for tile -1 by the map's size alone (RH_BY_SIZE -- not the frame's rule), else none
    if (plan_conv(L, Cout, Cin, KS, stride, dil, act, false, (long)Ho * Wo, o, tile < 0 ? -1 : tile, 1, in16, out16, force_rh ? force_rh : tile < 0 ? RH_BY_SIZE : CD_NONE, no_rowimg)) return -1;
    if (force_rh == CD_256x256 && L.CoutPad % 256) return td_fail("%s: the 256 x 256 tile needs Cout padded to a multiple of 256", who);
    if (force_rh && !conv_dma_supports(Cin, Cout, KS, L.tile)) return td_fail("%s: this shape cannot run on the LDS-DMA kernel", who);
    return 0;
}
// The fp16-MFMA conv of tdnet_opts.precision = 1 with the storage a frame gives it: in16: the input and the residual are rounded to fp16 maps in
// HBM (k_f2h) and the kernel reads those (IN16; the residual's type follows the input's), else it reads the fp32 arguments and rounds while staging;
// out16: the kernel writes an fp16 map (OUT16) that is widened into out (k_h2f), else it writes out.  The output never aliases the residual.
static int op_conv2d_h(const char* who, const float* in, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout,
                       int KS, int stride, int dil, const float* resid, int act, int tile, bool in16, bool out16, float* out, void* stream) {
    ConvLayer L;
    TD_TRY(op_plan_conv_h(who, L, H, W, Cin, Cout, KS, stride, dil, act, tile, in16, out16));
    hipStream_t s = (hipStream_t)stream;
    std::vector<float> w(w_host, w_host + (size_t)Cout * Cin * KS * KS), b;
    if (bias_host) b.assign(bias_host, bias_host + Cout);
    const int Ho = out_size(H, KS, stride, dil, L.pad), Wo = out_size(W, KS, stride, dil, L.pad);
    _Float16 *hin = nullptr, *hres = nullptr, *hout = nullptr;
    const long nin = (long)H * W * Cin, nout = (long)Ho * Wo * Cout;
    auto cleanup = [&]() {                                             // one release path, also for the error returns
        for (_Float16* q : {hin, hout, hres}) if (q) hipFree(q);
        free_conv_layer(L);
    };
    if (upload_conv(L, w, b) || (in16 && dev_alloc(&hin, (size_t)nin)) || (out16 && dev_alloc(&hout, (size_t)nout)) ||
        (in16 && resid && dev_alloc(&hres, (size_t)nout))) { cleanup(); return -1; }
    if (in16) TD_LAUNCH(k_f2h, dim3(td_grid_for(nin)), dim3(256), 0, s, in, hin, nin);
    if (in16 && resid) TD_LAUNCH(k_f2h, dim3(td_grid_for(nout)), dim3(256), 0, s, resid, hres, nout);
    int rc = run_conv(nullptr, L, in16 ? (const float*)hin : in, H, W, in16 ? (const float*)hres : resid, out16 ? (float*)hout : out, s);
    if (out16) TD_LAUNCH(k_h2f, dim3(td_grid_for(nout)), dim3(256), 0, s, (const _Float16*)hout, out, nout);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    cleanup();
    return rc;
}
// Test entry for the fp16-activation storage of tdnet_opts.precision = 1: the fp32 arguments are rounded to fp16 maps in HBM, the
// conv runs with fp16 input / residual / output (k_conv_igemm_h<.., IN16, OUT16>), and the fp16 result is widened into out.
extern "C" int tdnet_op_conv2d_f16io(const float* in, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout,
                                     int KS, int stride, int dil, const float* resid, int act, int tile, float* out, void* stream) {
    return op_conv2d_h("tdnet_op_conv2d_f16io", in, H, W, Cin, w_host, bias_host, Cout, KS, stride, dil, resid, act, tile, true, true, out, stream);
}
// The same with the storage of each side chosen: the forms only the rim of a frame's fp16 backbone reaches.  in16 = 0, out16 = 1: the deep stem's second
// conv; in16 = 1, out16 = 0: the backbone's last conv (fp16 residual, fp32 c4, not in place) and -- on the LDS-DMA tile codes and -1 -- the head conv
// reading the fp16 LayerNorm map.  The LDS-DMA codes need in16.
extern "C" int tdnet_op_conv2d_f16mix(const float* in, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout,
                                      int KS, int stride, int dil, const float* resid, int act, int tile, int in16, int out16, float* out, void* stream) {
    return op_conv2d_h("tdnet_op_conv2d_f16mix", in, H, W, Cin, w_host, bias_host, Cout, KS, stride, dil, resid, act, tile, in16 != 0, out16 != 0, out, stream);
}
// Up to three convs of tdnet_opts.precision = 1 through run_conv_group -- the grouping decision and the launch of a frame (td_launch.h; the Encoding's
// first / second layers, a BasicBlock's conv1 beside its downsample).  Member g is the layer tdnet_op_conv2d_f16mix plans for (tile, in16, out16); no
// residual.  Members that name the same in_dev read ONE fp16 map (in16), as the Encoding's first layers read z.  fusion: tdnet_opts.fusion (bit
// 131072 decides).  *grouped: 1 = k_conv_igemm_h_group ran, 0 = the members one by one.
extern "C" int tdnet_op_conv_group_f16(int ng, const float* const* in, const int* H, const int* W, const int* Cin, const float* const* w_host,
                                       const float* const* bias_host, const int* Cout, const int* KS, const int* stride, const int* dil, const int* act,
                                       float* const* out, int tile, int in16, int out16, int fusion, int* grouped, void* stream) {
    const char* who = "tdnet_op_conv_group_f16";
    if (ng < 1 || ng > 3) return td_fail("%s: 1 .. 3 members expected", who);
    hipStream_t s = (hipStream_t)stream;
    ConvLayer L[3];
    int src[3] = {0, 1, 2};                                            // the member whose fp16 input map member g reads
    long nin[3], nout[3];
    // every member is validated and planned BEFORE anything is allocated (plan_conv is host arithmetic)
    for (int g = 0; g < ng; ++g) {
        if (!in[g] || !out[g] || !w_host[g]) return td_fail("%s: member %d: in, weight and out expected", who, g);
        TD_TRY(op_plan_conv_h(who, L[g], H[g], W[g], Cin[g], Cout[g], KS[g], stride[g], dil[g], act[g], tile, in16 != 0, out16 != 0));
        nin[g] = (long)H[g] * W[g] * Cin[g];
        nout[g] = (long)out_size(H[g], KS[g], stride[g], dil[g], L[g].pad) * out_size(W[g], KS[g], stride[g], dil[g], L[g].pad) * Cout[g];
        for (int j = g - 1; j >= 0; --j)
            if (in[j] == in[g]) {
                if (nin[j] != nin[g] || W[j] != W[g]) return td_fail("%s: members %d and %d share an input of different sizes", who, j, g);
                src[g] = j;
            }
    }
    _Float16 *hin[3] = {nullptr, nullptr, nullptr}, *hout[3] = {nullptr, nullptr, nullptr};
    auto cleanup = [&]() {                                             // one release path, also for the error returns
        for (int g = 0; g < ng; ++g) {
            if (hin[g]) hipFree(hin[g]);
            if (hout[g]) hipFree(hout[g]);
            free_conv_layer(L[g]);
        }
    };
    int rc = 0;
    for (int g = 0; g < ng && !rc; ++g) {
        std::vector<float> w(w_host[g], w_host[g] + (size_t)Cout[g] * Cin[g] * KS[g] * KS[g]), b;
        if (bias_host && bias_host[g]) b.assign(bias_host[g], bias_host[g] + Cout[g]);
        if (upload_conv(L[g], w, b) || (in16 && src[g] == g && dev_alloc(&hin[g], (size_t)nin[g])) || (out16 && dev_alloc(&hout[g], (size_t)nout[g]))) rc = -1;
    }
    if (rc) { cleanup(); return rc; }
    ConvCall c[3];
    for (int g = 0; g < ng; ++g) {
        if (in16 && src[g] == g) TD_LAUNCH(k_f2h, dim3(td_grid_for(nin[g])), dim3(256), 0, s, in[g], hin[g], nin[g]);
        c[g] = ConvCall{&L[g], in16 ? (const float*)hin[src[g]] : in[g], H[g], W[g], out16 ? (float*)hout[g] : out[g]};
    }
    tdnet_opts o = opts_or_default(nullptr);
    o.precision = 1;
    o.fusion = fusion;
    rc = run_conv_group(nullptr, o, c, ng, s, nullptr, nullptr, grouped);
    for (int g = 0; g < ng; ++g)
        if (out16) TD_LAUNCH(k_h2f, dim3(td_grid_for(nout[g])), dim3(256), 0, s, (const _Float16*)hout[g], out[g], nout[g]);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    cleanup();
    return rc;
}
// Both cache entries of a frame (Encoding(pre=True)'s q_ and v_): q [h,w,C1], v [h,w,C2] -> q_out [hk,wk,C1], v_out [hk,wk,C2], the stride-4
// sub-sample, through the launch encode_frame makes (launch_cache_subsample: its grid formula, one launch for both).
extern "C" int tdnet_op_cache_subsample(const float* q, const float* v, int h, int w, int C1, int C2, float* q_out, float* v_out, void* stream) {
    if (h < 1 || w < 1 || C1 < 4 || C1 % 4 || C2 < 4 || C2 % 4) return td_fail("tdnet_op_cache_subsample: a map of at least 1 x 1 with C1, C2 multiples of 4 expected");
    if (!q || !v || !q_out || !v_out) return td_fail("tdnet_op_cache_subsample: q, v, q_out and v_out expected");
    hipStream_t s = (hipStream_t)stream;
    launch_cache_subsample(q, q_out, C1, v, v_out, C2, w, key_size(h), key_size(w), s);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) return td_fail("tdnet_op_cache_subsample: device error");
    return 0;
}
// A stride-1 1x1 conv on the image rows y = ny * i + cy only, through run_ds_rows (td_frame.h: the downsample conv of one row-parity chain -- a batched
// GEMM, batch = row).  The layer is planned for the WHOLE map, as tdnet_op_conv2d plans it with tile -1; the rows of the other classes of out are not
// written.  An error, with nothing allocated or launched, where the plan is not the persistent-GEMM route (a frame then runs no row chains).
extern "C" int tdnet_op_conv1x1_rows(const float* in, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout, int act,
                                     const tdnet_opts* opts, int ny, int cy, float* out, void* stream) {
    if (H < 1 || W < 1 || Cin < 1 || Cout < 1) return td_fail("tdnet_op_conv1x1_rows: empty input");
    if (ny < 1 || cy < 0 || cy >= ny) return td_fail("tdnet_op_conv1x1_rows: a row class cy in 0 .. ny - 1 expected");
    const tdnet_opts o = opts_or_default(opts);
    ConvLayer L;
    if (plan_conv(L, Cout, Cin, 1, 1, 1, act, false, (long)H * W, o, -1, (o.overlap & TDNET_OVERLAP_CHAINS) ? 2 : 1)) return -1;
    if (L.route != CR_GEMM1X1) return td_fail("tdnet_op_conv1x1_rows: this conv is not planned as a persistent GEMM: a frame would not run it on image rows");
    std::vector<float> w(w_host, w_host + (size_t)Cout * Cin), b;
    if (bias_host) b.assign(bias_host, bias_host + Cout);
    int rc = upload_conv(L, w, b);
    if (!rc) rc = run_ds_rows(nullptr, L, in, H, W, out, ny, cy, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_conv1x1_rows: device error");
    free_conv_layer(L);
    return rc;
}
// MaxPool2d(3, stride 2, pad 1) alone: NHWC [H,W,C] -> [Ho,Wo,C].  mode = run_maxpool's pool16: 0: k_maxpool3s2, fp32 in and out; 1: k_maxpool3s2_h<false>,
// fp32 in, the fp16 map widened into out; 2: k_maxpool3s2_h<true>, the input rounded to an fp16 map first (k_f2h).
extern "C" int tdnet_op_maxpool(const float* in, int H, int W, int C, int mode, float* out, void* stream) {
    if (H < 1 || W < 1 || C < 4 || C % 4) return td_fail("tdnet_op_maxpool: a map of at least 1 x 1 with C a multiple of 4 expected");
    if (mode < 0 || mode > 2) return td_fail("tdnet_op_maxpool: mode must be 0, 1 or 2");
    hipStream_t s = (hipStream_t)stream;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long nin = (long)H * W * C, nout = (long)Ho * Wo * C;
    _Float16 *hin = nullptr, *hout = nullptr;
    auto cleanup = [&]() { for (_Float16* q : {hin, hout}) if (q) hipFree(q); };
    if ((mode == 2 && dev_alloc(&hin, (size_t)nin)) || (mode && dev_alloc(&hout, (size_t)nout))) { cleanup(); return -1; }
    if (mode == 2) TD_LAUNCH(k_f2h, dim3(td_grid_for(nin)), dim3(256), 0, s, in, hin, nin);
    run_maxpool(nullptr, mode == 2 ? (const float*)hin : in, H, W, C, mode ? (float*)hout : out, s, mode);
    if (mode) TD_LAUNCH(k_h2f, dim3(td_grid_for(nout)), dim3(256), 0, s, (const _Float16*)hout, out, nout);
    int rc = 0;
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_maxpool: device error");
    cleanup();
    return rc;
}
// The stem as a frame of tdnet_opts.precision = 1 runs it: NCHW image -> the 7x7 conv on the fp16 MFMA writing an fp16 map (CR_STEM_H planned with
// out16) -> k_maxpool3s2_h<true> -> [H2,W2,64] widened into out.  tile: -1 = the heuristic's, else forced; a tile conv_stem_h_supports refuses --
// where a frame would fall back to the fp32 stem -- is an error before anything is allocated or launched.
extern "C" int tdnet_op_stem_f16(const float* img, int H, int W, const float* w_host, const float* bias_host, int tile, float* out, void* stream) {
    if (H < 1 || W < 1) return td_fail("tdnet_op_stem_f16: empty image");
    if (tile >= CT_COUNT) return td_fail("tdnet_op_stem_f16: tile must be < %d", CT_COUNT);
    tdnet_opts o = opts_or_default(nullptr);
    o.precision = 1;
    hipStream_t s = (hipStream_t)stream;
    const int H1 = (H - 1) / 2 + 1, W1 = (W - 1) / 2 + 1, H2 = (H1 - 1) / 2 + 1, W2 = (W1 - 1) / 2 + 1;
    ConvLayer L;
    if (plan_conv(L, 64, 3, 7, 2, 1, 1, true, (long)H1 * W1, o, tile < 0 ? -1 : tile, 1, false, true)) return -1;
    if (L.route != CR_STEM_H || !L.out16) return td_fail("tdnet_op_stem_f16: tile %d is not one the fp16-MFMA stem runs on", (int)L.tile);
    std::vector<float> w(w_host, w_host + 64 * 3 * 49), b;
    if (bias_host) b.assign(bias_host, bias_host + 64);
    float* img4 = nullptr;
    _Float16 *s1 = nullptr, *pooled = nullptr;
    auto cleanup = [&]() {
        if (img4) hipFree(img4);
        for (_Float16* q : {s1, pooled}) if (q) hipFree(q);
        free_conv_layer(L);
    };
    const long nout = (long)H2 * W2 * 64;
    if (upload_conv(L, w, b) || dev_alloc(&img4, (size_t)H * W * 4) || dev_alloc(&s1, (size_t)H1 * W1 * 64) || dev_alloc(&pooled, (size_t)nout)) { cleanup(); return -1; }
    run_stem_pre(nullptr, frame_input_f32(img), H, W, img4, s, false);
    int rc = run_conv(nullptr, L, img4, H, W, nullptr, (float*)s1, s);
    run_maxpool(nullptr, (const float*)s1, H1, W1, 64, (float*)pooled, s, 2);
    TD_LAUNCH(k_h2f, dim3(td_grid_for(nout)), dim3(256), 0, s, (const _Float16*)pooled, out, nout);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_stem_f16: device error");
    cleanup();
    return rc;
}
extern "C" int tdnet_op_stem(const float* img, int H, int W, const float* w_host, const float* bias_host, const tdnet_opts* opts,
                             float* out, void* stream) {
    const tdnet_opts o = opts_or_default(opts);
    hipStream_t s = (hipStream_t)stream;
    const int H1 = (H - 1) / 2 + 1, W1 = (W - 1) / 2 + 1;
    ConvLayer L;
    std::vector<float> w(w_host, w_host + 64 * 3 * 49), b;
    if (bias_host) b.assign(bias_host, bias_host + 64);
    if (plan_conv(L, 64, 3, 7, 2, 1, 1, true, (long)H1 * W1, o) || upload_conv(L, w, b)) return -1;
    float *img4 = nullptr, *s1 = nullptr;
    const size_t img_floats = std::max((size_t)H * W * 4, (size_t)stem_rows_hp(H) * stem_rows_wp(W) * 3 + 4);
    if (dev_alloc(&img4, img_floats) || dev_alloc(&s1, (size_t)H1 * W1 * 64)) return -1;
    if (L.stem_rows()) TD_HIP(hipMemsetAsync(img4, 0, img_floats * sizeof(float), s));   // the packed-row image's zero border
    run_stem_pre(nullptr, frame_input_f32(img), H, W, img4, s, L.stem_rows());
    run_conv(nullptr, L, img4, H, W, nullptr, s1, s);
    run_maxpool(nullptr, s1, H1, W1, 64, out, s);
    TD_HIP(hipStreamSynchronize(s));
    TD_HIP(hipGetLastError());
    hipFree(img4); hipFree(s1);
    free_conv_layer(L);
    return 0;
}
extern "C" int tdnet_op_attention(const float* q, const float* k, const float* vp, const float* bias, const float* resid, int Lq,
                                  int Lk, int DV, int online, const float* ln_g, const float* ln_b, float* ln_out, float* out,
                                  void* stream) {
    if (Lk < 1 || Lq < 1) return td_fail("tdnet_op_attention: empty input");
    hipStream_t s = (hipStream_t)stream;
    const bool padded = (online & 32) != 0;                            // online | 32: the caller's vp already has the padding rows (probes that time the kernel)
    const bool slices = (online & 64) != 0;                            // online | 64: DV = 512 as two 256-channel slices in one launch (the chain's cached-frame steps)
    online &= ~(32 | 64);
    // arguments are validated BEFORE anything is allocated; every later exit goes through cleanup()
    if (ln_out && (!ln_g || !ln_b)) return td_fail("tdnet_op_attention: ln_out needs ln_g and ln_b");
    const bool split = online >= 17 && online <= 19;                   // 17: the split kernels of precision 2 (td_attn_b3.h), form by size; 18: the 64-query form; 19: the 32-query form
    if (online != 16 && !split && (online < 0 || online > 2)) return td_fail("tdnet_op_attention: online must be 0, 1, 2 or 16 .. 19");
    float *part = nullptr, *mean = nullptr, *rstd = nullptr, *vpad = nullptr;
    _Float16* vt = nullptr;                                            // online == 16: the fp16-MFMA kernel of tdnet_opts.precision = 1 (td_attn_h.h)
    auto cleanup = [&]() {
        for (float* q2 : {part, mean, rstd, vpad}) if (q2) hipFree(q2);
        if (vt) hipFree(vt);
    };
    int rc = 0;
    if (ln_out && (dev_alloc(&part, (size_t)2 * attn_strips(Lq, DV) * DV) || dev_alloc(&mean, DV) || dev_alloc(&rstd, DV))) rc = -1;   // + plane LayerNorm of the result from the epilogue's strip statistics
    if (!rc && (online == 16 || split) && dev_alloc(&vt, (size_t)(split ? 3 : 1) * DV * attn_lkpad(Lk))) rc = -1;
    if (!rc && online != 16 && !split && !padded && attn_vp_rows(Lk) != Lk) {    // the kernels' contract: V' padded to attn_vp_rows(Lk) zero rows
        const size_t rows = (size_t)attn_vp_rows(Lk);
        if (dev_alloc(&vpad, rows * DV)) rc = -1;
        else if (hipMemsetAsync(vpad, 0, rows * DV * sizeof(float), s) != hipSuccess ||
                 hipMemcpyAsync(vpad, vp, (size_t)Lk * DV * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = td_fail("tdnet_op_attention: copy failed");
        else vp = vpad;
    }
    if (!rc) rc = run_attention(nullptr, q, k, vp, bias, resid, Lq, Lk, DV, out, s, online >= 16 ? 1 : online, part, vt, slices, false, online == 17 ? 1 : online == 18 ? 3 : online == 19 ? 2 : 0);
    if (!rc && ln_out) run_layernorm(nullptr, out, Lq, DV, ln_g, ln_b, part, mean, rstd, ln_out, s, attn_strips(Lq, DV));
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_attention: device error");
    cleanup();
    return rc;
}
extern "C" int tdnet_op_layernorm_hw(const float* x, int HW, int C, const float* g, const float* b, float* out, void* stream) {
    if (C % 4 || (C / 4 <= 256 ? 256 % (C / 4) != 0 : C / 4 > 512)) return td_fail("tdnet_op_layernorm_hw: C must be one of 4*{1,2,4,...,256} or 2048");
    float *part = nullptr, *mean = nullptr, *rstd = nullptr;
    if (dev_alloc(&part, (size_t)2 * 512 * C) || dev_alloc(&mean, C) || dev_alloc(&rstd, C)) return -1;
    run_layernorm(nullptr, x, HW, C, g, b, part, mean, rstd, out, (hipStream_t)stream);
    TD_HIP(hipStreamSynchronize((hipStream_t)stream));
    TD_HIP(hipGetLastError());
    hipFree(part); hipFree(mean); hipFree(rstd);
    return 0;
}
// The plane LayerNorm writing its map as fp16 (run_layernorm with y16: k_ln_apply_h, what the head conv of a tdnet_opts.precision = 1 frame reads), widened into out
extern "C" int tdnet_op_layernorm_hw_f16(const float* x, int HW, int C, const float* g, const float* b, float* out, void* stream) {
    if (HW < 1 || C < 4 || C % 4 || (C / 4 <= 256 ? 256 % (C / 4) != 0 : C / 4 > 512)) return td_fail("tdnet_op_layernorm_hw_f16: C must be one of 4*{1,2,4,...,256} or 2048");
    hipStream_t s = (hipStream_t)stream;
    float *part = nullptr, *mean = nullptr, *rstd = nullptr;
    _Float16* y = nullptr;
    auto cleanup = [&]() {
        for (float* q : {part, mean, rstd}) if (q) hipFree(q);
        if (y) hipFree(y);
    };
    const long n = (long)HW * C;
    if (dev_alloc(&part, (size_t)2 * 512 * C) || dev_alloc(&mean, C) || dev_alloc(&rstd, C) || dev_alloc(&y, (size_t)n)) { cleanup(); return -1; }
    run_layernorm(nullptr, x, HW, C, g, b, part, mean, rstd, (float*)y, s, 0, true);
    TD_LAUNCH(k_h2f, dim3(td_grid_for(n)), dim3(256), 0, s, (const _Float16*)y, out, n);
    int rc = 0;
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_layernorm_hw_f16: device error");
    cleanup();
    return rc;
}
extern "C" int tdnet_op_ppm(const float* c4, int h, int w, const float* w_host, const float* b_host, int path_num, int pid, float* z,
                            void* stream) {
    const int C = 512, FS = C / (path_num * 4);
    if (path_num != 2) return td_fail("tdnet_op_ppm: path_num must be 2 (td4 passes path_num//2, td2 passes 2)");
    std::vector<float> pw((size_t)4 * FS * C), pb((size_t)4 * FS);
    for (int j = 0; j < 4; ++j)
        for (int o = 0; o < FS; ++o) {
            for (int c = 0; c < C; ++c) pw[((size_t)j * C + c) * FS + o] = w_host[((size_t)j * 128 + pid * FS + o) * C + c];
            pb[j * FS + o] = b_host[j * 128 + pid * FS + o];
        }
    float *dw = nullptr, *db = nullptr, *rowpart = nullptr, *pooled = nullptr, *ppmfeat = nullptr;
    if (upload(&dw, pw) || upload(&db, pb)) return -1;
    if (dev_alloc(&rowpart, (size_t)h * 36 * C) || dev_alloc(&pooled, 50 * C) || dev_alloc(&ppmfeat, 50 * FS)) return -1;
    run_ppm(nullptr, c4, h, w, C, C / 2, FS, dw, db, pid, rowpart, pooled, ppmfeat, z, (hipStream_t)stream);
    TD_HIP(hipStreamSynchronize((hipStream_t)stream));
    TD_HIP(hipGetLastError());
    for (float* q : {dw, db, rowpart, pooled, ppmfeat}) hipFree(q);
    return 0;
}
// The first layers of a path's Encoding on c4 as a frame runs them (td_frame.h encode_frame): pyramid pooling, then the value conv (C -> DV, no activation), the
// query conv (C -> 64, LeakyReLU) and the stride-4 key conv (C -> 64, LeakyReLU), planned with the default options for an h x w map.  fold = 1: the pyramid as 64
// basis columns (fusion bit 2097152: k_ppm_fold_g + the two-source kernels; an error, before anything is allocated, where plan_enc_fold refuses); fold = 0: through
// the assembled map z.  ppm_w [4][C/4][C] / ppm_b [4][C/4]: the BN-folded pyramid convs, of which path `pid` keeps channels pid * C/8 .. of each; wv / wq / wk [Cout][C]
// and their biases likewise folded.  basis_out (device, [h w][64], may be NULL): the fold's coefficient table.
extern "C" int tdnet_op_enc_first(const float* c4, int h, int w, int C, int pid, const float* ppm_w, const float* ppm_b, const float* wv, const float* bv, int DV,
                                  const float* wq, const float* bq, const float* wk, const float* bk, int fold, float* v_out, float* q_out, float* k_out,
                                  float* basis_out, void* stream) {
    const char* who = "tdnet_op_enc_first";
    if (h < 1 || w < 1 || C < 512 || C % 512 || DV < 1 || pid < 0 || pid > 1) return td_fail("%s: a map of at least 1 x 1, C a multiple of 512 and pid 0 / 1 expected", who);
    if (!c4 || !ppm_w || !ppm_b || !wv || !wq || !wk || !v_out || !q_out || !k_out) return td_fail("%s: null argument", who);
    hipStream_t s = (hipStream_t)stream;
    const tdnet_opts o = opts_or_default(nullptr);
    const int XS = C / 2, FS = C / 8, F4 = C / 4, hk = key_size(h), wk_ = key_size(w);
    ConvLayer L[3];
    if (plan_conv(L[0], DV, C, 1, 1, 1, 0, false, (long)h * w, o) || plan_conv(L[1], 64, C, 1, 1, 1, 2, false, (long)h * w, o) ||
        plan_conv(L[2], 64, C, 1, 4, 1, 2, false, (long)hk * wk_, o)) return -1;
    if (fold && !plan_enc_fold(o, L[0], L[1], L[2], XS, FS)) return td_fail("%s: a frame would not fold these layers", who);
    std::vector<float> pw((size_t)4 * FS * C), pb((size_t)4 * FS);
    for (int j = 0; j < 4; ++j)
        for (int f = 0; f < FS; ++f) {
            for (int c = 0; c < C; ++c) pw[((size_t)j * C + c) * FS + f] = ppm_w[((size_t)j * F4 + pid * FS + f) * C + c];
            pb[j * FS + f] = ppm_b[j * F4 + pid * FS + f];
        }
    float *dw = nullptr, *db = nullptr, *rowpart = nullptr, *pooled = nullptr, *ppmfeat = nullptr, *z = nullptr, *basis = nullptr, *g[3] = {nullptr, nullptr, nullptr};
    auto cleanup = [&]() {
        for (float* q : {dw, db, rowpart, pooled, ppmfeat, z, basis, g[0], g[1], g[2]}) if (q) hipFree(q);
        for (ConvLayer& l : L) free_conv_layer(l);
    };
    const float* const wh[3] = {wv, wq, wk};
    const float* const bh[3] = {bv, bq, bk};
    int rc = 0;
    for (int i = 0; i < 3 && !rc; ++i) {
        std::vector<float> wi(wh[i], wh[i] + (size_t)L[i].Cout * C), bi;
        if (bh[i]) bi.assign(bh[i], bh[i] + L[i].Cout);
        rc = upload_conv(L[i], wi, bi);
    }
    if (!rc && (upload(&dw, pw) || upload(&db, pb) || dev_alloc(&rowpart, (size_t)h * 36 * C) || dev_alloc(&pooled, (size_t)50 * C) || dev_alloc(&ppmfeat, (size_t)50 * FS))) rc = -1;
    if (!rc && !fold && dev_alloc(&z, (size_t)h * w * C)) rc = -1;
    if (!rc && fold) {
        std::vector<float> B;
        ppm_basis_table(h, w, B);
        if (upload(&basis, B)) rc = -1;
        for (int i = 0; i < 3 && !rc; ++i) {
            const size_t cnt = (size_t)2 * 8 * L[i].CoutPad * 4;
            if (dev_alloc(&g[i], cnt) || hipMemsetAsync(g[i], 0, cnt * sizeof(float), s) != hipSuccess) rc = -1;
        }
        if (!rc && basis_out && hipMemcpyAsync(basis_out, basis, B.size() * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = td_fail("%s: copy failed", who);
    }
    float* const outs[3] = {v_out, q_out, k_out};
    if (!rc) {
        const ConvLayer* const Lp[3] = {&L[0], &L[1], &L[2]};
        const PpmFoldArgs fa = fold ? ppm_fold_args(Lp, g, ppmfeat, XS, FS) : PpmFoldArgs();
        run_ppm(nullptr, c4, h, w, C, XS, FS, dw, db, pid, rowpart, pooled, ppmfeat, z, s, fold ? &fa : nullptr);
        for (int i = 0; i < 3 && !rc; ++i)
            rc = fold ? run_conv_src2(nullptr, L[i], c4 + pid * XS, C, XS / 32, XS / 32 + TD_PPM_BASIS / 32, basis, TD_PPM_BASIS, g[i], h, w, nullptr, outs[i], s)
                      : run_conv(nullptr, L[i], z, h, w, nullptr, outs[i], s);
    }
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    cleanup();
    return rc;
}
// A 1x1 conv planned as tdnet_op_conv2d plans it, run on the TWO-SOURCE form of its kernel with nothing behind the split (k_split == nsteps, null second
// source): the same products in the same order as the one-source kernel.  An error, with nothing allocated or launched, where the plan is neither the persistent
// fp32 GEMM nor the fp32 direct 1x1 conv (those two have the form).
extern "C" int tdnet_op_conv1x1_src2_null(const float* in, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout, int stride,
                                          const float* resid, int act, const tdnet_opts* opts, int tile, float* out, void* stream) {
    const char* who = "tdnet_op_conv1x1_src2_null";
    if (H < 1 || W < 1 || Cin < 1 || Cout < 1 || stride < 1) return td_fail("%s: empty input", who);
    if (tile >= CT_COUNT) return td_fail("%s: tile must be < %d", who, CT_COUNT);
    const tdnet_opts o = opts_or_default(opts);
    ConvLayer L;
    const long M = (long)out_size(H, 1, stride, 1, 0) * out_size(W, 1, stride, 1, 0);
    if (plan_conv(L, Cout, Cin, 1, stride, 1, act, false, M, o, tile < 0 ? -1 : tile)) return -1;
    if (!((L.route == CR_GEMM1X1 && L.gemm == GK_PERSISTENT) || (L.route == CR_ADIRECT && !resid))) return td_fail("%s: this conv's kernel has no two-source form", who);
    std::vector<float> w(w_host, w_host + (size_t)Cout * Cin), b;
    if (bias_host) b.assign(bias_host, bias_host + Cout);
    int rc = upload_conv(L, w, b);
    if (!rc) rc = run_conv_src2(nullptr, L, in, Cin, L.nsteps, L.nsteps, nullptr, 0, nullptr, H, W, resid, out, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    free_conv_layer(L);
    return rc;
}
extern "C" int tdnet_op_classifier(const float* x, int HW, int C, const float* w, const float* b, int NC, float* out, void* stream) {
    if (NC < 1 || NC > 256) return td_fail("tdnet_op_classifier: NC must be in 1..256");
    TD_TRY(run_classifier(nullptr, x, HW, C, NC, w, b, out, (hipStream_t)stream));
    TD_HIP(hipStreamSynchronize((hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
// The FCN head's 3x3 conv (stride 1, dilation 1) and its 1x1 classifier, planned as a frame plans head3.  fused = 1: the classifier inside the Winograd
// output transform (k_wino4_out_cls through run_conv's ClsArgs; the hidden map is not written); fused = 0: run_conv into a temporary hidden map, then
// run_classifier.  fused = 1 fails before anything is allocated or launched where a frame would not fuse.
extern "C" int tdnet_op_head_cls(const float* in, int H, int W, int Cin, const float* w3_host, const float* b3_host, int Cout, int act,
                                 const float* cls_w_host, const float* cls_b_host, int NC, const tdnet_opts* opts, int fused, float* out,
                                 void* stream) {
    if (H < 1 || W < 1 || Cin < 1 || Cout < 1) return td_fail("tdnet_op_head_cls: empty input");
    if (NC < 1 || NC > 256) return td_fail("tdnet_op_head_cls: NC must be in 1..256");
    if (act < 0 || act > 2) return td_fail("tdnet_op_head_cls: act must be 0, 1 or 2");
    if (!w3_host || !cls_w_host || !cls_b_host) return td_fail("tdnet_op_head_cls: w3_host, cls_w_host and cls_b_host expected");
    const tdnet_opts o = opts_or_default(opts);
    hipStream_t s = (hipStream_t)stream;
    ConvLayer L;
    if (plan_conv(L, Cout, Cin, 3, 1, 1, act, false, (long)H * W, o)) return -1;
    if (fused && (L.route != CR_WINO || L.chunks != 1 || !wino_out_cls_supports(Cout, NC) || wino_act_general(act)))
        return td_fail("tdnet_op_head_cls: a frame would not fuse this head (Winograd plan in one chunk, Cout 64 or 128, NC <= 32, act 0 or 1)");
    float *hidden = nullptr, *cw = nullptr, *cb = nullptr;
    auto cleanup = [&]() {                                             // one release path, also for the error returns
        for (float* q : {hidden, cw, cb}) if (q) hipFree(q);
        free_conv_layer(L);
    };
    std::vector<float> w(w3_host, w3_host + (size_t)Cout * Cin * 9), b;
    if (b3_host) b.assign(b3_host, b3_host + Cout);
    int rc = 0;
    if (upload_conv(L, w, b) || upload(&cw, std::vector<float>(cls_w_host, cls_w_host + (size_t)NC * Cout)) ||
        upload(&cb, std::vector<float>(cls_b_host, cls_b_host + NC)) || dev_alloc(&hidden, (size_t)H * W * Cout)) rc = -1;
    const ClsArgs ca = {cw, cb, out, NC};
    if (!rc) rc = run_conv(nullptr, L, in, H, W, nullptr, hidden, s, nullptr, nullptr, nullptr, fused ? &ca : nullptr);
    if (!rc && !fused) rc = run_classifier(nullptr, hidden, H * W, Cout, NC, cw, cb, out, s);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_head_cls: device error");
    cleanup();
    return rc;
}
extern "C" int tdnet_op_upsample(const float* in, int C, int h, int w, int H, int W, float* out, void* stream) {
    launch_upsample(in, C, h, w, H, W, out, (hipStream_t)stream);
    TD_HIP(hipStreamSynchronize((hipStream_t)stream));
    TD_HIP(hipGetLastError());
    return 0;
}
// The stem's image buffer, allocated and zeroed as the workspace does (td_weights.h alloc_workspace), filled from an fp32 NCHW image (img_f32 != NULL:
// run_stem_pre's fp32 kernels) or from a byte source (src: the ingest kernel with the tables the handle's tdnet_set_input_* would build for what `resolve`
// says the source is), then copied WHOLE -- border included -- to out_dev.  rows: the packed-row layout, else NHWC4.  Returns the buffer's float count
// (out_dev == NULL: only that).  ONE body for the four entries below; bad_ptr: what to say about the entry's pointers, or NULL.
template <class Resolve>   // int resolve(SrcView&, int& Hs, int& Ws): 0, or nonzero behind td_fail
static long op_stem_image(const char* who, const float* img_f32, const uint8_t* src, const char* bad_ptr, Resolve resolve, int H, int W, const double* mean,
                          const double* std_, int rows, float* out, size_t capacity, void* stream) {
    if (H < 1 || W < 1) return td_fail("%s: empty image", who);
    const size_t img_floats = std::max((size_t)H * W * 4, rows ? (size_t)stem_rows_hp(H) * stem_rows_wp(W) * 3 + 4 : (size_t)0);
    if (!out) return (long)img_floats;
    if (bad_ptr) return td_fail("%s: %s", who, bad_ptr);
    if (capacity < img_floats) return td_fail("%s: capacity %zu < %zu", who, capacity, img_floats);
    hipStream_t s = (hipStream_t)stream;
    U8Input u;
    if (src) {
        SrcView sv;
        int Hs = 0, Ws = 0;
        if (resolve(sv, Hs, Ws) || u8_build(u, sv, Hs, Ws, H, W, mean, std_, who)) return -1;
    }
    float* img4 = nullptr;
    if (dev_alloc(&img4, img_floats)) { u8_free(u); return -1; }
    long rc = (long)img_floats;
    if (hipMemsetAsync(img4, 0, img_floats * sizeof(float), s) != hipSuccess) rc = td_fail("%s: memset failed", who);
    if (rc >= 0) {
        run_stem_pre(nullptr, src ? FrameInput{src, TD_IMG_U8, &u} : frame_input_f32(img_f32), H, W, img4, s, rows != 0);
        if (hipMemcpyAsync(out, img4, img_floats * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) rc = td_fail("%s: copy failed", who);
    }
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    hipFree(img4);
    u8_free(u);
    return rc;
}
// from an fp32 image or a tight RGB image [Hs][Ws][3] (tdnet_set_input_u8)
extern "C" long tdnet_op_stem_image(const float* img_f32, const uint8_t* src_u8, int Hs, int Ws, int H, int W, const double* mean, const double* std_,
                                    int rows, float* out, size_t capacity, void* stream) {
    return op_stem_image("tdnet_op_stem_image", img_f32, src_u8, (img_f32 != nullptr) == (src_u8 != nullptr) ? "give exactly one of img_f32 and src_u8" : nullptr,
                         [&](SrcView& sv, int& hs, int& ws) { sv = src_view_rgb(Hs, Ws); hs = Hs; ws = Ws; return 0; }, H, W, mean, std_, rows, out, capacity, stream);
}
// from an NV12 surface (tdnet_set_input_nv12)
extern "C" long tdnet_op_stem_image_nv12(const uint8_t* surf, int Hs, int Ws, int pitch, size_t uv_offset, int standard, int H, int W, const double* mean,
                                         const double* std_, int rows, float* out, size_t capacity, void* stream) {
    return op_stem_image("tdnet_op_stem_image_nv12", nullptr, surf, surf ? nullptr : "surf is NULL",
                         [&](SrcView& sv, int& hs, int& ws) { sv = src_view_nv12(Hs, Ws, Nv12Layout{pitch, uv_offset, standard}); hs = Hs; ws = Ws; return 0; },
                         H, W, mean, std_, rows, out, capacity, stream);
}
// from a source view (tdnet_set_input_view)
extern "C" long tdnet_op_stem_image_view(const uint8_t* base, const tdnet_view* view, int H, int W, const double* mean, const double* std_, int rows, float* out,
                                         size_t capacity, void* stream) {
    const char* who = "tdnet_op_stem_image_view";
    return op_stem_image(who, nullptr, base, base ? nullptr : "base is NULL", [&](SrcView& sv, int& hs, int& ws) { return view_resolve(view, sv, hs, ws, who); },
                         H, W, mean, std_, rows, out, capacity, stream);
}
// from a YUV surface (tdnet_set_input_surface)
extern "C" long tdnet_op_stem_image_surface(const uint8_t* base, const tdnet_surface* surface, int H, int W, const double* mean, const double* std_, int rows, float* out,
                                            size_t capacity, void* stream) {
    const char* who = "tdnet_op_stem_image_surface";
    return op_stem_image(who, nullptr, base, base ? nullptr : "base is NULL", [&](SrcView& sv, int& hs, int& ws) { return surface_resolve(surface, sv, hs, ws, who); },
                         H, W, mean, std_, rows, out, capacity, stream);
}
// low-resolution logits [C][h][w] -> labels [H][W]: int32 through k_upsample_argmax (labels_i32 != NULL) and / or uint8 through
// k_upsample_argmax_u8 (labels_u8 != NULL)
extern "C" int tdnet_op_upsample_argmax(const float* in, int C, int h, int w, int H, int W, int32_t* labels_i32, uint8_t* labels_u8, void* stream) {
    if (C < 1 || C > 256) return td_fail("tdnet_op_upsample_argmax: C must be in 1..256");
    hipStream_t s = (hipStream_t)stream;
    if (labels_i32) launch_upsample_argmax(in, C, h, w, H, W, labels_i32, s);
    if (labels_u8) TD_TRY(launch_upsample_argmax_u8(in, C, h, w, H, W, labels_u8, s));
    TD_HIP(hipStreamSynchronize(s));
    TD_HIP(hipGetLastError());
    return 0;
}
// The colour map [oh][ow][3] of low-resolution logits [C][h][w] (labels_u8 == NULL: the fused form) or of a uint8 label map [H][W]
// (labels_u8 != NULL; in, C, h, w are ignored), through the tables and colour table rgb_build makes for a handle.
extern "C" int tdnet_op_upsample_argmax_rgb(const float* in, int C, int h, int w, int H, int W, int oh, int ow, const uint8_t* palette, int n_colours,
                                            uint8_t* rgb, const uint8_t* labels_u8, void* stream) {
    if (!rgb) return td_fail("tdnet_op_upsample_argmax_rgb: rgb_out is NULL");
    if (!labels_u8 && (!in || C < 1 || C > 256 || h < 1 || w < 1)) return td_fail("tdnet_op_upsample_argmax_rgb: logits [C,h,w] with C in 1..256 expected");
    hipStream_t s = (hipStream_t)stream;
    RgbOutput r;
    TD_TRY(rgb_build(r, H, W, oh, ow, palette, n_colours, "tdnet_op_upsample_argmax_rgb"));
    int rc = labels_u8 ? launch_labels_rgb(labels_u8, r, rgb, s) : launch_upsample_argmax_rgb(in, C, h, w, r, rgb, s);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_upsample_argmax_rgb: device error");
    rgb_free(r);
    return rc;
}
// The overlay [Hs][Ws][3] of low-resolution logits [C][h][w] (labels_u8 == NULL: the fused form) or of a uint8 label map [H][W] (labels_u8 != NULL; in, C, h, w
// are ignored) over the source frame `resolve` describes, through the byte-input description u8_build makes and the tables overlay_build / overlay_tables make
// for a handle; out in the source's colour order.  ONE body for the three entries below; src_name: what the entry calls its source pointer.
template <class Resolve>   // int resolve(SrcView&, int& Hs, int& Ws): 0, or nonzero behind td_fail
static int op_overlay(const char* who, const char* src_name, const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_u8, const uint8_t* src, Resolve resolve,
                      const uint8_t* palette_rgba, int n_colours, uint8_t* out, void* stream) {
    if (!src || !out) return td_fail("%s: %s and out expected", who, src_name);
    if (!labels_u8 && (!in || C < 1 || C > 256 || h < 1 || w < 1)) return td_fail("%s: logits [C,h,w] with C in 1..256 expected", who);
    hipStream_t s = (hipStream_t)stream;
    U8Input u;
    OverlayOutput o;
    SrcView sv;
    int Hs = 0, Ws = 0;
    TD_TRY(resolve(sv, Hs, Ws));
    TD_TRY(u8_build(u, sv, Hs, Ws, H, W, nullptr, nullptr, who));
    int rc = overlay_build(o, palette_rgba, n_colours, who, u.swap);
    if (!rc) rc = overlay_tables(o, H, W, Hs, Ws, who);
    if (!rc) rc = labels_u8 ? launch_labels_overlay(labels_u8, o, u, src, out, s) : launch_upsample_argmax_overlay(in, C, h, w, o, u, src, out, s);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    overlay_free(o);
    u8_free(u);
    return rc;
}
// over packed RGB [Hs][Ws][3] (nv12 == 0; pitch, uv_offset, standard ignored) or an NV12 surface
extern "C" int tdnet_op_overlay(const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_u8, const uint8_t* src, int nv12, int Hs, int Ws, int pitch,
                                size_t uv_offset, int standard, const uint8_t* palette_rgba, int n_colours, uint8_t* out, void* stream) {
    return op_overlay("tdnet_op_overlay", "src", in, C, h, w, H, W, labels_u8, src, [&](SrcView& sv, int& hs, int& ws) {
        sv = nv12 ? src_view_nv12(Hs, Ws, Nv12Layout{pitch, uv_offset, standard}) : src_view_rgb(Hs, Ws); hs = Hs; ws = Ws; return 0; }, palette_rgba, n_colours, out, stream);
}
// over a source view: out [h][w][3] of the view's rectangle
extern "C" int tdnet_op_overlay_view(const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_u8, const uint8_t* base, const tdnet_view* view,
                                     const uint8_t* palette_rgba, int n_colours, uint8_t* out, void* stream) {
    const char* who = "tdnet_op_overlay_view";
    return op_overlay(who, "base", in, C, h, w, H, W, labels_u8, base, [&](SrcView& sv, int& hs, int& ws) { return view_resolve(view, sv, hs, ws, who); },
                      palette_rgba, n_colours, out, stream);
}
// over a YUV surface: out [h][w][3] of the surface's rectangle, r g b
extern "C" int tdnet_op_overlay_surface(const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_u8, const uint8_t* base, const tdnet_surface* surface,
                                        const uint8_t* palette_rgba, int n_colours, uint8_t* out, void* stream) {
    const char* who = "tdnet_op_overlay_surface";
    return op_overlay(who, "base", in, C, h, w, H, W, labels_u8, base, [&](SrcView& sv, int& hs, int& ws) { return surface_resolve(surface, sv, hs, ws, who); },
                      palette_rgba, n_colours, out, stream);
}
// The picture into a destination view (include/tdnet.h "destination views", "surfaces") through exactly the kernels the frame entries launch with one in force: of
// low-resolution logits [C][h][w] (labels_u8 == NULL) or of a uint8 label map [H][W]; the overlay over the source (src_base, what resolve_src describes;
// palette [n][4]) or, src_base == NULL, the colour map oh x ow (palette [n][3]).  dst_base: the destination frame's base, at any byte address.  ONE body
// for the two entries below.
template <class ResolveDst, class ResolveSrc>   // int resolve_dst(DstOutput&), int resolve_src(SrcView&, int& Hs, int& Ws): 0, or nonzero behind td_fail
static int op_picture(const char* who, const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_u8, const uint8_t* palette, int n_colours,
                      const uint8_t* src_base, ResolveSrc resolve_src, int oh, int ow, uint8_t* dst_base, ResolveDst resolve_dst, void* stream) {
    if (!labels_u8 && (!in || C < 1 || C > 256 || h < 1 || w < 1)) return td_fail("%s: logits [C,h,w] with C in 1..256 expected", who);
    hipStream_t s = (hipStream_t)stream;
    DstOutput d;
    TD_TRY(resolve_dst(d));
    int rc = 0;
    if (!src_base) {
        RgbOutput r;
        TD_TRY(rgb_build(r, H, W, oh, ow, palette, n_colours, who));
        rc = launch_picture_dst(in, C, h, w, labels_u8, &r, nullptr, nullptr, nullptr, d, dst_base, s);
        if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
        rgb_free(r);
        return rc;
    }
    U8Input u;
    OverlayOutput o;
    SrcView sv;
    int Hs = 0, Ws = 0;
    TD_TRY(resolve_src(sv, Hs, Ws));
    TD_TRY(u8_build(u, sv, Hs, Ws, H, W, nullptr, nullptr, who));
    rc = overlay_build(o, palette, n_colours, who, u.swap);
    if (!rc) rc = overlay_tables(o, H, W, Hs, Ws, who);
    if (!rc) rc = launch_picture_dst(in, C, h, w, labels_u8, nullptr, &o, &u, src_base, d, dst_base, s);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    overlay_free(o);
    u8_free(u);
    return rc;
}
// views on both sides
extern "C" int tdnet_op_picture_view(const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_u8, const uint8_t* palette, int n_colours,
                                     const uint8_t* src_base, const tdnet_view* src_view, int oh, int ow, uint8_t* dst_base, const tdnet_view* dst_view, void* stream) {
    const char* who = "tdnet_op_picture_view";
    if (!dst_base || !dst_view) return td_fail("%s: dst_base and dst_view expected", who);
    return op_picture(who, in, C, h, w, H, W, labels_u8, palette, n_colours, src_base, [&](SrcView& sv, int& hs, int& ws) { return view_resolve(src_view, sv, hs, ws, who); },
                      oh, ow, dst_base, [&](DstOutput& d) { return dst_build(d, dst_view, who); }, stream);
}
// surfaces on either side: the destination a 4:2:0 surface (dst_surface) or a view (dst_view), the overlay's source a surface (src_surface) or a view (src_view)
extern "C" int tdnet_op_picture_surface(const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_u8, const uint8_t* palette, int n_colours,
                                        const uint8_t* src_base, const tdnet_surface* src_surface, const tdnet_view* src_view, int oh, int ow, uint8_t* dst_base,
                                        const tdnet_surface* dst_surface, const tdnet_view* dst_view, void* stream) {
    const char* who = "tdnet_op_picture_surface";
    if (!dst_base || (!dst_surface && !dst_view)) return td_fail("%s: dst_base and dst_surface or dst_view expected", who);
    return op_picture(who, in, C, h, w, H, W, labels_u8, palette, n_colours, src_base,
                      [&](SrcView& sv, int& hs, int& ws) { return src_surface ? surface_resolve(src_surface, sv, hs, ws, who) : view_resolve(src_view, sv, hs, ws, who); },
                      oh, ow, dst_base, [&](DstOutput& d) { return dst_surface ? dst_surface_build(d, dst_surface, who) : dst_build(d, dst_view, who); }, stream);
}
// cm_dev [C][C] (uint64, ACCUMULATED into, not cleared) += the confusion counts of ground truth gt [H][W] (through gt_map, 256 bytes on the host,
// NULL = identity) against the labels of low-resolution logits [C][h][w] (labels_in == NULL: k_upsample_argmax_score, which also writes the uint8
// label map if labels_u8 != NULL) or against a uint8 label map [H][W] (labels_in != NULL: k_labels_score; in, h, w, labels_u8 are ignored).
// TDNET_SCORE_WAVE_UNIFORM=1 / 0 in the environment (tools/score_probe.py) runs the kernels with / without their wave-uniform path; unset: the
// form the library's own entries launch.
extern "C" int tdnet_op_upsample_argmax_score(const float* in, int C, int h, int w, int H, int W, const uint8_t* gt, const uint8_t* gt_map, uint8_t* labels_u8,
                                              uint64_t* cm, const uint8_t* labels_in, void* stream) {
    if (!gt || !cm) return td_fail("tdnet_op_upsample_argmax_score: gt and cm expected");
    if (C < 1 || C > 256 || H < 1 || W < 1) return td_fail("tdnet_op_upsample_argmax_score: C in 1..256 and a size >= 1 x 1 expected");
    if (!labels_in && (!in || h < 1 || w < 1)) return td_fail("tdnet_op_upsample_argmax_score: logits [C,h,w] expected");
    const char* env = getenv("TDNET_SCORE_WAVE_UNIFORM");
    const bool uniform = env && *env ? atoi(env) != 0 : TD_SCORE_WAVE_UNIFORM;
    hipStream_t s = (hipStream_t)stream;
    unsigned char m[256], *dmap = nullptr;
    score_map_or_identity(gt_map, m);
    TD_TRY(dev_alloc(&dmap, 256));
    int rc = 0;
    if (hipMemcpy(dmap, m, 256, hipMemcpyHostToDevice) != hipSuccess) rc = td_fail("tdnet_op_upsample_argmax_score: map upload failed");
    if (!rc) rc = labels_in ? launch_labels_score(labels_in, C, H, W, gt, dmap, (unsigned long long*)cm, s, uniform)
                            : launch_upsample_argmax_score(in, C, h, w, H, W, gt, dmap, labels_u8, (unsigned long long*)cm, s, uniform);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_upsample_argmax_score: device error");
    hipFree(dmap);
    return rc;
}
// Labels (labels_u8 != NULL) and confidence bytes [H][W] of low-resolution logits [C][h][w] (logits_full == NULL: k_upsample_argmax_conf_u8) or of
// full-resolution logits [C][H][W] (logits_full != NULL: k_logits_conf_u8; in, h, w are ignored).  TDNET_CONF_PASSES=1 / 2 in the environment
// (tools/conf_probe.py) runs the one-pass / two-pass form of the kernels; unset: the form the library's own entries launch.
extern "C" int tdnet_op_upsample_argmax_conf(const float* in, int C, int h, int w, int H, int W, uint8_t* labels_u8, uint8_t* conf_u8, int min_conf, int reject_label,
                                             const float* logits_full, void* stream) {
    if (!conf_u8) return td_fail("tdnet_op_upsample_argmax_conf: a confidence map expected");
    if (C < 1 || C > 256 || H < 1 || W < 1) return td_fail("tdnet_op_upsample_argmax_conf: C in 1..256 and a size >= 1 x 1 expected");
    if (min_conf < 0 || min_conf > 255 || reject_label < 0 || reject_label > 255) return td_fail("tdnet_op_upsample_argmax_conf: min_conf and reject_label in 0..255 expected");
    if (!logits_full && (!in || h < 1 || w < 1)) return td_fail("tdnet_op_upsample_argmax_conf: logits [C,h,w] expected");
    const char* env = getenv("TDNET_CONF_PASSES");
    const bool online = env && *env ? atoi(env) != 2 : TD_CONF_ONLINE;
    hipStream_t s = (hipStream_t)stream;
    int rc = logits_full ? launch_logits_conf_u8(logits_full, C, (long)H * W, labels_u8, conf_u8, min_conf, reject_label, s, online)
                         : launch_upsample_argmax_conf_u8(in, C, h, w, H, W, labels_u8, conf_u8, min_conf, reject_label, s, online);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_upsample_argmax_conf: device error");
    return rc;
}
// Labels (labels_u8 != NULL) and matte bytes [H][W] of low-resolution logits [C][h][w] (logits_full == NULL: k_upsample_argmax_matte_u8) or of
// full-resolution logits [C][H][W] (logits_full != NULL: k_logits_matte_u8; in, h, w are ignored), for the class set classes[0 .. n) (host).
extern "C" int tdnet_op_upsample_argmax_matte(const float* in, int C, int h, int w, int H, int W, uint8_t* labels_u8, uint8_t* matte_u8, const uint8_t* classes, int n,
                                              const float* logits_full, void* stream) {
    if (!matte_u8) return td_fail("tdnet_op_upsample_argmax_matte: a matte map expected");
    if (C < 1 || C > 256 || H < 1 || W < 1) return td_fail("tdnet_op_upsample_argmax_matte: C in 1..256 and a size >= 1 x 1 expected");
    if (n < 0 || n > 256 || (n > 0 && !classes)) return td_fail("tdnet_op_upsample_argmax_matte: n in 0..256 class ids expected");
    if (!logits_full && (!in || h < 1 || w < 1)) return td_fail("tdnet_op_upsample_argmax_matte: logits [C,h,w] expected");
    MatteSet set = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < n; ++i) {
        if (classes[i] >= C) return td_fail("tdnet_op_upsample_argmax_matte: classes[%d] = %d is not a class id (C = %d)", i, (int)classes[i], C);
        set.w[classes[i] >> 5] |= 1u << (classes[i] & 31);
    }
    hipStream_t s = (hipStream_t)stream;
    int rc = logits_full ? launch_logits_matte_u8(logits_full, C, (long)H * W, labels_u8, matte_u8, set, s)
                         : launch_upsample_argmax_matte_u8(in, C, h, w, H, W, labels_u8, matte_u8, set, s);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("tdnet_op_upsample_argmax_matte: device error");
    return rc;
}
// The composite (include/tdnet.h "matte out") through exactly the kernels the composite entries launch: of low-resolution logits [C][h][w] and the class
// set classes[0 .. n) (matte_u8 == NULL) or of a matte map [H][W] (in, C, h, w, classes, n are then ignored), over the source src_base read through
// src_surface or src_view, into the contiguous block [Hs][Ws][3] at dst_base (dst_view == NULL) or into dst_view's rectangle of the frame at dst_base.
extern "C" int tdnet_op_composite(const float* in, int C, int h, int w, int H, int W, const uint8_t* classes, int n, const uint8_t* matte_u8, const uint8_t* src_base,
                                  const tdnet_view* src_view, const tdnet_surface* src_surface, uint8_t* dst_base, const tdnet_view* dst_view, int mode,
                                  const uint8_t* bg_rgb, void* stream) {
    const char* who = "tdnet_op_composite";
    if (!src_base || !dst_base || (!src_view && !src_surface)) return td_fail("%s: src_base, dst_base and src_view or src_surface expected", who);
    if (H < 1 || W < 1) return td_fail("%s: a network size >= 1 x 1 expected", who);
    if (!matte_u8 && (!in || C < 1 || C > 256 || h < 1 || w < 1)) return td_fail("%s: logits [C,h,w] with C in 1..256 expected", who);
    if (!matte_u8 && (n < 0 || n > 256 || (n > 0 && !classes))) return td_fail("%s: n in 0..256 class ids expected", who);
    if (mode != TDNET_COMPOSITE_COLOUR && mode != TDNET_COMPOSITE_ALPHA) return td_fail("%s: mode = %d must be 0 or 1", who, mode);
    if ((mode == TDNET_COMPOSITE_COLOUR) != (bg_rgb != nullptr)) return td_fail("%s: bg_rgb expected in mode 0 and only there", who);
    MatteSet set = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; !matte_u8 && i < n; ++i) {
        if (classes[i] >= C) return td_fail("%s: classes[%d] = %d is not a class id (C = %d)", who, i, (int)classes[i], C);
        set.w[classes[i] >> 5] |= 1u << (classes[i] & 31);
    }
    hipStream_t s = (hipStream_t)stream;
    DstOutput d;
    if (dst_view) TD_TRY(dst_build(d, dst_view, who));
    CompositeOutput c;
    c.set = true; c.mode = mode;
    if (bg_rgb) memcpy(c.bg, bg_rgb, 3);
    U8Input u;
    OverlayOutput o;
    SrcView sv;
    int Hs = 0, Ws = 0;
    TD_TRY(src_surface ? surface_resolve(src_surface, sv, Hs, Ws, who) : view_resolve(src_view, sv, Hs, Ws, who));
    TD_TRY(u8_build(u, sv, Hs, Ws, H, W, nullptr, nullptr, who));
    int rc = overlay_tables(o, H, W, Hs, Ws, who);
    if (!rc) rc = launch_composite(in, C, h, w, matte_u8, set, o, u, src_base, c, d, dst_base, s);
    if (rc) { const std::string msg = g_err; rc = td_fail("%s: %s", who, msg.c_str()); }
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    overlay_free(o);
    u8_free(u);
    return rc;
}
// Stage 1 of the refined matte (include/tdnet.h "refined matte") alone, through the launch tdnet_refine_matte enqueues first: the coefficient planes a_q
// (int16 [rows][cols]) and b_q (int32 [rows][cols]) of a guide and a matte at any byte addresses.  The scratch is allocated for the call.
extern "C" int tdnet_op_refine_coeff(const uint8_t* guide, size_t guide_pitch, const uint8_t* matte, size_t matte_pitch, int rows, int cols, int radius, int eps,
                                     int16_t* aq_dev, int32_t* bq_dev, void* stream) {
    const char* who = "tdnet_op_refine_coeff";
    if (!aq_dev || !bq_dev) return td_fail("%s: null argument", who);
    TD_TRY(refine_args_check(guide, guide_pitch, matte, matte_pitch, nullptr, 0, false, rows, cols, radius, eps, nullptr, who));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)rows * cols;
    void* scratch = nullptr;
    if (hipMalloc(&scratch, refine_scratch_bytes(rows, cols)) != hipSuccess) return td_fail("%s: hipMalloc failed", who);
    int rc = 0;
    launch_refine_coeff(guide, guide_pitch, matte, matte_pitch, rows, cols, radius, eps, scratch, s);
    if (hipMemcpyAsync(aq_dev, refine_aq(scratch, rows, cols), 2 * n, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(bq_dev, refine_bq(scratch), 4 * n, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = td_fail("%s: copy failed", who);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    hipFree(scratch);
    return rc;
}
// The gather launch of the refined frame entries (td_refine.h k_refine_gather) alone: luma and M_src [Hs][Ws] (tight, device, 4-byte aligned) of the source at
// src_base read through src_surface or src_view, the matte from low-resolution logits [C][h][w] and the class set (matte_u8 == NULL) or from a map [H][W].
extern "C" int tdnet_op_refine_gather(const float* in, int C, int h, int w, int H, int W, const uint8_t* classes, int n, const uint8_t* matte_u8, const uint8_t* src_base,
                                      const tdnet_view* src_view, const tdnet_surface* src_surface, uint8_t* luma_dev, uint8_t* msrc_dev, void* stream) {
    const char* who = "tdnet_op_refine_gather";
    if (!src_base || !luma_dev || !msrc_dev || (!src_view && !src_surface)) return td_fail("%s: src_base, the two planes and src_view or src_surface expected", who);
    if (((size_t)luma_dev | (size_t)msrc_dev) & 3u) return td_fail("%s: the planes must be 4-byte aligned", who);
    if (H < 1 || W < 1) return td_fail("%s: a network size >= 1 x 1 expected", who);
    if (!matte_u8 && (!in || C < 1 || C > 256 || h < 1 || w < 1)) return td_fail("%s: logits [C,h,w] with C in 1..256 expected", who);
    if (!matte_u8 && (n < 0 || n > 256 || (n > 0 && !classes))) return td_fail("%s: n in 0..256 class ids expected", who);
    MatteSet set = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; !matte_u8 && i < n; ++i) {
        if (classes[i] >= C) return td_fail("%s: classes[%d] = %d is not a class id (C = %d)", who, i, (int)classes[i], C);
        set.w[classes[i] >> 5] |= 1u << (classes[i] & 31);
    }
    hipStream_t s = (hipStream_t)stream;
    U8Input u;
    OverlayOutput o;
    SrcView sv;
    int Hs = 0, Ws = 0;
    TD_TRY(src_surface ? surface_resolve(src_surface, sv, Hs, Ws, who) : view_resolve(src_view, sv, Hs, Ws, who));
    TD_TRY(u8_build(u, sv, Hs, Ws, H, W, nullptr, nullptr, who));
    int rc = overlay_tables(o, H, W, Hs, Ws, who);
    if (!rc) {
        GatherArgs a = GatherArgs();
        a.in = in; a.map = matte_u8; a.ys = o.ys; a.xs = o.xs;
        a.C = C; a.h = h; a.w = w; a.H = H; a.W = W; a.oh = Hs; a.ow = Ws;
        a.swap = u.swap ? 1 : 0; a.luma = luma_dev; a.msrc = msrc_dev; a.set = set;
        rc = launch_refine_gather(a, u, src_base, s);
    }
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    overlay_free(o);
    u8_free(u);
    return rc;
}
// the tiles of the two launches (columns, rows of the coefficient launch's, rows of the apply launch's): the tests size their cases from them
extern "C" int tdnet_op_refine_tile(int* tx, int* ty_coeff, int* ty_apply) {
    if (tx) *tx = TD_RF_TX;
    if (ty_coeff) *ty_coeff = TD_RF_CY;
    if (ty_apply) *ty_apply = TD_RF_AY;
    return 0;
}
// The index table the colour-map kernels sample through (rgb_build's: dataloader.nearest_index restated in C) -> out_host [n_dst] int32.  Host only.
extern "C" int tdnet_op_nearest_index(int n_src, int n_dst, int32_t* out_host) {
    if (n_src < 1 || n_dst < 1 || !out_host) return td_fail("tdnet_op_nearest_index: sizes >= 1 and a host buffer expected");
    std::vector<int> idx;
    rgb_nearest_index(n_src, n_dst, idx);
    memcpy(out_host, idx.data(), idx.size() * sizeof(int));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// tuning / roofline hooks (not on the product path)
// ---------------------------------------------------------------------------------------------------------------
// Pure-MFMA loop: the practical fp32-MFMA ceiling of THIS chip at its sustained clock (4 independent accumulators per
// wave, `waves_per_simd` waves per SIMD, no memory traffic).
TD_KERNEL void k_mfma_peak(float* out, int iters) {
    f32x16 a0, a1, a2, a3;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a0[r] = 0.f; a1[r] = 1.f; a2[r] = 2.f; a3[r] = 3.f; }
    float x = 1.0f + (float)(threadIdx.x & 7) * 1e-3f, y = 1.0f - (float)(threadIdx.x & 3) * 1e-3f;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a0 = td_mfma32(x, y, a0); a1 = td_mfma32(y, x, a1); a2 = td_mfma32(x, x, a2); a3 = td_mfma32(y, y, a3);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += a0[r] + a1[r] + a2[r] + a3[r];
    if (s == 123.456f) out[0] = s;                      // keep the accumulators live
}
// returns achieved TFLOP/s (fp32 MFMA) or <0
extern "C" double tdnet_bench_mfma_peak(int waves_per_simd, int iters, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    float* d = nullptr;
    if (hipMalloc((void**)&d, 256) != hipSuccess) return -1.0;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const int blocks = 256 * waves_per_simd;            // 256 CUs x (4 SIMDs = one 256-thread block) x waves_per_simd
    TD_LAUNCH(k_mfma_peak, dim3(blocks), dim3(256), 0, s, d, 16);
    hipEventRecord(e0, s);
    TD_LAUNCH(k_mfma_peak, dim3(blocks), dim3(256), 0, s, d, iters);
    hipEventRecord(e1, s);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1); hipFree(d);
    const double flop = (double)blocks * 4 /*waves*/ * (double)iters * 32 /*mfma per iter*/ * 4096.0;
    return ms > 0.f ? flop / (ms * 1e-3) / 1e12 : -1.0;
}
// Average device time (ms, HIP events on `stream`) of `iters` launches of one conv configuration on random data.
extern "C" double tdnet_bench_conv(int H, int W, int Cin, int Cout, int KS, int stride, int dil, int tile, int iters,
                                   const tdnet_opts* opts, void* stream) {
    const tdnet_opts o = opts_or_default(opts);
    if ((KS != 1 && KS != 3) || Cin % 32 || tile < -2 || tile >= CT_COUNT) { td_fail("tdnet_bench_conv: bad arguments"); return -1.0; }
    hipStream_t s = (hipStream_t)stream;
    ConvLayer L;
    std::vector<float> w((size_t)Cout * Cin * KS * KS), x((size_t)H * W * Cin), b(Cout, 0.1f);
    unsigned st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xFFFF) / 32768.0f - 1.0f; };
    for (auto& v : w) v = rnd() * 0.05f;
    for (auto& v : x) v = rnd();
    const int pad_ = dil * (KS / 2);
    const long M_ = (long)out_size(H, KS, stride, dil, pad_) * out_size(W, KS, stride, dil, pad_);
    // tile -1: the heuristic's choice for this M; overlap bit 1: the conv as its 2 row classes one after the other on the stream
    // tile -2: the fused 64-channel Winograd kernel whatever the map size (tdnet_op_conv_wino_f64's plan; opts are not read)
    if ((tile == -2 ? op_plan_wino_f64("tdnet_bench_conv", L, H, W, Cin, Cout, KS, stride, dil, 1)
                    : plan_conv(L, Cout, Cin, KS, stride, dil, 1, false, M_, o, tile, (o.overlap & TDNET_OVERLAP_CHAINS) ? 2 : 1)) || upload_conv(L, w, b)) return -1.0;
    float *din = nullptr, *dout = nullptr;
    if (upload(&din, x)) return -1.0;
    const int Ho = out_size(H, KS, stride, dil, L.pad), Wo = out_size(W, KS, stride, dil, L.pad);
    if (dev_alloc(&dout, (size_t)Ho * Wo * Cout)) return -1.0;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    TdWeights none;
    tdnet tmp(&none);                                                 // only carries the Winograd workspace for run_conv
    if (L.wino) {
        const size_t T = (size_t)wino_tiles(H, W, dil, L.wino), nb = (size_t)(L.wino + 2) * (L.wino + 2);
        tmp.wino_v_floats = nb * T * Cin; tmp.wino_m_floats = nb * T * Cout;
        if (dev_alloc(&tmp.wino_v, tmp.wino_v_floats) || dev_alloc(&tmp.wino_m, tmp.wino_m_floats)) return -1.0;
    }
    tdnet* ws = L.wino ? &tmp : nullptr;
    for (int i = 0; i < 2; ++i) run_conv(ws, L, din, H, W, nullptr, dout, s);
    hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) run_conv(ws, L, din, H, W, nullptr, dout, s);
    hipEventRecord(e1, s);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(din); hipFree(dout);
    if (tmp.wino_v) hipFree(tmp.wino_v);
    if (tmp.wino_m) hipFree(tmp.wino_m);
    free_conv_layer(L);
    return ms / iters;
}
// Regions out (include/tdnet.h) through exactly the seven launches the entries enqueue, on maps the caller holds: from low-resolution logits [C][h][w]
// (labels_in == NULL: the labels go to labels_out [H][W] if given) or from a uint8 label map [H][W] at any byte address (in, h, w, labels_out are then
// ignored).  classes: n class ids below C on the host.  ids: int32 [H][W] or NULL; regions: 16 + 48 * max_regions bytes, 8-byte aligned.  The workspace is
// allocated here and released before the call returns.
extern "C" int tdnet_op_regions(const float* in, int C, int h, int w, int H, int W, const uint8_t* labels_in, uint8_t* labels_out, const uint8_t* classes, int n,
                                int connectivity, int max_regions, int min_area, int32_t* ids, void* regions, void* stream) {
    const char* who = "tdnet_op_regions";
    if (C < 1 || C > 256 || H < 1 || W < 1) return td_fail("%s: C in 1..256 and a size >= 1 x 1 expected", who);
    if (!labels_in && (!in || h < 1 || w < 1)) return td_fail("%s: logits [C,h,w] or a label map expected", who);
    if (n < 0 || n > 256 || (n > 0 && !classes)) return td_fail("%s: n in 0..256 class ids expected", who);
    RegionsOutput r;
    MatteSet set = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < n; ++i) {
        if (classes[i] >= C) return td_fail("%s: classes[%d] = %d is not a class id (C = %d)", who, i, (int)classes[i], C);
        set.w[classes[i] >> 5] |= 1u << (classes[i] & 31);
    }
    TD_TRY(regions_table_check(regions, who));
    TD_TRY(regions_alloc(r, H, W, who));
    r.classes = set; r.conn = connectivity; r.max_regions = max_regions; r.min_area = min_area; r.set = true;
    hipStream_t s = (hipStream_t)stream;
    int rc = run_regions(labels_in ? nullptr : in, C, h, w, H, W, labels_in, labels_out, ids, regions, r, s, who);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    regions_free(r);
    return rc;
}
// the tile of the first launch: the tests size their cases from it
extern "C" int tdnet_op_regions_tile(int* th, int* tw) {
    if (th) *th = TD_RG_TH;
    if (tw) *tw = TD_RG_TW;
    return 0;
}
// Tracks out (include/tdnet.h) through exactly the launches the tracks entries enqueue (TDNET_REGIONS_LAUNCHES + TDNET_TRACKS_LAUNCHES), one frame per call,
// from a uint8 label map [H][W] at any byte address.  state: tdnet_op_tracks_state_bytes(H, W) bytes the CALLER owns, 16-byte aligned, all zero = the reset
// state; it carries the tracks from call to call.  ids, track_ids: int32 [H][W] or NULL; regions: 16 + 48 * max_regions bytes, tracks: 16 + 24 * max_regions
// bytes, both 8-byte aligned.  The regions workspace is allocated here and released before the call returns.
extern "C" size_t tdnet_op_tracks_state_bytes(int H, int W) { return H < 1 || W < 1 || regions_size_check(H, W, "tdnet_op_tracks_state_bytes") ? 0 : tracks_layout(nullptr, H, W, nullptr); }
// the pair table's slots for an H x W map: the tests size the worst case (H W distinct pairs) from it
extern "C" long tdnet_op_tracks_capacity(int H, int W) { return H < 1 || W < 1 ? 0 : 1l << tracks_hash_lg(H, W); }
extern "C" int tdnet_op_tracks(const uint8_t* labels, int C, int H, int W, const uint8_t* classes, int n, int connectivity, int max_regions, int min_area, int min_overlap,
                               void* state, int32_t* ids, void* regions, int32_t* track_ids, void* tracks, void* stream) {
    const char* who = "tdnet_op_tracks";
    if (C < 1 || C > 256 || H < 1 || W < 1 || !labels) return td_fail("%s: a label map, C in 1..256 and a size >= 1 x 1 expected", who);
    if (n < 0 || n > 256 || (n > 0 && !classes)) return td_fail("%s: n in 0..256 class ids expected", who);
    if (min_overlap < 1) return td_fail("%s: min_overlap = %d must be at least 1", who, min_overlap);
    if (!state) return td_fail("%s: state_dev is NULL", who);
    if ((size_t)state & 15u) return td_fail("%s: state_dev = %p is not 16-byte aligned", who, state);
    MatteSet set = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < n; ++i) {
        if (classes[i] >= C) return td_fail("%s: classes[%d] = %d is not a class id (C = %d)", who, i, (int)classes[i], C);
        set.w[classes[i] >> 5] |= 1u << (classes[i] & 31);
    }
    TD_TRY(regions_table_check(regions, who));
    TD_TRY(tracks_table_check(tracks, who));
    RegionsOutput r;
    TD_TRY(regions_alloc(r, H, W, who));
    r.classes = set; r.conn = connectivity; r.max_regions = max_regions; r.min_area = min_area; r.set = true;
    TracksState st;
    tracks_layout(state, H, W, &st);
    hipStream_t s = (hipStream_t)stream;
    int32_t* cur = ids ? ids : st.cur;
    int rc = run_regions(nullptr, C, 0, 0, H, W, labels, nullptr, cur, regions, r, s, who);
    if (!rc) rc = run_tracks(H, W, cur, regions, track_ids, tracks, st, max_regions, min_overlap, s, who);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    regions_free(r);
    return rc;
}
// Runs out (include/tdnet.h) through exactly the launches the runs entries enqueue, on maps the caller holds: from low-resolution logits [C][h][w] (the label
// launch writes labels [H][W], required then), from a uint8 map at any byte address or from an int32 map, 4-byte aligned.  runs: 16 + 8 (max_runs + 1) bytes,
// 8-byte aligned.  The workspace is allocated here and released before the call returns.
extern "C" int tdnet_op_runs(const float* in, int C, int h, int w, int H, int W, uint8_t* labels, const uint8_t* map_u8, const int32_t* map_i32, int max_runs, void* runs,
                             void* stream) {
    const char* who = "tdnet_op_runs";
    if (H < 1 || W < 1) return td_fail("%s: a size >= 1 x 1 expected", who);
    if ((in != nullptr) + (map_u8 != nullptr) + (map_i32 != nullptr) != 1) return td_fail("%s: exactly one of logits, a uint8 map and an int32 map expected", who);
    if (in && (!labels || C < 1 || C > 256 || h < 1 || w < 1)) return td_fail("%s: logits [C,h,w] with C in 1..256 and a label map to write expected", who);
    TD_TRY(runs_table_check(runs, who));
    RunsState r;
    TD_TRY(runs_alloc(r, H, W, false, who));
    hipStream_t s = (hipStream_t)stream;
    const void* map = in ? (const void*)labels : map_u8 ? (const void*)map_u8 : (const void*)map_i32;
    int rc = runs_args_check(H, W, map, map_i32 != nullptr, runs, r, max_runs, who);
    if (!rc && in) rc = launch_upsample_argmax_u8(in, C, h, w, H, W, labels, s);
    if (!rc) rc = run_runs(H, W, map, map_i32 != nullptr, runs, r, max_runs, s, who);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    runs_free(r);
    return rc;
}
extern "C" int tdnet_op_runs_decode(const void* runs, int max_runs, int fill, int H, int W, uint8_t* out_u8, int32_t* out_i32, void* stream) {
    const char* who = "tdnet_op_runs_decode";
    if (H < 1 || W < 1) return td_fail("%s: a size >= 1 x 1 expected", who);
    if ((out_u8 != nullptr) + (out_i32 != nullptr) != 1) return td_fail("%s: exactly one of a uint8 and an int32 output expected", who);
    RunsState r;
    TD_TRY(runs_alloc(r, H, W, false, who));
    hipStream_t s = (hipStream_t)stream;
    int rc = run_runs_decode(H, W, runs, fill, out_u8 ? (void*)out_u8 : (void*)out_i32, out_i32 != nullptr, r, max_runs, s, who);
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) rc = td_fail("%s: device error", who);
    runs_free(r);
    return rc;
}
// the pixels a workgroup of the flat launches covers: the tests size their cases from it
extern "C" int tdnet_op_runs_block(void) { return TD_RN_BLOCK; }
