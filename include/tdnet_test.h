/*
 * tdnet_test.h -- entry points of libtdnet_hip_test.so ONLY: single-operator calls (tests/ check each kernel family against torch fp32 / fp64
 * through them) and tuning probes.  libtdnet_hip_test.so is built from the same sources as the product library plus tdnet_amd/csrc/td_ops_test.h
 * and exports everything include/tdnet.h declares as well; the PRODUCT library libtdnet_hip.so exports none of the names below.
 *
 * Every *_dev argument is a tensor of exactly the stated size: an entry reads and writes nothing outside it and asks for no alignment beyond a fresh
 * allocation's 256 bytes (padding a kernel wants -- the attention's 128-row V', the stem image's border -- is made inside the entry).  tests/opcheck.py's
 * guarded mems (GuardedNumpyMem / GuardedTorchMem: NaN bands around inputs, a fixed pattern around outputs) hold the entries to that, under the
 * emulator and on the device (tests/ops_edge_cases.py).
 */
#ifndef TDNET_TEST_H
#define TDNET_TEST_H
#include "tdnet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Roofline / tuning probes: sustained fp32-MFMA TFLOP/s of a register-only MFMA loop, and the average device ms of
 * `iters` launches of one conv configuration (random data, tile as in tdnet_op_conv2d).                             */
double tdnet_bench_mfma_peak(int waves_per_simd, int iters, void* stream);
double tdnet_bench_conv(int H, int W, int Cin, int Cout, int KS, int stride, int dil, int tile /* -1: heuristic, -2: the fused 64-channel Winograd kernel at any size */, int iters,
                        const tdnet_opts* opts /* NULL = defaults */, void* stream);

/* ---- single-operator entry points (used by tests/ to check each kernel family against torch fp32) -------------- */
/* NHWC conv: in [H,W,Cin] dev, weight OIHW host [Cout,Cin,KS,KS], bias host [Cout] or NULL, residual dev
 * [Ho,Wo,Cout] or NULL, act 0 none / 1 ReLU / 2 LeakyReLU(0.01); out [Ho,Wo,Cout] dev.                           */
int tdnet_op_conv2d(const float* in_dev, int H, int W, int Cin, const float* w_host, const float* bias_host,
                    int Cout, int KS, int stride, int dil, const float* resid_dev, int act,
                    const tdnet_opts* opts /* NULL = defaults */,
                    int tile /* -1 = heuristic; 0: 128x128, 1: 64x128, 2: 128x64, 3..5: the same on the two-stage pipeline */,
                    float* out_dev, void* stream);
/* A conv on the fused 64-channel Winograd F(4x4,3x3) kernel (k_wino4_f64, tdnet_opts.fusion bit 4194304) at ANY map size: a frame takes that route only from
 * 32768 output pixels on, so small maps reach the kernel through this entry alone.  Arguments as tdnet_op_conv2d's.  The route takes Cin = Cout = 64, KS 3,
 * stride 1, dil 1, act 0 / 1; anything else fails before a byte is allocated or a kernel launched.                                                     */
int tdnet_op_conv_wino_f64(const float* in_dev, int H, int W, int Cin, const float* w_host, const float* bias_host,
                           int Cout, int KS, int stride, int dil, const float* resid_dev, int act, float* out_dev, void* stream);
/* the same conv with the fp16 activation STORAGE of tdnet_opts.precision = 1: in / resid are rounded to fp16 maps in HBM, the kernel
 * reads and writes fp16 (fp16 MFMA, fp32 accumulate), the fp16 result is widened into out_dev.  Cin % 64 == 0.
 * tile: -1 = heuristic, 0..5 as tdnet_op_conv2d, or a form of the LDS-DMA kernel (td_conv_hd.h): 16 / 17 / 18 / 19 = 128 / 192 / 256 rows,
 * 256 x 256; 21 = 128 rows on two buffers; 22 = 128 rows, eight waves; 25 / 26 = 192 / 128-row row images, one barrier per K step;
 * 27 / 28 = 256 / 192 rows, early landing; 31 / 32 = 128 / 192 rows with loader waves; 34 / 35 = narrow 128 / 192 x 64 tiles.
 * 32 + (16 .. 29), i.e. 48 .. 61: the same tile staged tap by tap.  20, 23, 24, 29, 30, 33, 36 (removed forms) fail.                              */
int tdnet_op_conv2d_f16io(const float* in_dev, int H, int W, int Cin, const float* w_host, const float* bias_host,
                          int Cout, int KS, int stride, int dil, const float* resid_dev, int act, int tile, float* out_dev, void* stream);
/* the same conv with the storage of each side chosen -- the forms only the rim of a frame's fp16 backbone reaches.  in16 != 0: in / resid are rounded to
 * fp16 maps the kernel reads (the residual's type follows the input's), else the kernel reads the fp32 tensors and rounds while staging; out16 != 0: the
 * kernel writes an fp16 map that is widened into out_dev, else it writes out_dev.  in16 = 0, out16 = 1: a deep stem's second conv; in16 = 1, out16 = 0:
 * the backbone's last conv (fp16 residual, not in place) and, on the LDS-DMA tile codes and -1, the head conv on the fp16 LayerNorm map.  Tile codes as
 * tdnet_op_conv2d_f16io; the LDS-DMA ones need in16.                                                                                                  */
int tdnet_op_conv2d_f16mix(const float* in_dev, int H, int W, int Cin, const float* w_host, const float* bias_host,
                           int Cout, int KS, int stride, int dil, const float* resid_dev, int act, int tile, int in16, int out16, float* out_dev, void* stream);
/* ng = 1 .. 3 convs of tdnet_opts.precision = 1 through the grouping decision and the launch a frame uses for the Encoding's first / second layers and
 * for a BasicBlock's conv1 beside its downsample (tdnet_opts.fusion bit 131072: one launch of k_conv_igemm_h_group where the members share a kernel
 * form, else one launch each).  Every argument up to out_dev is an array of ng entries: member g is in_dev[g] [H[g],W[g],Cin[g]] -> out_dev[g]
 * [Ho,Wo,Cout[g]] with w_host[g] OIHW, bias_host[g] [Cout[g]] or NULL (bias_host itself may be NULL), act 0 / 1 / 2, no residual, planned as
 * tdnet_op_conv2d_f16mix plans it for (tile, in16, out16).  Members may name the same in_dev (same sizes): with in16 they read one fp16 map.
 * fusion: the tdnet_opts.fusion bits of the call.  *grouped (may be NULL): 1 = the grouped kernel ran, 0 = the members ran one by one.  The kernel
 * forms the same products in the same order either way: each out_dev[g] holds the bits of tdnet_op_conv2d_f16mix on that member alone.       */
int tdnet_op_conv_group_f16(int ng, const float* const* in_dev, const int* H, const int* W, const int* Cin, const float* const* w_host,
                            const float* const* bias_host, const int* Cout, const int* KS, const int* stride, const int* dil, const int* act,
                            float* const* out_dev, int tile, int in16, int out16, int fusion, int* grouped, void* stream);
/* Both cache entries of a frame in its one launch: q_dev [h,w,C1], v_dev [h,w,C2] -> q_out_dev [hk,wk,C1], v_out_dev [hk,wk,C2] with hk = (h - 1) / 4 + 1,
 * wk = (w - 1) / 4 + 1: x[::4, ::4] of either map (MaxPool2d(kernel 1, stride 4), transformer.py:26,36), with the grid formula of a frame (a frame
 * has C1 = 64; the grid is capped at 2048 workgroups of 256 lanes, one lane per float4, grid-stride beyond).  C1, C2 multiples of 4.                  */
int tdnet_op_cache_subsample(const float* q_dev, const float* v_dev, int h, int w, int C1, int C2, float* q_out_dev, float* v_out_dev, void* stream);
/* A stride-1 1x1 conv (+ bias, act) on the image rows y % ny == cy only: in [H,W,Cin] -> out [H,W,Cout], through the batched GEMM (batch = row, one
 * weight set) that runs the downsample conv of one row-parity chain of a frame.  The layer is planned for the whole map as tdnet_op_conv2d plans it with
 * tile -1, so the written rows hold tdnet_op_conv2d's bits; rows of the other classes are NOT written; a class without rows launches nothing.  An
 * error, with nothing launched, where the plan is not the persistent-GEMM route (gemm_persistent = 0, Cin % 64 != 0, precision = 1, ...).            */
int tdnet_op_conv1x1_rows(const float* in_dev, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout, int act,
                          const tdnet_opts* opts /* NULL = defaults */, int ny, int cy, float* out_dev, void* stream);
/* MaxPool2d(3, stride 2, pad 1) alone (resnet.py:137): NHWC [H,W,C] -> [(H-1)/2+1,(W-1)/2+1,C], C % 4 == 0.  mode 0: the fp32 kernel; 1: fp32 in, fp16 map
 * out (widened into out_dev): behind the fp32 stem of a tdnet_opts.precision = 1 frame; 2: the input rounded to an fp16 map first, fp16 in and out: behind
 * the fp16-MFMA stem and the deep stem (C = 128).                                                                                                        */
int tdnet_op_maxpool(const float* in_dev, int H, int W, int C, int mode, float* out_dev, void* stream);
/* the stem as a frame of tdnet_opts.precision = 1 runs it: the 7x7 conv on the fp16 MFMA writing an fp16 map, the max-pool reading and writing fp16,
 * the result widened into out_dev [H2,W2,64].  tile: -1 = the heuristic's, 0..5 forced; a tile the fp16-MFMA stem does not run on (a frame then keeps
 * the fp32 stem) is an error with nothing allocated or launched.                                                                                        */
int tdnet_op_stem_f16(const float* img_dev, int H, int W, const float* w_host, const float* bias_host, int tile, float* out_dev, void* stream);
/* stem: NCHW image [3,H,W] -> conv7x7 s2 p3 (+bias) -> ReLU -> maxpool3x3 s2 p1 -> NHWC [H2,W2,64] (resnet.py:205-208) */
int tdnet_op_stem(const float* img_dev, int H, int W, const float* w_host, const float* bias_host,
                  const tdnet_opts* opts /* NULL = defaults */, float* out_dev, void* stream);
/* softmax(q k^T / sqrt(dk)) v' + bias + resid: q [Lq,64], k [Lk,64], vp [Lk,DV], bias dev [DV]|NULL, resid [Lq,DV]|NULL.
 * online: tdnet_opts.attention (0 = exact two-pass softmax, 1 = single pass with a lazily moved reference, 2 = 1 pipelined to one
 * barrier per key tile), or 16 = the fp16-MFMA kernel of tdnet_opts.precision = 1 (single pass; operands and P rounded to fp16,
 * softmax and accumulation fp32), or 17 = the split kernel of tdnet_opts.precision = 2 (td_attn_b3.h: q, k, P and v' as three bf16 parts each, six
 * bf16-MFMA products per product, fp32 softmax and accumulation; at DV = 512 k the form is picked by Lq as in a frame; 18 forces the 64-query / eight-wave
 * form, 19 the 32-query form).  The fp32 kernels read V' in whole 128-key tiles: when Lk is not a multiple of 128 the op runs on a
 * zero-padded copy of vp, unless `online | 32` says vp_dev itself has ((Lk + 127) / 128) * 128 rows, the extra ones finite.
 * ln_out != NULL: also the plane LayerNorm (affine ln_g, ln_b [Lq]) of the result, from the strip statistics the kernel's epilogue
 * writes (tdnet_opts.fusion bit 2) -> ln_out [Lq,DV].                                                                          */
int tdnet_op_attention(const float* q_dev, const float* k_dev, const float* vp_dev, const float* bias_dev,
                       const float* resid_dev, int Lq, int Lk, int DV, int online, const float* ln_g_dev, const float* ln_b_dev,
                       float* ln_out_dev, float* out_dev, void* stream);
/* LayerNorm over the (h,w) plane of every channel, affine g,b [h*w] shared by channels (td4_psp18.py:306-312); NHWC */
int tdnet_op_layernorm_hw(const float* x_dev, int HW, int C, const float* g_dev, const float* b_dev, float* out_dev, void* stream);
/* the same with the map written as fp16 (what the head conv of a tdnet_opts.precision = 1 frame reads), widened into out_dev: half() of the above bit for bit */
int tdnet_op_layernorm_hw_f16(const float* x_dev, int HW, int C, const float* g_dev, const float* b_dev, float* out_dev, void* stream);
/* PPM (td4_psp18.py:271-284): c4 NHWC [h,w,512] -> z NHWC [h,w,512]; w_host: 4 folded [128,512] matrices, b_host 4x[128] */
int tdnet_op_ppm(const float* c4_dev, int h, int w, const float* w_host, const float* b_host, int path_num, int pid,
                 float* z_dev, void* stream);
/* The first layers of a path's Encoding on c4 [h,w,C] dev as a frame runs them: pyramid pooling, then the value conv (C -> DV), the query conv (C -> 64, LeakyReLU)
 * and the stride-4 key conv (C -> 64, LeakyReLU).  fold = 1: the pyramid as 64 basis columns (tdnet_opts.fusion bit 2097152: no z map; an error, with nothing
 * allocated, where a frame would not fold); fold = 0: through the assembled z.  ppm_w_host [4][C/4][C], ppm_b_host [4][C/4] (BN folded; path pid keeps channels
 * pid C/8 .. of each level); wv / wq / wk_host [Cout][C] with biases (NULL = 0).  v_out [h w][DV], q_out [h w][64], k_out [hk wk][64] dev;
 * basis_out_dev [h w][64] or NULL: the fold's table of bilinear coefficients (fold = 1 only).                                                            */
int tdnet_op_enc_first(const float* c4_dev, int h, int w, int C, int pid, const float* ppm_w_host, const float* ppm_b_host, const float* wv_host,
                       const float* bv_host, int DV, const float* wq_host, const float* bq_host, const float* wk_host, const float* bk_host, int fold,
                       float* v_out_dev, float* q_out_dev, float* k_out_dev, float* basis_out_dev, void* stream);
/* A 1x1 conv (stride >= 1) planned as tdnet_op_conv2d plans it, on the TWO-SOURCE form of its kernel with nothing behind the split (k_split == nsteps, null
 * second source): bit-identical to tdnet_op_conv2d.  An error where the plan is neither the persistent fp32 GEMM nor the fp32 direct 1x1 conv.           */
int tdnet_op_conv1x1_src2_null(const float* in_dev, int H, int W, int Cin, const float* w_host, const float* bias_host, int Cout, int stride,
                               const float* resid_dev, int act, const tdnet_opts* opts, int tile, float* out_dev, void* stream);
/* 1x1 classifier conv (+bias): x NHWC [HW,C] dev, w [NC,C] dev, b [NC] dev -> planar out [NC,HW] dev; the frame's routing by NC
 * (<= 32: k_classifier, all weights in one workgroup's LDS: (NC * C + 256 * NC) * 4 bytes <= 160 KiB, i.e. C <= 1024 at 32 classes;
 * 33 .. 256: the class-tiled k_classifier_ct, C <= 512).  C a multiple of 16; anything else is an error before a launch.            */
int tdnet_op_classifier(const float* x_dev, int HW, int C, const float* w_dev, const float* b_dev, int NC, float* out_dev, void* stream);
/* The FCN head (td4_psp18.py:295-299): conv3x3 stride 1 (+ bias, act 0 none / 1 ReLU) -> 1x1 classifier (+ bias), planned as a frame plans its head
 * conv.  in [H,W,Cin] dev; w3_host OIHW [Cout,Cin,3,3], b3_host [Cout] or NULL, cls_w_host [NC,Cout], cls_b_host [NC]; out planar [NC,H*W] dev.
 * fused = 1: the classifier inside the Winograd output transform (tdnet_opts.fusion bit 262144's kernel) -- an error, with nothing launched, where a
 * frame would not fuse: the plan is not Winograd (opts), Cout is not 64 or 128, NC > 32, act = 2.  fused = 0: the conv into a temporary hidden
 * map, then the classifier kernel of tdnet_op_classifier.  The two forms give the same bits.                                                     */
int tdnet_op_head_cls(const float* in_dev, int H, int W, int Cin, const float* w3_host, const float* b3_host, int Cout, int act,
                      const float* cls_w_host, const float* cls_b_host, int NC, const tdnet_opts* opts /* NULL = defaults */, int fused,
                      float* out_dev, void* stream);
/* bilinear align_corners=True (td4_psp18.py:227): planar [C,h,w] -> [C,H,W]                                       */
int tdnet_op_upsample(const float* in_dev, int C, int h, int w, int H, int W, float* out_dev, void* stream);
/* The stem's image buffer -- allocated and zeroed as a handle's workspace does -- filled from an fp32 NCHW image [3,H,W] (img_f32_dev) or from
 * uint8 bytes [Hs,Ws,3] at any byte address (src_u8_dev; mean / std as tdnet_set_input_u8; Hs, Ws are ignored with img_f32_dev): exactly one
 * of the two.  rows != 0: the packed-row image of the 7x7 stem [H+7][Wp][3], else NHWC4.  The COMPLETE buffer, border included, is copied to
 * out_dev.  Returns its float count (out_dev == NULL: nothing else happens), <0 on error.                              */
long tdnet_op_stem_image(const float* img_f32_dev, const uint8_t* src_u8_dev, int Hs, int Ws, int H, int W, const double* mean, const double* std,
                         int rows, float* out_dev, size_t capacity, void* stream);
/* tdnet_op_stem_image from an NV12 surface at any byte address (include/tdnet.h "NV12 frames in"; the arguments of tdnet_set_input_nv12).   */
long tdnet_op_stem_image_nv12(const uint8_t* surf_dev, int Hs, int Ws, int pitch, size_t uv_offset, int standard, int H, int W, const double* mean,
                              const double* std, int rows, float* out_dev, size_t capacity, void* stream);
/* tdnet_op_stem_image from a source view (include/tdnet.h "source views"; the arguments of tdnet_set_input_view): base_dev at any byte address. */
long tdnet_op_stem_image_view(const uint8_t* base_dev, const tdnet_view* view, int H, int W, const double* mean, const double* std, int rows, float* out_dev,
                              size_t capacity, void* stream);
/* tdnet_op_stem_image from a YUV surface (include/tdnet.h "surfaces"; the arguments of tdnet_set_input_surface): base_dev at any byte address. */
long tdnet_op_stem_image_surface(const uint8_t* base_dev, const tdnet_surface* surface, int H, int W, const double* mean, const double* std, int rows, float* out_dev,
                                 size_t capacity, void* stream);
/* low-resolution logits [C,h,w] -> labels [H,W] (bilinear align_corners=True, first maximum): int32 through the kernel of tdnet_forward_labels
 * (labels_i32_dev != NULL) and / or uint8 (labels_u8_dev != NULL) through the kernel of its uint8 form.  C in 1..256. */
int tdnet_op_upsample_argmax(const float* in_dev, int C, int h, int w, int H, int W, int32_t* labels_i32_dev, uint8_t* labels_u8_dev, void* stream);
/* The colour map [oh,ow,3] (uint8, any byte address) of low-resolution logits [C,h,w] upsampled to [H,W] -- through the last kernel of tdnet_forward_rgb
 * (labels_u8_dev == NULL) -- or of a uint8 label map [H,W] through tdnet_labels_rgb's kernel (labels_u8_dev != NULL; in_dev, C, h, w are then
 * ignored).  Index tables and colour table are built by the host function tdnet_set_output_rgb uses; palette [n_colours][3] on the host.          */
int tdnet_op_upsample_argmax_rgb(const float* in_dev, int C, int h, int w, int H, int W, int oh, int ow, const uint8_t* palette, int n_colours,
                                 uint8_t* rgb_dev, const uint8_t* labels_u8_dev, void* stream);
/* The overlay [Hs,Ws,3] (uint8, any byte address; include/tdnet.h "overlay out") of low-resolution logits [C,h,w] upsampled to [H,W] -- through the last
 * kernel of the overlay frame entries (labels_u8_dev == NULL) -- or of a uint8 label map [H,W] through the kernel of the unfused overlay entry
 * (labels_u8_dev != NULL; in_dev, C, h, w are then ignored), over the source frame src_dev: packed RGB [Hs,Ws,3] (nv12 = 0; pitch, uv_offset and standard
 * are ignored) or an NV12 surface (nv12 = 1) of that layout, at any byte address.  The source description, the index tables and the colour table are
 * built by the host functions the handle's configuration calls use; palette_rgba [n_colours][4] on the host.                                         */
int tdnet_op_overlay(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* labels_u8_dev, const uint8_t* src_dev, int nv12, int Hs, int Ws,
                     int pitch, size_t uv_offset, int standard, const uint8_t* palette_rgba, int n_colours, uint8_t* out_dev, void* stream);
/* tdnet_op_overlay with a source view in place of its source arguments: out_dev [h,w,3] of the view's rectangle h x w, in the source's colour order. */
int tdnet_op_overlay_view(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* labels_u8_dev, const uint8_t* base_dev, const tdnet_view* view,
                          const uint8_t* palette_rgba, int n_colours, uint8_t* out_dev, void* stream);
/* tdnet_op_overlay with a YUV surface in place of its source arguments: out_dev [h,w,3] of the surface's rectangle h x w, r g b. */
int tdnet_op_overlay_surface(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* labels_u8_dev, const uint8_t* base_dev, const tdnet_surface* surface,
                             const uint8_t* palette_rgba, int n_colours, uint8_t* out_dev, void* stream);
/* tdnet_op_picture_view with surfaces: the destination is dst_surface (a 4:2:0 layout) or, dst_surface == NULL, dst_view; the overlay's source is src_surface
 * or, src_surface == NULL, src_view; src_base_dev == NULL: the colour map oh x ow.  Exactly the kernels the frame entries launch for that pair.       */
int tdnet_op_picture_surface(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* labels_u8_dev, const uint8_t* palette, int n_colours,
                             const uint8_t* src_base_dev, const tdnet_surface* src_surface, const tdnet_view* src_view, int oh, int ow, uint8_t* dst_base_dev,
                             const tdnet_surface* dst_surface, const tdnet_view* dst_view, void* stream);
/* The picture into a destination view (include/tdnet.h "destination views"), through exactly the kernels the frame entries launch with one in force:
 * of low-resolution logits [C,h,w] (labels_u8_dev == NULL) or of a uint8 label map [H,W] (in_dev, C, h, w are then ignored); the overlay over the source
 * view (src_base_dev, src_view; palette [n_colours][4] r g b a on the host) or, src_base_dev == NULL, the colour map oh x ow (palette [n_colours][3];
 * src_view ignored).  dst_base_dev: the destination frame's base, at any byte address; the view's rectangle must be the picture's size.           */
int tdnet_op_picture_view(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* labels_u8_dev, const uint8_t* palette, int n_colours,
                          const uint8_t* src_base_dev, const tdnet_view* src_view, int oh, int ow, uint8_t* dst_base_dev, const tdnet_view* dst_view, void* stream);
/* cm_dev [C,C] uint64 -- ACCUMULATED into, not cleared -- += the confusion counts (include/tdnet.h "score out") of gt_dev [H,W] uint8 (any byte
 * address) through gt_map (256 bytes on the host, NULL = identity) against the labels of low-resolution logits [C,h,w] upsampled to [H,W], through
 * tdnet_forward_score's last kernel (labels_in_u8_dev == NULL; it also writes the uint8 label map if labels_u8_dev != NULL), or against a uint8
 * label map [H,W] through tdnet_labels_score's kernel (labels_in_u8_dev != NULL; in_dev, h, w and labels_u8_dev are then ignored).  C in 1..256. */
int tdnet_op_upsample_argmax_score(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* gt_dev, const uint8_t* gt_map, uint8_t* labels_u8_dev,
                                   uint64_t* cm_dev, const uint8_t* labels_in_u8_dev, void* stream);
/* labels_u8_dev [H,W] (or NULL) and conf_u8_dev [H,W] (include/tdnet.h "confidence out"; any byte addresses) of low-resolution logits [C,h,w]
 * upsampled to [H,W], through the last kernel of the frame entries that give labels and confidence (logits_full_dev == NULL), or of
 * full-resolution logits [C,H,W] through the kernel of the unfused entry (logits_full_dev != NULL; in_dev, h, w are then ignored).
 * min_conf, reject_label in 0..255; C in 1..256.  TDNET_CONF_PASSES=1 / 2 in the environment picks the one-pass / two-pass form of the kernels
 * (tools/conf_probe.py); unset: the form the library's own entries launch.                                                               */
int tdnet_op_upsample_argmax_conf(const float* in_dev, int C, int h, int w, int H, int W, uint8_t* labels_u8_dev, uint8_t* conf_u8_dev, int min_conf,
                                  int reject_label, const float* logits_full_dev, void* stream);
/* labels_u8_dev [H,W] (or NULL) and matte_u8_dev [H,W] (include/tdnet.h "matte out"; any byte addresses) of low-resolution logits [C,h,w]
 * upsampled to [H,W], through the last kernel of the matte frame entries (logits_full_dev == NULL), or of full-resolution logits [C,H,W] through
 * the kernel of the unfused entry (logits_full_dev != NULL; in_dev, h, w are then ignored).  classes: n class ids below C on the HOST (n in
 * 0..256, duplicates legal, NULL with n = 0); C in 1..256.                                                                                   */
int tdnet_op_upsample_argmax_matte(const float* in_dev, int C, int h, int w, int H, int W, uint8_t* labels_u8_dev, uint8_t* matte_u8_dev, const uint8_t* classes,
                                   int n, const float* logits_full_dev, void* stream);
/* The composite of include/tdnet.h "matte out" through the kernels the composite entries launch: of low-resolution logits [C,h,w] and the class set
 * classes[0 .. n) (matte_u8_dev == NULL) or of a matte map [H,W] (matte_u8_dev != NULL; in_dev, C, h, w, classes, n are then ignored), over the source at
 * src_base read through src_surface (if not NULL) or src_view, into the contiguous block [Hs,Ws,3] at dst_base (dst_view == NULL) or into dst_view's
 * rectangle of the pitched frame at dst_base.  mode: TDNET_COMPOSITE_COLOUR with bg_rgb [3] (host), or TDNET_COMPOSITE_ALPHA with bg_rgb NULL and a
 * 32-bit dst_view.  Any byte addresses.                                                                                                       */
int tdnet_op_composite(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* classes, int n, const uint8_t* matte_u8_dev, const uint8_t* src_base,
                       const tdnet_view* src_view, const tdnet_surface* src_surface, uint8_t* dst_base, const tdnet_view* dst_view, int mode, const uint8_t* bg_rgb,
                       void* stream);
/* Stage 1 of the refined matte (include/tdnet.h "refined matte") alone, through the launch the operator entry enqueues first: the coefficient planes a_q
 * (aq_dev, int16 [rows,cols]) and b_q (bq_dev, int32 [rows,cols]) of a guide and a matte at any byte addresses.  The scratch is allocated for the call. */
int tdnet_op_refine_coeff(const uint8_t* guide_dev, size_t guide_pitch, const uint8_t* matte_dev, size_t matte_pitch, int rows, int cols, int radius, int eps,
                          int16_t* aq_dev, int32_t* bq_dev, void* stream);
/* The gather launch of the refined frame entries alone: luma and M_src [Hs,Ws] (tight, 4-byte aligned) of the source at src_base read through src_surface (if not
 * NULL) or src_view; the matte from logits [C,h,w] and the class set classes[0 .. n) (matte_u8_dev == NULL) or from a matte map [H,W].                 */
int tdnet_op_refine_gather(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* classes, int n, const uint8_t* matte_u8_dev, const uint8_t* src_base,
                           const tdnet_view* src_view, const tdnet_surface* src_surface, uint8_t* luma_dev, uint8_t* msrc_dev, void* stream);
/* the tiles of the operator's two launches (columns; rows of the first; rows of the second): the tests size their cases from them */
int tdnet_op_refine_tile(int* tx, int* ty_coeff, int* ty_apply);
/* Regions out (include/tdnet.h) through exactly the launches the regions entries enqueue, on maps the caller holds: from low-resolution logits [C,h,w]
 * (labels_in_u8_dev == NULL; the uint8 labels go to labels_u8_dev [H,W] if given) or from a uint8 label map [H,W] at any byte address (in_dev, h, w and
 * labels_u8_dev are then ignored).  classes: n class ids below C on the HOST; connectivity 4 | 8; ids_dev: int32 [H,W] or NULL; regions_dev: 16 + 48
 * max_regions bytes, 8-byte aligned.  The workspace is allocated for the call.                                                                 */
int tdnet_op_regions(const float* in_dev, int C, int h, int w, int H, int W, const uint8_t* labels_in_u8_dev, uint8_t* labels_u8_dev, const uint8_t* classes, int n,
                     int connectivity, int max_regions, int min_area, int32_t* ids_dev, void* regions_dev, void* stream);
/* the tile (rows, columns) of the first launch: the tests size their cases from it */
int tdnet_op_regions_tile(int* th, int* tw);
/* Tracks out (include/tdnet.h) through exactly the launches the tracks entries enqueue, one frame per call, from a uint8 label map [H,W] at any byte
 * address.  state_dev: tdnet_op_tracks_state_bytes(H, W) bytes the CALLER owns, 16-byte aligned; all zero is the reset state, and the blob carries the
 * tracks from call to call.  ids_dev, track_ids_dev: int32 [H,W] or NULL; regions_dev: 16 + 48 max_regions bytes, tracks_dev: 16 + 24 max_regions bytes,
 * both 8-byte aligned.  The regions workspace is allocated for the call.                                                                       */
size_t tdnet_op_tracks_state_bytes(int H, int W);
int tdnet_op_tracks(const uint8_t* labels_u8_dev, int C, int H, int W, const uint8_t* classes, int n, int connectivity, int max_regions, int min_area, int min_overlap,
                    void* state_dev, int32_t* ids_dev, void* regions_dev, int32_t* track_ids_dev, void* tracks_dev, void* stream);
/* the slots of the internal pair table for an H x W map (a power of two >= 2 H W): the tests size the worst case from it */
long tdnet_op_tracks_capacity(int H, int W);
/* Runs out (include/tdnet.h) through exactly the launches the runs entries enqueue, on maps the caller holds.  Exactly one source: low-resolution logits
 * [C,h,w] (in_dev; the label launch writes labels_u8_dev [H,W], which is then required), a uint8 map [H,W] at any byte address (map_u8_dev) or an int32 map
 * [H,W], 4-byte aligned (map_i32_dev).  runs_dev: 16 + 8 (max_runs + 1) bytes, 8-byte aligned.  The workspace is allocated for the call.            */
int tdnet_op_runs(const float* in_dev, int C, int h, int w, int H, int W, uint8_t* labels_u8_dev, const uint8_t* map_u8_dev, const int32_t* map_i32_dev, int max_runs,
                  void* runs_dev, void* stream);
/* the way back, one launch: exactly one of out_u8_dev (any byte address) and out_i32_dev (4-byte aligned) */
int tdnet_op_runs_decode(const void* runs_dev, int max_runs, int fill, int H, int W, uint8_t* out_u8_dev, int32_t* out_i32_dev, void* stream);
/* the pixels a workgroup of the flat launches covers: the tests size their cases from it */
int tdnet_op_runs_block(void);
/* that host function's index table for one axis (tdnet_amd/dataloader.py nearest_index): out_host [n_dst] int32.  No device work.             */
int tdnet_op_nearest_index(int n_src, int n_dst, int32_t* out_host);

#ifdef __cplusplus
}
#endif
#endif
