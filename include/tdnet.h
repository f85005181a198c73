/*
 * tdnet.h -- C ABI of the MI355X-native TDNet per-frame inference hot path (libtdnet_hip.so).
 *
 * The reference's boundary for this path is a Python nn.Module API, not a C API:
 *     model = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=...)      Testing/test.py:26
 *     out   = model(image, pos_id=i % path_num)                               Testing/test.py:53
 * tdnet_amd/model/{td4_psp18,td2_psp50,pspnet}.py keep that Python API and call the entry points below through
 * ctypes; INTEGRATION.md shows the stub.  Plain pointers and sizes only -- no torch types cross this line.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; tdnet_last_error() gives the message (thread-local).
 *   - "dev" pointers are device (HBM) pointers owned by the caller; the handle owns weights, workspace and
 *     the K/Q/V FIFO.  One handle per video stream and per GPU; a handle is not thread-safe.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  The frame calls (tdnet_forward*, tdnet_encode,
 *     tdnet_propagate*, tdnet_cache_*) only ENQUEUE work and never synchronise with the host -- with one exception a caller can
 *     remove: a handle whose frame uses a second internal stream (row-parity chains) checks ONCE per caller stream that this stream
 *     sits on another hardware queue than the caller's (two 40-us spin kernels, a host synchronisation of both streams).
 *     tdnet_warmup(h, stream) does that check explicitly; a frame call on a stream tdnet_warmup has not seen does it lazily
 *     (skipped while the stream is being captured into a hipGraph).  Every caller stream is checked ONCE per handle (the handle remembers
 *     the streams it has seen; alternating between two streams does not repeat the check), for at most 8 distinct streams.  tdnet_finalize_weights, tdnet_create_shared, tdnet_get_stage
 *     and tdnet_score_read synchronise, the configuration calls tdnet_set_input_u8 / tdnet_set_input_nv12 / tdnet_set_output_rgb / tdnet_set_score may; tdnet_score_reset
 *     and tdnet_score_export only enqueue (as do the test library's tdnet_op_* / tdnet_bench_* entries, include/tdnet_test.h).
 *   - tensors are fp32 unless an entry says otherwise: image in / logits out are NCHW like the reference, labels int32 [H,W]; internal
 *     layout is NHWC.  The *_u8 entries are the byte ends of the same frame: the image as uint8 HWC RGB at its SOURCE size (resized and
 *     normalised on the device exactly as tdnet_amd/dataloader.py does on the host), labels as uint8 [H,W] (nclass <= 256 always).
 */
#ifndef TDNET_H
#define TDNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdnet tdnet_t;

typedef struct tdnet_cfg {
    int32_t model;      /* 4 = td4 (Testing/model/pspnet/td4_psp18.py:29-120), 2 = td2 (td2_psp50.py:29-96),
                           1 = pspnet, the stateless comparison model (pspnet.py:31-115)                             */
    int32_t backbone;   /* 18 / 34 (BasicBlock, resnet.py:218-236), 50 / 101 (Bottleneck + deep stem, :62-111,122-131)     */
    int32_t nclass;     /* 1..256: 19 for Cityscapes (test.py:26), 40 for NYUD-v2                                    */
    int32_t height;     /* input H; the LayerNorm affine is the feature map's [h, w] (td4_psp18.py:107-110): [ceil(H/8), ceil(W/8)]
                           with the dilated backbone, five halvings n -> (n-1)/2+1 with dilated = 0 (tdnet_feature_dims)   */
    int32_t width;      /* input W                                                                                   */
    int32_t device;     /* HIP device ordinal                                                                        */
} tdnet_cfg;

/* Per-handle kernel configuration.  Nothing in this library is process-wide: two handles in one process may differ.
 * tdnet_opts_default() fills the defaults; fields left 0 by a caller that memset()s the struct select the plain variants. */
#define TDNET_WINOGRAD_DEFAULT 3
#define TDNET_ATTENTION_DEFAULT 2
/* The live bits of tdnet_opts.fusion and tdnet_opts.overlap by name (what each does: the field comments below, which cite them by value). */
#define TDNET_FUSION_LN_STATS 2            /* LayerNorm strip statistics from the attention epilogue */
#define TDNET_FUSION_LN_IN_HEAD 4          /* LayerNorm inside the head's Winograd input transform */
#define TDNET_FUSION_A_DIRECT 32           /* Cout <= 64 convs: A operand straight from global memory */
#define TDNET_FUSION_DMA_LOADERS 8192      /* precision 1: LDS-DMA conv tiles with dedicated loader waves */
#define TDNET_FUSION_DMA_NARROW 32768      /* precision 1: narrow LDS-DMA conv tiles on small maps and ResNet layer1 */
#define TDNET_FUSION_STEM_ROWS 65536       /* the 7x7 stem on a packed-row image */
#define TDNET_FUSION_CONV_GROUPS 131072    /* precision 1: convs that share a kernel form in one launch */
#define TDNET_FUSION_CLS_IN_HEAD 262144    /* the classifier inside the head conv's Winograd output transform */
#define TDNET_FUSION_SPLIT_NARROW 524288   /* precision 2: the narrow direct convs and the packed-row stem on the split bf16 MFMA */
#define TDNET_FUSION_LATE_CHAIN 1048576    /* the cache-only attention chain forks in front of the first dilated block */
#define TDNET_FUSION_PPM_FOLD 2097152      /* fp32: the pyramid folded through the Encoding's first 1x1 convs as 64 basis columns (no `z` map) */
#define TDNET_FUSION_WINO_F64 4194304     /* fp32: ResNet layer1's 64 -> 64 3x3 convs on the fused Winograd F(4x4) kernel (large maps) */
#define TDNET_OVERLAP_CHAINS 1             /* row-parity chains on two streams */
#define TDNET_OVERLAP_LOWREG_TRANSFORMS 2  /* the low-register F(4x4) transform kernels everywhere */
#define TDNET_OVERLAP_CHAINS_ANY_SIZE 4    /* the chains at any map size */
#define TDNET_OVERLAP_GEMM_DMA 8           /* the Winograd GEMMs on the LDS-DMA-fed kernel */
#define TDNET_OVERLAP_VW_SHIFT 4           /* bits 4-5: log2 of the channels per lane of the chunked transform kernels */
#define TDNET_OVERLAP_VW_MASK 0x30
/* 8364070: the measured default (measurements: DESIGN.md 5, DESIGN_experiments.md) */
#define TDNET_FUSION_DEFAULT (TDNET_FUSION_LN_STATS | TDNET_FUSION_LN_IN_HEAD | TDNET_FUSION_A_DIRECT | TDNET_FUSION_DMA_LOADERS | TDNET_FUSION_DMA_NARROW | \
                              TDNET_FUSION_STEM_ROWS | TDNET_FUSION_CONV_GROUPS | TDNET_FUSION_CLS_IN_HEAD | TDNET_FUSION_SPLIT_NARROW | TDNET_FUSION_LATE_CHAIN | TDNET_FUSION_PPM_FOLD | \
                              TDNET_FUSION_WINO_F64)
#define TDNET_FUSION_MASK TDNET_FUSION_DEFAULT   /* the bits of tdnet_opts.fusion that exist (= the default); the others are cleared and ignored */
/* 41: row-parity chains with 4 channels per lane (+2 %) on the LDS-DMA-fed GEMM (+0.9 %): profiles/r03a_*, r03m_* */
#define TDNET_OVERLAP_DEFAULT (TDNET_OVERLAP_CHAINS | TDNET_OVERLAP_GEMM_DMA | (2 << TDNET_OVERLAP_VW_SHIFT))
/* 0x3f: the bits of tdnet_opts.overlap that exist: 1 | 2 | 4 | 8 | 16 | 32 */
#define TDNET_OVERLAP_MASK (TDNET_OVERLAP_CHAINS | TDNET_OVERLAP_LOWREG_TRANSFORMS | TDNET_OVERLAP_CHAINS_ANY_SIZE | TDNET_OVERLAP_GEMM_DMA | TDNET_OVERLAP_VW_MASK)
typedef struct tdnet_opts {
    int32_t winograd;        /* conv algorithm: 0 = direct implicit GEMM everywhere, 3 (default) = Winograd F(4x4,3x3) for the stride-1 3x3
                                convs with Cin, Cout >= 128 (ResNet layers 2-4 + FCN head), 4 = F(4x4,3x3) for every stride-1 3x3 (test
                                hook).  All fp32.  (1, 2 were F(2x2,3x3), removed in round 5; they are read as 3, 4.)                  */
    int32_t precision;       /* 0 = exact fp32 MFMA (default; the headline), 1 = fp16 MFMA with fp32 accumulation (BASELINE config 5),
                                2 = OPT-IN, fp32-ACCURATE on the 16x faster bf16 MFMA: operands as the exact sum of three bf16 parts, six bf16 products
                                    with fp32 accumulation (every product to 2^-26 relative; not bit-identical to the fp32 MFMA, held to the SAME gates:
                                    tests/test_gpu_b3.py).  On the split kernels: the 36 batched GEMMs of every Winograd F(4x4) conv and the large
                                    stride-1 1x1 convs where the split GEMM wins (td_gemm_b3.h), the final attention of every frame (td_attn_b3.h),
                                    and with fusion bit 524288 the direct convs of <= 128 output channels and the packed-row stem (td_conv_ad_b3.h).
                                    Everything else (the cached-frame attention steps, the other direct convs, transforms, storage) is the fp32 path.
                                3 = TEST HOOK: 2 with the split kernel at ANY GEMM size (small maps in the tests)                        */
    int32_t pipeline;        /* conv software pipeline: 0 = one-stage prefetch, 1 (default) = two-stage                           */
    int32_t gemm_persistent; /* 1 (default) = stride-1 1x1 convs and the Winograd GEMMs on the persistent multi-tile GEMM kernel,
                                0 = one tile per workgroup on the conv kernel, n > 1 = persistent with the grid forced to n (tests)  */
    int32_t reserved0;       /* must be 0 (rounds 1-4: `stagger`, a start delay of co-resident workgroups; measured neutral, removed) */
    int32_t attention;       /* 0 = exact two-pass softmax (row maxima first), 1 = single pass, lazily moved reference, 2 (default) = the same pipelined to one barrier per key tile        */
    int32_t fusion;          /* bit mask of launch-level fusions (TDNET_FUSION_MASK), each measured on its own; default TDNET_FUSION_DEFAULT:
                                2 = LayerNorm strip statistics written by the attention epilogue (no separate pass over the map),
                                4 = LayerNorm normalisation applied inside the head's Winograd input transform (no `ln` map in HBM),
                                32 = Cout <= 64 convs (layer1, the stems) read their A operand straight from global memory in MFMA fragment layout (td_conv_ad.h),
                                8192 = precision 1: the 128 / 192 x 128 LDS-DMA conv tiles with four dedicated loader waves (k_conv_dma_h3p); bit-identical,
                                32768 = precision 1: on maps of <= 16384 output pixels the 3x3 "same" convs of <= 256 output channels, and ResNet layer1, on
                                     NARROW tiles (128 / 192 rows x 64 channels, k_conv_dma_h3n); bit-identical,
                                65536 = fp32, with bit 32: the 7x7 stem reads a packed-row image ([H + 7][~W + 9][3], zero border): K = 168 instead of 224 (td_conv_ad.h STEM = 2),
                                131072 = precision 1: a BasicBlock's conv1 and 1x1 downsample in one launch, the Encoding's five 1x1 convs in two
                                     (k_conv_igemm_h_group); bit-identical,
                                262144 = fp32 / precision 2: the FCN head's 1x1 classifier inside its 3x3 conv's Winograd output transform (k_wino4_out_cls); bit-identical,
                                524288 = precision 2: the convs of bit 32, the packed-row stem and the direct convs of 65 .. 128 output channels on the
                                     split bf16 MFMA (td_conv_ad_b3.h),
                                1048576 = fp32 / precision 2: the cache-only attention chain forks in front of the backbone's first dilated block (layer3)
                                     instead of at the frame's start; bit-identical (ignored with precision 1),
                                2097152 = fp32 (precision 0; ignored otherwise and by the single-frame PSPNet): the pyramid half of the map `z` is never assembled.  Its
                                     4 FS channels are a linear function of the 50 pooled vectors, so the Encoding's first 1x1 convs (value, query, strided key) run
                                     over K = XS + 64 instead of XS + 4 FS: c4's channel slice, then a constant [h w][64] table of bilinear coefficients against 64 rows
                                     G = pooled features x the layer's pyramid weights, computed per frame (k_ppm_fold_g).  Same gates, not bit-identical (another
                                     summation order); tdnet_get_stage("z") assembles the map on request.  Taken where those convs are planned on the persistent
                                     GEMM / the direct 1x1 kernel and XS % 64 == 0; otherwise the frame runs as without the bit.
                                4194304 = fp32 (precision 0) with winograd >= 3: a 3x3 stride-1 conv from 64 to 64 channels (ResNet layer1, the deep stem's second conv)
                                     on a map of >= 32768 output pixels runs on ONE fused Winograd F(4x4,3x3) kernel that keeps the transformed tiles in LDS
                                     (k_wino4_f64, td_wino_f64.h) instead of the direct kernel.  Same gates, not bit-identical; smaller maps keep the direct kernel.
                                Retired, ignored: 1, 8, 16, 64, 128, 256, 512, 1024, 2048, 4096, 16384 (DESIGN_experiments.md 4.4, 10.10).   */
    int32_t overlap;         /* bit mask (default TDNET_OVERLAP_DEFAULT), on BasicBlock backbones:
                                1 = the trailing run of even-dilation convs (ResNet layers 3-4: resnet.py:181-198) as its even-row and odd-row halves
                                    (independent chains) on two HIP streams; fp32 / precision 2 with winograd >= 3, on maps of >= 24000 feature pixels
                                    (h w) (precision 1: ignored),
                                2 = the low-register transform kernels for every F(4x4) conv, chained or not,
                                4 = the chains of bit 1 at ANY map size (tests, A/B),
                                8 = the Winograd GEMMs on the LDS-DMA-fed kernel (td_gemm_dma.h: no staging registers, 82 VGPRs),
                                bits 4-5 = channels per lane of the chunked transform kernels: 0 -> 1, 1 -> 2, 2 -> 4.
                                Retired, ignored: 64, 128 (DESIGN_experiments.md 4.1d, 9.2, 10.10).                                   */
    int32_t reserved[8];     /* must be 0 (round 4: cu_reserve / cu_mode, the CU-mask-partitioned pipeline, -2.5x, removed)        */
} tdnet_opts;
void tdnet_opts_default(tdnet_opts* o);

/* Backbone layout: the `dilated` / `multi_grid` arguments of the reference constructors (resnet.py:138-158).  Every field is 0 or 1. */
typedef struct tdnet_arch {
    int32_t dilated;      /* 1 (default) = layers 3-4 at stride 1, dilation 2 / 4: output stride 8 (resnet.py:140-149);
                             0 = layers 3-4 at stride 2, dilation 1: output stride 32 (resnet.py:150-158)                        */
    int32_t multi_grid;   /* with dilated = 1: 1 (default) = layer-4 conv1 dilations 4, 8, 16 (resnet.py:181,196), 0 = 2, 4, 4
                             (BasicBlock conv2 and every later block: 4; resnet.py:188,199).  Ignored with dilated = 0.          */
    int32_t reserved[6];  /* must be 0                                                                                           */
} tdnet_arch;
void tdnet_arch_default(tdnet_arch* a);                                                  /* {1, 1}: the backbone the reference ships */

/* ---- lifecycle: replaces the nn.Module constructor + load_state_dict (td4_psp18.py:32-120, :232-240) ---------- */
int  tdnet_create(const tdnet_cfg* cfg, tdnet_t** out);                                  /* default options */
int  tdnet_create_opts(const tdnet_cfg* cfg, const tdnet_opts* opts /* NULL = defaults */, tdnet_t** out);
/* Any backbone layout.  tdnet_create_opts(cfg, opts) is this with arch {1, 1}, except that it keeps refusing the single-frame
 * PSPNet (model 1) on the BasicBlock backbones 18 / 34, which only this entry accepts (pspnet.py:50-57: 7x7 stem, PSPHead(512)).  */
int  tdnet_create_arch(const tdnet_cfg* cfg, const tdnet_arch* arch /* NULL = {1, 1} */, const tdnet_opts* opts /* NULL = defaults */,
                       tdnet_t** out);
int  tdnet_get_opts(const tdnet_t* h, tdnet_opts* out);
int  tdnet_get_arch(const tdnet_t* h, tdnet_arch* out);
/* Size of the backbone's output map (and of the LayerNorm affine, the attention's query grid and the low-resolution logits). */
int  tdnet_feature_dims(const tdnet_t* h, int* height, int* width);
void tdnet_destroy(tdnet_t* h);

/* One call per state_dict entry, reference key names ("pretrained1.layer4.1.conv2.weight", ...), host fp32
 * data in the reference's own layout (conv OIHW).  Unknown names and wrong sizes are errors (strict=True,
 * td4_psp18.py:237); unused reference tensors (pretrainedN.fc.*, *.num_batches_tracked) are accepted and ignored. */
int  tdnet_set_weight(tdnet_t* h, const char* name, const float* host, size_t count);
/* Folds BN (fp64), repacks to the kernels' layouts, uploads; then allocates the handle's workspace, FIFO and streams.
 * Fails listing the first missing tensor.  Synchronises the device.                                               */
int  tdnet_finalize_weights(tdnet_t* h);
/* A further handle on the SAME weight block as `weights_of` (which must be finalized): own workspace, own K/Q/V FIFO, own
 * streams -- another video stream on this GPU, the samples 1..N-1 of a batch (the reference's batch shares one nn.Module's
 * parameters: td4_psp18.py:216-229), or the second lane of a frame-pipelined clip -- without a second copy of the packed weights
 * and without folding / packing / uploading them again; the backbone layout (tdnet_arch) is the block's too.  `opts` must be NULL (inherit) or equal to the block's options: the
 * packing depends on them.  The block is reference-counted (atomically): handles may be destroyed in any order, the weights go with the
 * last.  Threading: a HANDLE is single-threaded (one host thread at a time), but tdnet_create_shared / tdnet_destroy of DIFFERENT handles
 * on one block may run concurrently on different host threads (a garbage collector's finaliser thread, say).                    */
int  tdnet_create_shared(const tdnet_t* weights_of, const tdnet_opts* opts /* NULL = inherit */, tdnet_t** out);
/* One-time placement of the handle's internal streams for frames that will arrive on `stream` (see "Conventions"): host-
 * synchronising, idempotent per stream.  Call it before capturing frames into a hipGraph or before a latency-critical first frame. */
int  tdnet_warmup(tdnet_t* h, void* stream);
/* HBM held by the weight block (*weights_bytes, shared) and by this handle alone (*handle_bytes: workspace + FIFO).  Returns the
 * number of handles currently sharing the block, <0 on error.                                                             */
int  tdnet_memory_bytes(const tdnet_t* h, size_t* weights_bytes, size_t* handle_bytes);

/* ---- the hot path: replaces model(image, pos_id) (td4_psp18.py:216-229 / td2_psp50.py:146-155) ---------------- */
/* img_nchw_dev [1,3,H,W] -> logits_nchw_dev [1,nclass,H,W].  Mutates the K/Q/V FIFO exactly like
 * buffer_contral (td4_psp18.py:123-134): frames must arrive in order with pos_id = t mod path_num.              */
int  tdnet_forward(tdnet_t* h, const float* img_nchw_dev, int pos_id, float* logits_nchw_dev, void* stream);
/* argmax over classes with first-max tie-break = output.max(1)[1] (test.py:61); labels int32 [H,W].  +/-inf logits included.  Where a
 * pixel's logits hold a NaN the label is NOT the reference's (which names the first NaN): class 0 starts the running maximum and a NaN
 * never replaces it, nor is a NaN in class 0 replaced.  The same rule holds for every label entry below (uint8, colour map, overlay,
 * score, confidence, matte, views, surfaces): they share one comparison.                                                          */
int  tdnet_argmax(tdnet_t* h, const float* logits_nchw_dev, int32_t* labels_dev, void* stream);
/* forward + argmax without materialising the full-resolution logits (labels identical to the two calls above).  */
int  tdnet_forward_labels(tdnet_t* h, const float* img_nchw_dev, int pos_id, int32_t* labels_dev, void* stream);
/* ---- uint8 frames in, uint8 labels out ---------------------------------------------------------------------------
 * What every caller of the fp32 entries does on the host per frame -- cv2.resize to the network size, (x / 255 - mean) / std in float64,
 * HWC -> CHW, fp32 (Testing/dataloader.py:64-71; tdnet_amd/dataloader.py resize_linear_u8 + cityscapesLoader.normalise) -- done by the
 * frame's first kernel instead, BIT-IDENTICALLY: the resize is integer arithmetic on coefficient tables built like the loader builds them,
 * the normalisation a 3 x 256 table evaluated in double and rounded once.  A frame given as bytes computes what the same frame given as the
 * loader's fp32 tensor computes, and takes the same number of launches.
 * tdnet_set_input_u8: configuration (not a frame call: it may synchronise; idempotent for equal arguments).  Frames will arrive as
 * [src_height][src_width][3] bytes; mean / std: 3 doubles each, NULL = {.485, .456, .406} / {.229, .224, .225} (dataloader.py:52-53).
 * Builds the tables on the host and uploads them into memory the handle owns (a tdnet_create_shared handle has its own configuration).
 * Fails on a handle that is not finalized, sizes below 1, a zero or non-finite std, and a column downscale beyond about 20x.           */
int  tdnet_set_input_u8(tdnet_t* h, int src_height, int src_width, const double* mean /* [3] | NULL */, const double* std /* [3] | NULL */);
/* tdnet_forward / tdnet_forward_labels / tdnet_encode with the image as device bytes [src_height][src_width][3], RGB, contiguous, at ANY
 * byte address (no alignment assumed).  Without a prior tdnet_set_input_u8 they fail.  Like the fp32 entries they only enqueue.  fp32 and
 * uint8 entries may be mixed frame by frame on one handle: the FIFO does not care how the image arrived.                                */
int  tdnet_forward_u8(tdnet_t* h, const uint8_t* img_hwc_dev, int pos_id, float* logits_nchw_dev, void* stream);
int  tdnet_forward_u8_labels(tdnet_t* h, const uint8_t* img_hwc_dev, int pos_id, uint8_t* labels_dev /* [H,W] */, void* stream);
/* tdnet_argmax with uint8 labels [H,W] (the same labels, one byte each).                                            */
int  tdnet_argmax_u8(tdnet_t* h, const float* logits_nchw_dev, uint8_t* labels_dev, void* stream);
/* ---- NV12 frames in -------------------------------------------------------------------------------------------------
 * What a video decoder hands over, taken by the frame's first kernel as it is: the colour conversion joins the resize and the normalisation
 * in that ONE launch (no RGB intermediate, no extra launch), BIT-IDENTICALLY to converting on the host and calling the uint8 entries.
 * Surface: one device allocation.  Y plane at `base`: row y starts at base + y * pitch and holds src_width bytes.  UV plane at
 * base + uv_offset: chroma row j starts at base + uv_offset + j * pitch and holds U, V byte pairs -- ceil(src_height / 2) rows of
 * ceil(src_width / 2) pairs.  Odd sizes are legal, `base` may be any byte address.  Nothing outside
 * [base, base + uv_offset + (ceil(src_height / 2) - 1) * pitch + 2 * ceil(src_width / 2)) is read, and the result does not depend on the bytes
 * of the pitch padding or of the gap between the planes.
 * Per source pixel (y, x): Y = Yplane[y][x], (U, V) = UVplane[y >> 1][x >> 1] (chroma replicated, as OpenCV's COLOR_YUV2RGB_NV12), then in int32
 *     yy = max(0, Y - yoff) * CY;  u = U - 128;  v = V - 128
 *     R = clamp8((yy + (1 << 19) + CVR * v) >> 20)
 *     G = clamp8((yy + (1 << 19) + CVG * v + CUG * u) >> 20)
 *     B = clamp8((yy + (1 << 19) + CUB * u) >> 20)
 * with an arithmetic >>, clamp8 to 0..255 and the constants rint(c * 2^20) of the decimal coefficients, computed once on the host
 * (|sum| <= 6.0e8 < 2^31):
 *     standard                  decimals (CY, CUB, CUG, CVG, CVR)              yoff  CY       CUB      CUG      CVG      CVR
 *     0 TDNET_YUV_BT601_LIMITED 1.164, 2.018, -0.391, -0.813, 1.596            16    1220542  2116026  -409993  -852492  1673527   (OpenCV's integers)
 *     1 TDNET_YUV_BT709_LIMITED 1.164, 2.112, -0.213, -0.533, 1.793            16    1220542  2214593  -223347  -558891  1880097
 *     2 TDNET_YUV_BT601_FULL    1, 1.772, -0.344136, -0.714136, 1.402          0     1048576  1858077  -360853  -748826  1470104
 *     3 TDNET_YUV_BT709_FULL    1, 1.8556, -0.187324, -0.468124, 1.5748        0     1048576  1945738  -196423  -490864  1651297
 * The frame is then exactly what tdnet_set_input_u8 defines on those RGB bytes: each of the four taps of the resize is converted and clamped
 * FIRST, then interpolated (never YUV interpolated and converted afterwards), then normalised.
 * tdnet_set_input_nv12: configuration (not a frame call: it may synchronise; idempotent for equal arguments; per handle).  A handle has ONE
 * byte-input configuration at a time: after this call the byte entries (the tdnet_forward_u8* entries and tdnet_encode_u8) read their image
 * pointer as the surface's `base`; a later tdnet_set_input_u8 switches back to packed RGB.  Fails -- leaving the previous configuration in
 * force and the FIFO alone -- on a handle that is not finalized, sizes below 1, pitch < 2 * ceil(src_width / 2),
 * uv_offset < src_height * pitch, an extent of 2^31 bytes or more, a standard outside 0..3, a zero or non-finite std, a non-finite mean, and a
 * column downscale beyond what the kernel stages.                                                                      */
#define TDNET_YUV_BT601_LIMITED 0
#define TDNET_YUV_BT709_LIMITED 1
#define TDNET_YUV_BT601_FULL 2
#define TDNET_YUV_BT709_FULL 3
int  tdnet_set_input_nv12(tdnet_t* h, int src_height, int src_width, int pitch, size_t uv_offset, int standard,
                          const double* mean /* [3] | NULL */, const double* std /* [3] | NULL */);
/* ---- source views -----------------------------------------------------------------------------------------------------
 * What producers really hand over: b g r or 4-byte pixels (cv2, capture APIs), rows with a pitch (image libraries, mapped surfaces), and a frame of
 * another aspect than the network's, of which a rectangle is wanted (a centre crop, a region of interest, a decoder's display rectangle).  A VIEW is a
 * rectangle of a pitched frame in one of five pixel formats; the handle reads it in the frame's first launch (and, for "overlay out", in its last),
 * BIT-IDENTICALLY to cropping and reordering on the host and calling the existing entries, with the same tdnet_last_launch_count.
 *   definition  (h, w) = (crop_height, crop_width) -- all four crop fields 0: the whole frame -- and rgb[y][x] = the R, G, B of frame pixel
 *               (crop_y + y, crop_x + x).  Packed formats: the three colour bytes at base + (crop_y + y) * pitch + (crop_x + x) * bpp, in the order the
 *               format names.  NV12: the conversion of "NV12 frames in" at the frame's ABSOLUTE coordinates, Y = Yplane[crop_y + y][crop_x + x],
 *               (U, V) = UVplane[(crop_y + y) >> 1][(crop_x + x) >> 1] -- an odd origin shifts the chroma phase.  The frame is then exactly what
 *               tdnet_set_input_u8(h, w, mean, std) computes on those contiguous RGB bytes: every resize tap converted first, interpolated afterwards,
 *               the same coefficient tables for h x w -> H x W.
 *   memory      nothing outside [base, base + extent) is read; packed: extent = (height - 1) * pitch + width * bpp, NV12: the extent "NV12 frames in"
 *               defines for the whole frame.  `base` may be any byte address.  The result does not depend on any byte outside the rectangle's pixels
 *               (NV12: outside the chroma pairs covering it): not on pitch padding, the x byte of the 32-bit formats, the plane gap or the rest of
 *               the frame.
 *   overlay     with a view in force "overlay out" writes out [h][w][3], contiguous 3-byte pixels in the SOURCE's colour order -- r g b for RGB24,
 *               RGBA32 and NV12, b g r for BGR24 and BGRA32 (what a cv2 caller displays) -- over the view's pixels; only bytes of the rectangle's
 *               pixels are read (NV12: and their chroma pairs; 32-bit: possibly the pixel's x byte), and out must not overlap the FRAME's extent.
 * tdnet_set_input_view: configuration like its two siblings (not a frame call: it may synchronise; idempotent for equal arguments; per handle; ONE
 * byte-input configuration at a time): afterwards every byte entry (tdnet_forward_u8*, tdnet_encode_u8, tdnet_propagate_overlay,
 * tdnet_labels_overlay) reads its image pointer as the frame's `base`.  tdnet_set_input_u8 / tdnet_set_input_nv12 are the two obvious views.
 * Fails -- leaving the previous configuration in force and the FIFO alone, the message naming the offending field -- on a handle that is not
 * finalized, a NULL view, a format outside 0..4, frame or rectangle sizes below 1, a rectangle not inside the frame, a negative origin, a pitch below
 * a row's bytes, a non-zero reserved, a non-zero standard / uv_offset on a packed format, the NV12 conditions of tdnet_set_input_nv12, an extent of
 * 2^31 bytes or more, a bad mean or std, and a column downscale beyond what the kernel stages (a strip of 256 output columns may span about
 * 10400 source columns of 3 bytes, 7800 of 4 bytes, 15600 of NV12).                                                                     */
#define TDNET_PIX_RGB24  0   /* 3 bytes per pixel: r g b                      */
#define TDNET_PIX_BGR24  1   /* 3 bytes per pixel: b g r                      */
#define TDNET_PIX_RGBA32 2   /* 4 bytes per pixel: r g b x, x is never used   */
#define TDNET_PIX_BGRA32 3   /* 4 bytes per pixel: b g r x                    */
#define TDNET_PIX_NV12   4   /* "NV12 frames in": Y plane + interleaved U,V   */
typedef struct tdnet_view {
    int32_t  format;                 /* TDNET_PIX_*                                                                  */
    int32_t  height, width;          /* the WHOLE frame, in pixels: the extent follows from it                       */
    int32_t  pitch;                  /* bytes per row; 0 = tight (width * bpp; NV12: 2 * ceil(width / 2))           */
    int32_t  crop_y, crop_x, crop_height, crop_width;   /* the rectangle; all four 0 = the whole frame              */
    int32_t  standard;               /* NV12: TDNET_YUV_*; otherwise must be 0                                       */
    int32_t  reserved[5];            /* must be 0                                                                    */
    uint64_t uv_offset;              /* NV12: 0 = height * pitch; otherwise must be 0                                */
} tdnet_view;
int  tdnet_set_input_view(tdnet_t* h, const tdnet_view* v, const double* mean /* [3] | NULL */, const double* std /* [3] | NULL */);
/* ---- surfaces: NV21, I420 / YV12, P010, YUY2, UYVY, and NV12 with a chroma pitch of its own ------------------------------
 * What the other producers hand over: 10-bit hardware decoders (P010), software decoders (I420 / YV12: three planes, a chroma pitch of its own), Android and
 * camera stacks (NV21), webcams and capture cards (YUY2 / UYVY, packed 4:2:2).  A SURFACE is a rectangle of a YUV frame whose planes lie in ONE allocation
 * behind `base`; the handle reads it in the frame's first launch (and, for "overlay out", in its last), BIT-IDENTICALLY to converting on the host and calling
 * the uint8 entries, with the same FIFO step and the same tdnet_last_launch_count.  The contract of "source views"; a struct of its own because tdnet_view
 * has one pitch and one chroma offset.
 *   samples     (Y, X) = a pixel's ABSOLUTE frame coordinates, crop origin + rectangle coordinates (an odd origin shifts the chroma phase).
 *               w16(p) = p[0] | p[1] << 8, read bytewise: `base` may be any byte address, an odd one included, also for P010.
 *                 layout  luma                            U                                                              V
 *                 NV12    base[Y pitch + X]               base[u_offset + (Y >> 1) chroma_pitch + 2 (X >> 1)]            the next byte
 *                 NV21    as NV12                         the byte after V                                               base[u_offset + (Y >> 1) chroma_pitch + 2 (X >> 1)]
 *                 I420    as NV12                         base[u_offset + (Y >> 1) chroma_pitch + (X >> 1)]              base[v_offset + ...], the same index
 *                 P010    w16(base + Y pitch + 2 X) >> 6  w16(base + u_offset + (Y >> 1) chroma_pitch + 4 (X >> 1)) >> 6 the next word >> 6
 *                 YUY2    base[Y pitch + 2 X]             base[Y pitch + 4 (X >> 1) + 1]                                 ... + 3
 *                 UYVY    base[Y pitch + 2 X + 1]         base[Y pitch + 4 (X >> 1)]                                     ... + 2
 *               Row bytes, the lower bounds of the pitches, cw = ceil(width / 2): luma width (P010: 2 width; 4:2:2: 4 cw); chroma 2 cw (I420: cw; P010: 4 cw).
 *   8 bit       exactly the int32 formulas and constants of "NV12 frames in" on that (Y, U, V).
 *   P010        the same five decimals per standard with K = rint(c * 2^18), on the 10-bit samples (the low 6 bits of every word are ignored):
 *                 yy = max(0, Y10 - 4 yoff) * CY + (1 << 19);  u = U10 - 512;  v = V10 - 512
 *                 R = clamp8((yy + CVR v) >> 20);  G = clamp8((yy + CVG v + CUG u) >> 20);  B = clamp8((yy + CUB u) >> 20)
 *               (|sum| <= 5.96e8 < 2^31 over the four standards; BT.709 limited: CY 305136, CUB 553648, CUG -55837, CVG -139723, CVR 470024).  ONE rounding
 *               from 10 bits: the samples are not truncated to 8 bits first.
 *               The frame is then exactly what tdnet_set_input_u8(crop_height, crop_width, mean, std) computes on those RGB bytes: every resize tap converted
 *               and clamped first, then interpolated, then normalised.  "Overlay out" over a surface writes r g b, as for NV12.
 *   memory      extent = the largest end over the planes (last row's start + row bytes).  Nothing outside [base, base + extent) is read, and the result does
 *               not depend on any byte that is not a sample covering the rectangle: not on pitch padding, plane gaps, the other samples of the frame or the
 *               low 6 bits of P010's words.  The overlay entries keep refusing an out that overlaps the extent.
 * tdnet_set_input_surface: the fourth sibling of tdnet_set_input_u8 / tdnet_set_input_nv12 / tdnet_set_input_view (configuration, not a frame call: it may
 * synchronise; idempotent for equal arguments; per handle; ONE byte-input configuration at a time; independent of the order of the other tdnet_set_* calls):
 * afterwards every byte entry reads its image pointer as the surface's `base`.  Its tables are counted in tdnet_memory_bytes.  Fails -- leaving the previous
 * configuration in force and the FIFO alone, the message naming this call and the offending field -- on a handle that is not finalized, a NULL surface, a layout
 * outside 0..5, frame or rectangle sizes below 1, a rectangle not inside the frame, a negative origin, a pitch or chroma_pitch below its row's bytes, a
 * non-zero reserved, a standard outside 0..3, chroma_pitch / u_offset / v_offset non-zero where the struct says 0, planes that overlap each other or the luma
 * plane (in any order: V before U is legal), an extent of 2^31 bytes or more, a bad mean or std, and a column downscale beyond what one strip stages (P010
 * stages twice the bytes of the 8-bit layouts).
 * Surfaces as DESTINATIONS: the mirror, with the contract of "destination views" -- the picture entries' picture pointer is the surface's `base`, the
 * rectangle must be the picture's size (the frame entry checks, naming both), the same picture, FIFO step and tdnet_last_launch_count, entries only enqueue and
 * work inside a hipGraph capture.  Layouts NV12, NV21, I420 and P010; YUY2 / UYVY are refused by name (no encoder takes them).  crop_y and crop_x must be even;
 * h and w may be odd.
 *   8 bit       the forward formulas, constants K = rint(c * 2^20) and chroma averaging (S over the n in {1, 2, 4} pixels of a pair, m = 4 / n) of
 *               "destination views"; the bytes are placed by the table above.
 *   P010        the same K:
 *                 Y10 = clamp10((KYR R + KYG G + KYB B + (yoff << 20) + (1 << 17)) >> 18)
 *                 U10 = clamp10((m (KUR S_R + KUG S_G + KUB S_B) + (128 << 22) + (1 << 19)) >> 20),  V10 likewise with the V row,
 *               each stored as the word value << 6, little-endian, the low bits zero (BT.601 limited white: 940 / 512 / 512; BT.709 limited: 940 / 511 / 512, its U decimals sum to -0.001).  Every sum stays below 2^31.
 *   memory      only the sample bytes of the rectangle are written (its luma samples and the chroma samples covering it); everything else inside and outside
 *               [base, base + extent) keeps its bytes.  The overlay entries refuse a destination extent that overlaps the source extent.
 * tdnet_set_output_surface and tdnet_set_output_view replace each other: ONE destination at a time, NULL to either restores the contiguous [h][w][3] block.
 * Configuration like tdnet_set_output_view (plain host state: nothing is allocated; idempotent; per handle; independent of the order of the other tdnet_set_*
 * calls).  Fails -- leaving the previous destination in force and the FIFO alone, the message naming this call and the offending field -- on the conditions of
 * tdnet_set_input_surface that concern the surface, a YUY2 / UYVY layout, an odd origin, and a rectangle of more than 65535 rows.                        */
#define TDNET_SURF_NV12 0   /* Y plane; U,V byte pairs                                  4:2:0 */
#define TDNET_SURF_NV21 1   /* Y plane; V,U byte pairs                                  4:2:0 */
#define TDNET_SURF_I420 2   /* Y, U, V planes (YV12 = the two chroma offsets exchanged) 4:2:0 */
#define TDNET_SURF_P010 3   /* NV12 in 16-bit little-endian words, the sample in bits 15..6    */
#define TDNET_SURF_YUY2 4   /* one plane, per pixel pair the bytes Y0 U Y1 V            4:2:2 */
#define TDNET_SURF_UYVY 5   /* one plane, per pixel pair the bytes U Y0 V Y1            4:2:2 */
typedef struct tdnet_surface {
    int32_t  layout;                 /* TDNET_SURF_* */
    int32_t  height, width;          /* the WHOLE frame, in pixels */
    int32_t  pitch;                  /* bytes per luma (or packed) row; 0 = tight */
    int32_t  chroma_pitch;           /* bytes per chroma row; 0 = pitch (NV12, NV21, P010), (pitch + 1) / 2 (I420); must be 0 for 4:2:2 */
    int32_t  crop_y, crop_x, crop_height, crop_width;   /* all four 0 = the whole frame */
    int32_t  standard;               /* TDNET_YUV_* */
    int32_t  reserved[4];            /* must be 0 */
    uint64_t u_offset;               /* the interleaved chroma plane, or I420's U plane; 0 = height * pitch; must be 0 for 4:2:2 */
    uint64_t v_offset;               /* I420's V plane; 0 = u_offset + ceil(height / 2) * chroma_pitch; otherwise must be 0 */
} tdnet_surface;
int  tdnet_set_input_surface(tdnet_t* h, const tdnet_surface* s, const double* mean /* [3] | NULL */, const double* std /* [3] | NULL */);
int  tdnet_set_output_surface(tdnet_t* h, const tdnet_surface* s /* NULL = contiguous [h][w][3] */);
/* ---- colour map out ------------------------------------------------------------------------------------------------
 * What the reference's loop does on the host behind the labels (Testing/test.py:61-71): the label map resized with nearest sampling and
 * decode_segmap -- done by the frame's LAST kernel instead.  It evaluates the x8 upsample only at the sampled pixels, takes the first-maximum
 * argmax there and writes the colour: rgb [out_height][out_width][3] uint8 (at any byte address) ==
 * decode_segmap(labels[ys][:, xs]) of the labels the label entries give for the same frame, byte for byte, ys / xs =
 * tdnet_amd/dataloader.py nearest_index(H, out_height) / (W, out_width): min((long)(o * ((double)n / n_out)), n - 1).
 * tdnet_set_output_rgb: configuration (not a frame call: it may synchronise; idempotent for equal arguments).  Any output size >= 1 x 1, smaller
 * than, equal to or larger than the network's.  palette_rgb: [n_colours][3] bytes on the HOST, copied (the library has no colour table of its
 * own); a label >= n_colours comes out grey (l, l, l), as decode_segmap leaves it.  Per handle: a tdnet_create_shared handle configures its own.
 * Fails on a handle that is not finalized, sizes below 1, n_colours outside 1..256 and a NULL palette.                                        */
int  tdnet_set_output_rgb(tdnet_t* h, int out_height, int out_width, const uint8_t* palette_rgb /* [n_colours][3], host */, int n_colours /* 1..256 */);
/* tdnet_forward_labels / tdnet_forward_u8_labels with the picture in place of the label map: the same frame, the same FIFO step, the same number
 * of launches.  Without a prior tdnet_set_output_rgb they fail (and change nothing).  They only enqueue.                                       */
int  tdnet_forward_rgb(tdnet_t* h, const float* img_nchw_dev, int pos_id, uint8_t* rgb_dev, void* stream);
int  tdnet_forward_u8_rgb(tdnet_t* h, const uint8_t* img_hwc_dev, int pos_id, uint8_t* rgb_dev, void* stream);
/* the picture of a uint8 label map [H,W] the caller already holds (tdnet_forward_u8_labels, tdnet_argmax_u8, ...)   */
int  tdnet_labels_rgb(tdnet_t* h, const uint8_t* labels_u8_dev, uint8_t* rgb_dev, void* stream);
/* ---- overlay out --------------------------------------------------------------------------------------------------
 * The picture people look at for video segmentation: the class colours blended over the frame they belong to, at the FRAME's own size, written by
 * the frame's LAST kernel.  Exact, integer:
 *   geometry   out [Hs][Ws][3] uint8 RGB, contiguous, at any byte address; Hs x Ws = the source size of the handle's byte-input configuration in
 *              force (tdnet_set_input_u8 or tdnet_set_input_nv12).  Source pixel (y, x) takes the label of network pixel (ys[y], xs[x]),
 *              ys = nearest_index(H, Hs), xs = nearest_index(W, Ws) -- the rule of "colour map out", i.e. exactly what the colour-map entries sample
 *              for out_height = Hs, out_width = Ws; the label is the first-maximum argmax there, the label the label entries give.
 *   source     s = (sR, sG, sB) of pixel (y, x), read at the source's own resolution (nothing is resized).  Packed RGB: the three bytes at
 *              src[(y * Ws + x) * 3 ..].  NV12: the conversion "NV12 frames in" defines for that pixel -- Y = Yplane[y][x],
 *              (U, V) = UVplane[y >> 1][x >> 1], the 20-bit integer formulas with the configured standard's constants, clamped to 0..255.
 *   colour     palette_rgba [n_colours][4] bytes on the HOST, copied: r, g, b, a.  a = 0 leaves the source pixel untouched, a = 255 replaces it;
 *              the blend weight is A = a + (a >> 7), 0..255 -> 0..256.  A label >= n_colours has A = 0: the source pixel shows through unchanged
 *              (so a reject_label >= n_colours from the confidence entries shows the bare frame).  This differs ON PURPOSE from the colour map's
 *              grey (l, l, l): an overlay has a frame to fall back on, a colour map has not.
 *   blend      per channel, in int32: out = (c * A + s * (256 - A) + 128) >> 8.  At most (255 * 256 + 128) >> 8 = 255: no clamp; A = 0 gives s
 *              and A = 256 gives c, exactly.
 *   memory     nothing outside the source extent is read (packed RGB: [src, src + 3 Hs Ws); NV12: the extent "NV12 frames in" defines), the result
 *              does not depend on pitch padding or on the gap between the planes, nothing outside [out, out + 3 Hs Ws) is written.  out must not
 *              overlap the source extent: the entries check this on the host and fail without enqueueing anything.
 * tdnet_set_output_overlay: configuration (not a frame call: it may synchronise; idempotent for equal arguments; per handle: a tdnet_create_shared
 * handle configures its own).  Independent of the order of the input configuration: it may come before or after it, and a later input configuration
 * with another source size or format takes effect on the next frame (the index tables belong to the pair network size / source size and are rebuilt
 * when either changes).  Its tables are counted in tdnet_memory_bytes.  Fails -- leaving the previous configuration in force -- on a handle that is not
 * finalized, n_colours outside 1..256 and a NULL palette.                                                                                      */
int  tdnet_set_output_overlay(tdnet_t* h, const uint8_t* palette_rgba /* [n_colours][4], host */, int n_colours /* 1..256 */);
/* tdnet_forward_u8_labels with the overlay in place of the label map: img_dev is read by the handle's byte-input configuration (packed RGB, or the
 * surface's base) and is BOTH the frame's image (first launch) and the overlay's source (last launch).  The same frame, the same FIFO step, the same
 * tdnet_last_launch_count.  It only enqueues and works inside a hipGraph capture.  It fails -- changing nothing, a pending encoded frame stays
 * pending -- when the overlay or the byte input is not configured (the message names the missing tdnet_set_* call), on a NULL argument and on
 * overlap.  There is no fp32-image entry: an fp32 tensor has no source bytes to blend over.                                                  */
int  tdnet_forward_u8_overlay(tdnet_t* h, const uint8_t* img_dev, int pos_id, uint8_t* out_dev, void* stream);
/* the unfused form: the overlay of a uint8 label map [H,W] the caller already holds over the source img_dev; after tdnet_forward_u8_labels_conf it is
 * the overlay over the ACCEPTED pixels only (given a reject_label >= n_colours)                                                               */
int  tdnet_labels_overlay(tdnet_t* h, const uint8_t* labels_u8_dev, const uint8_t* img_dev, uint8_t* out_dev, void* stream);
/* ---- destination views --------------------------------------------------------------------------------------------
 * The mirror of "source views": the picture a frame's LAST kernel writes -- the colour map or the overlay -- goes straight into a rectangle of a
 * pitched RGB / BGR / RGBA / BGRA frame or of an NV12 surface, the forms a compositor or an encoder takes, instead of a contiguous [h][w][3] block.
 * While a destination view is in force the picture pointer of EVERY picture entry (tdnet_forward_rgb, tdnet_forward_u8_rgb, tdnet_propagate_rgb,
 * tdnet_labels_rgb, tdnet_forward_u8_overlay, tdnet_propagate_overlay, tdnet_labels_overlay) is the destination frame's `base`, at any byte address.
 * The same picture, the same FIFO step, the same tdnet_last_launch_count; the entries still only enqueue and work inside a hipGraph capture.  Label,
 * logit, score and confidence entries are unaffected.  Let P[y][x] = (R, G, B) be the picture the entry writes without a view, as true r, g, b (an
 * overlay over a b g r source view writes the bytes B, G, R today).  The view's rectangle h x w must be the picture's size -- out_height x out_width
 * for the colour map, the source (rectangle's) size for the overlay: nothing is resized.  The configuration calls are independent of each other's
 * order, so the FRAME entry checks this: on a mismatch it fails without enqueueing, naming both sizes; a pending encoded frame stays pending.
 *   packed     at base + (crop_y + y) * pitch + (crop_x + x) * bpp the three colour bytes in the order the DESTINATION format names (the source's
 *              order no longer decides); the x byte of the 32-bit formats is written as 255.
 *   NV12       crop_y and crop_x must be even (the rectangle starts on the chroma grid); h and w may be odd.  K = rint(c * 2^20) of
 *                standard           yoff   Y: r, g, b            U: r, g, b                  V: r, g, b
 *                0 BT601 limited    16     .257 .504 .098        -.148 -.291 .439            .439 -.368 -.071
 *                1 BT709 limited    16     .183 .614 .062        -.101 -.339 .439            .439 -.399 -.040
 *                2 BT601 full        0     .299 .587 .114        -.168736 -.331264 .5        .5 -.418688 -.081312
 *                3 BT709 full        0     .2126 .7152 .0722     -.114572 -.385428 .5        .5 -.454153 -.045847
 *              in int32 with arithmetic shifts:
 *                Yplane[crop_y + y][crop_x + x] = clamp8((KYR R + KYG G + KYB B + (yoff << 20) + (1 << 19)) >> 20)
 *              and for the chroma pair (j, i) of the FRAME: S = the per-channel sum of P over the rectangle's pixels whose frame coordinates
 *              (Y >> 1, X >> 1) are (j, i), n in {1, 2, 4} their number, m = 4 / n,
 *                U = clamp8((m (KUR S_R + KUG S_G + KUB S_B) + (128 << 22) + (1 << 21)) >> 22),  V likewise with the V row.
 *              Every sum stays below 2^31 in magnitude (m S <= 1020, the positive coefficients of a row sum to <= 0.5).
 *   memory     only the bytes of the rectangle's pixels are written (NV12: its Y bytes and the chroma pairs covering it): pitch padding, the plane
 *              gap, the rest of the frame and everything outside [base, base + extent) keep their bytes.  The destination FRAME's extent must not
 *              overlap the source frame's extent: the overlay entries check this on the host and fail without enqueueing.  In-place compositing is
 *              not supported.
 * tdnet_set_output_view: configuration like its siblings (not a frame call; idempotent for equal arguments; per handle: a tdnet_create_shared handle
 * has its own; independent of the order of the other tdnet_set_* calls).  It allocates nothing: the view travels as kernel arguments, read when an
 * entry enqueues (a captured graph replays the view it was captured with).  v = NULL: contiguous [h][w][3] again, byte for byte.  Fails -- leaving
 * the previous configuration in force and the FIFO alone, the message naming the offending field -- on a handle that is not finalized, a format outside
 * 0..4, frame or rectangle sizes below 1, a rectangle not inside the frame, a negative origin, a pitch below a row's bytes, a non-zero reserved, a
 * non-zero standard / uv_offset on a packed format, the NV12 conditions of tdnet_set_input_nv12 (pitch, uv_offset, standard, extent), an odd NV12
 * origin, and a rectangle of more than 65535 rows.                                                                                            */
int  tdnet_set_output_view(tdnet_t* h, const tdnet_view* v /* NULL = contiguous [h][w][3] */);
/* ---- score out ----------------------------------------------------------------------------------------------------
 * What the reference's validation loop does on the host behind the labels (Training/validate.py:59-70, ptsemseg/metrics.py:12-21): the
 * n_class x n_class confusion matrix, hist[g][l] += 1 over the pixels with 0 <= g < n_class -- counted by the frame's LAST kernel instead, into
 * a matrix of uint64 [nclass][nclass] the handle owns.  g = gt_map[gt[y][x]], gt uint8 [H,W] at the network size on the device (any byte
 * address); g >= nclass means "ignore" (255 is Cityscapes' ignore value).  l is the label the label entries give for the same frame.  Integer
 * counts: exact, independent of the order of the additions.
 * tdnet_set_score: configuration (not a frame call: it may synchronise; idempotent for an equal map).  gt_map: 256 bytes on the HOST, copied,
 * NULL = identity; it lets a caller feed raw dataset ids and have them folded to train ids or to "ignore" on the device (the library carries no
 * dataset table of its own).  Allocates the zeroed matrix; a different map starts a new zeroed matrix.  Per handle: a tdnet_create_shared handle
 * configures and owns its own.  Matrix and map are counted in tdnet_memory_bytes.  Fails on a handle that is not finalized.                     */
int  tdnet_set_score(tdnet_t* h, const uint8_t* gt_map /* [256], host | NULL */);
/* tdnet_forward_labels / tdnet_forward_u8_labels with the other last launch: the frame's counts are ADDED to the handle's matrix, and the uint8
 * label map [H,W] is written too unless labels_u8_dev is NULL.  The same frame, the same FIFO step, the same number of launches (the fused
 * form; DESIGN.md 5.7 says what a measurement would have to show for that to change to "one more").  They only
 * enqueue, and work inside a hipGraph capture (every replay adds its frame).  Without a prior tdnet_set_score they fail naming it and change
 * nothing (a pending encoded frame stays pending).                                                                                         */
int  tdnet_forward_score(tdnet_t* h, const float* img_nchw_dev, int pos_id, const uint8_t* gt_u8_dev, uint8_t* labels_u8_dev /* | NULL */, void* stream);
int  tdnet_forward_u8_score(tdnet_t* h, const uint8_t* img_hwc_dev, int pos_id, const uint8_t* gt_u8_dev, uint8_t* labels_u8_dev /* | NULL */, void* stream);
/* the counts of a uint8 label map [H,W] the caller already holds (the unfused form; a label >= nclass is not counted) */
int  tdnet_labels_score(tdnet_t* h, const uint8_t* labels_u8_dev, const uint8_t* gt_u8_dev, void* stream);
/* enqueued: the matrix set to zero / copied (nclass * nclass uint64) into a caller's DEVICE buffer, e.g. for an all-reduce without a host hop */
int  tdnet_score_reset(tdnet_t* h, void* stream);
int  tdnet_score_export(tdnet_t* h, uint64_t* cm_dev, void* stream);
/* synchronises `stream`, then copies the matrix to the host; returns the element count (nclass * nclass), <0 on error (capacity too small) */
long tdnet_score_read(tdnet_t* h, uint64_t* cm_host, size_t capacity, void* stream);
/* ---- confidence out ------------------------------------------------------------------------------------------------
 * How sure the network is of a pixel's label, from the frame's LAST kernel (every class's upsampled logit passes through its registers
 * anyway) instead of 4 * nclass bytes of fp32 logits per pixel and a softmax pass of the caller's.  For a pixel (Y, X) let v_c be the
 * upsampled fp32 logit of class c -- the label entries' expression (bilinear, align_corners, the coefficients of the uint8 label kernel) --
 * and l the first-maximum argmax, i.e. the label the label entries give.
 *   confidence  p = 1 / sum_c exp(v_c - v_l), evaluated in fp32 with the maximum subtracted (logits of +-300 do not overflow);
 *               conf = (uint8) floor(255 p + 0.5): 255 = certain; nclass = 1 gives 255 everywhere.
 *   layout      uint8 [H][W] at the network size, at any byte address, like the uint8 label map.
 *   rejection   is defined on the BYTE, so it is exact: the label written is conf < min_conf ? reject_label : l.  min_conf = 0 (the default)
 *               rejects nothing: the labels are then the label entries' labels byte for byte, whatever the logits hold.  The confidence
 *               map itself is never altered by rejection.
 *   non-finite logits: the confidence byte is unspecified; the labels with min_conf = 0 still equal the label entries'.
 * tdnet_set_confidence: plain host state of the handle -- no allocation, no synchronisation; per handle (a tdnet_create_shared handle has its
 * own, starting at 0 / 255); fails on values outside 0..255 and then changes nothing.                                                     */
int  tdnet_set_confidence(tdnet_t* h, int min_conf /* 0..255, 0 = reject nothing */, int reject_label /* 0..255 */);
/* tdnet_forward_labels / tdnet_forward_u8_labels with the other last launch: the confidence map is written, and the uint8 label map [H,W]
 * (with the rejection applied) too unless labels_dev is NULL.  The same frame, the same FIFO step, the same tdnet_last_launch_count.  They
 * work without a prior tdnet_set_confidence (min_conf = 0), only enqueue, and work inside a hipGraph capture: threshold and reject label are
 * kernel ARGUMENTS read when the entry enqueues, so a captured graph replays the values in force at capture time, not later ones.  A call
 * rejected by its argument checks changes nothing (a pending encoded frame stays pending).
 * Composition with the unfused entries: a reject_label >= nclass is not counted by tdnet_labels_score, and one >= n_colours comes out grey
 * from tdnet_labels_rgb -- so labels_conf followed by tdnet_labels_score is the confusion matrix over the ACCEPTED pixels.                 */
int  tdnet_forward_labels_conf(tdnet_t* h, const float* img_nchw_dev, int pos_id, uint8_t* labels_dev /* | NULL */, uint8_t* conf_dev, void* stream);
int  tdnet_forward_u8_labels_conf(tdnet_t* h, const uint8_t* img_hwc_dev, int pos_id, uint8_t* labels_dev /* | NULL */, uint8_t* conf_dev, void* stream);
/* the unfused form: labels and confidence of full-resolution NCHW logits [nclass,H,W] the caller already holds (v_c = those logits)      */
int  tdnet_logits_conf(tdnet_t* h, const float* logits_nchw_dev, uint8_t* labels_dev /* | NULL */, uint8_t* conf_dev, void* stream);
/* ---- matte out -----------------------------------------------------------------------------------------------------
 * A SOFT mask of a class set -- "everything that moves" (Cityscapes train ids 11..18) in front of a mapping stage, "person + rider" for a
 * background replacement, "road + sidewalk" as a drivable-area prior -- from the frame's LAST kernel, instead of 4 * nclass bytes of fp32
 * logits per pixel and a softmax, a class sum and a rounding of the caller's.  For a pixel let v_c be the upsampled fp32 logit of class c (the
 * label entries' expression, as in "confidence out"), l the first-maximum argmax and S the configured class set:
 *   matte       den = sum_c exp(v_c - v_l),  num = sum_{c in S} exp(v_c - v_l), in fp32 with the maximum subtracted (logits of +-300 do not
 *               overflow);  matte = (uint8) floor(255 num / den + 0.5).
 *   exact       S = every class gives 255 at every pixel, S = the empty set gives 0 at every pixel, nclass = 1 with S = {0} gives 255: num and
 *               den are accumulated by the same operations in the same order, so with every class a member they are the same float.
 *   labels      the labels written beside the matte are the label entries' labels byte for byte, whatever the logits hold: there is no
 *               rejection here.  For non-finite logits the matte byte is unspecified; the labels are not.
 *   one byte    a pixel's byte does not depend on which lane or which geometry computed it.
 *   layout      uint8 [H][W] at the network size, at any byte address, like the confidence map.
 * tdnet_set_matte: plain host state of the handle -- no allocation, no synchronisation, no finalized weights needed (only cfg.nclass); per handle
 * (a tdnet_create_shared handle has its own, unset at creation).  classes: n class ids on the HOST, duplicates are legal, n = 0 is the empty
 * set.  Fails, changing nothing, on an id >= nclass, on n outside 0..256 and on NULL with n > 0.  The set travels to the kernels as ARGUMENTS
 * (256 membership bits in eight 32-bit words) read when an entry enqueues: a captured hipGraph replays the set of capture time, as it does
 * min_conf.  Nothing of it lives in device memory.                                                                                          */
int  tdnet_set_matte(tdnet_t* h, const uint8_t* classes /* [n], host: class ids */, int n /* 0..256 */);
/* tdnet_forward_labels / tdnet_forward_u8_labels with the other last launch: the matte is written, and the uint8 label map [H,W] too unless
 * labels_dev is NULL.  The same frame, the same FIFO step, the same tdnet_last_launch_count.  They only enqueue and work inside a hipGraph
 * capture.  Without a prior tdnet_set_matte they fail naming it and change nothing (a pending encoded frame stays pending).  Only
 * [matte_dev, matte_dev + H W) is written, and [labels_dev, labels_dev + H W) when labels are given.                                         */
int  tdnet_forward_matte(tdnet_t* h, const float* img_nchw_dev, int pos_id, uint8_t* labels_dev /* | NULL */, uint8_t* matte_dev, void* stream);
int  tdnet_forward_u8_matte(tdnet_t* h, const uint8_t* img_hwc_dev, int pos_id, uint8_t* labels_dev /* | NULL */, uint8_t* matte_dev, void* stream);
/* the unfused form: labels and matte of full-resolution NCHW logits [nclass,H,W] the caller already holds (v_c = those logits)            */
int  tdnet_logits_matte(tdnet_t* h, const float* logits_nchw_dev, uint8_t* labels_dev /* | NULL */, uint8_t* matte_dev, void* stream);
/* The COMPOSITE: the source frame seen through the matte, at the SOURCE's size, written by the frame's last launch.
 *   geometry   that of "overlay out": Hs x Ws = the source (rectangle's) size of the byte-input configuration in force (any of tdnet_set_input_u8 / _nv12 /
 *              _view / _surface); source pixel (y, x) takes the matte byte M of network pixel (ys[y], xs[x]), ys = nearest_index(H, Hs),
 *              xs = nearest_index(W, Ws) -- the very byte the matte entries write for that network pixel; s = the source pixel as "overlay out" /
 *              "source views" / "surfaces" define it.
 *   blend      per channel, in int32, A = M + (M >> 7) (0..255 -> 0..256).
 *   mode 0     TDNET_COMPOSITE_COLOUR: out_c = (s_c A + bg_c (256 - A) + 128) >> 8 -- the overlay's blend with the source as the colour, M as its alpha
 *              and bg underneath.  M = 255 gives s exactly, M = 0 gives bg exactly, nothing needs a clamp.  Into the contiguous [Hs][Ws][3] block, or
 *              with a destination VIEW in force into a rectangle of a pitched RGB / BGR / RGBA / BGRA frame with the x byte 255.
 *   mode 1     TDNET_COMPOSITE_ALPHA: the source pixel's colour bytes UNCHANGED and the x byte of a 32-bit destination view = M; a compositor then
 *              blends over whatever it likes.  Requires an RGBA32 / BGRA32 destination view: the frame entry checks that and fails without
 *              enqueueing, naming the destination it found.
 *   colour     the rules of "overlay out" and "destination views", unchanged: the source's byte order into the contiguous block, the destination's
 *              into a view.  bg_rgb is always true r, g, b.
 *   4:2:0      destinations (tdnet_set_output_surface, or an NV12 view, in force) are refused by name: composite into 4:2:0 is not built.
 *   memory     the overlay's contract: nothing outside the source extent is read, the result does not depend on padding or gaps, only the rectangle's
 *              pixel bytes are written; out (or the destination frame's extent) must not overlap the source extent -- checked on the host before
 *              anything is enqueued.
 * tdnet_set_output_composite: configuration like tdnet_set_output_overlay (it may synchronise; idempotent for equal arguments; per handle; independent of
 * the order of the other tdnet_set_* calls and of tdnet_set_output_overlay: a handle may have both).  It shares the overlay's index tables for the pair
 * network size / source size: rebuilt when either changes, counted once in tdnet_memory_bytes.  Fails, leaving the previous configuration in force, on a
 * handle that is not finalized, a mode outside 0..1, a NULL bg_rgb in mode 0 and a bg_rgb in mode 1.
 * The frame entries are tdnet_forward_u8_labels with the other last launch: the same frame, FIFO step and tdnet_last_launch_count; they only enqueue and
 * work inside a hipGraph capture.  They fail -- changing nothing, a pending encoded frame stays pending, the message naming the missing call or the
 * field -- without tdnet_set_matte, tdnet_set_output_composite or a byte input, on a rectangle that is not the source's size, on the alpha mode without a
 * 32-bit view, on a 4:2:0 destination and on overlap.  There is no fp32-image entry: an fp32 tensor has no source bytes.                       */
#define TDNET_COMPOSITE_COLOUR 0
#define TDNET_COMPOSITE_ALPHA  1
int  tdnet_set_output_composite(tdnet_t* h, int mode, const uint8_t* bg_rgb /* [3], host; mode 0: required, mode 1: must be NULL */);
int  tdnet_forward_u8_composite(tdnet_t* h, const uint8_t* img_dev, int pos_id, uint8_t* out_dev, void* stream);
/* the unfused form: from a matte map [H][W] the caller already holds (any byte address); needs no tdnet_set_matte */
int  tdnet_matte_composite(tdnet_t* h, const uint8_t* matte_u8_dev, const uint8_t* img_dev, uint8_t* out_dev, void* stream);
/* ---- refined matte -------------------------------------------------------------------------------------------------
 * A matte byte is a x8 bilinear upsample of 1/8-resolution logits: its outline is soft and ignores the real edge, which the frame shows.  The standard
 * remedy is He et al.'s guided filter of the matte with the frame's luma as the guide.  It is defined here so that EVERY STEP IS AN INTEGER OPERATION OR ONE
 * CORRECTLY ROUNDED fp32 OPERATION: box sums of integers do not depend on the order of the additions, so the device result does not depend on how the
 * kernels tile the map, and the oracle (tdnet_amd/dataloader.py refine_matte_u8) is matched byte for byte.
 *   inputs      G (guide) and M (matte): uint8 [rows][cols]; radius r in 1..16; eps in 4..65025, an integer in SQUARED BYTE units (65 ~ 1e-3 * 255^2)
 *   window      of pixel (y, x): rows max(0, y - r) .. min(rows - 1, y + r), columns likewise -- the box clipped to the map; N its pixel count, S_x the sum
 *               of x over it
 *   stage 1     cov = N S_GM - S_G S_M;   den = N S_GG - S_G^2 + eps N^2 (> 0);   a = f32(cov) / f32(den);
 *               a_q = clamp(rint(a * 1024.f), -32767, 32767);   b_q = rint(f32(1024 S_M - a_q S_G) / f32(16 N))      -- the slope in Q10, the offset in Q6
 *   stage 2     A = sum a_q, B = sum b_q over the window;   out = clamp8(rint(f32(A G + 16 B) / f32(1024 N)))
 *   arithmetic  f32 is the round-to-nearest-even conversion of the integer, / the IEEE fp32 division, rint rounds halves to even (rintf); the library is
 *               built with -ffp-contract=off
 *   bounds      the box sums fit 32 bits (S_GG, S_GM <= 1089 * 65025); cov, den, 1024 S_M - a_q S_G and A G + 16 B need 64 (N S_GM reaches 7.7e10);
 *               |a_q| <= 32767 fits 16 bits; |b_q| <= 33791 * 255 / 16; |A| <= 3.6e7 and |B| <= 5.9e8 fit 32.  With eps >= 4, |a| <= sigma_M / (2 sqrt(eps)) < 32:
 *               the clamp on a_q is a guard that never binds
 *   exact       a constant matte comes back unchanged for any guide, r and eps (cov = 0, and 1024 N c is representable); an all-255 guide and matte give
 *               255; the result does not depend on the byte address or the pitch of any of the three maps
 *   guide       of a frame: Y = (77 R + 150 G + 29 B + 128) >> 8 of the converted, clamped r g b pixel (dataloader.py luma_u8)
 * tdnet_refine_matte is the operator on maps the caller holds: any size up to 65535 per side and 2^30 - 16 pixels, any byte addresses, rows guide_pitch /
 * matte_pitch / out_pitch >= cols bytes apart (only the pixels' bytes are read or written, never the padding).  It needs no configuration, only enqueues
 * its TDNET_REFINE_OP_LAUNCHES launches (the coefficient planes, then the bytes) and works inside a hipGraph capture; radius and eps travel as kernel
 * arguments read at enqueue, so a captured graph replays those of capture time.  scratch_dev: tdnet_refine_scratch_bytes bytes (6 per pixel), 4-byte aligned,
 * the caller's; its contents afterwards are unspecified.  Checked on the host before anything is enqueued, the message naming the argument: the ranges of
 * radius and eps, the size, pitch >= cols, the scratch's alignment, and that out overlaps neither input nor the scratch and the scratch neither input.
 * THE FRAME ENTRIES refine the frame's matte at the SOURCE's size: the guide is the luma of the source pixel as "overlay out" / "source views" / "surfaces" define it,
 * the matte M_src[y][x] = matte[ys[y]][xs[x]] with the composite's nearest_index tables -- the very byte the composite uses.  The frame's last launch writes both
 * planes into the handle's workspace (in place of the label launch), the operator's two launches follow: TDNET_REFINE_LAUNCHES = 3, and tdnet_last_launch_count
 * = the label entry's + 2.  out_dev: [Hs][Ws] bytes, tight, any byte address, not overlapping the source extent.
 * tdnet_set_matte_refine: radius 0 = off (the default), else radius 1..16 and eps 4..65025.  Configuration: it may allocate and synchronise, is idempotent for
 * equal arguments, per handle, and accepted before or after the byte-input configuration; the workspace follows the source size -- 2 + 6 + 1 bytes per source
 * pixel and two index tables -- and is counted in tdnet_memory_bytes.  A failed call leaves the previous state in force.
 * tdnet_forward_u8_matte_refined / tdnet_propagate_matte_refined (the split frame: the caller passes the source again) need tdnet_set_matte, a byte input and a
 * non-zero radius; otherwise they fail naming the missing call and change nothing (a pending encoded frame stays pending).  They only enqueue.
 * WITH A NON-ZERO RADIUS IN FORCE tdnet_forward_u8_composite, tdnet_propagate_composite and tdnet_matte_composite composite through the refined matte: the three
 * launches, then the existing composite kernel from the refined map -- the label entry's launch count + 3; every rule of "matte out" holds (4:2:0 destinations
 * stay refused).  With radius 0 they are byte for byte and launch for launch what they are without this section.                                     */
#define TDNET_REFINE_MAX_RADIUS 16
#define TDNET_REFINE_MIN_EPS 4
#define TDNET_REFINE_MAX_EPS 65025
#define TDNET_REFINE_OP_LAUNCHES 2
#define TDNET_REFINE_LAUNCHES 3
int  tdnet_set_matte_refine(tdnet_t* h, int radius /* 0: off */, int eps);
int  tdnet_forward_u8_matte_refined(tdnet_t* h, const uint8_t* img_dev, int pos_id, uint8_t* out_dev /* [Hs][Ws] */, void* stream);
int  tdnet_propagate_matte_refined(tdnet_t* h, const uint8_t* img_dev, uint8_t* out_dev /* [Hs][Ws] */, void* stream);
size_t tdnet_refine_scratch_bytes(int rows, int cols);      /* 0 for a size below 1 x 1 */
int  tdnet_refine_matte(tdnet_t* h, const uint8_t* guide_dev, size_t guide_pitch, const uint8_t* matte_dev, size_t matte_pitch, uint8_t* out_dev, size_t out_pitch,
                        int rows, int cols, int radius, int eps, void* scratch_dev, void* stream);
/* ---- regions out ---------------------------------------------------------------------------------------------------
 * What a video pipeline does next with a semantic map is not per pixel: the "thing" classes become objects -- a box, an area and a centroid per blob
 * for a tracker, a counter or an alert.  These entries label the connected components of a class set on the device, behind the frame's labels, instead
 * of a download of the label map and a connected-components pass on a host core.  Let L[Y][X] be the label the label entries give (first-maximum argmax
 * of the upsampled logits, H x W, the network size), S the configured class set, connectivity 4 or 8:
 *   region      a maximal set of pixels with L in S that are pairwise connected through neighbours carrying the SAME label: two adjacent member
 *               classes are two regions.  A label outside S, or >= nclass (a reject_label written by the confidence entries and handed to the unfused
 *               entry), is background.
 *   numbering   a region's key is the raster index Y W + X of its first pixel (its smallest raster index).  Regions with area < min_area are dropped;
 *               the survivors are numbered 1, 2, ... by growing key (the order scipy.ndimage.label gives for one class).  count = the survivors.
 *   id map      optional: int32 [H][W], the region's number, 0 for background and for dropped regions.  Ids run up to count, also beyond max_regions.
 *   table       a device buffer of tdnet_regions_bytes bytes, 8-byte aligned (any other alignment is refused, the message naming regions_dev): a 16-byte
 *               header tdnet_regions_header, then max_regions records tdnet_region of 48 bytes.  stored = min(count, max_regions); record i describes
 *               region i + 1; records from index stored on are zero.  The box is inclusive; first_y / first_x is the first pixel; the centroid is
 *               sum / area (64 bits: 2 Mpx x 2047 does not fit 2^32).  status bit TDNET_REGIONS_OVERFLOW: count > max_regions.  Bit TDNET_REGIONS_BOUND: a
 *               bounded loop of the kernels ran out -- never on a correct build; the table is then not to be trusted.
 *   exact       everything is an integer: the result does not depend on the launch geometry or on the order in which the atomics land.
 * tdnet_set_regions: configuration (it may synchronise; idempotent for equal arguments; per handle).  It allocates the handle's workspace -- three int32
 * [H][W] maps, a byte map and a few words, counted in tdnet_memory_bytes -- once.  classes: n class ids on the HOST (duplicates legal, n = 0: the empty
 * set).  Fails, changing nothing, on a handle that is not finalized, an id >= nclass, n outside 0..256, NULL classes with n > 0, a connectivity other than
 * 4 or 8, max_regions outside 1..65536 and min_area < 1.  The set (256 membership bits), the connectivity and the two limits travel as kernel
 * ARGUMENTS read when an entry enqueues: a captured hipGraph replays those of capture time.
 * The frame entries and the unfused entry only enqueue -- no host synchronisation, no memset or copy calls: every buffer is zeroed by a kernel -- and work
 * inside a hipGraph capture.  The frame entries keep tdnet_forward_u8_labels' FIFO step, and the labels they write (labels_dev may be NULL, ids_dev too)
 * are the label entries' labels byte for byte.  Without a prior tdnet_set_regions they fail naming it and change nothing (a pending encoded frame stays
 * pending).  tdnet_labels_regions, the unfused form on a uint8 label map [H][W] at any byte address, needs no frame state beyond the configuration and
 * enqueues TDNET_REGIONS_LAUNCHES launches; a frame entry's tdnet_last_launch_count is tdnet_forward_u8_labels' - 1 + TDNET_REGIONS_LAUNCHES: the
 * frame's label launch IS the first region launch.  One handle's entries share one workspace: enqueue them on one stream, or order them.             */
#define TDNET_REGIONS_LAUNCHES 7
#define TDNET_REGIONS_OVERFLOW 1u
#define TDNET_REGIONS_BOUND    2u
typedef struct tdnet_regions_header { uint32_t count, stored, status, reserved; } tdnet_regions_header;
typedef struct tdnet_region { int32_t label, area, x0, y0, x1, y1, first_y, first_x; uint64_t sum_x, sum_y; } tdnet_region;
int  tdnet_set_regions(tdnet_t* h, const uint8_t* classes /* [n], host: class ids */, int n /* 0..256 */, int connectivity /* 4 | 8 */,
                       int max_regions /* 1..65536 */, int min_area /* >= 1 */);
size_t tdnet_regions_bytes(const tdnet_t* h);   /* 16 + 48 max_regions; 0 before tdnet_set_regions */
int  tdnet_forward_regions(tdnet_t* h, const float* img_nchw_dev, int pos_id, uint8_t* labels_dev /* | NULL */, int32_t* ids_dev /* | NULL */, void* regions_dev,
                           void* stream);
int  tdnet_forward_u8_regions(tdnet_t* h, const uint8_t* img_dev, int pos_id, uint8_t* labels_dev /* | NULL */, int32_t* ids_dev /* | NULL */, void* regions_dev,
                              void* stream);
int  tdnet_labels_regions(tdnet_t* h, const uint8_t* labels_u8_dev, int32_t* ids_dev /* | NULL */, void* regions_dev, void* stream);
/* ---- tracks out ----------------------------------------------------------------------------------------------------
 * A region's number is the raster rank of its first pixel: it changes whenever anything appears above the object.  A tracker, a counter or an alert
 * needs to know that region 3 of this frame is region 5 of the last one.  These entries are the regions entries plus a match of this frame's regions
 * against those of the previous tracked frame of the handle, by pixel overlap, on the device -- instead of a download of two id maps per frame and a
 * count of their overlaps on a host core.  ids, count, stored and the records are those of "regions out" for the current frame under the regions
 * configuration in force; ids', stored', label'[p], track'[p], age'[p] are those of the previous tracked frame, kept in device memory the handle owns.
 * Only regions that have a record take part: a pixel whose id is 0 or greater than stored is background here, likewise with stored' on the other side.
 *   overlap     n(p, c) = the pixels with ids'[i] == p and ids[i] == c, for 1 <= p <= stored', 1 <= c <= stored and label'[p] == label[c]: a track
 *               keeps its class; pairs of different labels have n = 0.
 *   partners    bp(c) = the p with the largest n(p, c) > 0, ties to the smallest p, 0 if there is none; bc(p) = the c with the largest n(p, c) > 0,
 *               ties to the smallest c, 0 if there is none.
 *   match       c continues p iff bp(c) == p, bc(p) == c and n(p, c) >= min_overlap: track[c] = track'[p], age[c] = age'[p] + 1, prev_region = p,
 *               overlap = n(p, c), origin_track = track[c].
 *   birth       every other c is born: age = 1, prev_region = 0, overlap = 0, origin_track = track'[bp(c)] if bp(c) != 0 (the track it split from or
 *               re-formed out of), else 0.  Born regions take the ids next, next + 1, ... in growing c; next starts at 1 and advances by the number of
 *               births.  A track id is never 0; behaviour after 2^32 - 1 births is unspecified.
 *   first frame after tdnet_set_tracks on a fresh handle, and after tdnet_tracks_reset, stored' = 0: every region is born and next = 1.
 *   memory      ONE frame: a track with no mutual partner ends and is not found again later.  Re-identification (appearance, motion models, occlusion
 *               handling) is out of scope: a caller who needs it builds it on origin_track, the boxes and the centroids.
 *   table       a device buffer of tdnet_tracks_bytes = 16 + 24 max_regions bytes, 8-byte aligned (any other alignment is refused, the message naming
 *               tracks_dev): a header tdnet_tracks_header {count = stored, matched, ended = the previous regions 1..stored' without a match, status},
 *               then max_regions records tdnet_track; record i belongs to region i + 1 of the regions table written by the same call; records from
 *               index stored on are zero.  status bit TDNET_TRACKS_BOUND: a bounded loop of the kernels ran out -- never on a correct build.  There is
 *               no overflow bit: the internal pair table is sized for every pixel carrying a pair of its own.
 *   track map   optional: int32 [H][W], the track id of the pixel's region; 0 for background, for dropped regions and for regions beyond the table.
 *   exact       everything is an integer: the result does not depend on the launch geometry, on where a pair lands in any internal table or on the
 *               order in which atomics arrive.
 * tdnet_set_tracks: configuration, like tdnet_set_regions (it may synchronise; idempotent: a second call changes min_overlap and keeps the tracks; per
 * handle; independent of the order of the other tdnet_set_* calls).  It allocates the state once, sized from the handle alone (H, W and the ceiling of
 * 65536 regions: two int32 [H][W] maps, a pair table of 8-byte slots, the power of two >= 2 H W of them, and 28 bytes per possible region), counted in
 * tdnet_memory_bytes.  A later tdnet_set_regions with other arguments needs no reallocation: it changes what the next frame's ids are, and the match is
 * defined on the two id maps as they are.  min_overlap travels as a kernel ARGUMENT read when an entry enqueues.  Fails, changing nothing, on
 * min_overlap < 1 and on a handle that is not finalized.
 * The frame entries and the unfused entry are the regions entries plus TDNET_TRACKS_LAUNCHES launches: labels, id map and regions table are the same
 * byte for byte, the FIFO step is the same, tdnet_last_launch_count is the regions entry's + TDNET_TRACKS_LAUNCHES.  They only enqueue -- no host
 * synchronisation, no memset or copy calls -- and ALL state between frames (previous ids, labels, tracks, ages, stored', next) lives at fixed device
 * addresses; nothing on the host changes per frame, so a captured hipGraph replays as the eager loop does, and successive replays continue the tracks.
 * They fail -- changing nothing, naming the call and the field, a pending encoded frame stays pending -- without tdnet_set_regions or tdnet_set_tracks
 * (the message names the missing call) and on a NULL or misaligned table.  A regions entry or a label entry between two tracked frames does not touch
 * the track state: the "previous frame" is the previous TRACKED frame.  tdnet_tracks_reset is enqueued on the stream (one launch) and ordered like a
 * frame entry.  tdnet_reset does NOT touch the track state: it has no stream to order the change against.                                       */
#define TDNET_TRACKS_LAUNCHES 4
#define TDNET_TRACKS_BOUND    1u
typedef struct tdnet_tracks_header { uint32_t count, matched, ended, status; } tdnet_tracks_header;
typedef struct tdnet_track { uint32_t track, age, prev_region, overlap, origin_track, reserved; } tdnet_track;
int  tdnet_set_tracks(tdnet_t* h, int min_overlap /* >= 1 */);
size_t tdnet_tracks_bytes(const tdnet_t* h);   /* 16 + 24 max_regions; 0 until both tdnet_set_regions and tdnet_set_tracks */
int  tdnet_forward_tracks(tdnet_t* h, const float* img_nchw_dev, int pos_id, uint8_t* labels_dev /* | NULL */, int32_t* ids_dev /* | NULL */, void* regions_dev,
                          int32_t* track_ids_dev /* | NULL */, void* tracks_dev, void* stream);
int  tdnet_forward_u8_tracks(tdnet_t* h, const uint8_t* img_dev, int pos_id, uint8_t* labels_dev /* | NULL */, int32_t* ids_dev /* | NULL */, void* regions_dev,
                             int32_t* track_ids_dev /* | NULL */, void* tracks_dev, void* stream);
int  tdnet_labels_tracks(tdnet_t* h, const uint8_t* labels_u8_dev, int32_t* ids_dev /* | NULL */, void* regions_dev, int32_t* track_ids_dev /* | NULL */,
                         void* tracks_dev, void* stream);
int  tdnet_tracks_reset(tdnet_t* h, void* stream);   /* enqueued */
/* ---- runs out ------------------------------------------------------------------------------------------------------
 * A semantic map is long horizontal runs of one value, and masks travel between tools as run-length codes.  These entries code a map as a table of runs on
 * the device -- behind the frame's label launch, or from a map the caller holds -- so that a recorder, a sender or a host-side rule engine downloads the
 * table instead of the [H][W] map; tdnet_runs_labels / tdnet_runs_ids turn a table back into a map on a receiving handle.  Let V[Y][X] be a map of the
 * network size H x W -- the uint8 labels the label entries give, or an int32 map: the id map or the track map of the regions / tracks entries -- and
 * i = Y W + X the flat index:
 *   run         a maximal horizontal segment of equal value: pixel i starts a run iff X == 0 or V[i] != V[i - 1].  Runs never cross a row start, also where
 *               the value goes on into the next row.  The runs partition the map; none is filtered.  They are numbered 1, 2, ... by growing start;
 *               count is their number, H <= count <= H W.
 *   table       a device buffer of tdnet_runs_bytes = 16 + 8 (max_runs + 1) bytes, 8-byte aligned (any other alignment is refused, the message naming
 *               runs_dev): a header tdnet_runs_header with stored = min(count, max_runs), then records tdnet_run; record j < stored is run j + 1; record
 *               `stored`, the closing record, is {the start of run stored + 1 if stored < count, else H W; 0}: every stored run ends where the next record
 *               starts.  Records behind the closing one are NOT written: the bytes there stay what they were (a table sized for the worst case costs
 *               no 8 max_runs bytes of stores per frame).  status bit TDNET_RUNS_OVERFLOW: count > max_runs; count is the true count either way.
 *   exact       integers only; the result does not depend on the launch geometry.  The coder uses no atomics: every rank is a prefix sum.
 * tdnet_set_runs: configuration (it may synchronise; idempotent for equal arguments; per handle).  It allocates the workspace -- a byte map for the calls
 * that ask for no labels, and the block counts -- once, counted in tdnet_memory_bytes.  max_runs must be in 1 .. H W; the map may have up to 2^30 - 16
 * pixels (the regions' limit: a flat index fits its word).  It fails, changing nothing, on a handle that is not finalized and on a max_runs out of range.
 * max_runs travels as a kernel ARGUMENT read when an entry enqueues: a captured hipGraph replays capture time's.  tdnet_runs_bytes is 0 before it.
 * The frame entries follow the label entries' rules: the same FIFO step, labels (labels_dev may be NULL) byte for byte those of tdnet_forward_u8_labels.
 * All coding entries only enqueue -- no host synchronisation, no memset or copy calls -- and work inside a hipGraph capture; a pending encoded frame stays
 * pending on any refusal.  A frame entry's tdnet_last_launch_count is the label entry's - 1 + TDNET_RUNS_LAUNCHES: the frame's label launch (unchanged; it
 * does not count starts) is the first runs launch, and count, scan and emit follow it.  tdnet_labels_runs takes a uint8 map at any byte address,
 * tdnet_ids_runs an int32 map, 4-byte aligned, of arbitrary values, negative ones included -- called behind a regions or tracks entry on the same stream;
 * both enqueue TDNET_RUNS_LAUNCHES - 1 launches.  Without a prior tdnet_set_runs every entry fails naming it.
 * Decoding, TDNET_RUNS_DECODE_LAUNCHES launch: the kernel reads `stored` from the device header, clamped to the handle's max_runs.  Pixel i below the
 * closing record's start gets the value of the run that holds it (the uint8 form: its low byte), every other pixel `fill` -- which covers an overflowed
 * table.  The output may sit at any byte address (uint8) or any 4-byte aligned address (int32).  A table the coder did not write gives unspecified values;
 * the kernel still reads nothing outside tdnet_runs_bytes and writes nothing outside the map: its searches are bounded by max_runs, not by the records.
 * One handle's entries share one workspace: enqueue them on one stream, or order them.                                                          */
#define TDNET_RUNS_LAUNCHES 4
#define TDNET_RUNS_DECODE_LAUNCHES 1
#define TDNET_RUNS_OVERFLOW 1u
typedef struct tdnet_runs_header { uint32_t count, stored, status, reserved; } tdnet_runs_header;
typedef struct tdnet_run { uint32_t start; int32_t value; } tdnet_run;
int  tdnet_set_runs(tdnet_t* h, int max_runs /* 1 .. H W */);
size_t tdnet_runs_bytes(const tdnet_t* h);   /* 16 + 8 (max_runs + 1); 0 before tdnet_set_runs */
int  tdnet_forward_runs(tdnet_t* h, const float* img_nchw_dev, int pos_id, uint8_t* labels_dev /* | NULL */, void* runs_dev, void* stream);
int  tdnet_forward_u8_runs(tdnet_t* h, const uint8_t* img_dev, int pos_id, uint8_t* labels_dev /* | NULL */, void* runs_dev, void* stream);
int  tdnet_labels_runs(tdnet_t* h, const uint8_t* labels_u8_dev, void* runs_dev, void* stream);
int  tdnet_ids_runs(tdnet_t* h, const int32_t* ids_i32_dev, void* runs_dev, void* stream);
int  tdnet_runs_labels(tdnet_t* h, const void* runs_dev, int fill, uint8_t* labels_u8_dev, void* stream);
int  tdnet_runs_ids(tdnet_t* h, const void* runs_dev, int fill, int32_t* ids_i32_dev, void* stream);
/* Empties the FIFO (the reference never resets between clips; needed to feed a second clip).  The track state of "tracks out" stays: tdnet_tracks_reset. */
int  tdnet_reset(tdnet_t* h);
int  tdnet_fifo_len(const tdnet_t* h);

/* ---- split frame + cache transport: path-parallel single stream (SURVEY 8e "alternative" / 8f-N4) ----------------
 * tdnet_forward == tdnet_encode followed by tdnet_propagate.  The split exists so that W GPUs can serve ONE video
 * stream, GPU g taking the frames t = g (mod W): the cache entry (q,k,v) a frame contributes to its successors
 * (Encoding pre=True, transformer.py:34-50; pushed by buffer_contral td4_psp18.py:123-134) exists after tdnet_encode,
 * is read out with tdnet_cache_export, travels to the peers (one all-gather per round over xGMI), and is inserted into
 * their FIFOs with tdnet_cache_push in frame order; tdnet_propagate then runs attention propagation + head against
 * the FIFO as it stands and commits the frame's own entry.  All calls are stream-ordered on `stream`.                */
/* backbone + pyramid slice + Encoding of one frame; leaves its cache entry pending (td4_psp18.py:138-140,153).     */
int  tdnet_encode(tdnet_t* h, const float* img_nchw_dev, int pos_id, void* stream);
/* attention propagation + LayerNorm + head + x8 upsample of the pending frame (td4_psp18.py:142-152), then FIFO push */
int  tdnet_propagate(tdnet_t* h, float* logits_nchw_dev, void* stream);
int  tdnet_propagate_labels(tdnet_t* h, int32_t* labels_dev, void* stream);
/* the byte forms (see "uint8 frames in, uint8 labels out")                                                        */
int  tdnet_encode_u8(tdnet_t* h, const uint8_t* img_hwc_dev, int pos_id, void* stream);
int  tdnet_propagate_labels_u8(tdnet_t* h, uint8_t* labels_dev, void* stream);
int  tdnet_propagate_rgb(tdnet_t* h, uint8_t* rgb_dev, void* stream);   /* see "colour map out" */
/* the split frame's overlay: the caller passes the source again (the library does not remember pointers across calls); see "overlay out" */
int  tdnet_propagate_overlay(tdnet_t* h, const uint8_t* img_dev, uint8_t* out_dev, void* stream);
int  tdnet_propagate_score(tdnet_t* h, const uint8_t* gt_u8_dev, uint8_t* labels_u8_dev /* | NULL */, void* stream);   /* see "score out" */
int  tdnet_propagate_labels_conf(tdnet_t* h, uint8_t* labels_dev /* | NULL */, uint8_t* conf_dev, void* stream);   /* see "confidence out" */
int  tdnet_propagate_matte(tdnet_t* h, uint8_t* labels_dev /* | NULL */, uint8_t* matte_dev, void* stream);   /* see "matte out" */
/* the split frame's composite: the caller passes the source again, as for tdnet_propagate_overlay; see "matte out" */
int  tdnet_propagate_composite(tdnet_t* h, const uint8_t* img_dev, uint8_t* out_dev, void* stream);
int  tdnet_propagate_regions(tdnet_t* h, uint8_t* labels_dev /* | NULL */, int32_t* ids_dev /* | NULL */, void* regions_dev, void* stream);   /* see "regions out" */
int  tdnet_propagate_tracks(tdnet_t* h, uint8_t* labels_dev /* | NULL */, int32_t* ids_dev /* | NULL */, void* regions_dev, int32_t* track_ids_dev /* | NULL */,
                            void* tracks_dev, void* stream);   /* see "tracks out" */
int  tdnet_propagate_runs(tdnet_t* h, uint8_t* labels_dev /* | NULL */, void* runs_dev, void* stream);   /* see "runs out" */
/* cache entry geometry: q,k are [Lk,dk], v is [Lk,dv] fp32                                                         */
int  tdnet_cache_dims(const tdnet_t* h, int* Lk, int* dk, int* dv);
/* copy the pending frame's entry into caller-owned device buffers                                                  */
int  tdnet_cache_export(tdnet_t* h, float* q_dev, float* k_dev, float* v_dev, void* stream);
/* append an entry computed by a peer to the FIFO (oldest entry drops out when the FIFO is full)                    */
int  tdnet_cache_push(tdnet_t* h, const float* q_dev, const float* k_dev, const float* v_dev, void* stream);

/* ---- introspection for the parity tests ------------------------------------------------------------------------ */
/* Copies an internal stage buffer of the LAST frame to host, converted to the reference's layout
 * (NCHW for maps, [L,C] for q/k/v).  names: c4 z q_cur v_cur feat ln lowres cache_q cache_k cache_v.
 * Returns the element count, or <0.                                                                              */
long tdnet_get_stage(tdnet_t* h, const char* name, float* host, size_t capacity);
/* Algorithmic FLOP (2*MAC, conv + attention matmuls) of one steady-state frame for this configuration.          */
double tdnet_flops_per_frame(const tdnet_t* h);
/* Device time of the dominant kernel family inside the last tdnet_forward (HIP events on the forward's stream):
 * which: 0 = all conv/GEMM kernels, 1 = attention kernels, 2 = everything else, 3 = the dominant kernel only
 * (fp32: the Winograd GEMMs, or the 128x128-tile 3x3 implicit-GEMM conv when Winograd is off; fp16 mode: the LDS-DMA / 128x128 3x3
 * convs), 4 = EVERY 3x3 conv that reads an fp16 map (fp16 mode: a fixed set of layers, whatever kernel each is routed to).
 * ms, <0 if profiling is off.                                                                                       */
int    tdnet_set_profiling(tdnet_t* h, int on);
double tdnet_last_ms(const tdnet_t* h, int which);
/* same selection: summed algorithmic FLOP / number of launches of that family in the last forward.              */
double tdnet_last_flops(const tdnet_t* h, int which);
double tdnet_last_launches(const tdnet_t* h, int which);
/* Kernel launches the last tdnet_forward* / tdnet_encode / tdnet_propagate* of this handle enqueued (all streams, the final x8 upsample /
 * upsample + argmax kernel included; device copies included: none in a steady-state frame).  Counted in the launch macro itself,
 * profiling on or off.                                                                                              */
int    tdnet_last_launch_count(const tdnet_t* h);

/* Do two HIP streams run on ONE hardware queue (HIP deals streams onto a small pool of queues, GPU_MAX_HW_QUEUES per priority class, and
 * reuses them; kernels of two streams on one queue run one after the other)?  Two 40-us spin kernels started together: *shared = 1 when
 * they serialise.  Synchronises both streams with the host.  The module uses it to place the streams of the samples of a batch
 * (tdnet_amd/model/_base.py); a handle applies the same test to its internal streams at its first frame.                              */
int tdnet_streams_share_queue(void* stream_a, void* stream_b, int* shared);
const char* tdnet_last_error(void);
const char* tdnet_version(void);

#ifdef __cplusplus
}
#endif
#endif
