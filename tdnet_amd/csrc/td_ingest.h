// td_ingest.h -- the byte ends of a frame: uint8 HWC image in (resize + normalisation + the stem's layout in ONE launch, in place of
// k_nchw3_to_rgbpad / k_nchw3_to_nhwc4), uint8 label map out (upsample + argmax, argmax).  Plain C++ on the TD_* macros: compiles unchanged
// under tests/emu/td_device.h.
#pragma once
#include "td_device.h"
#include "td_conv.h"   // td_ld4 / td_st4
#include "td_misc.h"   // UpCoef / td_up_coef

typedef int td_i32x4 __attribute__((ext_vector_type(4)));

// ---- uint8 [Hs][Ws][3] -> the stem's image buffer ----------------------------------------------------------------------------------
// What the host loader computes per frame (tdnet_amd/dataloader.py: resize_linear_u8, then cityscapesLoader.normalise), bit for bit:
//   resize  OpenCV's 11-bit fixed point, all int32: r = p[x0] a0 + p[x1] a1 on source rows y0 and y1 (<= 255 * 2048), then
//           (((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2 clamped to 0..255 (b (r >> 4) <= 2048 * 32640); the coefficient
//           tables are built on the host with _linear_coeffs' operations in _linear_coeffs' types (td_handle.h u8_linear_coeffs).
//           Source and network size equal: the image is taken as it is (resize_linear_u8 returns a copy).
//   normalise  depends on (byte, channel) only: lut[c][v] = (float)((v / 255.0 - mean[c]) / std[c]), evaluated in double on the host.
// grid = (strips of 4 * blockDim.x output columns, H): the row comes from the block index, the vertical coefficients are wave-uniform.
// A workgroup stages the bytes of source rows y0 and y1 its strip reads (columns x0[first] .. x1[last]: the tables are monotone) into LDS
// in 16-byte chunks of the ALIGNED address range around them -- a source row is 3 Ws bytes and starts at any byte (3 * 1537 is odd, sample
// 1 of a batch starts wherever sample 0 ends) -- a chunk that is not wholly inside [src, src + 3 Hs Ws) (the first and the last of the
// image at most) is assembled byte by byte from the bytes that are; nothing outside the image is read.  The 3 KB table sits in LDS too.
// A lane then produces 4 consecutive pixels = 12 floats: three 16-byte stores into the packed-row image out[(y + 3) Wp + x + 4][3]
// (k_nchw3_to_rgbpad's pattern; scalar stores for the last, partial quad of a row whose W % 4 != 0), or four into NHWC4.  Only the interior
// is written: the packed-row image's zero border is written once, when the buffer is allocated.
struct IngestArgs {
    const unsigned char* src;      // [Hs][Ws][3] RGB, any byte alignment
    float* out;
    const float* lut;              // [3][256]
    const int* xt;                 // resize: [4][Wt] = x0 | x1 | a0 | a1 per output column, Wt = W rounded up to 4 (padding = the last column)
    const int* yt;                 // resize: [H][4] = y0, y1, b0, b1
    int Hs, Ws, H, W, Wt;
    int Wp;                        // stem_rows_wp(W): the packed-row image; 0: NHWC4 with a zero 4th channel
    int resize;                    // 0: same size, lookup only
    int span;                      // LDS bytes per staged source row (multiple of 16; td_handle.h u8_plan)
};
constexpr int TD_INGEST_LUT_BYTES = 3 * 256 * 4;

TD_DEV void ingest_stage_row(const IngestArgs& a, unsigned char* dst, size_t first, size_t nbytes) {   // bytes [first, first + nbytes) of the image -> dst + (first & 15)
    const size_t lo = (size_t)a.src, hi = lo + (size_t)a.Hs * a.Ws * 3;
    const size_t g0 = lo + first, al = g0 & ~(size_t)15;
    const int nchunks = (int)((g0 + nbytes - al + 15) >> 4);
    for (int k = threadIdx.x; k < nchunks; k += blockDim.x) {
        const size_t addr = al + (size_t)k * 16;
        if (addr >= lo && addr + 16 <= hi) {
            td_st4(reinterpret_cast<float*>(dst + k * 16), td_ld4(reinterpret_cast<const float*>(addr)));
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const size_t p = addr + b;
                dst[k * 16 + b] = (p >= lo && p < hi) ? *reinterpret_cast<const unsigned char*>(p) : (unsigned char)0;
            }
        }
    }
}

TD_KERNEL void k_ingest_u8(IngestArgs a) {
    TD_DYN_LDS(smem);
    float* lut = reinterpret_cast<float*>(smem);                                   // [3][256]
    unsigned char* row0 = reinterpret_cast<unsigned char*>(smem) + TD_INGEST_LUT_BYTES;   // the staged span of source row y0 ...
    unsigned char* row1 = row0 + a.span;                                           // ... and of y1 (resize only)
    const int y = blockIdx.y, xs = blockIdx.x * blockDim.x * 4;
    const int xe = xs + (int)blockDim.x * 4 < a.W ? xs + (int)blockDim.x * 4 : a.W;   // the strip: output columns [xs, xe)
    for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = a.lut[i];
    int y0 = y, y1 = y, b0 = 0, b1 = 0, cl = xs, ch = xe - 1;                      // source columns [cl, ch]
    if (a.resize) {
        const td_i32x4 t = *reinterpret_cast<const td_i32x4*>(a.yt + 4 * y);
        y0 = t[0]; y1 = t[1]; b0 = t[2]; b1 = t[3];
        cl = a.xt[xs]; ch = a.xt[a.Wt + xe - 1];
    }
    const size_t nbytes = (size_t)(ch - cl + 1) * 3;
    const size_t f0 = ((size_t)y0 * a.Ws + cl) * 3, f1 = ((size_t)y1 * a.Ws + cl) * 3;
    ingest_stage_row(a, row0, f0, nbytes);
    if (a.resize) ingest_stage_row(a, row1, f1, nbytes);
    __syncthreads();
    const int x = xs + (int)threadIdx.x * 4;
    if (x >= a.W) return;
    const int o0 = (int)(((size_t)a.src + f0) & 15) - cl * 3;                      // row0[o0 + 3 * column + c]: the byte of source row y0
    const int o1 = (int)(((size_t)a.src + f1) & 15) - cl * 3;
    float f[12];
    if (a.resize) {
        const td_i32x4 s0 = *reinterpret_cast<const td_i32x4*>(a.xt + x), s1 = *reinterpret_cast<const td_i32x4*>(a.xt + a.Wt + x);
        const td_i32x4 a0 = *reinterpret_cast<const td_i32x4*>(a.xt + 2 * a.Wt + x), a1 = *reinterpret_cast<const td_i32x4*>(a.xt + 3 * a.Wt + x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r0 = (int)row0[o0 + 3 * s0[e] + c] * a0[e] + (int)row0[o0 + 3 * s1[e] + c] * a1[e];
                const int r1 = (int)row1[o1 + 3 * s0[e] + c] * a0[e] + (int)row1[o1 + 3 * s1[e] + c] * a1[e];
                int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                v = v < 0 ? 0 : v > 255 ? 255 : v;
                f[3 * e + c] = lut[c * 256 + v];
            }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) f[3 * e + c] = x + e < a.W ? lut[c * 256 + row0[o0 + 3 * (x + e) + c]] : 0.f;
    }
    if (a.Wp) {
        float* o = a.out + ((size_t)(y + 3) * a.Wp + x + 4) * 3;                   // 16-byte aligned: Wp % 4 == 0, x % 4 == 0
        if (x + 4 <= a.W) {
            const f32x4 v0 = {f[0], f[1], f[2], f[3]}, v1 = {f[4], f[5], f[6], f[7]}, v2 = {f[8], f[9], f[10], f[11]};
            td_st4(o, v0); td_st4(o + 4, v1); td_st4(o + 8, v2);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < a.W) { o[3 * e] = f[3 * e]; o[3 * e + 1] = f[3 * e + 1]; o[3 * e + 2] = f[3 * e + 2]; }
        }
    } else {
        float* o = a.out + ((size_t)y * a.W + x) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x + e < a.W) { const f32x4 v = {f[3 * e], f[3 * e + 1], f[3 * e + 2], 0.f}; td_st4(o + 4 * e, v); }
    }
}

// ---- uint8 labels ------------------------------------------------------------------------------------------------------------------
// A lane's run of a label row of W bytes that starts at `row`: lane 0 the bytes in front of the first 4-byte boundary, lane q >= 1 the
// aligned quad behind it (k_upsample_row's split, in bytes): [xa, xb)
TD_DEV void td_u8_run(const unsigned char* row, long q, long W, long* xa, long* xb) {
    const long X0 = (long)((4u - (unsigned)((size_t)row & 3u)) & 3u);
    *xa = q == 0 ? 0 : X0 + 4 * (q - 1);
    *xb = q == 0 ? (X0 < W ? X0 : W) : (*xa + 4 < W ? *xa + 4 : W);
}
TD_DEV void td_u8_store(unsigned char* row, long q, long xa, long xb, const int* bi) {
    if (q > 0 && xb - xa == 4)
        *reinterpret_cast<unsigned*>(row + xa) = (unsigned)bi[0] | ((unsigned)bi[1] << 8) | ((unsigned)bi[2] << 16) | ((unsigned)bi[3] << 24);
    else
        for (long X = xa; X < xb; ++X) row[X] = (unsigned char)bi[X - xa];
}
// Fused upsample + argmax with uint8 labels [H][W] (nclass <= 256): per pixel k_upsample_argmax's expression and first-maximum rule, so the
// labels are the same numbers; laid out like k_upsample_row: grid = (ceil((W / 4 + 2) / 256), H), row from the block index, vertical
// coefficients wave-uniform, 4 consecutive pixels per lane packed into one 4-byte store where the row address allows (W is odd at 769x1537:
// the rows start at every alignment), scalar head and tail.
TD_KERNEL void k_upsample_argmax_u8(const float* __restrict__ in, unsigned char* __restrict__ labels, int C, int h, int w, int H, int W) {
    const float sy = (H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sx = (W > 1) ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    unsigned char* orow = labels + (size_t)Y * W;
    long xa, xb;
    td_u8_run(orow, q, W, &xa, &xb);
    if (xa >= xb) return;
    const UpCoef cy = td_up_coef(Y, sy, h);
    UpCoef cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cx[e] = td_up_coef((int)(xa + e < W ? xa + e : W - 1), sx, w);
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
        const float* pl = in + (size_t)c * h * w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v00 = pl[cy.i0 * w + cx[e].i0], v01 = pl[cy.i0 * w + cx[e].i1];
            const float v10 = pl[cy.i1 * w + cx[e].i0], v11 = pl[cy.i1 * w + cx[e].i1];
            const float v = (1.f - cy.l) * ((1.f - cx[e].l) * v00 + cx[e].l * v01) + cy.l * ((1.f - cx[e].l) * v10 + cx[e].l * v11);
            if (c == 0 || v > best[e]) { best[e] = v; bi[e] = c; }
        }
    }
    td_u8_store(orow, q, xa, xb, bi);
}
// argmax over classes with uint8 labels: k_argmax's rule (first maximum wins) on 4 consecutive pixels per lane; one 16-byte load per class
// where the planes allow it (HW % 4 == 0, 16-byte aligned logits, 4-byte aligned labels)
TD_KERNEL void k_argmax_u8(const float* __restrict__ logits, unsigned char* __restrict__ labels, int C, long HW) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long pa, pb;
    td_u8_run(labels, q, HW, &pa, &pb);
    if (pa >= pb) return;
    const bool vec = (HW & 3) == 0 && (((size_t)logits) & 15) == 0 && (pa & 3) == 0 && pb - pa == 4;
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
        const float* pl = logits + (size_t)c * HW;
        f32x4 v;
        if (vec) v = td_ld4(pl + pa);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pl[pa + e < HW ? pa + e : HW - 1];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c == 0 || v[e] > best[e]) { best[e] = v[e]; bi[e] = c; }
    }
    td_u8_store(labels, q, pa, pb, bi);
}

// ---- colour map out ----------------------------------------------------------------------------------------------------------------
// What the frame loop does on the host behind the labels (Testing/test.py:61-71; tdnet_amd/test.py save()): the nearest-index sample of the label
// map to [oh][ow] and decode_segmap.  rgb [oh][ow][3] bytes = lut[labels[ys[oy]][xs[ox]]]: ys / xs are dataloader.nearest_index's tables, built on
// the host (td_handle.h rgb_build), lut 256 words r | g << 8 | b << 16 (rows >= n_colours grey (l, l, l), as decode_segmap leaves them).
// A row is 3 ow bytes and starts at any byte address; 4 pixels = 12 bytes = three 4-byte words where row + 3 x is 4-byte aligned, i.e. from
// x = row (mod 4) on (3 x = -row  <=>  x = row (mod 4), 3 being its own inverse).  Lane 0 of a row: the row & 3 pixels in front of the first such
// group; lane q >= 1: the group behind it: [xa, xb)
TD_DEV void td_rgb_run(const unsigned char* row, long q, long ow, long* xa, long* xb) {
    const long X0 = (long)((size_t)row & 3u);
    *xa = q == 0 ? 0 : X0 + 4 * (q - 1);
    *xb = q == 0 ? (X0 < ow ? X0 : ow) : (*xa + 4 < ow ? *xa + 4 : ow);
}
TD_DEV void td_rgb_store(unsigned char* row, long q, long xa, long xb, const unsigned* px) {   // px[e]: the lut word of pixel xa + e
    if (q > 0 && xb - xa == 4) {
        unsigned* o = reinterpret_cast<unsigned*>(row + 3 * xa);
        o[0] = px[0] | (px[1] << 24);
        o[1] = (px[1] >> 8) | (px[2] << 16);
        o[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (long X = xa; X < xb; ++X) {
            const unsigned p = px[X - xa];
            row[3 * X] = (unsigned char)p; row[3 * X + 1] = (unsigned char)(p >> 8); row[3 * X + 2] = (unsigned char)(p >> 16);
        }
    }
}
// The frame's last launch when a picture is asked for: the x8 bilinear upsample evaluated ONLY at the sampled pixels (Y, X) = (ys[oy], xs[ox]) --
// td_up_coef and k_upsample_argmax's expression and first-maximum rule, so the label under every output pixel is the one the label entries
// give -- and the colour looked up.  grid = (ceil((ow / 4 + 2) / 256), oh): row from the block index, Y and the vertical coefficients wave-uniform.
TD_KERNEL void k_upsample_argmax_rgb(const float* __restrict__ in, const int* __restrict__ ys, const int* __restrict__ xs, const unsigned* __restrict__ lut,
                                     unsigned char* __restrict__ rgb, int C, int h, int w, int H, int W, int oh, int ow) {
    const float sy = (H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sx = (W > 1) ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const int q = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    if (oy >= oh) return;
    unsigned char* orow = rgb + (size_t)oy * ow * 3;
    long xa, xb;
    td_rgb_run(orow, q, ow, &xa, &xb);
    if (xa >= xb) return;
    const int Y = ys[oy];
    const UpCoef cy = td_up_coef(Y, sy, h);
    UpCoef cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cx[e] = td_up_coef(xs[xa + e < ow ? xa + e : ow - 1], sx, w);
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
        const float* pl = in + (size_t)c * h * w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v00 = pl[cy.i0 * w + cx[e].i0], v01 = pl[cy.i0 * w + cx[e].i1];
            const float v10 = pl[cy.i1 * w + cx[e].i0], v11 = pl[cy.i1 * w + cx[e].i1];
            const float v = (1.f - cy.l) * ((1.f - cx[e].l) * v00 + cx[e].l * v01) + cy.l * ((1.f - cx[e].l) * v10 + cx[e].l * v11);
            if (c == 0 || v > best[e]) { best[e] = v; bi[e] = c; }
        }
    }
    unsigned px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = lut[bi[e] & 255];
    td_rgb_store(orow, q, xa, xb, px);
}
// The same picture from a uint8 label map [H][W] the caller already holds (same store layout)
TD_KERNEL void k_labels_rgb(const unsigned char* __restrict__ labels, const int* __restrict__ ys, const int* __restrict__ xs, const unsigned* __restrict__ lut,
                            unsigned char* __restrict__ rgb, int W, int oh, int ow) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    if (oy >= oh) return;
    unsigned char* orow = rgb + (size_t)oy * ow * 3;
    long xa, xb;
    td_rgb_run(orow, q, ow, &xa, &xb);
    if (xa >= xb) return;
    const unsigned char* lrow = labels + (size_t)ys[oy] * W;
    unsigned px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = lut[lrow[xs[xa + e < ow ? xa + e : ow - 1]]];
    td_rgb_store(orow, q, xa, xb, px);
}
