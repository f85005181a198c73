// td_ingest.h -- the byte end a frame comes in by: uint8 HWC image in (resize + normalisation + the stem's layout in ONE launch, in place of
// k_nchw3_to_rgbpad / k_nchw3_to_nhwc4).  The byte ends it leaves by are td_out.h's.  Plain C++ on the TD_* macros: compiles unchanged
// under tests/emu/td_device.h.
#pragma once
#include "td_device.h"
#include "td_conv.h"   // td_ld4 / td_st4

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
