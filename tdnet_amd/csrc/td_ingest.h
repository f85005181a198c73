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
// A source VIEW (include/tdnet.h "source views"): the Hs x Ws image is the rectangle at (oy, ox) of a frame whose rows lie `pitch` bytes apart
// and whose pixels are BPP = 3 or 4 bytes (the 4th never indexed), colour bytes in the order r g b or (SWAP) b g r.  A row's staged span starts
// at (oy + y0) pitch + (ox + cl) BPP and holds cols * BPP bytes; taps step by BPP and channel c reads byte c or 2 - c.  [src, src + extent) is
// the WHOLE frame: nothing outside it is read.  The tight RGB image of tdnet_set_input_u8 is the view pitch = 3 Ws, oy = ox = 0.
struct IngestArgs {
    const unsigned char* src;      // the frame's base, any byte alignment
    float* out;
    const float* lut;              // [3][256]
    const int* xt;                 // resize: [4][Wt] = x0 | x1 | a0 | a1 per output column, Wt = W rounded up to 4 (padding = the last column)
    const int* yt;                 // resize: [H][4] = y0, y1, b0, b1
    int Hs, Ws, H, W, Wt;
    int Wp;                        // stem_rows_wp(W): the packed-row image; 0: NHWC4 with a zero 4th channel
    int resize;                    // 0: same size, lookup only
    int span;                      // LDS bytes per staged source row (multiple of 16; td_handle.h u8_build)
    int pitch, oy, ox;             // the view: bytes per frame row, the rectangle's origin
    unsigned extent;               // < 2^31: the bytes of the whole frame
};
constexpr int TD_INGEST_LUT_BYTES = 3 * 256 * 4;

// bytes [first, first + nbytes) behind address lo -> dst + ((lo + first) & 15); [lo, hi) is the extent nothing outside of which is read
TD_DEV void ingest_stage_row(size_t lo, size_t hi, unsigned char* dst, size_t first, size_t nbytes) {
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

template <int BPP, bool SWAP>
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
    const size_t nbytes = (size_t)(ch - cl + 1) * BPP;
    const size_t f0 = (size_t)(a.oy + y0) * a.pitch + (size_t)(a.ox + cl) * BPP, f1 = (size_t)(a.oy + y1) * a.pitch + (size_t)(a.ox + cl) * BPP;
    const size_t lo = (size_t)a.src, hi = lo + a.extent;
    ingest_stage_row(lo, hi, row0, f0, nbytes);
    if (a.resize) ingest_stage_row(lo, hi, row1, f1, nbytes);
    __syncthreads();
    const int x = xs + (int)threadIdx.x * 4;
    if (x >= a.W) return;
    const int o0 = (int)(((size_t)a.src + f0) & 15) - cl * BPP + (SWAP ? 2 : 0);   // row0[o0 + BPP * column + c] (SWAP: - c): the byte of source row y0
    const int o1 = (int)(((size_t)a.src + f1) & 15) - cl * BPP + (SWAP ? 2 : 0);
    constexpr int CS = SWAP ? -1 : 1;
    float f[12];
    if (a.resize) {
        const td_i32x4 s0 = *reinterpret_cast<const td_i32x4*>(a.xt + x), s1 = *reinterpret_cast<const td_i32x4*>(a.xt + a.Wt + x);
        const td_i32x4 a0 = *reinterpret_cast<const td_i32x4*>(a.xt + 2 * a.Wt + x), a1 = *reinterpret_cast<const td_i32x4*>(a.xt + 3 * a.Wt + x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r0 = (int)row0[o0 + BPP * s0[e] + CS * c] * a0[e] + (int)row0[o0 + BPP * s1[e] + CS * c] * a1[e];
                const int r1 = (int)row1[o1 + BPP * s0[e] + CS * c] * a0[e] + (int)row1[o1 + BPP * s1[e] + CS * c] * a1[e];
                int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                v = v < 0 ? 0 : v > 255 ? 255 : v;
                f[3 * e + c] = lut[c * 256 + v];
            }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) f[3 * e + c] = x + e < a.W ? lut[c * 256 + row0[o0 + BPP * (x + e) + CS * c]] : 0.f;
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

// ---- NV12 surface -> the stem's image buffer ---------------------------------------------------------------------------------------
// What a video decoder hands over (include/tdnet.h "NV12 frames in"): a Y plane [Hs] rows of Ws bytes at src, an interleaved U, V plane of
// ceil(Hs / 2) rows of ceil(Ws / 2) byte pairs at src + uv_offset, both with the row pitch `pitch`.  Per source pixel (y, x), all int32:
//   Y = Yplane[y][x], (U, V) = UVplane[y >> 1][x >> 1] (chroma replicated);  yy = max(0, Y - yoff) CY, u = U - 128, v = V - 128
//   R = clamp8((yy + 2^19 + CVR v) >> 20), G = clamp8((yy + 2^19 + CVG v + CUG u) >> 20), B = clamp8((yy + 2^19 + CUB u) >> 20)
// (|sum| <= 6.0e8 < 2^31 for the four coefficient rows of td_handle.h nv12_coeffs), and the frame is what k_ingest_u8 makes of THOSE bytes:
// each of the four taps is converted and clamped first, then resize_linear_u8's fixed point interpolates, then the table normalises.
// The same grid, strip, tables and stores as k_ingest_u8.  A workgroup stages the spans of Y rows y0 and y1 (columns cl .. ch) and of chroma
// rows y0 >> 1 and y1 >> 1 (byte pairs cl >> 1 .. ch >> 1, i.e. from column cl & ~1; once when the two rows coincide -- wave-uniform) with
// ingest_stage_row: nothing outside [src, src + extent) is read, extent = uv_offset + (ceil(Hs / 2) - 1) pitch + 2 ceil(Ws / 2); bytes of the
// pitch padding or of the gap between the planes may land in LDS but no tap indexes them.  The taps are converted in registers (3
// multiply-adds, a shift and a clamp per channel): no second pass over LDS, no second barrier.
// A source view (oy, ox) shifts every address to the frame's absolute coordinates: Y at (oy + y) pitch + ox + column, chroma row (oy + y) >> 1 (the
// `two` test is on those rows), chroma byte (ox + column) & ~1; the staged chroma span runs from (ox + cl) & ~1 to the pair of ox + ch.  An odd
// origin therefore shifts the chroma phase, as cropping the converted picture on the host does.
struct IngestNv12Args {
    const unsigned char* src;      // the surface's base, any byte alignment
    float* out;
    const float* lut;              // [3][256]
    const int* xt;                 // as IngestArgs
    const int* yt;
    int Hs, Ws, H, W, Wt;
    int Wp;                        // as IngestArgs
    int resize;
    int span, span_c;              // LDS bytes per staged Y span / chroma span (multiples of 16; td_handle.h u8_build)
    int pitch;
    unsigned uv_offset, extent;    // < 2^31
    int yoff, cy, cub, cug, cvg, cvr;
    int oy, ox;                    // a source view's origin (0, 0: the whole surface): source pixel (y, x) is frame pixel (oy + y, ox + x)
};
TD_DEV int ingest_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
TD_DEV void ingest_nv12_rgb(const IngestNv12Args& a, int Y, int U, int V, int* p) {
    int yy = Y - a.yoff;
    yy = (yy < 0 ? 0 : yy) * a.cy + (1 << 19);
    const int u = U - 128, v = V - 128;
    p[0] = ingest_clamp8((yy + a.cvr * v) >> 20);
    p[1] = ingest_clamp8((yy + a.cvg * v + a.cug * u) >> 20);
    p[2] = ingest_clamp8((yy + a.cub * u) >> 20);
}

TD_KERNEL void k_ingest_nv12(IngestNv12Args a) {
    TD_DYN_LDS(smem);
    float* lut = reinterpret_cast<float*>(smem);                                   // [3][256]
    unsigned char* yr0 = reinterpret_cast<unsigned char*>(smem) + TD_INGEST_LUT_BYTES;   // the staged span of Y row y0 ...
    unsigned char* yr1 = yr0 + a.span;                                             // ... of y1 (resize only) ...
    unsigned char* uv0 = yr1 + a.span;                                             // ... of chroma row y0 >> 1 ...
    unsigned char* uv1 = uv0 + a.span_c;                                           // ... and of y1 >> 1 where that is another row
    const int y = blockIdx.y, xs = blockIdx.x * blockDim.x * 4;
    const int xe = xs + (int)blockDim.x * 4 < a.W ? xs + (int)blockDim.x * 4 : a.W;   // the strip: output columns [xs, xe)
    for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = a.lut[i];
    int y0 = y, y1 = y, b0 = 0, b1 = 0, cl = xs, ch = xe - 1;                      // source columns [cl, ch]
    if (a.resize) {
        const td_i32x4 t = *reinterpret_cast<const td_i32x4*>(a.yt + 4 * y);
        y0 = t[0]; y1 = t[1]; b0 = t[2]; b1 = t[3];
        cl = a.xt[xs]; ch = a.xt[a.Wt + xe - 1];
    }
    const int g0 = a.oy + y0, g1 = a.oy + y1;                                      // the frame's rows and ...
    const int gl = a.ox + cl, gh = a.ox + ch;                                      // ... columns: chroma goes by THEIR parity
    const int cc = gl & ~1;                                                        // the chroma span's first byte within its row
    const size_t ny = (size_t)(ch - cl + 1), nc = (size_t)((gh >> 1) - (gl >> 1) + 1) * 2;
    const size_t f0 = (size_t)g0 * a.pitch + gl, f1 = (size_t)g1 * a.pitch + gl;
    const size_t c0 = (size_t)a.uv_offset + (size_t)(g0 >> 1) * a.pitch + cc, c1 = (size_t)a.uv_offset + (size_t)(g1 >> 1) * a.pitch + cc;
    const bool two = (g0 >> 1) != (g1 >> 1);                                       // false without resize: y0 == y1
    const size_t lo = (size_t)a.src, hi = lo + a.extent;
    ingest_stage_row(lo, hi, yr0, f0, ny);
    if (a.resize) ingest_stage_row(lo, hi, yr1, f1, ny);
    ingest_stage_row(lo, hi, uv0, c0, nc);
    if (two) ingest_stage_row(lo, hi, uv1, c1, nc);
    __syncthreads();
    const int x = xs + (int)threadIdx.x * 4;
    if (x >= a.W) return;
    const int o0 = (int)((lo + f0) & 15) - cl, o1 = (int)((lo + f1) & 15) - cl;    // yr0[o0 + column]: the Y byte of source row y0
    const int q0 = (int)((lo + c0) & 15) - cc;                                     // uv0[q0 + ((ox + column) & ~1)]: its U, the next byte its V
    const unsigned char* uvb = two ? uv1 : uv0;                                    // the chroma row of source row y1
    const int q1 = two ? (int)((lo + c1) & 15) - cc : q0;
    float f[12];
    if (a.resize) {
        const td_i32x4 s0 = *reinterpret_cast<const td_i32x4*>(a.xt + x), s1 = *reinterpret_cast<const td_i32x4*>(a.xt + a.Wt + x);
        const td_i32x4 a0 = *reinterpret_cast<const td_i32x4*>(a.xt + 2 * a.Wt + x), a1 = *reinterpret_cast<const td_i32x4*>(a.xt + 3 * a.Wt + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ca = (a.ox + s0[e]) & ~1, cb = (a.ox + s1[e]) & ~1;
            int p00[3], p01[3], p10[3], p11[3];                                    // the four taps, converted and clamped
            ingest_nv12_rgb(a, yr0[o0 + s0[e]], uv0[q0 + ca], uv0[q0 + ca + 1], p00);
            ingest_nv12_rgb(a, yr0[o0 + s1[e]], uv0[q0 + cb], uv0[q0 + cb + 1], p01);
            ingest_nv12_rgb(a, yr1[o1 + s0[e]], uvb[q1 + ca], uvb[q1 + ca + 1], p10);
            ingest_nv12_rgb(a, yr1[o1 + s1[e]], uvb[q1 + cb], uvb[q1 + cb + 1], p11);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r0 = p00[c] * a0[e] + p01[c] * a1[e];
                const int r1 = p10[c] * a0[e] + p11[c] * a1[e];
                const int v = ingest_clamp8((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
                f[3 * e + c] = lut[c * 256 + v];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int p[3] = {0, 0, 0};
            const bool in = x + e < a.W;
            if (in) { const int cx = (a.ox + x + e) & ~1; ingest_nv12_rgb(a, yr0[o0 + x + e], uv0[q0 + cx], uv0[q0 + cx + 1], p); }
#pragma unroll
            for (int c = 0; c < 3; ++c) f[3 * e + c] = in ? lut[c * 256 + p[c]] : 0.f;
        }
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

// ---- YUV surfaces -> the stem's image buffer ---------------------------------------------------------------------------------------
// What decoders and capture devices hand over beside NV12 (include/tdnet.h "surfaces"): NV12 with a chroma pitch of its own, NV21, I420 / YV12,
// P010, YUY2, UYVY.  The layout is a handful of wave-uniform ARGUMENTS, not an instantiation; only the sample width is a template parameter.  For
// frame pixel (Y, X) -- absolute coordinates: origin + rectangle coordinates --
//   luma   base[Y pitch + lstride X + loff]
//   U      base[u_off + (Y >> cshift) cpitch + cstep (X >> 1) + uo]        V      base[v_off + (Y >> cshift) cpitch + cstep (X >> 1) + vo]
// and a 16-bit sample is the little-endian word at that address, read bytewise, >> 6:
//   layout   lstride loff  cshift cstep  uo vo   u_off / v_off
//   NV12     1       0     1      2      0  1    the chroma plane, twice
//   NV21     1       0     1      2      1  0    the chroma plane, twice
//   I420     1       0     1      1      0  0    the U plane / the V plane
//   P010     2       0     1      4      0  2    the chroma plane, twice                (WIDE)
//   YUY2     2       0     0      4      1  3    0 / 0: the chroma lies in the luma row (cpitch = pitch)
//   UYVY     2       1     0      4      0  2    0 / 0
// Conversion: ingest_nv12_rgb's formulas with the sample's mid-point and luma offset as arguments (8 bit: 128, yoff, K = rint(c 2^20); P010: 512,
// 4 yoff, K = rint(c 2^18): one rounding from 10 bits, |sum| <= 5.96e8 < 2^31).
// k_ingest_nv12's grid, strip, tables and stores.  A workgroup stages with ingest_stage_row, per source row y0 / y1: the luma span (4:2:2: widened to
// whole pixel pairs, so that the row's chroma is in it), and -- 4:2:0 only -- the span of the chroma row (I420: one of the U and one of the V
// plane), the second row's only where it is another chroma row.  One barrier; the taps are assembled and converted in registers.
struct SurfLayout {
    int pitch, cpitch;             // bytes per luma (or packed) row / per chroma row
    unsigned u_off, v_off;         // < 2^31
    int lstride, loff, cshift, cstep, uo, vo;
    int planes;                    // chroma spans staged per source row: 0 (4:2:2), 1 (interleaved), 2 (I420)
    int yoff, mid, cy, cub, cug, cvg, cvr;
    int oy, ox;                    // the rectangle's origin
};
struct IngestSurfArgs {
    const unsigned char* src;      // the surface's base, any byte alignment
    float* out;
    const float* lut;              // [3][256]
    const int* xt;                 // as IngestArgs
    const int* yt;
    int Hs, Ws, H, W, Wt;
    int Wp;                        // as IngestArgs
    int resize;
    int span, span_c;              // LDS bytes per staged luma span / chroma span (multiples of 16; td_handle.h u8_build)
    unsigned extent;               // < 2^31
    SurfLayout l;
};
TD_DEV void ingest_surf_rgb(const SurfLayout& l, int Y, int U, int V, int* p) {
    int yy = Y - l.yoff;
    yy = (yy < 0 ? 0 : yy) * l.cy + (1 << 19);
    const int u = U - l.mid, v = V - l.mid;
    p[0] = ingest_clamp8((yy + l.cvr * v) >> 20);
    p[1] = ingest_clamp8((yy + l.cvg * v + l.cug * u) >> 20);
    p[2] = ingest_clamp8((yy + l.cub * u) >> 20);
}
// the sample at p: a byte, or the 10 bits in bits 15..6 of the little-endian word there (p at any byte address)
template <bool WIDE>
TD_DEV int surf_sample(const unsigned char* p) { return WIDE ? (int)(((unsigned)p[0] | ((unsigned)p[1] << 8)) >> 6) : (int)p[0]; }
// frame column gx of a staged source row: sm + lp, + up, + vp are where column 0's luma sample / pair 0's U / V would lie in LDS (offsets, possibly
// negative: only columns of the staged span are asked for)
template <bool WIDE>
TD_DEV void ingest_surf_tap(const SurfLayout& l, const unsigned char* sm, int lp, int up, int vp, int gx, int* p) {
    const int c = l.cstep * (gx >> 1);
    ingest_surf_rgb(l, surf_sample<WIDE>(sm + lp + l.lstride * gx), surf_sample<WIDE>(sm + up + c), surf_sample<WIDE>(sm + vp + c), p);
}

template <bool WIDE>
TD_KERNEL void k_ingest_surface(IngestSurfArgs a) {
    TD_DYN_LDS(smem);
    const SurfLayout& l = a.l;
    float* lut = reinterpret_cast<float*>(smem);                                   // [3][256]
    unsigned char* yr0 = reinterpret_cast<unsigned char*>(smem) + TD_INGEST_LUT_BYTES;   // the staged luma span of source row y0 ...
    unsigned char* yr1 = yr0 + a.span;                                             // ... of y1 (resize only) ...
    unsigned char* cs = yr1 + a.span;                                              // ... and the chroma spans: [row][planes] of span_c bytes
    const int y = blockIdx.y, xs = blockIdx.x * blockDim.x * 4;
    const int xe = xs + (int)blockDim.x * 4 < a.W ? xs + (int)blockDim.x * 4 : a.W;   // the strip: output columns [xs, xe)
    for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = a.lut[i];
    int y0 = y, y1 = y, b0 = 0, b1 = 0, cl = xs, ch = xe - 1;                      // source columns [cl, ch]
    if (a.resize) {
        const td_i32x4 t = *reinterpret_cast<const td_i32x4*>(a.yt + 4 * y);
        y0 = t[0]; y1 = t[1]; b0 = t[2]; b1 = t[3];
        cl = a.xt[xs]; ch = a.xt[a.Wt + xe - 1];
    }
    const int g0 = l.oy + y0, g1 = l.oy + y1;                                      // the frame's rows and ...
    const int gl = l.ox + cl, gh = l.ox + ch;                                      // ... columns: chroma goes by THEIR parity
    const int npair = (gh >> 1) - (gl >> 1) + 1;
    const int lb = l.planes ? l.lstride * gl : 4 * (gl >> 1);                       // the luma span's first byte within its row (4:2:2: the pair's)
    const size_t ny = l.planes ? (size_t)l.lstride * (size_t)(ch - cl + 1) : (size_t)4 * npair;
    const int cb = l.cstep * (gl >> 1);                                            // the chroma span's first byte within its row
    const size_t nc = (size_t)l.cstep * npair;
    const size_t f0 = (size_t)g0 * l.pitch + lb, f1 = (size_t)g1 * l.pitch + lb;
    const size_t cu0 = (size_t)l.u_off + (size_t)(g0 >> 1) * l.cpitch + cb, cu1 = (size_t)l.u_off + (size_t)(g1 >> 1) * l.cpitch + cb;
    const size_t cv0 = (size_t)l.v_off + (size_t)(g0 >> 1) * l.cpitch + cb, cv1 = (size_t)l.v_off + (size_t)(g1 >> 1) * l.cpitch + cb;
    const bool two = (g0 >> 1) != (g1 >> 1);                                       // false without resize: y0 == y1
    const size_t lo = (size_t)a.src, hi = lo + a.extent;
    ingest_stage_row(lo, hi, yr0, f0, ny);
    if (a.resize) ingest_stage_row(lo, hi, yr1, f1, ny);
    if (l.planes) {                                                                // wave-uniform
        ingest_stage_row(lo, hi, cs, cu0, nc);
        if (l.planes == 2) ingest_stage_row(lo, hi, cs + a.span_c, cv0, nc);
        if (two) {
            ingest_stage_row(lo, hi, cs + l.planes * a.span_c, cu1, nc);
            if (l.planes == 2) ingest_stage_row(lo, hi, cs + 3 * a.span_c, cv1, nc);
        }
    }
    __syncthreads();
    const int x = xs + (int)threadIdx.x * 4;
    if (x >= a.W) return;
    const unsigned char* sm = reinterpret_cast<const unsigned char*>(smem);
    const int q0 = TD_INGEST_LUT_BYTES, q1 = q0 + a.span, qc = q1 + a.span;        // LDS offsets of yr0, yr1, cs
    const int lp0 = q0 + (int)((lo + f0) & 15) - lb + l.loff;                      // sm[lp0 + lstride * column]: the luma sample of frame column `column`, row y0
    const int lp1 = q1 + (int)((lo + f1) & 15) - lb + l.loff;
    int up0, vp0, up1, vp1;                                                        // sm[up0 + cstep * pair]: the U sample of that pair, row y0; ...
    if (l.planes == 0) {                                                           // 4:2:2: in the luma row
        up0 = lp0 - l.loff + l.uo; vp0 = lp0 - l.loff + l.vo;
        up1 = lp1 - l.loff + l.uo; vp1 = lp1 - l.loff + l.vo;
    } else {
        up0 = qc + (int)((lo + cu0) & 15) - cb + l.uo;
        vp0 = l.planes == 2 ? qc + a.span_c + (int)((lo + cv0) & 15) - cb : up0 - l.uo + l.vo;
        up1 = two ? qc + l.planes * a.span_c + (int)((lo + cu1) & 15) - cb + l.uo : up0;
        vp1 = !two ? vp0 : l.planes == 2 ? qc + 3 * a.span_c + (int)((lo + cv1) & 15) - cb : up1 - l.uo + l.vo;
    }
    float f[12];
    if (a.resize) {
        const td_i32x4 s0 = *reinterpret_cast<const td_i32x4*>(a.xt + x), s1 = *reinterpret_cast<const td_i32x4*>(a.xt + a.Wt + x);
        const td_i32x4 a0 = *reinterpret_cast<const td_i32x4*>(a.xt + 2 * a.Wt + x), a1 = *reinterpret_cast<const td_i32x4*>(a.xt + 3 * a.Wt + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int p00[3], p01[3], p10[3], p11[3];                                    // the four taps, converted and clamped
            ingest_surf_tap<WIDE>(l, sm, lp0, up0, vp0, l.ox + s0[e], p00);
            ingest_surf_tap<WIDE>(l, sm, lp0, up0, vp0, l.ox + s1[e], p01);
            ingest_surf_tap<WIDE>(l, sm, lp1, up1, vp1, l.ox + s0[e], p10);
            ingest_surf_tap<WIDE>(l, sm, lp1, up1, vp1, l.ox + s1[e], p11);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r0 = p00[c] * a0[e] + p01[c] * a1[e];
                const int r1 = p10[c] * a0[e] + p11[c] * a1[e];
                const int v = ingest_clamp8((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
                f[3 * e + c] = lut[c * 256 + v];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int p[3] = {0, 0, 0};
            const bool in = x + e < a.W;
            if (in) ingest_surf_tap<WIDE>(l, sm, lp0, up0, vp0, l.ox + x + e, p);
#pragma unroll
            for (int c = 0; c < 3; ++c) f[3 * e + c] = in ? lut[c * 256 + p[c]] : 0.f;
        }
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
