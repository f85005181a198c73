// td_ingest.h -- the byte end a frame comes in by: a uint8 frame in (resize + normalisation + the stem's layout in ONE launch, in place of
// k_nchw3_to_rgbpad / k_nchw3_to_nhwc4).  The byte ends it leaves by are td_out.h's.  Plain C++ on the TD_* macros: compiles unchanged
// under tests/emu/td_device.h.
#pragma once
#include "td_device.h"
#include "td_conv.h"   // td_ld4 / td_st4

typedef int td_i32x4 __attribute__((ext_vector_type(4)));

// ---- a byte frame -> the stem's image buffer ---------------------------------------------------------------------------------------
// What the host loader computes per frame (tdnet_amd/dataloader.py: resize_linear_u8, then cityscapesLoader.normalise), bit for bit:
//   resize  OpenCV's 11-bit fixed point, all int32: r = p[x0] a0 + p[x1] a1 on source rows y0 and y1 (<= 255 * 2048), then
//           (((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2 clamped to 0..255 (b (r >> 4) <= 2048 * 32640); the coefficient
//           tables are built on the host with _linear_coeffs' operations in _linear_coeffs' types (td_handle.h u8_linear_coeffs).
//           Source and network size equal: the image is taken as it is (resize_linear_u8 returns a copy).
//   normalise  depends on (byte, channel) only: lut[c][v] = (float)((v / 255.0 - mean[c]) / std[c]), evaluated in double on the host.
// ONE kernel body, k_ingest<Reader>: the strip prologue, the interpolation and the store tail are the same for every source; a Reader (below:
// IngestPacked, IngestYuv) says what a workgroup stages per source row and how a tap -- (row y0 | y1, column) -- becomes (R, G, B).
// grid = (strips of 4 * blockDim.x output columns, H): the row comes from the block index, the vertical coefficients are wave-uniform.
// A workgroup stages the bytes of source rows y0 and y1 its strip reads (columns x0[first] .. x1[last]: the tables are monotone) into LDS
// in 16-byte chunks of the ALIGNED address range around them -- a source row starts at any byte (3 * 1537 is odd, sample 1 of a batch starts
// wherever sample 0 ends) -- a chunk that is not wholly inside [src, src + extent) (the first and the last of the frame at most) is assembled
// byte by byte from the bytes that are; nothing outside the frame is read.  The 3 KB table sits in LDS too.  One barrier; the taps are
// assembled and, for YUV, converted in registers.
// A lane then produces 4 consecutive pixels = 12 floats: three 16-byte stores into the packed-row image out[(y + 3) Wp + x + 4][3]
// (k_nchw3_to_rgbpad's pattern; scalar stores for the last, partial quad of a row whose W % 4 != 0), or four into NHWC4.  Only the interior
// is written: the packed-row image's zero border is written once, when the buffer is allocated.
struct IngestArgs {                // what every reader's kernel takes; the source's own description (SrcLayout) goes behind it
    const unsigned char* src;      // the frame's base, any byte alignment
    float* out;
    const float* lut;              // [3][256]
    const int* xt;                 // resize: [4][Wt] = x0 | x1 | a0 | a1 per output column, Wt = W rounded up to 4 (padding = the last column)
    const int* yt;                 // resize: [H][4] = y0, y1, b0, b1
    int Hs, Ws, H, W, Wt;
    int Wp;                        // stem_rows_wp(W): the packed-row image; 0: NHWC4 with a zero 4th channel
    int resize;                    // 0: same size, lookup only
    int span, span_c;              // LDS bytes per staged source row (luma span) / per staged chroma span (multiples of 16; td_handle.h u8_build)
    unsigned extent;               // < 2^31: the bytes of the whole frame
};
constexpr int TD_INGEST_LUT_BYTES = 3 * 256 * 4;

// ---- the source frame as the kernels see it (these and td_out.h's overlay readers) -------------------------------------------------
// Packed pixels (include/tdnet.h "source views"): the Hs x Ws image is the rectangle at (oy, ox) of a frame whose rows lie `pitch` bytes apart and
// whose pixels are BPP = 3 or 4 bytes (the 4th never indexed), colour bytes in the order r g b or (SWAP) b g r.  The tight RGB image of
// tdnet_set_input_u8 is the view pitch = 3 Ws, oy = ox = 0.  Only pitch, oy, ox are read.
// YUV (include/tdnet.h "NV12 frames in", "surfaces"): NV12, NV12 with a chroma pitch of its own, NV21, I420 / YV12, P010, YUY2, UYVY.  For frame
// pixel (Y, X) -- absolute coordinates: origin + rectangle coordinates, so an odd origin shifts the chroma phase, as cropping the converted picture
// on the host does --
//   luma   base[Y pitch + lstride X + loff]
//   U      base[u_off + (Y >> cshift) cpitch + cstep (X >> 1) + uo]        V      base[v_off + (Y >> cshift) cpitch + cstep (X >> 1) + vo]
// and a 16-bit sample is the little-endian word at that address, read bytewise, >> 6:
//   layout   lstride loff  cshift cstep  uo vo  planes   u_off / v_off
//   NV12     1       0     1      2      0  1   1        the chroma plane, twice
//   NV21     1       0     1      2      1  0   1        the chroma plane, twice
//   I420     1       0     1      1      0  0   2        the U plane / the V plane
//   P010     2       0     1      4      0  2   1        the chroma plane, twice                (WIDE)
//   YUY2     2       0     0      4      1  3   0        0 / 0: the chroma lies in the luma row (cpitch = pitch)
//   UYVY     2       1     0      4      0  2   0        0 / 0
// Conversion, per source pixel, all int32:  yy = max(0, Y - yoff) CY, u = U - mid, v = V - mid
//   R = clamp8((yy + 2^19 + CVR v) >> 20), G = clamp8((yy + 2^19 + CVG v + CUG u) >> 20), B = clamp8((yy + 2^19 + CUB u) >> 20)
// (8 bit: mid 128, K = rint(c 2^20), |sum| <= 6.0e8 < 2^31 for the four coefficient rows of td_handle.h nv12_coeffs; P010: mid 512, 4 yoff,
// K = rint(c 2^18): one rounding from 10 bits, |sum| <= 5.96e8), and the frame is what the packed reader makes of THOSE bytes: each of the four
// taps is converted and clamped first, then resize_linear_u8's fixed point interpolates, then the table normalises.
struct SrcLayout {
    int pitch, cpitch;             // bytes per luma (or packed) row / per chroma row
    unsigned u_off, v_off;         // < 2^31
    int lstride, loff, cshift, cstep, uo, vo;
    int planes;                    // chroma spans staged per source row: 0 (4:2:2), 1 (interleaved), 2 (I420)
    int yoff, mid, cy, cub, cug, cvg, cvr;
    int oy, ox;                    // the rectangle's origin
};
// A FORM says where a layout's numbers come from.  YuvFormArgs: the kernel's arguments -- the layout is a handful of wave-uniform values, not an
// instantiation.  YuvFormNv12: the NV12 row of the table as constants, with both planes on the luma pitch (cpitch = pitch, u_off = v_off = the chroma
// plane's offset): what tdnet_set_input_nv12 and an NV12 view describe compiles to what it was before the other layouts came.  L: SrcLayout, or a
// destination of the same field names (td_out.h PicDst).  luma_bytes: the luma samples of four consecutive columns are four consecutive bytes.
struct YuvFormArgs {
    static constexpr bool luma_bytes = false;
    template <class L> TD_DEV_MEMBER int lstride(const L& l) { return l.lstride; }
    template <class L> TD_DEV_MEMBER int loff(const L& l) { return l.loff; }
    template <class L> TD_DEV_MEMBER int cshift(const L& l) { return l.cshift; }
    template <class L> TD_DEV_MEMBER int cstep(const L& l) { return l.cstep; }
    template <class L> TD_DEV_MEMBER int uo(const L& l) { return l.uo; }
    template <class L> TD_DEV_MEMBER int vo(const L& l) { return l.vo; }
    template <class L> TD_DEV_MEMBER int planes(const L& l) { return l.planes; }
    template <class L> TD_DEV_MEMBER int mid(const L& l) { return l.mid; }
    template <class L> TD_DEV_MEMBER int cpitch(const L& l) { return l.cpitch; }
    template <class L> TD_DEV_MEMBER unsigned u_off(const L& l) { return l.u_off; }
    template <class L> TD_DEV_MEMBER unsigned v_off(const L& l) { return l.v_off; }
};
struct YuvFormNv12 {
    static constexpr bool luma_bytes = true;
    template <class L> TD_DEV_MEMBER int lstride(const L&) { return 1; }
    template <class L> TD_DEV_MEMBER int loff(const L&) { return 0; }
    template <class L> TD_DEV_MEMBER int cshift(const L&) { return 1; }
    template <class L> TD_DEV_MEMBER int cstep(const L&) { return 2; }
    template <class L> TD_DEV_MEMBER int uo(const L&) { return 0; }
    template <class L> TD_DEV_MEMBER int vo(const L&) { return 1; }
    template <class L> TD_DEV_MEMBER int planes(const L&) { return 1; }
    template <class L> TD_DEV_MEMBER int mid(const L&) { return 128; }
    template <class L> TD_DEV_MEMBER int cpitch(const L& l) { return l.pitch; }
    template <class L> TD_DEV_MEMBER unsigned u_off(const L& l) { return l.u_off; }
    template <class L> TD_DEV_MEMBER unsigned v_off(const L& l) { return l.u_off; }
};
TD_DEV int ingest_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
template <class F>
TD_DEV void yuv_rgb(const SrcLayout& l, int Y, int U, int V, int* p) {
    int yy = Y - l.yoff;
    yy = (yy < 0 ? 0 : yy) * l.cy + (1 << 19);
    const int u = U - F::mid(l), v = V - F::mid(l);
    p[0] = ingest_clamp8((yy + l.cvr * v) >> 20);
    p[1] = ingest_clamp8((yy + l.cvg * v + l.cug * u) >> 20);
    p[2] = ingest_clamp8((yy + l.cub * u) >> 20);
}
// the sample at p: a byte, or the 10 bits in bits 15..6 of the little-endian word there (p at any byte address)
template <bool WIDE>
TD_DEV int surf_sample(const unsigned char* p) { return WIDE ? (int)(((unsigned)p[0] | ((unsigned)p[1] << 8)) >> 6) : (int)p[0]; }

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

// ---- the readers -------------------------------------------------------------------------------------------------------------------
// stage(): the workgroup's part before the barrier -- the spans of source rows y0 and y1 (the second only with resize), source columns cl .. ch, into
// the LDS behind the table -- and where the taps will find them.  tap(): source pixel (row r = 0 | 1, rectangle column) as p[3] = R, G, B in 0..255.
// Where the taps find the staged rows: byte offsets from the workgroup's LDS base (possibly below a span's start: only columns of the staged span
// are asked for) of column 0's first colour byte / luma sample of row r, and of chroma pair 0's U and V samples
struct IngestRows { int lp[2], up[2], vp[2]; };

// Packed pixels: a row's staged span starts at (oy + y) pitch + (ox + cl) BPP and holds cols * BPP bytes; taps step by BPP and channel c reads byte c
// or 2 - c.  The format is the instantiation: RGB24 pays nothing for the others.
template <int BPP, bool SWAP>
struct IngestPacked {
    // the same-size branch taps the up to 3 columns behind the row's end too and drops them: no branch per pixel.  k_ingest_u8 guarded these taps in its
    // text and the compiler speculated the loads; here the text leaves the guard away (guarded like the YUV reader's the 1024x2048 same-size launch measured
    // 12.13 against 11.71 us: DESIGN.md 5.14).  They stay inside this workgroup's LDS: row 0's bytes begin at most 15 behind q0 and are cols * BPP long, the
    // taps reach at most 3 * BPP <= 12 further, span >= cols * BPP + 15 (td_handle.h u8_build), and the launch always reserves the second span, which the
    // same-size branch does not stage: the last byte read is below q0 + span + 12 < q0 + 2 * span.
    static constexpr bool guard_taps = false;
    TD_DEV_MEMBER void stage(const IngestArgs& a, const SrcLayout& l, unsigned char* sm, int y0, int y1, int cl, int ch, IngestRows& t) {
        const size_t nbytes = (size_t)(ch - cl + 1) * BPP;
        const size_t f0 = (size_t)(l.oy + y0) * l.pitch + (size_t)(l.ox + cl) * BPP, f1 = (size_t)(l.oy + y1) * l.pitch + (size_t)(l.ox + cl) * BPP;
        const size_t lo = (size_t)a.src, hi = lo + a.extent;
        const int q0 = TD_INGEST_LUT_BYTES, q1 = q0 + a.span;
        ingest_stage_row(lo, hi, sm + q0, f0, nbytes);
        if (a.resize) ingest_stage_row(lo, hi, sm + q1, f1, nbytes);
        t.lp[0] = q0 + (int)((lo + f0) & 15) - cl * BPP + (SWAP ? 2 : 0);
        t.lp[1] = q1 + (int)((lo + f1) & 15) - cl * BPP + (SWAP ? 2 : 0);
    }
    TD_DEV_MEMBER void tap(const SrcLayout&, const unsigned char* sm, const IngestRows& t, int r, int col, int* p) {
        const unsigned char* b = sm + t.lp[r] + BPP * col;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = b[SWAP ? -c : c];
    }
};
// YUV, sample width WIDE, layout by form F.  Per source row: the luma span (4:2:2: widened to whole pixel pairs, so that the row's chroma is in it),
// and -- 4:2:0 only -- the span of the chroma row (I420: one of the U and one of the V plane; pairs (ox + cl) >> 1 .. (ox + ch) >> 1), the second row's
// only where it is another chroma row (wave-uniform).  Bytes of the pitch padding or of the gap between the planes may land in LDS but no tap indexes
// them.  A tap is 3 multiply-adds, a shift and a clamp per channel: no second pass over LDS, no second barrier.
template <bool WIDE, class F>
struct IngestYuv {
    static constexpr bool guard_taps = true;                                      // same-size: only columns of the row are tapped
    TD_DEV_MEMBER void stage(const IngestArgs& a, const SrcLayout& l, unsigned char* sm, int y0, int y1, int cl, int ch, IngestRows& t) {
        const int planes = F::planes(l);
        const int q0 = TD_INGEST_LUT_BYTES, q1 = q0 + a.span, qc = q1 + a.span;    // LDS offsets of the luma spans and of the chroma spans: [row][planes] of span_c bytes
        const int g0 = l.oy + y0, g1 = l.oy + y1;                                  // the frame's rows and ...
        const int gl = l.ox + cl, gh = l.ox + ch;                                  // ... columns: chroma goes by THEIR parity
        const int npair = (gh >> 1) - (gl >> 1) + 1;
        const int lb = planes ? F::lstride(l) * gl : 4 * (gl >> 1);                // the luma span's first byte within its row (4:2:2: the pair's)
        const size_t ny = planes ? (size_t)F::lstride(l) * (size_t)(ch - cl + 1) : (size_t)4 * npair;
        const int cb = F::cstep(l) * (gl >> 1);                                    // the chroma span's first byte within its row
        const size_t nc = (size_t)F::cstep(l) * npair;
        const size_t f0 = (size_t)g0 * l.pitch + lb, f1 = (size_t)g1 * l.pitch + lb;
        const size_t cu0 = (size_t)F::u_off(l) + (size_t)(g0 >> 1) * F::cpitch(l) + cb, cu1 = (size_t)F::u_off(l) + (size_t)(g1 >> 1) * F::cpitch(l) + cb;
        const size_t cv0 = (size_t)F::v_off(l) + (size_t)(g0 >> 1) * F::cpitch(l) + cb, cv1 = (size_t)F::v_off(l) + (size_t)(g1 >> 1) * F::cpitch(l) + cb;
        const bool two = (g0 >> 1) != (g1 >> 1);                                   // false without resize: y0 == y1
        const size_t lo = (size_t)a.src, hi = lo + a.extent;
        ingest_stage_row(lo, hi, sm + q0, f0, ny);
        if (a.resize) ingest_stage_row(lo, hi, sm + q1, f1, ny);
        if (planes) {                                                              // wave-uniform
            ingest_stage_row(lo, hi, sm + qc, cu0, nc);
            if (planes == 2) ingest_stage_row(lo, hi, sm + qc + a.span_c, cv0, nc);
            if (two) {
                ingest_stage_row(lo, hi, sm + qc + planes * a.span_c, cu1, nc);
                if (planes == 2) ingest_stage_row(lo, hi, sm + qc + 3 * a.span_c, cv1, nc);
            }
        }
        const int uo = F::uo(l), vo = F::vo(l), loff = F::loff(l);
        t.lp[0] = q0 + (int)((lo + f0) & 15) - lb + loff;                          // sm[lp + lstride * column]: the luma sample of frame column `column`
        t.lp[1] = q1 + (int)((lo + f1) & 15) - lb + loff;
        if (planes == 0) {                                                         // 4:2:2: in the luma row
            t.up[0] = t.lp[0] - loff + uo; t.vp[0] = t.lp[0] - loff + vo;          // sm[up + cstep * pair]: the U sample of that pair; ...
            t.up[1] = t.lp[1] - loff + uo; t.vp[1] = t.lp[1] - loff + vo;
        } else {
            t.up[0] = qc + (int)((lo + cu0) & 15) - cb + uo;
            t.vp[0] = planes == 2 ? qc + a.span_c + (int)((lo + cv0) & 15) - cb : t.up[0] - uo + vo;
            t.up[1] = two ? qc + planes * a.span_c + (int)((lo + cu1) & 15) - cb + uo : t.up[0];
            t.vp[1] = !two ? t.vp[0] : planes == 2 ? qc + 3 * a.span_c + (int)((lo + cv1) & 15) - cb : t.up[1] - uo + vo;
        }
    }
    TD_DEV_MEMBER void tap(const SrcLayout& l, const unsigned char* sm, const IngestRows& t, int r, int col, int* p) {
        const int gx = l.ox + col, c = F::cstep(l) * (gx >> 1);
        yuv_rgb<F>(l, surf_sample<WIDE>(sm + t.lp[r] + F::lstride(l) * gx), surf_sample<WIDE>(sm + t.up[r] + c), surf_sample<WIDE>(sm + t.vp[r] + c), p);
    }
};

template <class R>
TD_KERNEL void k_ingest(IngestArgs a, SrcLayout l) {
    TD_DYN_LDS(smem);
    unsigned char* sm = reinterpret_cast<unsigned char*>(smem);
    float* lut = reinterpret_cast<float*>(smem);                                   // [3][256]; the staged spans lie behind it
    const int y = blockIdx.y, xs = blockIdx.x * blockDim.x * 4;
    const int xe = xs + (int)blockDim.x * 4 < a.W ? xs + (int)blockDim.x * 4 : a.W;   // the strip: output columns [xs, xe)
    for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = a.lut[i];
    int y0 = y, y1 = y, b0 = 0, b1 = 0, cl = xs, ch = xe - 1;                      // source columns [cl, ch]
    if (a.resize) {
        const td_i32x4 t = *reinterpret_cast<const td_i32x4*>(a.yt + 4 * y);
        y0 = t[0]; y1 = t[1]; b0 = t[2]; b1 = t[3];
        cl = a.xt[xs]; ch = a.xt[a.Wt + xe - 1];
    }
    IngestRows rows;
    R::stage(a, l, sm, y0, y1, cl, ch, rows);
    __syncthreads();
    const int x = xs + (int)threadIdx.x * 4;
    if (x >= a.W) return;
    float f[12];
    if (a.resize) {
        const td_i32x4 s0 = *reinterpret_cast<const td_i32x4*>(a.xt + x), s1 = *reinterpret_cast<const td_i32x4*>(a.xt + a.Wt + x);
        const td_i32x4 a0 = *reinterpret_cast<const td_i32x4*>(a.xt + 2 * a.Wt + x), a1 = *reinterpret_cast<const td_i32x4*>(a.xt + 3 * a.Wt + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int p00[3], p01[3], p10[3], p11[3];                                    // the four taps
            R::tap(l, sm, rows, 0, s0[e], p00);
            R::tap(l, sm, rows, 0, s1[e], p01);
            R::tap(l, sm, rows, 1, s0[e], p10);
            R::tap(l, sm, rows, 1, s1[e], p11);
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
            if (in || !R::guard_taps) R::tap(l, sm, rows, 0, x + e, p);
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
