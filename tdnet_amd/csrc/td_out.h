// td_out.h -- the output stage: what happens behind the low-resolution logits [C][h][w].  The x8 bilinear upsample (align_corners=True), the
// argmax over classes, and the forms in which a frame's labels leave: fp32 logits, int32 labels, uint8 labels, a colour map, an overlay.  td_score.h
// (confusion counts) and td_conf.h (confidence bytes) add their accumulator and store to the same body.
//
// ONE definition each of what every output form must agree on bit for bit:
//   td_bilerp (td_misc.h)  the bilinear expression of a pixel from its four source values
//   td_up_coef             source index pair and weight of an output row / column
//   td_first_max           the argmax rule: the first maximum wins
//   td_up_classes          the per-lane body of the sampled kernels: 4 pixels of a row, every class's upsampled logit handed to a step
//   td_u8_run / _store     the lane split of a byte row that starts at any address, and its packed store
//   td_px4_*               4 pixels of a full-resolution plane, one 16-byte load where the plane allows
// The library and the emulator are both built with -ffp-contract=off: the one inlined expression rounds the same at every site.
// Plain C++ on the TD_* macros: compiles unchanged under tests/emu/td_device.h.
#pragma once
#include "td_device.h"
#include "td_conv.h"   // td_ld4 / td_st4
#include "td_misc.h"   // td_bilerp
#include <type_traits>
#include "td_ingest.h" // SrcLayout, the forms, yuv_rgb: the one YUV -> RGB conversion (overlay out reads the source frame)

// ---- bilinear, align_corners=True (td4_psp18.py:227): planar [C][h][w] -> [C][H][W] ------------------------------
struct UpCoef { int i0, i1; float l; };
TD_DEV UpCoef td_up_coef(int d, float scale, int n_in) {
    const float f = scale * (float)d;
    UpCoef c;
    c.i0 = (int)f;
    c.i1 = c.i0 + (c.i0 < n_in - 1 ? 1 : 0);
    c.l = f - (float)c.i0;
    return c;
}
TD_DEV float td_up_scale(int n_in, int n_out) { return (n_out > 1) ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }
// output column X of an output row whose source rows are r0 (cy.i0) and r1 (cy.i1)
TD_DEV float td_up_value(const float* r0, const float* r1, const UpCoef& cy, int X, float sx, int w) {
    const UpCoef cx = td_up_coef(X, sx, w);
    return td_bilerp(cy.l, cx.l, r0[cx.i0], r0[cx.i1], r1[cx.i0], r1[cx.i1]);
}
TD_KERNEL void k_upsample(const float* __restrict__ in, float* __restrict__ out, int C, int h, int w, int H, int W) {
    const float sy = td_up_scale(h, H), sx = td_up_scale(w, W);
    const long total = (long)C * H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int X = (int)(i % W);
        const long t = i / W;
        const int Y = (int)(t % H), c = (int)(t / H);
        const UpCoef cy = td_up_coef(Y, sy, h);
        const float* pl = in + (size_t)c * h * w;
        out[i] = td_up_value(pl + cy.i0 * w, pl + cy.i1 * w, cy, X, sx, w);
    }
}
// Any W (769x1537, the reference's native size, is not a multiple of 4, so the rows of the [C][H][W] output start at every alignment).
// grid = (ceil((W / 4 + 2) / 256), H, C): row and channel from the block index, vertical coefficients wave-uniform.  Lane q >= 1 of a row
// writes the 16-byte ALIGNED quad X0 + 4 (q - 1) .. + 3 with one store, X0 = the row's first aligned column; lane 0 writes the X0 head
// elements, the lane of the last (partial) quad its tail, as scalars.  Same expression per element as k_upsample: bit-identical.
// (Round 5: the grid-stride k_upsample with a 64-bit div / mod per element took 70 us for the 90 MB of a 769x1537 frame, one 4-byte store
// per lane 48 us.)
TD_KERNEL void k_upsample_row(const float* __restrict__ in, float* __restrict__ out, int C, int h, int w, int H, int W) {
    const float sy = td_up_scale(h, H), sx = td_up_scale(w, W);
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y, c = blockIdx.z;
    float* orow = out + ((size_t)c * H + Y) * W;
    const int X0 = (int)((4u - (unsigned)(((size_t)orow >> 2) & 3u)) & 3u);      // columns before the first 16-byte boundary of this row
    const int xa = q == 0 ? 0 : X0 + 4 * (q - 1), xb = q == 0 ? (X0 < W ? X0 : W) : (xa + 4 < W ? xa + 4 : W);
    if (xa >= xb) return;
    const UpCoef cy = td_up_coef(Y, sy, h);
    const float* r0 = in + ((size_t)c * h + cy.i0) * w;
    const float* r1 = in + ((size_t)c * h + cy.i1) * w;
    if (q > 0 && xb - xa == 4) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = td_up_value(r0, r1, cy, xa + e, sx, w);
        td_st4(orow + xa, o);
    } else {
        for (int X = xa; X < xb; ++X) orow[X] = td_up_value(r0, r1, cy, X, sx, w);
    }
}
// same arithmetic, 4 consecutive output columns per lane and one 16-byte store (W % 4 == 0): the 159 MB logits write
// of a 1024x2048 frame is the largest single HBM stream of the path
// grid = (ceil(W/4 / 256), H, C): the row and channel come from the block index (no 64-bit div/mod per thread), the row's
// vertical coefficients are wave-uniform
TD_KERNEL void k_upsample_x4(const float* __restrict__ in, float* __restrict__ out, int C, int h, int w, int H, int W) {
    const float sy = td_up_scale(h, H), sx = td_up_scale(w, W);
    const int X4 = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y, c = blockIdx.z;
    if (X4 >= (W >> 2)) return;
    const UpCoef cy = td_up_coef(Y, sy, h);
    const float* r0 = in + ((size_t)c * h + cy.i0) * w;
    const float* r1 = in + ((size_t)c * h + cy.i1) * w;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = td_up_value(r0, r1, cy, X4 * 4 + e, sx, w);
    td_st4(out + ((size_t)c * H + Y) * W + X4 * 4, o);
}

// ---- argmax: the first maximum wins (== output.max(1)[1], test.py:61, wherever no logit of the pixel is a NaN) ----------------------
// Class c's value v joins the running maximum `best` (class `bi`) of the classes 0 .. c - 1; true if it took its place.
// +/-inf compare like any value, so those labels are the reference's too.  A NaN is where the two part: torch's max names the first NaN,
// here class 0 starts the running maximum and `v > best` is false with a NaN on either side -- a NaN never replaces it, and a NaN in
// class 0 is never replaced.  A label under a NaN means nothing in the reference either, so the class loop carries no isnan for it; the
// rule is pinned as it is by tests/nonfinite_cases.py.
TD_DEV bool td_first_max(int c, float v, float& best, int& bi) {
    const bool up = c == 0 || v > best;
    if (up) { best = v; bi = c; }
    return up;
}
// labels int32 [H][W] of full-resolution logits
TD_KERNEL void k_argmax(const float* __restrict__ logits, int32_t* __restrict__ labels, int C, long HW) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (long)gridDim.x * blockDim.x) {
        float best = 0.f;
        int bi = 0;
        for (int c = 0; c < C; ++c) td_first_max(c, logits[(size_t)c * HW + p], best, bi);
        labels[p] = bi;
    }
}
// fused upsample + argmax: the same arithmetic as k_upsample followed by k_argmax, without the [C][H][W] round trip
TD_KERNEL void k_upsample_argmax(const float* __restrict__ in, int32_t* __restrict__ labels, int C, int h, int w, int H, int W) {
    const float sy = td_up_scale(h, H), sx = td_up_scale(w, W);
    const long total = (long)H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int X = (int)(i % W), Y = (int)(i / W);
        const UpCoef cy = td_up_coef(Y, sy, h), cx = td_up_coef(X, sx, w);
        float best = 0.f;
        int bi = 0;
        for (int c = 0; c < C; ++c) {
            const float* pl = in + (size_t)c * h * w;
            td_first_max(c, td_bilerp(cy.l, cx.l, pl[cy.i0 * w + cx.i0], pl[cy.i0 * w + cx.i1], pl[cy.i1 * w + cx.i0], pl[cy.i1 * w + cx.i1]), best, bi);
        }
        labels[i] = bi;
    }
}

// ---- the sampled kernels' per-lane body ----------------------------------------------------------------------------------------------
// A lane's 4 pixels of one output row: the upsampled logit of every class c at full-resolution pixel (Y, xsrc(e)), e = 0 .. 3, handed to
// step(c, e, v) class by class -- k_upsample_argmax's expression, four gathers per pixel and class.  Y and the vertical coefficients are
// wave-uniform where Y comes from the block index.  The callers keep their accumulators as plain locals and the step is called inside the
// unrolled loop over e: everything stays in registers (a coefficient struct handed around cost 10 - 25 VGPRs).
template <class XSrc, class Step>
TD_DEV void td_up_classes(const float* __restrict__ in, int C, int h, int w, int H, int W, int Y, XSrc xsrc, Step step) {
    const float sy = td_up_scale(h, H), sx = td_up_scale(w, W);
    const UpCoef cy = td_up_coef(Y, sy, h);
    UpCoef cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cx[e] = td_up_coef(xsrc(e), sx, w);
    for (int c = 0; c < C; ++c) {
        const float* pl = in + (size_t)c * h * w;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            step(c, e, td_bilerp(cy.l, cx[e].l, pl[cy.i0 * w + cx[e].i0], pl[cy.i0 * w + cx[e].i1], pl[cy.i1 * w + cx[e].i0], pl[cy.i1 * w + cx[e].i1]));
    }
}
// pixel e of a lane's run that starts at xa, in a row (or plane) of n: the lanes of a partial run repeat the last pixel
TD_DEV long td_run_px(long xa, int e, long n) { return xa + e < n ? xa + e : n - 1; }

// ---- uint8 labels ------------------------------------------------------------------------------------------------------------------
// A lane's run of a label row of W bytes that starts at `row`: lane 0 the bytes in front of the first 4-byte boundary, lane q >= 1 the
// aligned quad behind it (k_upsample_row's split, in bytes): [xa, xb)
TD_DEV void td_u8_run(const unsigned char* row, long q, long W, long* xa, long* xb) {
    const long X0 = (long)((4u - (unsigned)((size_t)row & 3u)) & 3u);
    *xa = q == 0 ? 0 : X0 + 4 * (q - 1);
    *xb = q == 0 ? (X0 < W ? X0 : W) : (*xa + 4 < W ? *xa + 4 : W);
}
// The bytes b[0 .. xb - xa) of a run: one 4-byte store where the run is a whole quad at an aligned address -- every full quad of the row the
// split followed (lane 0's run is at most 3 bytes), and those of a second row of the same pixels (td_conf.h) that shares its alignment.
TD_DEV void td_u8_store(unsigned char* row, long xa, long xb, const int* b) {
    if (xb - xa == 4 && (((size_t)(row + xa)) & 3u) == 0)
        *reinterpret_cast<unsigned*>(row + xa) = (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
    else
        for (long X = xa; X < xb; ++X) row[X] = (unsigned char)b[X - xa];
}
// Fused upsample + argmax with uint8 labels [H][W] (nclass <= 256), laid out like k_upsample_row: grid = (ceil((W / 4 + 2) / 256), H), row
// from the block index, 4 consecutive pixels per lane packed into one 4-byte store where the row address allows (W is odd at 769x1537: the
// rows start at every alignment), scalar head and tail.
TD_KERNEL void k_upsample_argmax_u8(const float* __restrict__ in, unsigned char* __restrict__ labels, int C, int h, int w, int H, int W) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    unsigned char* orow = labels + (size_t)Y * W;
    long xa, xb;
    td_u8_run(orow, q, W, &xa, &xb);
    if (xa >= xb) return;
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    td_up_classes(in, C, h, w, H, W, Y, [&](int e) { return (int)td_run_px(xa, e, W); }, [&](int c, int e, float v) { td_first_max(c, v, best[e], bi[e]); });
    td_u8_store(orow, xa, xb, bi);
}
// 4 pixels pa .. pa + 3 of a full-resolution plane of HW floats: one 16-byte load where the planes allow it (HW % 4 == 0, 16-byte aligned
// logits and a whole quad that starts at a multiple of 4), scalar loads otherwise
TD_DEV bool td_px4_vec(const float* logits, long HW, long pa, long pb) { return (HW & 3) == 0 && (((size_t)logits) & 15) == 0 && (pa & 3) == 0 && pb - pa == 4; }
TD_DEV f32x4 td_px4_load(const float* pl, long pa, long HW, bool vec) {
    if (vec) return td_ld4(pl + pa);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = pl[td_run_px(pa, e, HW)];
    return v;
}
// argmax over classes with uint8 labels: k_argmax's rule on 4 consecutive pixels per lane, the HW pixels as one run
TD_KERNEL void k_argmax_u8(const float* __restrict__ logits, unsigned char* __restrict__ labels, int C, long HW) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long pa, pb;
    td_u8_run(labels, q, HW, &pa, &pb);
    if (pa >= pb) return;
    const bool vec = td_px4_vec(logits, HW, pa, pb);
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
        const f32x4 v = td_px4_load(logits + (size_t)c * HW, pa, HW, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) td_first_max(c, v[e], best[e], bi[e]);
    }
    td_u8_store(labels, pa, pb, bi);
}

// ---- pictures out ------------------------------------------------------------------------------------------------------------------
// The colour map (include/tdnet.h "colour map out"): what the frame loop does on the host behind the labels (Testing/test.py:61-71; tdnet_amd/test.py
// save()): the nearest-index sample of the label map to [oh][ow] and decode_segmap.  rgb [oh][ow][3] bytes = lut[labels[ys[oy]][xs[ox]]]: ys / xs are
// dataloader.nearest_index's tables, built on the host (td_handle.h rgb_build), lut 256 words r | g << 8 | b << 16 (rows >= n_colours grey (l, l, l), as
// decode_segmap leaves them).
// The overlay ("overlay out"): the class colours blended over the SOURCE frame, at the source's size -- the same geometry with oh x ow = Hs x Ws
// (ys / xs = nearest_index(H, Hs) / (W, Ws)), and per pixel the source bytes s and the table word r | g << 8 | b << 16 | a << 24 (0 for a label >= n_colours):
//   A = a + (a >> 7)  (0..255 -> 0..256),   out_c = (c A + s_c (256 - A) + 128) >> 8   per channel, int32: A = 0 gives s, A = 256 gives c, no clamp.
// Either picture goes into a contiguous [oh][ow][3] block, or into a rectangle of a pitched frame ("destination views", "surfaces"): packed 3-byte
// pixels, packed 4-byte pixels (x = 255), or a 4:2:0 surface.
// ONE per-lane body (td_picture_px4: the label from the class loop or from a label map, the colour word, the source pixel and the blend) under TWO
// geometries: k_picture_rows -- a lane owns 4 pixels of one row -- for the contiguous and the packed destinations, k_picture_420 -- a lane owns a
// 2-row x 4-column block on the chroma grid -- for the 4:2:0 ones.  What differs beyond that is a policy: the source form (td_src_px4), the destination
// of a row, the form (td_ingest.h YuvFormArgs / YuvFormNv12) a 4:2:0 destination's layout comes from.
struct PicArgs {
    const float* in;               // low-resolution logits [C][h][w] (the fused forms)
    const unsigned char* labels;   // uint8 label map [H][W] (the label-map forms)
    const int* ys; const int* xs;  // [oh], [ow]: the sampled network pixel of a picture row / column
    const unsigned* lut;           // [256]: the colour-map or the overlay table
    int C, h, w, H, W, oh, ow;
};
// The source forms of the overlay; TD_SRC_NONE: the colour map.  The source is described by td_ingest.h's SrcLayout and read at its own resolution,
// directly from the caller's buffer -- no LDS, no barrier, the early returns stay (why not ingest_stage_row: DESIGN.md 5.10).  A b g r source needs no
// form of its own: the blend is per channel, so the host exchanges r and b in the colour table and the picture comes out b g r too.
//   P24T, NV12T   the whole frame, packed 3-byte pixels tight / an NV12 surface: the origin (and the packed pitch, 3 ow) are constants of the form, not
//                 arguments -- what the entries that predate the views reach compiles to what it was (measured: DESIGN.md 5.11)
//   P24, P32      packed 3- / 4-byte pixels (the 4th byte read with its pixel, never used) of a view: origin and pitch are arguments
//   NV12          an NV12 view.  Both NV12 forms are the YUV reader with the layout's numbers as constants (YuvFormNv12)
//   SURF8, SURF16 a YUV surface of 8- / 16-bit samples: the layout is arguments (YuvFormArgs)
enum { TD_SRC_NONE = 0, TD_SRC_P24T, TD_SRC_P24, TD_SRC_P32, TD_SRC_NV12T, TD_SRC_NV12, TD_SRC_SURF8, TD_SRC_SURF16 };
// The destination forms (PicDst below)
enum { TD_DST_RGB = 0, TD_DST_P24 = 1, TD_DST_P32 = 2,              // k_picture_rows' DST
       TD_DST_NV12 = 3, TD_DST_YUV420 = 4 };                         // k_picture_420 with YuvFormNv12 / YuvFormArgs (the launch's names for them)
// R and B share one multiply: the fields (c A + s (256 - A) + 128) <= 65408 of bits 0..15 and 16..31 do not carry into each other
TD_DEV unsigned td_overlay_blend(unsigned lutw, unsigned s) {         // s = sR | sG << 8 | sB << 16
    const unsigned a = lutw >> 24, A = a + (a >> 7), B = 256u - A;
    const unsigned rb = (((lutw & 0x00FF00FFu) * A + (s & 0x00FF00FFu) * B + 0x00800080u) >> 8) & 0x00FF00FFu;
    const unsigned g = (((lutw >> 8) & 0xFFu) * A + ((s >> 8) & 0xFFu) * B + 128u) & 0xFF00u;
    return rb | g;
}
// s[e] = the source pixel (y, xa + e) as sR | sG << 8 | sB << 16 (a partial run repeats its last pixel, td_run_px).  quad: the run is a whole group the
// lane may read at once -- its 12 or 16 packed bytes, or (NV12) its 4 Y bytes -- with byte-aligned loads the compiler is free to merge; otherwise, and for
// a surface's samples and all chroma, pixel by pixel.  Only bytes of pixels (y, x < ow) and of the chroma samples covering them are addressed: nothing
// outside the source extent, none of the pitch padding or of the gap between the planes.
template <int SRC>
TD_DEV void td_src_px4(const unsigned char* src, const SrcLayout& l, int y, long xa, long ow, bool quad, unsigned* s) {
    constexpr bool VIEW = SRC != TD_SRC_P24T && SRC != TD_SRC_NV12T;
    const int oy = VIEW ? l.oy : 0, ox = VIEW ? l.ox : 0;
    if (SRC >= TD_SRC_NV12T) {
        typedef typename std::conditional<(SRC >= TD_SRC_SURF8), YuvFormArgs, YuvFormNv12>::type F;
        constexpr bool WIDE = SRC == TD_SRC_SURF16;
        const int gy = oy + y;
        const unsigned char* lr = src + (size_t)gy * l.pitch + F::loff(l);               // wave-uniform like y
        const size_t crow = (size_t)(gy >> F::cshift(l)) * F::cpitch(l);
        const unsigned char* ur = src + F::u_off(l) + crow + F::uo(l);
        const unsigned char* vr = src + F::v_off(l) + crow + F::vo(l);
        unsigned yw = 0;
        if (F::luma_bytes && quad) __builtin_memcpy(&yw, lr + ox + xa, 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long gx = ox + td_run_px(xa, e, ow), c = (long)F::cstep(l) * (gx >> 1);
            const int Y = F::luma_bytes && quad ? (int)((yw >> (8 * e)) & 255u) : surf_sample<WIDE>(lr + (long)F::lstride(l) * gx);
            int p[3];
            yuv_rgb<F>(l, Y, surf_sample<WIDE>(ur + c), surf_sample<WIDE>(vr + c), p);
            s[e] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
        }
    } else if (SRC == TD_SRC_P32) {
        const unsigned char* r = src + (size_t)(oy + y) * l.pitch + (size_t)ox * 4;
        if (quad) {
            unsigned v[4];
            __builtin_memcpy(v, r + 4 * xa, 16);                       // ONE 16-byte read: four whole pixels of the rectangle
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] = v[e] & 0xFFFFFFu;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned char* p = r + 4 * td_run_px(xa, e, ow);
                s[e] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
            }
        }
    } else {
        const unsigned char* r = VIEW ? src + (size_t)(oy + y) * l.pitch + (size_t)ox * 3 : src + (size_t)y * ow * 3;   // tight: pitch = 3 ow
        if (quad) {
            unsigned v[3];
            __builtin_memcpy(v, r + 3 * xa, 12);
            s[0] = v[0] & 0xFFFFFFu;
            s[1] = ((v[0] >> 24) | (v[1] << 8)) & 0xFFFFFFu;
            s[2] = ((v[1] >> 16) | (v[2] << 16)) & 0xFFFFFFu;
            s[3] = v[2] >> 8;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned char* p = r + 3 * td_run_px(xa, e, ow);
                s[e] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
            }
        }
    }
}
// The 4 pixels xa .. xa + 3 of picture row y as words c0 | c1 << 8 | c2 << 16 (a partial run repeats its last pixel): the colour table's word of
// the label -- the first-maximum argmax of the x8 bilinear upsample evaluated ONLY at the sampled pixel (Y, X) = (ys[y], xs[x]), or the label map's
// byte -- blended over the source pixel for the overlay.  No branch on A: the blend with A = 0 returns the source.
template <bool LABELS, int SRC, int DST>
TD_DEV void td_picture_px4(const PicArgs& a, const unsigned char* src, const SrcLayout& l, int y, int q, long xa, long xb, unsigned* px) {
    if (!LABELS && SRC != TD_SRC_NONE && DST == TD_DST_RGB) {
        // The fused overlay into the contiguous block keeps the text of the kernel it had before this body (k_upsample_argmax_overlay): the arguments in
        // locals, the source pixel before the table word.  Through the text below the same loads cost the allocator 6 - 10 VGPRs more.
        const float* in = a.in;
        const int* ys = a.ys; const int* xs = a.xs;
        const unsigned* lut = a.lut;
        const int C = a.C, h = a.h, w = a.w, H = a.H, W = a.W, ow = a.ow;
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int bi[4] = {0, 0, 0, 0};
        td_up_classes(in, C, h, w, H, W, ys[y], [&](int e) { return xs[td_run_px(xa, e, ow)]; }, [&](int c, int e, float v) { td_first_max(c, v, best[e], bi[e]); });
        unsigned s[4];
        td_src_px4<SRC>(src, l, y, xa, ow, q > 0 && xb - xa == 4, s);
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = td_overlay_blend(lut[bi[e] & 255], s[e]);
        return;
    }
    // One cell reads its source in front of the label map, as the fused block above does: the label map over an NV12 view into a 3-byte view.  Behind
    // it the allocator takes 33 VGPRs where the kernel this body replaced (k_picture_packed<1, true, true, 1>) took 32; the loads are independent, the
    // bytes read and written the same.
    constexpr bool SRC_FIRST = LABELS && SRC == TD_SRC_NV12 && DST == TD_DST_P24;
    unsigned s[4];
    if (SRC_FIRST) td_src_px4<SRC>(src, l, y, xa, a.ow, xa + 4 <= a.ow, s);
    if (LABELS) {
        const unsigned char* lrow = a.labels + (size_t)a.ys[y] * a.W;
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = a.lut[lrow[a.xs[td_run_px(xa, e, a.ow)]]];
    } else {
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int bi[4] = {0, 0, 0, 0};
        td_up_classes(a.in, a.C, a.h, a.w, a.H, a.W, a.ys[y], [&](int e) { return a.xs[td_run_px(xa, e, a.ow)]; }, [&](int c, int e, float v) { td_first_max(c, v, best[e], bi[e]); });
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = a.lut[bi[e] & 255];
    }
    if (SRC != TD_SRC_NONE) {
        if (!SRC_FIRST) td_src_px4<SRC>(src, l, y, xa, a.ow, DST == TD_DST_RGB ? q > 0 && xb - xa == 4 : xa + 4 <= a.ow, s);
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = td_overlay_blend(px[e], s[e]);
    }
}

// Where a picture goes.  TD_DST_RGB: the contiguous block [oh][ow][3] at `base` -- nothing else of this is read; the packed views: the rectangle at
// (oy, ox) of a frame of rows `pitch` bytes apart; 4:2:0: td_ingest.h's layout table, by the form's choice from these fields or as its constants.
struct PicDst {
    unsigned char* base;           // the block, or the destination frame's base; any byte address
    int pitch, cpitch;             // bytes per luma (or packed) row / per chroma row
    unsigned u_off, v_off;         // 4:2:0: < 2^31 (one chroma plane: equal)
    int oy, ox;                    // the rectangle's origin: picture pixel (y, x) is frame pixel (oy + y, ox + x); 4:2:0: both even
    int swap;                      // packed: the destination's colour order is not the picture word's -- bytes 0 and 2 are exchanged at the store
    int cstep, uo, vo;             // 4:2:0: bytes between the chroma pairs of a plane's row; where U and V lie in a pair
    int yoff, ky[3], ku[3], kv[3]; // 4:2:0: rint(c 2^20) of the forward matrix, in the order of the picture word's bytes (the host exchanges r and b behind a b g r source)
};
// A row of 3-byte pixels is 3 ow bytes and starts at any byte address; 4 pixels = 12 bytes = three 4-byte words where row + 3 x is 4-byte aligned, i.e. from
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
TD_DEV unsigned td_swap_rb(unsigned p) { return (p & 0xFF00u) | ((p >> 16) & 0xFFu) | ((p & 0xFFu) << 16); }
// A lane's run of a row of 4-byte pixels that starts at `row`: lane 0 the pixels in front of the first 16-byte boundary (none where the row is not
// 4-byte aligned: no run of it is ever aligned), lane q >= 1 the four behind it: [xa, xb)
TD_DEV void td_p32_run(const unsigned char* row, long q, long ow, long* xa, long* xb) {
    const unsigned r = (unsigned)((size_t)row & 15u);
    const long X0 = (r & 3u) ? 0 : (long)(((16u - r) & 15u) >> 2);
    *xa = q == 0 ? 0 : X0 + 4 * (q - 1);
    *xb = q == 0 ? (X0 < ow ? X0 : ow) : (*xa + 4 < ow ? *xa + 4 : ow);
}
struct alignas(16) TdPx4 { unsigned v[4]; };
// px[e]: the colour word of pixel xa + e; the x byte is 255.  ONE 16-byte store where the run is four pixels at a 16-byte boundary
TD_DEV void td_p32_store(unsigned char* row, long xa, long xb, const unsigned* px) {
    unsigned char* p = row + 4 * xa;
    if (xb - xa == 4 && (((size_t)p) & 15u) == 0) {
        TdPx4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.v[e] = px[e] | 0xFF000000u;
        *reinterpret_cast<TdPx4*>(p) = v;
    } else {
        for (long X = xa; X < xb; ++X, p += 4) {
            const unsigned w = px[X - xa];
            p[0] = (unsigned char)w; p[1] = (unsigned char)(w >> 8); p[2] = (unsigned char)(w >> 16); p[3] = 255;
        }
    }
}
// The row geometry: grid = (ceil((ow / 4 + 2) / 256), oh), the row from the block index, Y and the vertical coefficients wave-uniform, the lane split by
// the row's address (td_rgb_run / td_p32_run).  The frame's last launch when a picture into a contiguous block or a packed view is asked for.
// The contiguous destination's row address is a constant of the form: no origin, pitch or swap is read; a lane of it reads its source group at once
// where its run is an aligned group (q > 0), a lane of a view where the run is whole (xa + 4 <= ow): which bytes a lane reads is part of the memory
// contract (include/tdnet.h).
// The launch bound asks for 5 waves per SIMD: without it the allocator settles the fused overlay forms at 98 / 100 VGPRs and 4 waves, with it at 84 / 86
// (the colour map: 84), no spill either way.  The kernels the label-map forms into a contiguous block replace had no bound, and these
// keep none: (1024, 1) is the compiler's default for a kernel without the attribute, spelled out because a template cannot leave the attribute away
// per instantiation.  It promises nothing about the launch, which is 256 threads like every form's (at most 38 VGPRs, 8 waves).
constexpr int td_rows_threads(bool labels, int dst) { return labels && dst == TD_DST_RGB ? 1024 : 256; }
constexpr int td_rows_waves(bool labels, int dst) { return labels && dst == TD_DST_RGB ? 1 : 5; }
template <bool LABELS, int SRC, int DST>
TD_KERNEL void TD_LAUNCH_BOUNDS(td_rows_threads(LABELS, DST), td_rows_waves(LABELS, DST)) k_picture_rows(PicArgs a, const unsigned char* src, SrcLayout l, PicDst d) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= a.oh) return;
    unsigned char* row = DST == TD_DST_RGB ? d.base + (size_t)y * a.ow * 3 : d.base + (size_t)(d.oy + y) * d.pitch + (size_t)d.ox * (DST == TD_DST_P32 ? 4 : 3);
    long xa, xb;
    if (DST == TD_DST_P32) td_p32_run(row, q, a.ow, &xa, &xb);
    else td_rgb_run(row, q, a.ow, &xa, &xb);
    if (xa >= xb) return;
    unsigned px[4];
    td_picture_px4<LABELS, SRC, DST>(a, src, l, y, q, xa, xb, px);
    if (DST != TD_DST_RGB && d.swap) {                                 // wave-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = td_swap_rb(px[e]);
    }
    if (DST == TD_DST_P32) td_p32_store(row, xa, xb, px);
    else td_rgb_store(row, q, xa, xb, px);
}

// The block geometry: a 4:2:0 destination -- NV12, NV12 with a chroma pitch of its own, NV21, I420 / YV12, P010.  A lane owns the 2-row x 4-column block
// (j, q) of the rectangle, which the even origin aligns to the frame's chroma grid: rows 2 j and 2 j + 1, columns 4 q .. 4 q + 3, the chroma pairs
// (oy / 2 + j, ox / 2 + 2 q) and the one behind it.  Row by row: the picture's four pixels, their luma samples stored, their colours added to the two
// pairs' sums; then the pairs.  At the rectangle's odd last row / column a pair covers n = 2 or 1 pixels and its sum is scaled by m = 4 / n.  All in
// int32 (|m S K| <= 1020 * 0.5 * 2^20, + 2^29 + 2^21 < 2^31), arithmetic shifts.  No LDS, no barrier, no cross-lane traffic;
// grid = (ceil(ceil(ow / 4) / 256), ceil(oh / 2)).  The destination's sample width is the instantiation, its layout the form F's:
//   8 bit   Y = clamp8((K . c + (yoff << 20) + (1 << 19)) >> 20),   U = clamp8((m K . S + (128 << 22) + (1 << 21)) >> 22)     (td_chroma8)
//   P010    Y10 = clamp10((K . c + (yoff << 20) + (1 << 17)) >> 18), U10 = clamp10((m K . S + (128 << 22) + (1 << 19)) >> 20), stored as value << 6,
//           little-endian, bytewise unless the run is 8-byte aligned (the base may be an odd address).
// YuvFormNv12: the NV12 view, and an NV12 surface whose planes share one pitch; YuvFormArgs: every other surface, and any 4:2:0 destination behind a
// surface source.
TD_DEV int td_chroma8(const int* k, const int* s, int m) { return ingest_clamp8((m * (k[0] * s[0] + k[1] * s[1] + k[2] * s[2]) + (128 << 22) + (1 << 21)) >> 22); }
TD_DEV int td_clamp10(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }
TD_DEV int td_chroma10(const int* k, const int* s, int m) { return td_clamp10((m * (k[0] * s[0] + k[1] * s[1] + k[2] * s[2]) + (128 << 22) + (1 << 19)) >> 20); }
// n (1..4) 10-bit values as words value << 6 at p: ONE 8-byte store where all four are there and p is 8-byte aligned, bytes otherwise
struct alignas(8) TdW4 { unsigned v[2]; };
TD_DEV void td_w16_store(unsigned char* p, int n, const int* b) {
    if (n == 4 && (((size_t)p) & 7u) == 0) {
        TdW4 w;
        w.v[0] = ((unsigned)b[0] << 6) | ((unsigned)b[1] << 22);
        w.v[1] = ((unsigned)b[2] << 6) | ((unsigned)b[3] << 22);
        *reinterpret_cast<TdW4*>(p) = w;
    } else {
        for (int i = 0; i < n; ++i) { const unsigned w = (unsigned)b[i] << 6; p[2 * i] = (unsigned char)w; p[2 * i + 1] = (unsigned char)(w >> 8); }
    }
}
// The launch bound asks for 4 waves per SIMD, not the row kernel's 5: two rows' worth of state (the pairs' six sums beside the class loop's accumulators and
// coefficients) does not fit 96 VGPRs -- the fused overlay forms spilled 2 - 21 registers there -- and a lane does two rows' work anyway.
template <bool LABELS, int SRC, bool WIDE, class F>
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 4) k_picture_420(PicArgs a, const unsigned char* src, SrcLayout l, PicDst d) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    const long xa = 4L * q;
    if (2 * j >= a.oh || xa >= a.ow) return;
    const int nx = a.ow - xa < 4 ? (int)(a.ow - xa) : 4, ny = a.oh - 2 * j < 2 ? 1 : 2;
    int s0[3] = {0, 0, 0}, s1[3] = {0, 0, 0};                          // the colour sums of the pair of columns 0, 1 and of columns 2, 3
    for (int r = 0; r < ny; ++r) {
        unsigned px[4];
        td_picture_px4<LABELS, SRC, TD_DST_YUV420>(a, src, l, 2 * j + r, q, xa, xa + nx, px);
        int yb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c0 = (int)(px[e] & 255u), c1 = (int)((px[e] >> 8) & 255u), c2 = (int)((px[e] >> 16) & 255u);
            const int t = d.ky[0] * c0 + d.ky[1] * c1 + d.ky[2] * c2 + (d.yoff << 20);
            yb[e] = WIDE ? td_clamp10((t + (1 << 17)) >> 18) : ingest_clamp8((t + (1 << 19)) >> 20);
            if (e < nx) {
                int* s = e < 2 ? s0 : s1;
                s[0] += c0; s[1] += c1; s[2] += c2;
            }
        }
        unsigned char* yrow = d.base + (size_t)(d.oy + 2 * j + r) * d.pitch;
        if (WIDE) td_w16_store(yrow + 2 * ((size_t)d.ox + xa), nx, yb);
        else td_u8_store(yrow + d.ox, xa, xa + nx, yb);
    }
    const int m0 = 4 / (ny * (nx < 2 ? nx : 2)), m1 = nx > 2 ? 4 / (ny * (nx - 2)) : 0;
    const int np = nx > 2 ? 2 : 1;                                     // chroma pairs of this block
    const int u0 = WIDE ? td_chroma10(d.ku, s0, m0) : td_chroma8(d.ku, s0, m0), v0 = WIDE ? td_chroma10(d.kv, s0, m0) : td_chroma8(d.kv, s0, m0);
    const int u1 = WIDE ? td_chroma10(d.ku, s1, m1) : td_chroma8(d.ku, s1, m1), v1 = WIDE ? td_chroma10(d.kv, s1, m1) : td_chroma8(d.kv, s1, m1);
    const size_t crow = (size_t)((d.oy >> 1) + j) * F::cpitch(d), pair = (size_t)(d.ox >> 1) + 2 * (size_t)q;   // the chroma row, the block's first pair
    if (WIDE) {                                                        // U, V word pairs: 8 bytes per two pairs
        const int cb[4] = {u0, v0, u1, v1};
        td_w16_store(d.base + F::u_off(d) + crow + 4 * pair, 2 * np, cb);
    } else if (F::cstep(d) == 2) {                                     // interleaved byte pairs, U first or (NV21) V first: wave-uniform
        const bool vu = F::uo(d) != 0;
        const int cb[4] = {vu ? v0 : u0, vu ? u0 : v0, vu ? v1 : u1, vu ? u1 : v1};
        td_u8_store(d.base + F::u_off(d) + crow + d.ox, xa, xa + 2 * np, cb);
    } else {                                                           // I420: a row of the U plane and a row of the V plane
        unsigned char* up = d.base + F::u_off(d) + crow + pair;
        unsigned char* vp = d.base + F::v_off(d) + crow + pair;
        up[0] = (unsigned char)u0; vp[0] = (unsigned char)v0;
        if (np == 2) { up[1] = (unsigned char)u1; vp[1] = (unsigned char)v1; }
    }
}
