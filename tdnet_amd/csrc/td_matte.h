// td_matte.h -- matte out: the softmax mass of a SET of classes as a byte, beside (or instead of) the uint8 label map -- in the frame's LAST
// kernel, where every class's upsampled logit already passes through registers (td_conf.h keeps the sum over all classes there; this keeps a
// second sum over the members of the set).
//
// The contract (include/tdnet.h "matte out"): v_c the fp32 logit of class c at the pixel, l the first-maximum argmax (the label entries' label),
// S the configured set,
//   den = sum_c exp(v_c - v_l),   num = sum_{c in S} exp(v_c - v_l)   in fp32, the maximum subtracted,   matte = floor(255 num / den + 0.5).
// One pass over the classes with a running maximum, td_conf.h's ONLINE form: a class above the maximum rescales, one below adds -- and BOTH sums
// take the SAME operations in the SAME order: the rescale multiplies both, a member's term is added to both (a non-member adds 0.f to num, which
// changes nothing).  With every class a member num and den are therefore the same float, num / den is exactly 1 and the byte exactly 255; with
// no member num stays 0.f and the byte is 0.  The quotient is a true division for that reason (x / x = 1; x * (1 / x) need not be).
//
// The set travels as kernel ARGUMENTS: 256 membership bits in eight 32-bit words (MatteSet), wave-uniform like the class index that selects
// the bit -- no table in device memory, and a captured graph replays the set it was captured with.
//
// Two output rows, one lane split (td_conf.h): the lanes' runs follow the MATTE row -- it is always there, the label map may be NULL -- with
// td_u8_run's split; the label bytes of the same 4 pixels leave through the same td_u8_store.  There is no rejection here: the labels are the
// label entries' labels byte for byte, whatever the logits hold (the comparisons that pick l are k_upsample_argmax_u8's).
//
// Plain C++ on the TD_* macros: no LDS, no atomics, no inline assembly, nothing wave-wide; tests/emu runs this file unchanged.
#pragma once
#include "td_device.h"
#include "td_out.h"      // td_up_coef / td_first_max / td_u8_run / td_u8_store / td_px4_load
#include "td_conf.h"     // TD_CONF_LOG2E

// bit c & 31 of word c >> 5: class c is a member.  The word is picked by a chain of selects on constant indices: an INDEXED read of the array would
// make it a private array, which the compiler moves to LDS.  c is wave-uniform, so the selects are scalar -- but in the compiled class loop the words are
// not all held in registers: the compiler loads some of them from the argument segment inside the loop (4 scalar loads and 19 waits per two classes
// against the confidence kernel's 1 and 12; DESIGN.md 5.15 has the measurement and the two rewrites that were tried and did no better).
struct MatteSet { unsigned w[8]; };
TD_DEV bool td_matte_member(const MatteSet& s, int c) {
    const int i = c >> 5;
    unsigned word = s.w[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) word = i == k ? s.w[k] : word;
    return ((word >> (c & 31)) & 1u) != 0u;
}

// The classes seen so far of a lane's 4 pixels: the running (first) maximum, its index, the sum of exp(v - best) over all of them and over the members
struct MatteAcc {
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    float den[4] = {1.f, 1.f, 1.f, 1.f};
    float num[4] = {0.f, 0.f, 0.f, 0.f};
};
// class c's logit v joins pixel e; m: c is a member (wave-uniform).  The output stage's first-maximum rule, so bi is the label entries' label.
// Class 0 is the first maximum and its own term exactly 1: den = 1, num = 1 or 0.  Every later class: ex = exp(-|v - best|) in (0, 1]; above the
// maximum both sums are rescaled by it and the class's own 1 joins, below it the class's ex joins -- into num only through the select.
TD_DEV void td_matte_step(MatteAcc& a, int c, int e, float v, bool m) {
    const float old = a.best[e];
    const bool up = td_first_max(c, v, a.best[e], a.bi[e]);
    if (c == 0) {
        a.num[e] = m ? 1.f : 0.f;
    } else {
        const float ex = td_exp2((up ? old - v : v - old) * TD_CONF_LOG2E);
        const float term = up ? 1.f : ex;
        a.den[e] = (up ? a.den[e] * ex : a.den[e]) + term;
        a.num[e] = (up ? a.num[e] * ex : a.num[e]) + (m ? term : 0.f);
    }
}
// floor(255 num / den + 0.5) as a byte; written so that a NaN or an infinity converts to a defined byte (0 / 255) instead of undefined behaviour
TD_DEV int td_matte_byte(float num, float den) {
    const float t = 255.f * (num / den) + 0.5f;
    return t >= 0.f ? (t < 256.f ? (int)t : 255) : 0;
}
// Store a lane's run [xa, xb) of the matte row (mrow; the lane split is this row's: td_u8_run) and, lrow != NULL, of the label row
TD_DEV void td_matte_store(unsigned char* lrow, unsigned char* mrow, long xa, long xb, const MatteAcc& a) {
    int mb[4], lb[4];                                                  // copies: td_u8_store indexes its bytes by a variable, and must not do that to the accumulator
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mb[e] = td_matte_byte(a.num[e], a.den[e]);
        lb[e] = a.bi[e];
    }
    td_u8_store(mrow, xa, xb, mb);
    if (lrow) td_u8_store(lrow, xa, xb, lb);
}

// The frame's last launch when the matte is asked for.  k_upsample_argmax_conf_u8's geometry -- grid = (ceil((W / 4 + 2) / 256), H), row from the
// block index, 4 consecutive pixels per lane -- its written-out class loop (td_conf.h says why not td_up_classes) and the output stage's
// expression and first-maximum rule, over the classes once.  labels may be NULL (matte only); matte [H][W] bytes at any address.
// The launch bound asks for the confidence kernel's 6 waves per SIMD: without it the four registers of num take the allocator from that kernel's
// 78 VGPRs to 82, one allocation step up and 5 waves; with it 78, no spill.
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 6) k_upsample_argmax_matte_u8(const float* __restrict__ in, unsigned char* __restrict__ labels, unsigned char* __restrict__ matte, int C, int h, int w,
                                          int H, int W, MatteSet set) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    unsigned char* mrow = matte + (size_t)Y * W;
    long xa, xb;
    td_u8_run(mrow, q, W, &xa, &xb);
    if (xa >= xb) return;
    const float sy = td_up_scale(h, H), sx = td_up_scale(w, W);
    const UpCoef cy = td_up_coef(Y, sy, h);
    UpCoef cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cx[e] = td_up_coef((int)td_run_px(xa, e, W), sx, w);
    MatteAcc a;
    for (int c = 0; c < C; ++c) {
        const float* pl = in + (size_t)c * h * w;
        const bool m = td_matte_member(set, c);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] = td_bilerp(cy.l, cx[e].l, pl[cy.i0 * w + cx[e].i0], pl[cy.i0 * w + cx[e].i1], pl[cy.i1 * w + cx[e].i0], pl[cy.i1 * w + cx[e].i1]);
#pragma unroll
        for (int e = 0; e < 4; ++e) td_matte_step(a, c, e, v[e], m);
    }
    td_matte_store(labels ? labels + (size_t)Y * W : nullptr, mrow, xa, xb, a);
}
// The unfused form: label and matte of full-resolution NCHW logits the caller already holds (v_c = the given logits).  k_logits_conf_u8's
// geometry and loads over the HW pixels as one run.  The lane split follows the MATTE map.
TD_KERNEL void k_logits_matte_u8(const float* __restrict__ logits, unsigned char* __restrict__ labels, unsigned char* __restrict__ matte, int C, long HW, MatteSet set) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long pa, pb;
    td_u8_run(matte, q, HW, &pa, &pb);
    if (pa >= pb) return;
    const bool vec = td_px4_vec(logits, HW, pa, pb);
    MatteAcc a;
    for (int c = 0; c < C; ++c) {
        const f32x4 v = td_px4_load(logits + (size_t)c * HW, pa, HW, vec);
        const bool m = td_matte_member(set, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) td_matte_step(a, c, e, v[e], m);
    }
    td_matte_store(labels, matte, pa, pb, a);
}

// ---- the composite -------------------------------------------------------------------------------------------------------------------
// The source frame seen through the matte, at the SOURCE's size (include/tdnet.h "matte out", the composite): source pixel (y, x) takes the matte
// byte M of network pixel (ys[y], xs[x]) -- "overlay out"'s geometry and tables -- and
//   colour mode   out_c = (s_c A + bg_c (256 - A) + 128) >> 8, A = M + (M >> 7): td_overlay_blend with the source as the colour, M as its alpha and
//                 bg underneath; M = 255 gives s and M = 0 gives bg, exactly
//   alpha mode    the source's colour bytes unchanged and M as the x byte of a 32-bit destination pixel.
// k_picture_rows' row geometry and run splits (td_out.h), td_src_px4 for the source.  M comes from td_up_classes with the matte step evaluated
// ONLY at the sampled pixel (the same operations on the same values as k_upsample_argmax_matte_u8: the same byte), or from a matte map [H][W]
// the caller holds.
struct CompArgs {
    const float* in;               // low-resolution logits [C][h][w] (the fused form)
    const unsigned char* map;      // uint8 matte map [H][W] (the map form)
    const int* ys; const int* xs;  // [oh], [ow]: the sampled network pixel of a picture row / column
    int C, h, w, H, W, oh, ow;
    unsigned bg;                   // colour mode: the background in the order of the picture word's bytes, c0 | c1 << 8 | c2 << 16
    MatteSet set;                  // the fused form's class set
};
// px[e]: colour bytes in bits 0..23 and the x byte in bits 24..31 of pixel xa + e.  ONE 16-byte store where the run is four pixels at a 16-byte boundary
TD_DEV void td_p32a_store(unsigned char* row, long xa, long xb, const unsigned* px) {
    unsigned char* p = row + 4 * xa;
    if (xb - xa == 4 && (((size_t)p) & 15u) == 0) {
        TdPx4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.v[e] = px[e];
        *reinterpret_cast<TdPx4*>(p) = v;
    } else {
        unsigned w[4];                                                 // a copy: indexed by a variable below
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = px[e];
        for (long X = xa; X < xb; ++X, p += 4) {
            const unsigned v = w[X - xa];
            p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24);
        }
    }
}
// DST: TD_DST_RGB (the contiguous block), TD_DST_P24, TD_DST_P32 (a rectangle of a pitched frame); ALPHA with TD_DST_P32 only.  SRC: the view forms
// and the surfaces (a tight whole frame is a view with origin 0).  The launch bound is k_picture_rows' for its fused forms.
template <bool FROM_MAP, int SRC, int DST, bool ALPHA>
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 5) k_composite_rows(CompArgs a, const unsigned char* src, SrcLayout l, PicDst d) {
    static_assert(!ALPHA || DST == TD_DST_P32, "the alpha byte needs a 32-bit destination pixel");
    const int q = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= a.oh) return;
    unsigned char* row = DST == TD_DST_RGB ? d.base + (size_t)y * a.ow * 3 : d.base + (size_t)(d.oy + y) * d.pitch + (size_t)d.ox * (DST == TD_DST_P32 ? 4 : 3);
    long xa, xb;
    if (DST == TD_DST_P32) td_p32_run(row, q, a.ow, &xa, &xb);
    else td_rgb_run(row, q, a.ow, &xa, &xb);
    if (xa >= xb) return;
    unsigned M[4];
    if (FROM_MAP) {
        const unsigned char* mrow = a.map + (size_t)a.ys[y] * a.W;
#pragma unroll
        for (int e = 0; e < 4; ++e) M[e] = mrow[a.xs[td_run_px(xa, e, a.ow)]];
    } else {
        MatteAcc acc;
        td_up_classes(a.in, a.C, a.h, a.w, a.H, a.W, a.ys[y], [&](int e) { return a.xs[td_run_px(xa, e, a.ow)]; },
                      [&](int c, int e, float v) { td_matte_step(acc, c, e, v, td_matte_member(a.set, c)); });
#pragma unroll
        for (int e = 0; e < 4; ++e) M[e] = (unsigned)td_matte_byte(acc.num[e], acc.den[e]);
    }
    unsigned s[4], px[4];
    td_src_px4<SRC>(src, l, y, xa, a.ow, DST == TD_DST_RGB ? q > 0 && xb - xa == 4 : xa + 4 <= a.ow, s);
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = ALPHA ? (s[e] & 0xFFFFFFu) : td_overlay_blend((s[e] & 0xFFFFFFu) | (M[e] << 24), a.bg);
    if (DST != TD_DST_RGB && d.swap) {                                 // wave-uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = td_swap_rb(px[e]);
    }
    if (ALPHA) {
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] |= M[e] << 24;
        td_p32a_store(row, xa, xb, px);
    } else if (DST == TD_DST_P32) td_p32_store(row, xa, xb, px);
    else td_rgb_store(row, q, xa, xb, px);
}
