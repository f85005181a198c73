// td_conf.h -- confidence out: the softmax probability of a pixel's label as a byte, beside (or instead of) the uint8 label map, and the
// rejection of low-confidence labels -- in the frame's LAST kernel, where every class's upsampled logit already passes through registers.
//
// The contract (include/tdnet.h "confidence out"): v_c the fp32 logit of class c at the pixel, l the first-maximum argmax (the label entries'
// label), p = 1 / sum_c exp(v_c - v_l) in fp32 (the maximum subtracted: every exponent is <= 0, the label's own term is exactly 1, nothing
// overflows), conf = floor(255 p + 0.5) as a byte; the label written is conf < min_conf ? reject_label : l.  The comparison is on the BYTE, so
// it is exact, and min_conf = 0 rejects nothing whatever the logits hold (a NaN changes the confidence byte, which is then unspecified, but not
// the comparisons that pick l: those are k_upsample_argmax_u8's).
//
// Pass structure (template parameter ONLINE; which one the library's entries launch: td_launch.h TD_CONF_ONLINE):
//   ONLINE   one pass over the classes with a running maximum m and a running sum s of exp(v - m): a class above m rescales,
//            s = s exp(m - v) + 1, one below adds exp(v - m).  Either way ONE exp2 per class and pixel, of -|v - m| log2(e), and the
//            gathers of k_upsample_argmax_u8, once.
//   two-pass the argmax loop as it is, then a second loop that evaluates every v_c again (the same gathers a second time) and adds
//            exp(v_c - v_l).  The definition taken literally; no rescaling.
// Both give the label entries' labels bit for bit (the same expression, the same comparisons in the same order); their confidence bytes agree
// except where 255 p is within rounding of a half.
//
// Two output rows, one lane split: the label row and the confidence row of a pixel row start at independent byte addresses (W is odd at
// 769x1537, and the two maps are separate allocations).  The lanes' runs follow the CONFIDENCE row -- it is always there, the label map may be
// NULL -- with td_u8_run's split: lane 0 the bytes in front of that row's first 4-byte boundary, lane q >= 1 the aligned quad behind it, so
// the confidence bytes leave as one packed 4-byte store per full quad.  The label bytes of the same 4 pixels leave as one packed store too
// where their address happens to be 4-byte aligned (the two rows share their alignment mod 4: always the case for two maps of one allocator
// with the same W), and as 4 byte stores where it is not.
//
// Plain C++ on the TD_* macros: no LDS, no atomics, no inline assembly; tests/emu runs this file unchanged.
#pragma once
#include "td_device.h"
#include "td_conv.h"     // td_ld4
#include "td_misc.h"     // UpCoef / td_up_coef
#include "td_ingest.h"   // td_u8_run / td_u8_store

#define TD_CONF_LOG2E 1.44269504088896340736f

// The classes seen so far of a lane's 4 pixels: the running (first) maximum, its index, and -- ONLINE -- the sum of exp(v - best)
struct ConfAcc {
    float best[4];
    int bi[4];
    float sum[4];
};
// class c's logits v[0..4) join: k_upsample_argmax_u8's comparison (c == 0 || v > best), so bi is its label
template <bool ONLINE>
TD_DEV void td_conf_step(ConfAcc& a, int c, const float* v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (c == 0) { a.best[e] = v[e]; a.bi[e] = 0; a.sum[e] = 1.f; continue; }
        const bool up = v[e] > a.best[e];
        if (ONLINE) {
            const float ex = td_exp2((up ? a.best[e] - v[e] : v[e] - a.best[e]) * TD_CONF_LOG2E);   // exp(-|v - best|) in (0, 1]
            a.sum[e] = up ? a.sum[e] * ex + 1.f : a.sum[e] + ex;
        }
        if (up) { a.best[e] = v[e]; a.bi[e] = c; }
    }
}
// the second pass of the two-pass form: class c != label adds exp(v - best) (the label's own 1 is there since class 0 / is kept by the caller)
TD_DEV void td_conf_add(ConfAcc& a, int c, const float* v) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c != a.bi[e]) a.sum[e] += td_exp2((v[e] - a.best[e]) * TD_CONF_LOG2E);
}
// p = 1 / sum as the byte floor(255 p + 0.5); written so that a NaN or an infinity converts to a defined byte (0 / 255) instead of undefined behaviour
TD_DEV int td_conf_byte(float sum) {
    const float t = 255.f * (1.f / sum) + 0.5f;
    return t >= 0.f ? (t < 256.f ? (int)t : 255) : 0;
}
// Store a lane's run [xa, xb) of the confidence row (crow; the lane split is this row's: td_u8_run) and, lrow != NULL, of the label row with the
// rejection applied to the byte: conf < min_conf ? reject : label.
TD_DEV void td_conf_store(unsigned char* lrow, unsigned char* crow, long q, long xa, long xb, const ConfAcc& a, int min_conf, int reject) {
    int cb[4], lb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        cb[e] = td_conf_byte(a.sum[e]);
        lb[e] = cb[e] < min_conf ? reject : a.bi[e];
    }
    td_u8_store(crow, q, xa, xb, cb);
    if (!lrow) return;
    if (xb - xa == 4 && (((size_t)(lrow + xa)) & 3u) == 0)
        *reinterpret_cast<unsigned*>(lrow + xa) = (unsigned)lb[0] | ((unsigned)lb[1] << 8) | ((unsigned)lb[2] << 16) | ((unsigned)lb[3] << 24);
    else
        for (long X = xa; X < xb; ++X) lrow[X] = (unsigned char)lb[X - xa];
}

// The frame's last launch when confidence is asked for.  k_upsample_argmax_u8's geometry: grid = (ceil((W / 4 + 2) / 256), H), row from the
// block index, vertical coefficients wave-uniform, 4 consecutive pixels per lane; its expression and first-maximum rule, so with min_conf = 0
// the labels are its labels.  labels may be NULL (confidence only); conf [H][W] bytes at any address.  The lane split follows the CONFIDENCE
// row (see the head of this file).
template <bool ONLINE>
TD_KERNEL void k_upsample_argmax_conf_u8(const float* __restrict__ in, unsigned char* __restrict__ labels, unsigned char* __restrict__ conf, int C, int h, int w,
                                         int H, int W, int min_conf, int reject) {
    const float sy = (H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sx = (W > 1) ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    unsigned char* crow = conf + (size_t)Y * W;
    long xa, xb;
    td_u8_run(crow, q, W, &xa, &xb);
    if (xa >= xb) return;
    const UpCoef cy = td_up_coef(Y, sy, h);
    UpCoef cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cx[e] = td_up_coef((int)(xa + e < W ? xa + e : W - 1), sx, w);
    ConfAcc a;
    for (int pass = 0; pass < (ONLINE ? 1 : 2); ++pass)
        for (int c = 0; c < C; ++c) {
            const float* pl = in + (size_t)c * h * w;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v00 = pl[cy.i0 * w + cx[e].i0], v01 = pl[cy.i0 * w + cx[e].i1];
                const float v10 = pl[cy.i1 * w + cx[e].i0], v11 = pl[cy.i1 * w + cx[e].i1];
                v[e] = (1.f - cy.l) * ((1.f - cx[e].l) * v00 + cx[e].l * v01) + cy.l * ((1.f - cx[e].l) * v10 + cx[e].l * v11);
            }
            if (pass == 0) td_conf_step<ONLINE>(a, c, v);
            else td_conf_add(a, c, v);
        }
    td_conf_store(labels ? labels + (size_t)Y * W : nullptr, crow, q, xa, xb, a, min_conf, reject);
}
// The unfused form: label and confidence of full-resolution NCHW logits the caller already holds (v_c = the given logits).  k_argmax_u8's
// geometry over the HW pixels as one run: 4 consecutive pixels per lane, one 16-byte load per class where the planes allow it (HW % 4 == 0,
// 16-byte aligned logits and a quad that starts at a multiple of 4), scalar loads otherwise.  The lane split follows the CONFIDENCE map.
template <bool ONLINE>
TD_KERNEL void k_logits_conf_u8(const float* __restrict__ logits, unsigned char* __restrict__ labels, unsigned char* __restrict__ conf, int C, long HW,
                                int min_conf, int reject) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long pa, pb;
    td_u8_run(conf, q, HW, &pa, &pb);
    if (pa >= pb) return;
    const bool vec = (HW & 3) == 0 && (((size_t)logits) & 15) == 0 && (pa & 3) == 0 && pb - pa == 4;
    ConfAcc a;
    for (int pass = 0; pass < (ONLINE ? 1 : 2); ++pass)
        for (int c = 0; c < C; ++c) {
            const float* pl = logits + (size_t)c * HW;
            float v[4];
            if (vec) {
                const f32x4 t = td_ld4(pl + pa);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = t[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = pl[pa + e < HW ? pa + e : HW - 1];
            }
            if (pass == 0) td_conf_step<ONLINE>(a, c, v);
            else td_conf_add(a, c, v);
        }
    td_conf_store(labels, conf, q, pa, pb, a, min_conf, reject);
}
