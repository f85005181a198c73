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
// the confidence bytes leave as one packed 4-byte store per full quad.  The label bytes of the same 4 pixels leave through the same
// td_u8_store, which decides by the address: one packed store too where it is 4-byte aligned (the two rows share their alignment mod 4:
// always the case for two maps of one allocator with the same W), 4 byte stores where it is not.
//
// Plain C++ on the TD_* macros: no LDS, no atomics, no inline assembly; tests/emu runs this file unchanged.
#pragma once
#include "td_device.h"
#include "td_out.h"      // td_up_coef / td_first_max / td_u8_run / td_u8_store / td_px4_load

#define TD_CONF_LOG2E 1.44269504088896340736f

// The classes seen so far of a lane's 4 pixels: the running (first) maximum, its index, and the sum of exp(v - best)
struct ConfAcc {
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    int bi[4] = {0, 0, 0, 0};
    float sum[4] = {1.f, 1.f, 1.f, 1.f};
};
// class c's logit v joins pixel e: the output stage's first-maximum rule, so bi is the label entries' label.  ONLINE also keeps the sum: a class
// above the maximum rescales it, one below adds to it -- exp(-|v - best|) in (0, 1] either way; class 0 leaves the label's own 1.
template <bool ONLINE>
TD_DEV void td_conf_step(ConfAcc& a, int c, int e, float v) {
    const float old = a.best[e];
    const bool up = td_first_max(c, v, a.best[e], a.bi[e]);
    if (ONLINE && c != 0) {
        const float ex = td_exp2((up ? old - v : v - old) * TD_CONF_LOG2E);
        a.sum[e] = up ? a.sum[e] * ex + 1.f : a.sum[e] + ex;
    }
}
// the second pass of the two-pass form: class c != label adds exp(v - best) (the label's own 1 is there from the start)
TD_DEV void td_conf_add(ConfAcc& a, int c, int e, float v) {
    if (c != a.bi[e]) a.sum[e] += td_exp2((v - a.best[e]) * TD_CONF_LOG2E);
}
// p = 1 / sum as the byte floor(255 p + 0.5); written so that a NaN or an infinity converts to a defined byte (0 / 255) instead of undefined behaviour
TD_DEV int td_conf_byte(float sum) {
    const float t = 255.f * (1.f / sum) + 0.5f;
    return t >= 0.f ? (t < 256.f ? (int)t : 255) : 0;
}
// Store a lane's run [xa, xb) of the confidence row (crow; the lane split is this row's: td_u8_run) and, lrow != NULL, of the label row with the
// rejection applied to the byte: conf < min_conf ? reject : label.
TD_DEV void td_conf_store(unsigned char* lrow, unsigned char* crow, long xa, long xb, const ConfAcc& a, int min_conf, int reject) {
    int cb[4], lb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        cb[e] = td_conf_byte(a.sum[e]);
        lb[e] = cb[e] < min_conf ? reject : a.bi[e];
    }
    td_u8_store(crow, xa, xb, cb);
    if (lrow) td_u8_store(lrow, xa, xb, lb);
}

// The frame's last launch when confidence is asked for.  k_upsample_argmax_u8's geometry -- grid = (ceil((W / 4 + 2) / 256), H), row from the
// block index, 4 consecutive pixels per lane -- and the output stage's expression and first-maximum rule (td_out.h), over the classes once
// (ONLINE) or twice, so with min_conf = 0 the labels are the label entries' labels.  labels may be NULL (confidence only); conf [H][W] bytes at any address.  The lane
// split follows the CONFIDENCE row (see the head of this file).
template <bool ONLINE>
TD_KERNEL void k_upsample_argmax_conf_u8(const float* __restrict__ in, unsigned char* __restrict__ labels, unsigned char* __restrict__ conf, int C, int h, int w,
                                         int H, int W, int min_conf, int reject) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    unsigned char* crow = conf + (size_t)Y * W;
    long xa, xb;
    td_u8_run(crow, q, W, &xa, &xb);
    if (xa >= xb) return;
    // The class loop written out, not td_up_classes: through the shared body this kernel measured 38.9 us against 37.8 (one pass) and 80.6
    // against 58.4 (two passes) at 1024x2048 x 19 classes, the only one of the family outside the spread of two runs.
    const float sy = td_up_scale(h, H), sx = td_up_scale(w, W);
    const UpCoef cy = td_up_coef(Y, sy, h);
    UpCoef cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cx[e] = td_up_coef((int)td_run_px(xa, e, W), sx, w);
    ConfAcc a;
    for (int pass = 0; pass < (ONLINE ? 1 : 2); ++pass)
        for (int c = 0; c < C; ++c) {
            const float* pl = in + (size_t)c * h * w;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[e] = td_bilerp(cy.l, cx[e].l, pl[cy.i0 * w + cx[e].i0], pl[cy.i0 * w + cx[e].i1], pl[cy.i1 * w + cx[e].i0], pl[cy.i1 * w + cx[e].i1]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (pass == 0) td_conf_step<ONLINE>(a, c, e, v[e]);
                else td_conf_add(a, c, e, v[e]);
            }
        }
    td_conf_store(labels ? labels + (size_t)Y * W : nullptr, crow, xa, xb, a, min_conf, reject);
}
// The unfused form: label and confidence of full-resolution NCHW logits the caller already holds (v_c = the given logits).  k_argmax_u8's
// geometry and loads over the HW pixels as one run.  The lane split follows the CONFIDENCE map.
template <bool ONLINE>
TD_KERNEL void k_logits_conf_u8(const float* __restrict__ logits, unsigned char* __restrict__ labels, unsigned char* __restrict__ conf, int C, long HW,
                                int min_conf, int reject) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long pa, pb;
    td_u8_run(conf, q, HW, &pa, &pb);
    if (pa >= pb) return;
    const bool vec = td_px4_vec(logits, HW, pa, pb);
    ConfAcc a;
    for (int pass = 0; pass < (ONLINE ? 1 : 2); ++pass)
        for (int c = 0; c < C; ++c) {
            const f32x4 v = td_px4_load(logits + (size_t)c * HW, pa, HW, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (pass == 0) td_conf_step<ONLINE>(a, c, e, v[e]);
                else td_conf_add(a, c, e, v[e]);
            }
        }
    td_conf_store(labels, conf, pa, pb, a, min_conf, reject);
}
