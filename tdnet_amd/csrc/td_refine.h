// td_refine.h -- refined matte: He et al.'s guided filter of a matte byte map, with a guide byte map of the same size, restated so that every
// step is an integer operation or ONE correctly rounded fp32 operation (include/tdnet.h "refined matte" is the contract, dataloader.refine_matte_u8
// the oracle).  Box sums of integers do not depend on the order of the additions, so a pixel's bytes do not depend on the tiling and every test of
// these kernels compares with ==.
//
//   window of (y, x): rows max(0, y - r) .. min(h - 1, y + r), columns likewise; N its pixel count; S_x the sums over it
//   stage 1   cov = N S_GM - S_G S_M,  den = N S_GG - S_G^2 + eps N^2 (> 0),  a = f32(cov) / f32(den),
//             a_q = clamp(rint(1024 a), -32767, 32767)   (Q10),   b_q = rint(f32(1024 S_M - a_q S_G) / f32(16 N))   (Q6)
//   stage 2   A = sum a_q, B = sum b_q over the window,   out = clamp8(rint(f32(A G + 16 B) / f32(1024 N)))
//
// Widths, r <= 16 (N <= 1089):
//   a row's box sums      S_G, S_M <= 33 * 255 = 8415: the two share one 32-bit word of LDS;  S_GG, S_GM <= 33 * 65025 < 2^22
//   the window's          S_G, S_M <= 277695;  S_GG, S_GM <= 1089 * 65025 = 70812225: unsigned 32 bits
//   cov, den, 1024 S_M - a_q S_G, A G + 16 B    64 bits (N S_GM reaches 7.7e10, a_q S_G 9.1e9, A G 9.2e9); each is below 2^53 in magnitude, so its
//                                               conversion to double is exact and f32() = (float)(double) is the one round-to-nearest-even conversion
//   |a_q| <= 32767 (int16; with eps >= 4, |a| <= sigma_M / (2 sqrt(eps)) < 32: the clamp is a guard that never binds)
//   |b_q| <= 33791 * 255 / 16 (int32);  |A| <= 1089 * 32767 = 3.6e7,  |B| <= 1089 * 538545 = 5.9e8: int32
//   16 N <= 17424 and 1024 N <= 1115136 are exact in fp32
//
// Two tile kernels of one shape: a workgroup of 256 lanes owns a tile of TY x 64 outputs, stages the tile and a halo of r of its inputs in LDS -- a
// pixel outside the map is staged as 0 and contributes nothing; N comes from the coordinates -- and forms the box sums separably with RUNNING sums:
//   rows      one lane per (staged row, run of 16 output columns): the first window is summed (2 r + 1 terms), every next one adds the column that
//             enters and subtracts the one that leaves; the row sums go to LDS
//   columns   one lane per (output column, run of rows): the same down the row sums, and the pixel's arithmetic from the four (two) window sums
// so a pixel costs one addition and one subtraction per quantity and pass, plus its share of a run's first window.  No atomics, every output is
// written by exactly one lane, nothing is read in the launch that writes it.  LDS at r = 16: 62720 bytes (coefficients), 54016 bytes (apply): two
// workgroups per CU.  The row strides in LDS are odd numbers of 32-bit words, so the lanes of a pass, which differ in their ROW, spread over the banks.
//
// Plain C++ on the TD_* macros, vector stores only; tests/emu runs this file unchanged.
#pragma once
#include "td_device.h"
#include "td_out.h"      // td_u8_run / td_u8_store / td_run_px / td_src_px4 / td_up_classes
#include "td_matte.h"    // MatteSet / td_matte_step / td_matte_byte: the gather kernel evaluates the matte entries' byte

#define TD_RF_MAX_RADIUS 16
#define TD_RF_MIN_EPS 4
#define TD_RF_MAX_EPS 65025
#define TD_RF_TX 64                                                    // a tile's columns
#define TD_RF_HRUN 16                                                  // columns of one lane's run in the row pass
#define TD_RF_CY 32                                                    // a tile's rows, the coefficient kernel
#define TD_RF_AY 16                                                    // ... the apply kernel: its staged planes are 6 bytes per pixel, not 2
#define TD_RF_HS (TD_RF_TX + 1)                                        // 32-bit words per row of the row sums

TD_HOSTDEV int td_rf_odd(int words) { return words | 1; }
// dynamic LDS of a workgroup, bytes (the launch and the kernels' carving agree through these)
TD_HOSTDEV size_t td_rf_coeff_lds(int r) {
    const int rows = TD_RF_CY + 2 * r, sbd = td_rf_odd((TD_RF_TX + 2 * r + 3) >> 2);
    return (size_t)rows * (2 * sbd + 3 * TD_RF_HS) * 4;
}
TD_HOSTDEV size_t td_rf_apply_lds(int r) {
    const int rows = TD_RF_AY + 2 * r, sw = TD_RF_TX + 2 * r, sad = td_rf_odd((sw + 1) >> 1), sbd = td_rf_odd(sw);
    return (size_t)rows * (sad + sbd + 2 * TD_RF_HS) * 4 + (size_t)TD_RF_AY * TD_RF_TX;
}

// f32() of the contract for |v| < 2^53: exact to double, then the one rounding
TD_DEV float td_rf_f32(long long v) { return (float)(double)v; }
// pixels of the window of coordinate c on an axis of n
TD_DEV int td_rf_span(int c, int n, int r) { return (c + r < n - 1 ? c + r : n - 1) - (c - r > 0 ? c - r : 0) + 1; }

// stage 1 of one pixel, from its window sums
TD_DEV void td_rf_coeff(unsigned sg, unsigned sm, unsigned sgg, unsigned sgm, int N, int eps, int* aq, int* bq) {
    const long long n = N;
    const long long cov = n * (long long)sgm - (long long)sg * (long long)sm;
    const long long den = n * (long long)sgg - (long long)sg * (long long)sg + (long long)eps * n * n;
    const float a = td_rf_f32(cov) / td_rf_f32(den);
    float t = rintf(a * 1024.f);
    t = t < -32767.f ? -32767.f : (t > 32767.f ? 32767.f : t);
    const int q = (int)t;
    *aq = q;
    *bq = (int)rintf(td_rf_f32(1024ll * (long long)sm - (long long)q * (long long)sg) / (float)(16 * N));
}
// stage 2 of one pixel
TD_DEV int td_rf_out(int A, int B, int g, int N) {
    const float t = rintf(td_rf_f32((long long)A * g + 16ll * (long long)B) / (float)(1024 * N));
    return t < 0.f ? 0 : (t > 255.f ? 255 : (int)t);
}

// Bytes gx .. gx + 3 of row gy of a byte map [h][w] (rows `pitch` bytes apart, any address) as one word, byte e in bits 8 e; 0 for a pixel outside the
// map.  One 4-byte load where the four lie in the row at an aligned address; only bytes of pixels are addressed, never the pitch padding.
TD_DEV unsigned td_rf_ld4(const unsigned char* p, size_t pitch, int gy, int gx, int h, int w) {
    if (gy < 0 || gy >= h || gx + 3 < 0 || gx >= w) return 0u;
    const unsigned char* row = p + (size_t)gy * pitch;
    if (gx >= 0 && gx + 3 < w && (((size_t)(row + gx)) & 3u) == 0) return *reinterpret_cast<const unsigned*>(row + gx);
    unsigned v = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int x = gx + e;
        if (x >= 0 && x < w) v |= (unsigned)row[x] << (8 * e);
    }
    return v;
}

// a_q (int16) and b_q (int32) planes [h][w], tight, of the guide G and the matte M.  grid = (ceil(w / 64), ceil(h / 32)), 256 lanes,
// td_rf_coeff_lds(r) bytes of LDS.
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 2) k_refine_coeff(const unsigned char* __restrict__ G, size_t gpitch, const unsigned char* __restrict__ M, size_t mpitch,
                                                       short* __restrict__ aq, int* __restrict__ bq, int h, int w, int r, int eps) {
    TD_DYN_LDS(lds);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TD_RF_TX, y0 = blockIdx.y * TD_RF_CY;
    const int rows = TD_RF_CY + 2 * r, ngrp = (TD_RF_TX + 2 * r + 3) >> 2, sbd = td_rf_odd(ngrp);
    unsigned* sG = reinterpret_cast<unsigned*>(lds);                   // [rows][sbd]: the staged guide bytes, 4 per word
    unsigned* sM = sG + rows * sbd;                                    // ... matte bytes
    unsigned* hP = sM + rows * sbd;                                    // [rows][TD_RF_HS]: a row's S_G | S_M << 16
    unsigned* hGG = hP + rows * TD_RF_HS;
    unsigned* hGM = hGG + rows * TD_RF_HS;
    // stage: 32 lanes along a row (ngrp <= 24 words), 8 rows at a time
    for (int sy = tid >> 5; sy < rows; sy += 8) {
        const int k = tid & 31;
        if (k < ngrp) {
            sG[sy * sbd + k] = td_rf_ld4(G, gpitch, y0 - r + sy, x0 - r + 4 * k, h, w);
            sM[sy * sbd + k] = td_rf_ld4(M, mpitch, y0 - r + sy, x0 - r + 4 * k, h, w);
        }
    }
    __syncthreads();
    // rows: lane = (staged row, run of 16 output columns); output column c of the tile sums the staged columns c .. c + 2 r
    for (int sy = (tid & 15) + 16 * (tid >> 6); sy < rows; sy += 64) {
        const unsigned char* g = reinterpret_cast<const unsigned char*>(sG + sy * sbd);
        const unsigned char* m = reinterpret_cast<const unsigned char*>(sM + sy * sbd);
        const int c0 = ((tid >> 4) & 3) * TD_RF_HRUN;
        // The products that ENTER and those that LEAVE are summed apart (ingg / ingm, outgg / outgm) and subtracted once per output.  Written as one
        // running sum, s += a b - a0 b0, hipcc (ROCm 7.2) gathers the byte products of two steps into one v_dot4_u32_u8 and ADDS the leaving product of
        // the first: every output behind a run's second was wrong on the device, none in the emulator.  Two sums of products only are what that
        // instruction computes.
        unsigned sg = 0u, sm = 0u, ingg = 0u, ingm = 0u, outgg = 0u, outgm = 0u;
        for (int j = 0; j <= 2 * r; ++j) {
            const unsigned a = g[c0 + j], b = m[c0 + j];
            sg += a; sm += b; ingg += a * a; ingm += a * b;
        }
        for (int i = 0;; ++i) {
            const int o = sy * TD_RF_HS + c0 + i;
            hP[o] = sg | (sm << 16);
            hGG[o] = ingg - outgg;
            hGM[o] = ingm - outgm;
            if (i == TD_RF_HRUN - 1) break;
            const unsigned a = g[c0 + i + 2 * r + 1], b = m[c0 + i + 2 * r + 1], a0 = g[c0 + i], b0 = m[c0 + i];
            sg += a; sg -= a0; sm += b; sm -= b0;
            ingg += a * a; ingm += a * b; outgg += a0 * a0; outgm += a0 * b0;
        }
    }
    __syncthreads();
    // columns: lane = (output column, run of 8 rows); output row j of the tile sums the staged rows j .. j + 2 r
    const int col = tid & 63, j0 = (tid >> 6) * (TD_RF_CY / 4), x = x0 + col;
    if (x < w && y0 + j0 < h) {
        unsigned sg = 0u, sm = 0u, sgg = 0u, sgm = 0u;
        for (int j = j0; j <= j0 + 2 * r; ++j) {
            const unsigned p = hP[j * TD_RF_HS + col];
            sg += p & 0xFFFFu; sm += p >> 16; sgg += hGG[j * TD_RF_HS + col]; sgm += hGM[j * TD_RF_HS + col];
        }
        const int nx = td_rf_span(x, w, r);
        for (int i = 0;; ++i) {
            const int y = y0 + j0 + i;
            int a, b;
            td_rf_coeff(sg, sm, sgg, sgm, nx * td_rf_span(y, h, r), eps, &a, &b);
            aq[(size_t)y * w + x] = (short)a;
            bq[(size_t)y * w + x] = b;
            if (i == TD_RF_CY / 4 - 1 || y + 1 >= h) break;
            const int ja = (j0 + i + 2 * r + 1) * TD_RF_HS + col, js = (j0 + i) * TD_RF_HS + col;
            const unsigned pa = hP[ja], ps = hP[js];
            sg += (pa & 0xFFFFu) - (ps & 0xFFFFu); sm += (pa >> 16) - (ps >> 16); sgg += hGG[ja] - hGG[js]; sgm += hGM[ja] - hGM[js];
        }
    }
}

// The refined bytes out [h][w] (rows opitch apart, any address) of the coefficient planes and the guide.  grid = (ceil(w / 64), ceil(h / 16)),
// 256 lanes, td_rf_apply_lds(r) bytes of LDS.  The tile's bytes meet in LDS, and a lane stores 4 of a row: one 4-byte store where they are a whole
// quad at an aligned address.
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 2) k_refine_apply(const unsigned char* __restrict__ G, size_t gpitch, const short* __restrict__ aq, const int* __restrict__ bq,
                                                       unsigned char* __restrict__ out, size_t opitch, int h, int w, int r) {
    TD_DYN_LDS(lds);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TD_RF_TX, y0 = blockIdx.y * TD_RF_AY;
    const int rows = TD_RF_AY + 2 * r, sw = TD_RF_TX + 2 * r, sad = td_rf_odd((sw + 1) >> 1), sbd = td_rf_odd(sw);
    int* sA32 = reinterpret_cast<int*>(lds);                           // [rows][sad] words = [rows][2 sad] int16: the staged a_q
    int* sB = sA32 + rows * sad;                                       // [rows][sbd]: the staged b_q
    int* hA = sB + rows * sbd;                                         // [rows][TD_RF_HS]: a row's sums
    int* hB = hA + rows * TD_RF_HS;
    unsigned char* ob = reinterpret_cast<unsigned char*>(hB + rows * TD_RF_HS);   // [TD_RF_AY][TD_RF_TX]: the tile's bytes
    short* sA = reinterpret_cast<short*>(sA32);
    // stage: 128 lanes along a row (sw <= 96), 2 rows at a time; 0 outside the map
    for (int sy = tid >> 7; sy < rows; sy += 2) {
        const int k = tid & 127, gy = y0 - r + sy, gx = x0 - r + k;
        if (k < sw) {
            const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
            sA[sy * 2 * sad + k] = in ? aq[(size_t)gy * w + gx] : (short)0;
            sB[sy * sbd + k] = in ? bq[(size_t)gy * w + gx] : 0;
        }
    }
    __syncthreads();
    for (int sy = (tid & 15) + 16 * (tid >> 6); sy < rows; sy += 64) {
        const short* a = sA + sy * 2 * sad;
        const int* b = sB + sy * sbd;
        const int c0 = ((tid >> 4) & 3) * TD_RF_HRUN;
        int sa = 0, sb = 0;
        for (int j = 0; j <= 2 * r; ++j) { sa += a[c0 + j]; sb += b[c0 + j]; }
        for (int i = 0;; ++i) {
            hA[sy * TD_RF_HS + c0 + i] = sa;
            hB[sy * TD_RF_HS + c0 + i] = sb;
            if (i == TD_RF_HRUN - 1) break;
            sa += a[c0 + i + 2 * r + 1] - a[c0 + i];
            sb += b[c0 + i + 2 * r + 1] - b[c0 + i];
        }
    }
    __syncthreads();
    const int col = tid & 63, j0 = (tid >> 6) * (TD_RF_AY / 4), x = x0 + col;
    if (x < w && y0 + j0 < h) {
        int sa = 0, sb = 0;
        for (int j = j0; j <= j0 + 2 * r; ++j) { sa += hA[j * TD_RF_HS + col]; sb += hB[j * TD_RF_HS + col]; }
        const int nx = td_rf_span(x, w, r);
        for (int i = 0;; ++i) {
            const int y = y0 + j0 + i;
            ob[(j0 + i) * TD_RF_TX + col] = (unsigned char)td_rf_out(sa, sb, (int)G[(size_t)y * gpitch + x], nx * td_rf_span(y, h, r));
            if (i == TD_RF_AY / 4 - 1 || y + 1 >= h) break;
            const int ja = (j0 + i + 2 * r + 1) * TD_RF_HS + col, js = (j0 + i) * TD_RF_HS + col;
            sa += hA[ja] - hA[js];
            sb += hB[ja] - hB[js];
        }
    }
    __syncthreads();
    // 256 lanes = 16 rows x 16 quads
    const int j = tid >> 4, c = (tid & 15) * 4, y = y0 + j, xq = x0 + c;
    if (y < h && xq < w) {
        unsigned char* p = out + (size_t)y * opitch + xq;
        const unsigned v = *reinterpret_cast<const unsigned*>(ob + j * TD_RF_TX + c);
        if (xq + 4 <= w && (((size_t)p) & 3u) == 0) *reinterpret_cast<unsigned*>(p) = v;
        else
            for (int e = 0; e < 4 && xq + e < w; ++e) p[e] = (unsigned char)(v >> (8 * e));
    }
}

// ---- the frame's end: guide and matte at the SOURCE's size ---------------------------------------------------------------------------------
// k_composite_rows' front half (td_matte.h): picture row y and 4 pixels per lane; the source pixel through td_src_px4, the matte byte of network pixel
// (ys[y], xs[x]) from td_up_classes + td_matte_step evaluated only there (the same operations on the same values as the matte entries: the same byte) or from
// a map [H][W] the caller holds.  Two tight byte planes [oh][ow] leave: luma Y = (77 R + 150 G + 29 B + 128) >> 8 of the converted, clamped pixel, and M_src.
// In the fused entries this IS the frame's last launch, in place of k_upsample_argmax_u8.  Both planes start at 4-byte aligned addresses of the handle's
// workspace, so one lane split (td_u8_run on the luma row) serves both rows.
struct GatherArgs {
    const float* in;               // low-resolution logits [C][h][w] (the fused form)
    const unsigned char* map;      // uint8 matte map [H][W] (the map form)
    const int* ys; const int* xs;  // [oh], [ow]: the sampled network pixel of a source row / column
    int C, h, w, H, W, oh, ow;
    int swap;                      // the source word's bytes are b g r
    unsigned char* luma; unsigned char* msrc;
    MatteSet set;
};
template <bool FROM_MAP, int SRC>
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 5) k_refine_gather(GatherArgs a, const unsigned char* src, SrcLayout l) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= a.oh) return;
    unsigned char* lrow = a.luma + (size_t)y * a.ow;
    unsigned char* mrow = a.msrc + (size_t)y * a.ow;
    long xa, xb;
    td_u8_run(lrow, q, a.ow, &xa, &xb);
    if (xa >= xb) return;
    int M[4];
    if (FROM_MAP) {
        const unsigned char* r = a.map + (size_t)a.ys[y] * a.W;
#pragma unroll
        for (int e = 0; e < 4; ++e) M[e] = r[a.xs[td_run_px(xa, e, a.ow)]];
    } else {
        MatteAcc acc;
        td_up_classes(a.in, a.C, a.h, a.w, a.H, a.W, a.ys[y], [&](int e) { return a.xs[td_run_px(xa, e, a.ow)]; },
                      [&](int c, int e, float v) { td_matte_step(acc, c, e, v, td_matte_member(a.set, c)); });
#pragma unroll
        for (int e = 0; e < 4; ++e) M[e] = td_matte_byte(acc.num[e], acc.den[e]);
    }
    unsigned s[4];
    td_src_px4<SRC>(src, l, y, xa, a.ow, xb - xa == 4, s);
    int Y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c0 = (int)(s[e] & 255u), c1 = (int)((s[e] >> 8) & 255u), c2 = (int)((s[e] >> 16) & 255u);
        Y[e] = (77 * (a.swap ? c2 : c0) + 150 * c1 + 29 * (a.swap ? c0 : c2) + 128) >> 8;
    }
    td_u8_store(lrow, xa, xb, Y);
    td_u8_store(mrow, xa, xb, M);
}
