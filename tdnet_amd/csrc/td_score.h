// td_score.h -- score out: the confusion matrix of a frame's labels against ground truth, counted on the device.
//
// What the reference's validation loop does on the host behind the labels (Training/validate.py:59-70, Training/ptsemseg/metrics.py:12-21):
// mask = (gt >= 0) & (gt < n_class), hist += bincount(n_class * gt[mask] + pred[mask]).reshape(n_class, n_class).  Here the frame's LAST kernel
// counts instead of (or beside) writing the label map: cm[g][l] += 1 for every pixel with g = map[gt[Y][X]] < nclass, l the label
// k_upsample_argmax_u8 gives for that pixel.  The counts are integers: the result does not depend on the order of the additions.
//
// Accumulation: while nclass * nclass bins fit TD_SCORE_LDS_CLASSES squared (16 KiB of LDS) every workgroup keeps a private uint32 histogram
// in LDS (a workgroup sees at most 256 lanes x 4 pixels = 1024 pixels: 32 bits cannot overflow), zeroed before the pixels and flushed after a
// __syncthreads(): the non-zero bins only, one 64-bit atomic add per bin into the handle's unsigned long long [nclass][nclass].  Above
// that (up to 256 classes, 65536 bins) the lanes add straight into the global matrix.  A lane merges equal keys among its own 4 pixels first.
// Wave-uniform path (template parameter; which instantiation the library's entries launch: td_launch.h TD_SCORE_WAVE_UNIFORM): labels and
// ground truth are spatially coherent, and 64 lanes adding to ONE LDS address serialise; when every counted pixel of the wave has the same
// key, lane 0 adds the wave's count once.
//
// Written on the TD_* macros only (tests/emu runs this file unchanged); the three wrappers below are the only build-dependent lines, and
// there is no inline assembly here: LDS atomics, 64-bit atomicAdd and ordinary vector stores from plain C++.
#pragma once
#include "td_device.h"
#include "td_out.h"      // td_up_classes / td_first_max / td_u8_run / td_u8_store

#define TD_SCORE_LDS_CLASSES 64                                        // private LDS histogram up to 64 x 64 x 4 bytes = 16 KiB per workgroup
#define TD_SCORE_NONE 0xffffffffu                                      // key of a pixel that is not counted

// One LDS bin += v.  The emulator runs the fibers of a workgroup on one OS thread: a plain add is atomic there.
TD_DEV void td_score_lds_add(unsigned* bin, unsigned v) {
#ifdef TD_EMU
    *bin += v;
#else
    atomicAdd(bin, v);
#endif
}
// One bin of the global matrix += v.  The emulator runs workgroups on several OS threads: a real atomic there too.
TD_DEV void td_score_global_add(unsigned long long* bin, unsigned long long v) {
#ifdef TD_EMU
    __atomic_fetch_add(bin, v, __ATOMIC_RELAXED);
#else
    atomicAdd(bin, v);
#endif
}
// Wave-collective helpers of the wave-uniform path (every lane of the wave calls them).  td_score_some_key: the key of ONE lane that has one
// (the lowest such lane on the device, the smallest such key in the emulator -- it is only ever compared for "all equal", which comes out the
// same), TD_SCORE_NONE if no lane has.  td_score_wave_sum: the sum over the wave of a per-lane count in 0..4.
TD_DEV unsigned td_score_some_key(bool has, unsigned key) {
#ifdef TD_EMU
    float f = has ? (float)key : 16777216.f;                           // keys are below 65536: exact in fp32
    for (int m = 1; m < 64; m <<= 1) { const float o = td_shfl_xor(f, m); f = o < f ? o : f; }
    return f == 16777216.f ? TD_SCORE_NONE : (unsigned)f;
#else
    const unsigned long long m = __builtin_amdgcn_ballot_w64(has);
    if (m == 0ull) return TD_SCORE_NONE;
    return (unsigned)__builtin_amdgcn_readlane((int)key, __builtin_ctzll(m));
#endif
}
TD_DEV unsigned td_score_wave_sum(unsigned n) {
#ifdef TD_EMU
    float f = (float)n;
    for (int m = 1; m < 64; m <<= 1) f += td_shfl_xor(f, m);
    return (unsigned)f;
#else
    return (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64((n & 1u) != 0)) + 2u * (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64((n & 2u) != 0)) +
           4u * (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64((n & 4u) != 0));
#endif
}

TD_DEV void td_score_add(unsigned* hist, unsigned long long* cm, unsigned key, unsigned v) {
    if (hist) td_score_lds_add(hist + key, v);
    else td_score_global_add(cm + key, (unsigned long long)v);
}
// Count a lane's (up to) 4 keys: hist != NULL the workgroup's LDS histogram, else the global matrix.  Every lane of the workgroup comes here,
// lanes without pixels with four TD_SCORE_NONE (the wave-uniform test is a wave collective).
template <bool UNIFORM>
TD_DEV void td_score_count(unsigned* hist, unsigned long long* cm, const unsigned* key) {
    unsigned k[4] = {key[0], key[1], key[2], key[3]}, n[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) n[e] = k[e] != TD_SCORE_NONE ? 1u : 0u;
#pragma unroll
    for (int e = 1; e < 4; ++e)                                        // merge equal keys into the first pixel that has them
#pragma unroll
        for (int f = 0; f < e; ++f)
            if (n[e] && n[f] && k[e] == k[f]) { n[f] += n[e]; n[e] = 0; }
    if (UNIFORM) {
        unsigned first = TD_SCORE_NONE, total = 0, kinds = 0;
#pragma unroll
        for (int e = 3; e >= 0; --e)
            if (n[e]) { first = k[e]; total += n[e]; ++kinds; }
        const unsigned wave_key = td_score_some_key(kinds != 0, first);
        if (!td_any(kinds > 1 || (kinds == 1 && first != wave_key))) {  // wave-uniform: every counted pixel of the wave has wave_key
            const unsigned wave_total = td_score_wave_sum(total);
            if (td_lane() == 0 && wave_total) td_score_add(hist, cm, wave_key, wave_total);
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (n[e]) td_score_add(hist, cm, k[e], n[e]);
}
// The workgroup's histogram: hist[0 .. bins) zeroed by all lanes / its non-zero bins added to the global matrix (bins == 0: nothing to do)
TD_DEV void td_score_zero(unsigned* hist, int bins) {
    for (int i = threadIdx.x; i < bins; i += blockDim.x) hist[i] = 0u;
    if (bins) __syncthreads();
}
TD_DEV void td_score_flush(const unsigned* hist, int bins, unsigned long long* cm) {
    if (bins) __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
        const unsigned v = hist[i];
        if (v) td_score_global_add(cm + i, (unsigned long long)v);
    }
}

// The frame's last launch when a score is asked for: the output stage's body (td_out.h td_up_classes), first-maximum rule, k_upsample_argmax_u8's
// grid and (labels != NULL) store -- the label under every pixel is the number the label entries give -- and cm[map[gt]][label] += 1 where
// map[gt] < C.  gt: [H][W] bytes at ANY byte address, read byte by byte (its rows need not share the label rows' alignment).  map: 256 bytes.
// lds_bins: C * C (private LDS histogram of that many uint32, the launch's dynamic LDS) or 0 (straight into cm).
// grid = (ceil((W / 4 + 2) / 256), H); no lane leaves before the flush: the barriers and the wave test need all of them.
template <bool UNIFORM>
TD_KERNEL void k_upsample_argmax_score(const float* __restrict__ in, const unsigned char* __restrict__ gt, const unsigned char* __restrict__ map,
                                       unsigned char* __restrict__ labels, unsigned long long* __restrict__ cm, int C, int h, int w, int H, int W, int lds_bins) {
    TD_DYN_LDS(smem);
    unsigned* hist = lds_bins ? reinterpret_cast<unsigned*>(smem) : nullptr;
    td_score_zero(hist, lds_bins);
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    // the lanes' runs follow the LABEL rows' alignment whether or not the map is written: the same split as k_upsample_argmax_u8
    const unsigned char* arow = reinterpret_cast<const unsigned char*>((size_t)labels + (size_t)Y * W);
    long xa, xb;
    td_u8_run(arow, q, W, &xa, &xb);
    unsigned key[4] = {TD_SCORE_NONE, TD_SCORE_NONE, TD_SCORE_NONE, TD_SCORE_NONE};
    if (xa < xb) {
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int bi[4] = {0, 0, 0, 0};
        td_up_classes(in, C, h, w, H, W, Y, [&](int e) { return (int)td_run_px(xa, e, W); }, [&](int c, int e, float v) { td_first_max(c, v, best[e], bi[e]); });
        if (labels) td_u8_store(labels + (size_t)Y * W, xa, xb, bi);
        const unsigned char* grow = gt + (size_t)Y * W;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (xa + e < xb) {
                const unsigned g = map[grow[xa + e]];
                if (g < (unsigned)C) key[e] = g * (unsigned)C + (unsigned)bi[e];
            }
    }
    td_score_count<UNIFORM>(hist, cm, key);
    td_score_flush(hist, lds_bins, cm);
}
// The same counts from a uint8 label map [H][W] the caller already holds (the unfused form).  A label >= C has no column in the matrix:
// such a pixel is not counted.  The labels are read as one aligned 4-byte word where the row address allows, gt byte by byte.
template <bool UNIFORM>
TD_KERNEL void k_labels_score(const unsigned char* __restrict__ labels, const unsigned char* __restrict__ gt, const unsigned char* __restrict__ map,
                              unsigned long long* __restrict__ cm, int C, int W, int lds_bins) {
    TD_DYN_LDS(smem);
    unsigned* hist = lds_bins ? reinterpret_cast<unsigned*>(smem) : nullptr;
    td_score_zero(hist, lds_bins);
    const int q = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
    const unsigned char* lrow = labels + (size_t)Y * W;
    long xa, xb;
    td_u8_run(lrow, q, W, &xa, &xb);
    unsigned key[4] = {TD_SCORE_NONE, TD_SCORE_NONE, TD_SCORE_NONE, TD_SCORE_NONE};
    if (xa < xb) {
        unsigned l[4] = {0u, 0u, 0u, 0u};
        if (q > 0 && xb - xa == 4) {
            const unsigned v = *reinterpret_cast<const unsigned*>(lrow + xa);
            l[0] = v & 255u; l[1] = (v >> 8) & 255u; l[2] = (v >> 16) & 255u; l[3] = v >> 24;
        } else {
            for (long X = xa; X < xb; ++X) l[X - xa] = lrow[X];
        }
        const unsigned char* grow = gt + (size_t)Y * W;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (xa + e < xb) {
                const unsigned g = map[grow[xa + e]];
                if (g < (unsigned)C && l[e] < (unsigned)C) key[e] = g * (unsigned)C + l[e];
            }
    }
    td_score_count<UNIFORM>(hist, cm, key);
    td_score_flush(hist, lds_bins, cm);
}
