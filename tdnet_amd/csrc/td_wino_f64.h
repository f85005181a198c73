// td_wino_f64.h -- ResNet layer1's 3x3 conv (64 -> 64 channels, stride 1, dilation 1, fp32) as ONE fused Winograd F(4x4,3x3) kernel.
//
// The unfused route (td_wino.h: input transform -> 36 GEMMs -> output transform) writes and reads V and M through HBM: 2.25x the map each, about
// 400 MB for a conv whose map is 33.5 MB -- as slow as the direct kernel's four times as many MACs.  Here V and M never leave the CU:
//
//   workgroup = 256 threads (4 waves) = a block of 32 tiles, 8 wide x 4 high (32 x 16 output pixels), x 32 output channels (blockIdx.y = channel half)
//   (a) per 16-channel chunk of Cin: thread (tile, 2 channels) loads its 6x6 patch (taps outside the image: zeros by the buffer range check, as in
//       k_wino4_in), applies B^T . B and writes 36 values per channel to LDS as V[36 positions][8 k-steps][2 halves][32 tiles].  The lanes run over the
//       CHANNEL PAIRS first (8 lanes = the chunk's 64 bytes of a pixel) and the tile index is XOR-swizzled (td_wf64_vidx), so the stores and the MFMA's
//       A reads (lane & 31 = tile, lane >> 5 = half) both stay on 32 different banks
//   (b) wave w owns positions 9 w .. 9 w + 8: per position and chunk 8 td_mfma32 (32 tiles x 32 channels x 2 k), A one LDS dword, B = the transformed
//       weights U[position][k][cout] straight from global memory / L2 (590 KB for the layer), packed on the host so that one 16-byte load per lane
//       feeds four consecutive k-steps (wino_f64_pack).  Nine f32x16 accumulators persist across the four chunks; the MFMAs go round-robin over them.
//   (c) the 36 positions of one (tile, channel) sit in four waves: they are exchanged through the same LDS in two rounds, M[36][32 channels][16 tiles]
//       each (the tile index XOR-swizzled by the channel: the accumulator layout's writes and the readers' reads are both conflict-free); thread
//       (tile, 2 channels) applies A^T . A, adds bias and residual, activates and stores; pixels outside the map are dropped by the range check.
//       A round is 16 TILES x all 32 channels, not 16 channels x all tiles: a lane's accumulator registers 0 .. 7 are the block's upper 16 tiles, so
//       half of the 144 accumulator registers are dead after the first round's write -- with rounds over channels all of them stay live through the
//       first output transform, and the kernel spills (two workgroups per CU = 256 registers per wave).
//       The residual may be the output buffer (a BasicBlock's conv2 in place): a thread reads exactly what it overwrites.
//
// Arithmetic: the transforms are td_wino4_bt_t / td_wino4_at_t in k_wino4_in's / k_wino4_out's operation order, and the sum over Cin is one fp32 fma chain
// in the persistent GEMMs' order (wino_f64_pack) -- the unfused route's bits.  Fixed order, no atomics: two runs are bit-identical.
// Only td_device.h primitives: the emulator (tests/emu) runs this file unchanged.
#pragma once
#include "td_wino.h"

constexpr int TD_WF64_C = 64;                                          // Cin = Cout
constexpr int TD_WF64_BX = 8, TD_WF64_BY = 4;                          // tiles of a block
constexpr int TD_WF64_LDS = 36 * 8 * 2 * 32 * 4;                       // bytes: the V image of a chunk = the M image of a round (73 728: two workgroups per CU)
// The smallest output map (pixels) plan_conv gives to this kernel: the smallest of the measured sizes (256x512, 193x385, 128x256) at which it beats the
// direct kernel by more than 5 % in isolation (tools/wino_f64_probe.py, profiles/wino_f64_probe.txt), and never below 16 384 -- the goldens, the
// emulator's frame tests and opcheck's small shapes keep the direct kernel.
constexpr long TD_WINO_F64_MIN_PIXELS = 32768;

struct WinoF64Args {
    const float* in;      // [H][W][64]
    const float* up;      // packed U (wino_f64_pack)
    const float* bias;    // [64]
    const float* resid;   // [H][W][64] or nullptr (may be `out`)
    float* out;           // [H][W][64]
    int H, W, BXN, act;   // BXN: blocks per block row
};

// everything about a conv but its size: what the kernel computes (plan_conv adds the options and the size rule)
static inline bool wino_f64_supports(int Cout, int Cin, int KS, int stride, int dil, int act, bool stem) {
    return !stem && KS == 3 && stride == 1 && dil == 1 && Cin == TD_WF64_C && Cout == TD_WF64_C && (act == 0 || act == 1);
}
// 32-bit byte offsets below TD_BUF_OOB
constexpr long TD_WINO_F64_MAX_PIXELS = (1l << 31) / (TD_WF64_C * 4) - 1;   // 8 388 607: plan_conv's upper bound, so that planning and the launch cannot disagree
static inline bool wino_f64_size_ok(int H, int W) { return H >= 1 && W >= 1 && (long)H * W <= TD_WINO_F64_MAX_PIXELS; }
constexpr int TD_WF64_PACKED_FLOATS = 2 * 36 * 8 * 64 * 4;            // [channel half][position][k-quad][lane][4]
static inline size_t wino_f64_packed_floats() { return (size_t)TD_WF64_PACKED_FLOATS; }
// U = G g G^T (fp64, rounded once: wino_transform_weights) in the B-fragment order of phase (b):
//   p[(((hb * 36 + pos) * 8 + kq) * 64 + lane) * 4 + j] = U[pos][cout = 32 hb + (lane & 31)][cin = 8 kq + 4 (lane >> 5) + j]
// k-step 4 kq + j multiplies the channels 8 kq + j (lane half 0) and 8 kq + 4 + j (half 1): the k-permutation and the one fma chain of the persistent
// GEMMs (td_conv.h: "inside a group of 8 k the two lane-halves take k = 4*half + s"), so M -- and with the shared transform arithmetic the conv --
// has the bits of the unfused route.
static inline void wino_f64_pack(const float* w, float* p) {
    std::vector<std::vector<float>> U;
    wino_transform_weights(w, TD_WF64_C, TD_WF64_C, 4, U);
    for (int hb = 0; hb < 2; ++hb)
        for (int pos = 0; pos < 36; ++pos)
            for (int kq = 0; kq < 8; ++kq)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j)
                        p[((((size_t)hb * 36 + pos) * 8 + kq) * 64 + lane) * 4 + j] =
                            U[pos][(size_t)(32 * hb + (lane & 31)) * TD_WF64_C + 8 * kq + 4 * (lane >> 5) + j];
}

// The LDS images.  In the transform phases a thread's lanes run over the CHANNELS first (8 lanes = 64 contiguous bytes of a pixel on the way in, 16 lanes =
// 128 bytes on the way out: with the lanes over the tiles every 8-byte access was a cache line of its own, and the kernel was bound by the vector-memory
// path's address rate, 69.8 us at 256 x 512), so the tile index is XOR-swizzled to keep every LDS access of a 32-lane group on 32 different banks of the 64:
//   V[pos][slot = 2 k-step + half][tile ^ 4 ((slot >> 2) & 3)]: a writer group is 8 channel pairs x 4 tiles -- the four pairs whose slots share a parity
//     differ in slot >> 2; the MFMA's A read is one slot x 32 tiles: a permutation.  slot >> 2 = k-step >> 1 for either half.
//   M[pos][channel j of the 32][tile t of the round's 16 ^ 2 (j >> 2)]: a writer group holds, per accumulator register, 32 channels x one tile:
//     16 (j & 3) + (t ^ 2 (j >> 2)); a reader group 16 channel pairs x 2 tiles: the pairs with equal j & 3 differ in j >> 2, the tiles in bit 0.
TD_DEV int td_wf64_vidx(int pos, int slot, int tile) { return pos * 512 + slot * 32 + (tile ^ (4 * ((slot >> 2) & 3))); }
TD_DEV int td_wf64_midx(int pos, int j, int t) { return pos * 512 + j * 16 + (t ^ (2 * (j >> 2))); }

TD_KERNEL void TD_LAUNCH_BOUNDS(256, 2) k_wino4_f64(WinoF64Args p) {
    TD_DYN_LDS(smem);
    float* lds = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = TD_UNIFORM(tid >> 6);
    const int bx = (int)blockIdx.x % p.BXN, by = (int)blockIdx.x / p.BXN, hb = (int)blockIdx.y;
    const unsigned map_bytes = (unsigned)p.H * (unsigned)p.W * (unsigned)TD_WF64_C * 4u;
    const TdBuf inb = td_make_buf(p.in, map_bytes);
    const TdBuf ub = td_make_buf(p.up, (unsigned)TD_WF64_PACKED_FLOATS * 4u);
    const TdBuf rb = td_make_buf(p.resid, p.resid ? map_bytes : 0u);
    const TdBuf ob = td_make_buf(p.out, map_bytes);
    // Two workgroups per CU leave a wave 256 registers, and 144 of them are the accumulators: what a phase needs is derived from `tid` where the phase
    // begins (TD_PIN: not hoisted out of the chunk loop), not carried through the MFMAs.
    f32x16 acc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const unsigned ulane = (unsigned)lane * 16u;
    const unsigned ubase = (unsigned)((hb * 36 + wave * 9) * 8) * 1024u;   // this wave's first position, k-quad 0
    const float* va[4];                                               // A operand of position 9 w, k-steps 2 g and 2 g + 1 (one swizzle per pair)
#pragma unroll
    for (int g = 0; g < 4; ++g) va[g] = lds + td_wf64_vidx(wave * 9, 4 * g + (lane >> 5), lane & 31);

#pragma unroll 1
    for (int kc = 0; kc < 4; ++kc) {
        // ---- (a) B^T d B of 2 channels -> LDS.  All 36 taps are requested at once; the other workgroup of the CU multiplies meanwhile.
        int t = tid;
        TD_PIN(t);
        const int tl = t >> 3, cp = t & 7;                            // this thread's tile of the block and channel pair of the chunk
        const int tx = bx * TD_WF64_BX + (tl & 7), ty = by * TD_WF64_BY + (tl >> 3);
        // byte offset of a tap = offy[r] + offx[c], each term TD_BUF_OOB outside the image, added with saturation (k_wino4_in)
        unsigned offy[6], offx[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int y = 4 * ty - 1 + r, x = 4 * tx - 1 + r;
            offy[r] = (unsigned)y < (unsigned)p.H ? (unsigned)y * (unsigned)p.W * (unsigned)(TD_WF64_C * 4) : TD_BUF_OOB;
            offx[r] = (unsigned)x < (unsigned)p.W ? (unsigned)x * (unsigned)(TD_WF64_C * 4) + (unsigned)(16 * kc + 2 * cp) * 4u : TD_BUF_OOB;
        }
        f32x2 dd[6][6];                                               // [c][r]
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) dd[c][r] = td_buf_ld2(inb, __builtin_elementwise_add_sat(offy[r], offx[c]), 0u);
        f32x2 tm[6][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            f32x2 col[6];
            td_wino4_bt_t(dd[c], col);                                // B^T d, one column
#pragma unroll
            for (int r = 0; r < 6; ++r) tm[r][c] = col[r];
        }
        if (kc) __syncthreads();                                      // the previous chunk's A reads are done
        // where the channels 2 cp, 2 cp + 1 of a chunk sit in a position's V image: channel c is k-step 4 (c >> 3) + (c & 3), half (c >> 2) & 1
        float* vd = lds + td_wf64_vidx(0, (4 * (cp >> 2) + ((2 * cp) & 3)) * 2 + ((cp >> 1) & 1), tl);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            f32x2 v[6];
            td_wino4_bt_t(tm[r], v);                                  // (.) B, one row
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                vd[(r * 6 + c) * 512] = v[c][0];
                vd[(r * 6 + c) * 512 + 64] = v[c][1];                 // the next channel: the next k-step, same half, same swizzle
            }
        }
        // this chunk's weights: the first k-quad in flight across the barrier, the second under the first's MFMAs
        f32x4 b0[9], b1[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) b0[q] = td_buf_ld4(ub, ulane, ubase + (unsigned)((q * 8 + 2 * kc) * 1024));
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 9; ++q) b1[q] = td_buf_ld4(ub, ulane, ubase + (unsigned)((q * 8 + 2 * kc + 1) * 1024));
        // ---- (b) 9 positions x 8 k-steps, round-robin over the positions
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 9; ++q) acc[q] = td_mfma32(va[j >> 1][q * 512 + (j & 1) * 64], b0[q][j], acc[q]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 9; ++q) acc[q] = td_mfma32(va[2 + (j >> 1)][q * 512 + (j & 1) * 64], b1[q][j], acc[q]);
    }

    // ---- (c) M through LDS in two rounds: the upper 16 tiles of the block (accumulator registers 0 .. 7), then the lower 16 (8 .. 15), all 32 channels each,
    // so that half of the accumulators are dead once the first round is written.  thread = (tile of the round, 2 channels).
    const int tl = tid >> 4, cpp = tid & 15;
    const TdBuf bb = td_make_buf(p.bias, (unsigned)(TD_WF64_C * 4));
    const f32x2 b = td_buf_ld2(bb, (unsigned)(32 * hb + 2 * cpp) * 4u, 0u);
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
        const int tx = bx * TD_WF64_BX + (tl & 7), ty = by * TD_WF64_BY + 2 * rd + (tl >> 3);
        unsigned offy[4], offx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = 4 * ty + r, x = 4 * tx + r;
            offy[r] = y < p.H ? (unsigned)y * (unsigned)p.W * (unsigned)(TD_WF64_C * 4) : TD_BUF_OOB;
            offx[r] = x < p.W ? (unsigned)x * (unsigned)(TD_WF64_C * 4) + (unsigned)(32 * hb + 2 * cpp) * 4u : TD_BUF_OOB;
        }
        f32x2 o[16];                                                  // the residual first: in flight across the barriers
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) o[r * 4 + c] = td_buf_ld2(rb, __builtin_elementwise_add_sat(offy[r], offx[c]), 0u);
        __syncthreads();                                              // the last chunk's A reads / the first round's M reads are done
        {
            // accumulator register r of lane l: tile (r & 3) + 8 (r >> 2) + 4 (l >> 5), channel l & 31; registers 8 rd .. 8 rd + 7 are the round's 16 tiles
            const int j = lane & 31, i4 = 4 * (lane >> 5);
#pragma unroll
            for (int q = 0; q < 9; ++q)
#pragma unroll
                for (int r = 0; r < 8; ++r) lds[td_wf64_midx(wave * 9 + q, j, (r & 3) + 8 * (r >> 2) + i4)] = acc[q][8 * rd + r];
        }
        __syncthreads();
        f32x2 sm[4][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {                                 // a column at a time
            f32x2 mc[6], col[4];
#pragma unroll
            for (int r = 0; r < 6; ++r) mc[r] = f32x2{lds[td_wf64_midx(r * 6 + c, 2 * cpp, tl)], lds[td_wf64_midx(r * 6 + c, 2 * cpp + 1, tl)]};
            td_wino4_at_t(mc, col);                                   // A^T m, one column
#pragma unroll
            for (int r = 0; r < 4; ++r) sm[r][c] = col[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            f32x2 o4[4];
            td_wino4_at_t(sm[r], o4);                                 // (.) A, one row
#pragma unroll
            for (int c = 0; c < 4; ++c) o[r * 4 + c] = (o4[c] + b) + o[r * 4 + c];
        }
        td_wino_activate<false>(o, p.act);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) td_buf_st2(ob, __builtin_elementwise_add_sat(offy[r], offx[c]), 0u, o[r * 4 + c]);
    }
}

// false, nothing launched: the map is outside the kernel's 32-bit byte offsets
static inline bool wino_f64_launch(const float* in, const float* up, const float* bias, const float* resid, float* out, int H, int W, int act, hipStream_t s) {
    if (!wino_f64_size_ok(H, W)) return false;
    const int TX = wino_tiles_1d(W, 1, 4), TY = wino_tiles_1d(H, 1, 4);
    const int bxn = (TX + TD_WF64_BX - 1) / TD_WF64_BX, byn = (TY + TD_WF64_BY - 1) / TD_WF64_BY;
    const WinoF64Args a = {in, up, bias, resid, out, H, W, bxn, act};
    TD_LAUNCH(k_wino4_f64, dim3((unsigned)(bxn * byn), 2), dim3(256), TD_WF64_LDS, s, a);
    return true;
}
