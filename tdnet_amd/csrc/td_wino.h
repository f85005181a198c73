// td_wino.h -- Winograd F(4x4, 3x3) for the stride-1 dilated 3x3 convolutions of layers 2-4 and the head (fp32).
//
// Y = A^T [ sum_ci (G g G^T) (.) (B^T d B) ] A  turns every m x m output tile into (m+2)^2 products per (ci, co) instead of
// 9 m^2: 36 instead of 144 for m = 4 (4x fewer MACs).  The contraction becomes 36 independent [tiles x Cin] x [Cin x Cout] GEMMs on the
// persistent fp32-MFMA GEMM (td_gemm.h / td_gemm_dma.h, nbatch = 36); the input/output transforms are HBM-bound passes over
// V = [36][T][Cin] and M = [36][T][Cout], 2.25x the size of the activation.  (F(2x2): 16 products instead of 36, 4x the activation in
// V / M -- rounds 1-4 carried it as tdnet_opts.winograd = 1 / 2; nothing routed to it since round 2 and it was removed in round 5,
// last commit 78dfa5a.  Its numerics are still on record: tests/numerics_winograd.py)
//
// A conv with dilation d (resnet.py:32-37: 2, 4, 8, 16 here) is d*d independent dilation-1 convs on the sub-grids
// {(py + d a, px + d b)}: a tile is (phase py, px; tile ty, tx) and its 4x4 input patch is read with stride d.
//   tile index t = ((py*d + px) * TY + ty) * TX + tx,  TY = ceil(ceil(H/d)/m), TX = ceil(ceil(W/d)/m)
// so all phases have the same tile count (out-of-range taps read zeros, out-of-range outputs are not written).
//
// Numerics: fp32 throughout (weights G g G^T are formed in fp64 on the host and rounded once).  Per conv the rms error vs fp64
// is 2.5x (F2) / 16x (F4, interpolation points 0, +-1, +-2) that of a direct fp32 conv; END TO END (td4 pipeline, CPU experiment
// tests/numerics_winograd.py) max|dlogit| vs fp64 is 1.2e-5 direct, 1.2e-5 F2, 2.6e-5 F4 -- BN, ReLU and the plane LayerNorm
// do not amplify it -- against a parity gate of 1e-3.
#pragma once
#include "td_conv.h"

#include <vector>

struct WinoArgs {
    const float* in;      // [H][W][C]
    float* V;             // [16][T][C]
    const float* Mb;      // [16][T][Cout]
    const float* bias;    // [Cout]
    const float* resid;   // [H][W][Cout] or nullptr
    float* out;           // [H][W][Cout]
    int H, W, C, Cout, dil, TY, TX, T, act;
    // Rows per plane of V / M INCLUDING padding rows (>= T).  T*C*4 is a power of two for the frame's layers (4 MiB at 512 channels),
    // so 36 unpadded planes put the 36 concurrent streams of a transform on the same HBM channels; TP = T + pad de-phases them.
    int TP;
    // Optional plane-LayerNorm fused into the INPUT transform (the FCN head reads LayerNorm(feat), td4_psp18.py:151,306-312): the
    // patch element at pixel p, channel c becomes (x - ln_mean[c]) * ln_rstd[c] * ln_g[p] + ln_b[p] -- the arithmetic of k_ln_apply,
    // same operation order, so fused and unfused results are bit-identical -- and stays 0 outside the image (the conv's zero padding
    // applies to the normalised map).  ln_mean == nullptr: off.
    const float* ln_mean; const float* ln_rstd; const float* ln_g; const float* ln_b;
    // Chunked transforms (k_wino4_in_c / k_wino4_out_c): a launch covers the Tc tiles whose phase row is py = ny * i + cy and whose
    // phase column is px = nx * j + cx (i < dil / ny, j < dil / nx); V / Mb then hold ONLY those tiles ([36][TP][C], TP >= Tc).  With
    // an even dilation and ny = 2 the two chunks are the even and the odd image rows: a dilated conv maps a row parity onto itself,
    // so through a run of even-dilation convs the two chunks are independent chains (td_frame.h run_parity_chains).
    int Tc, ny, cy, nx, cx;
    int pw;               // dil / nx: phase columns of the chunk
    // wino_magic() of the chunked kernels' wave-uniform divisors: channel slices of THIS launch, TX, TY, dil / nx
    unsigned long long mg_sl, mg_tx, mg_ty, mg_pw;
};
// n / d as a multiplication, exact for n < 2^24 and d < 2^16 (m d = 2^40 + e with 0 < e <= d, and n e < 2^40).  The GPU has no scalar integer
// division: the five divisions of a wave's tile decode were 25 VALU instructions and 6 v_readfirstlane; this is a handful of scalar ones.
static inline unsigned long long wino_magic(int d) { return (1ull << 40) / (unsigned long long)d + 1ull; }
static inline bool wino_magic_ok(long n, int d) { return n < (1l << 24) && d > 0 && d < (1 << 16); }
TD_DEV int td_w_div(int n, unsigned long long m) { return (int)(((unsigned long long)(unsigned)n * m) >> 40); }
// Buffer descriptors of a transform: every access is an UNCONDITIONAL range-checked buffer access (a tap outside the image, an output
// pixel outside the map or a missing residual turn into an out-of-range offset / a zero-record descriptor) -- no branch around any
// load or store, so all loads of a thread are in flight together and the waits are exact counts.  With `if (inside) load` /
// `if (resid) load ... store` the residual of the output transform was one load, one wait and one store sixteen times over.
struct WinoBufs { TdBuf in, g, b, resid, out; };
TD_DEV WinoBufs td_wino_bufs(const WinoArgs& p) {
    WinoBufs w;
    const unsigned pix = (unsigned)p.H * (unsigned)p.W;
    w.in = td_make_buf(p.in, pix * (unsigned)p.C * 4u);
    w.g = td_make_buf(p.ln_g, p.ln_mean ? pix * 4u : 0u);
    w.b = td_make_buf(p.ln_b, p.ln_mean ? pix * 4u : 0u);
    w.resid = td_make_buf(p.resid, p.resid ? pix * (unsigned)p.Cout * 4u : 0u);
    w.out = td_make_buf(p.out, pix * (unsigned)p.Cout * 4u);
    return w;
}
// ---- the transform arithmetic: ONE definition for every kernel of this file -----------------------------------------------
// A lane computes on float (1 channel), f32x2 (2) or f32x2p (4 channels as TWO packed halves).  gfx950 has packed fp32 add / mul / fma
// on register PAIRS (v_pk_*_f32) and nothing wider: a 4-wide expression is split by the compiler, and it splits the subtractions into
// four single-lane v_sub_f32 instead of two v_pk_add_f32 (528 of k_wino4_in_c<4>'s instructions were that).  On halves every operation
// is one packed instruction per pair.
struct f32x2p { f32x2 lo, hi; };
TD_DEV f32x2p operator+(f32x2p a, f32x2p b) { return f32x2p{a.lo + b.lo, a.hi + b.hi}; }
TD_DEV f32x2p operator-(f32x2p a, f32x2p b) { return f32x2p{a.lo - b.lo, a.hi - b.hi}; }
TD_DEV f32x2p operator-(f32x2p a) { return f32x2p{-a.lo, -a.hi}; }
TD_DEV f32x2p td_w_split(f32x4 v) { return f32x2p{f32x2{v[0], v[1]}, f32x2{v[2], v[3]}}; }
TD_DEV f32x4 td_w_join(f32x2p v) { return f32x4{v.lo[0], v.lo[1], v.hi[0], v.hi[1]}; }
// k * x + y with ONE rounding, used ONLY with k = +-2, +-4, +-8: the product with a power of two is exact, so the fused form rounds
// the same real number as `y + k * x` does with contraction off -- same bits, one instruction instead of two (tests/test_wino_exact_fma.py).
TD_DEV float td_w_fma(float k, float x, float y) { return __builtin_fmaf(k, x, y); }
TD_DEV f32x2 td_w_fma(float k, f32x2 x, f32x2 y) { return __builtin_elementwise_fma(f32x2{k, k}, x, y); }
TD_DEV f32x2p td_w_fma(float k, f32x2p x, f32x2p y) { return f32x2p{td_w_fma(k, x.lo, y.lo), td_w_fma(k, x.hi, y.hi)}; }
TD_DEV float td_w_mul(float k, float x) { return k * x; }
TD_DEV f32x2 td_w_mul(float k, f32x2 x) { return k * x; }
TD_DEV f32x2p td_w_mul(float k, f32x2p x) { return f32x2p{k * x.lo, k * x.hi}; }
// the fused plane LayerNorm of one patch element: the arithmetic of k_ln_apply, same operation order
TD_DEV float td_w_ln(float z, float m, float r, float g, float b) { return (z - m) * r * g + b; }
TD_DEV f32x2 td_w_ln(f32x2 z, f32x2 m, f32x2 r, float g, float b) { return (z - m) * r * g + b; }
// The same with WAVE-UNIFORM gamma and beta (the wave-per-tile kernels): the packed multiply and add read them from a scalar register pair,
// low half for both lanes (op_sel_hi 0) -- the compiler copies every such scalar into a VGPR first.
TD_DEV float td_w_ln_u(float z, float m, float r, float g, float b) { return (z - m) * r * g + b; }
TD_DEV f32x2 td_w_ln_u(f32x2 z, f32x2 m, f32x2 r, float g, float b) {
#ifdef TD_EMU
    return (z - m) * r * g + b;
#else
    const f32x2 t = (z - m) * r;
    const unsigned long long gp = __builtin_bit_cast(unsigned, g), bp = __builtin_bit_cast(unsigned, b);
    f32x2 u, v;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(u) : "v"(t), "s"(gp));
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(v) : "v"(u), "s"(bp));
    return v;
#endif
}
TD_DEV f32x2p td_w_ln_u(f32x2p z, f32x2p m, f32x2p r, float g, float b) { return f32x2p{td_w_ln_u(z.lo, m.lo, r.lo, g, b), td_w_ln_u(z.hi, m.hi, r.hi, g, b)}; }
TD_DEV f32x2p td_w_ln(f32x2p z, f32x2p m, f32x2p r, float g, float b) { return f32x2p{td_w_ln(z.lo, m.lo, r.lo, g, b), td_w_ln(z.hi, m.hi, r.hi, g, b)}; }

// ---- F(4x4, 3x3): interpolation points 0, +-1, +-2, inf (Lavin & Gray) -----------------------------------------------------
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// 14 and 10 operations.  The values are those of the plain forms (in comments), bit for bit; 5 x stays a multiplication.
template <typename T>
TD_DEV void td_wino4_bt_t(const T (&d)[6], T (&t)[6]) {
    const T a = td_w_fma(-4.f, d[2], d[4]), b = td_w_fma(-4.f, d[1], d[3]);       // d4 - 4 d2, d3 - 4 d1
    const T c = d[4] - d[2], x = d[3] - d[1];
    t[0] = td_w_fma(4.f, d[0], -td_w_mul(5.f, d[2])) + d[4];                      // 4 d0 - 5 d2 + d4
    t[1] = a + b;
    t[2] = a - b;
    t[3] = td_w_fma(2.f, x, c);                                                   // c + 2 (d3 - d1)
    t[4] = td_w_fma(-2.f, x, c);                                                  // c - 2 (d3 - d1)
    t[5] = td_w_fma(4.f, d[1], -td_w_mul(5.f, d[3])) + d[5];                      // 4 d1 - 5 d3 + d5
}
template <typename T>
TD_DEV void td_wino4_at_t(const T (&m)[6], T (&y)[4]) {
    const T p = m[1] + m[2], q = m[1] - m[2], r = m[3] + m[4], s = m[3] - m[4];
    y[0] = m[0] + p + r;
    y[1] = td_w_fma(2.f, s, q);                                                   // q + 2 s
    y[2] = td_w_fma(4.f, r, p);                                                   // p + 4 r
    y[3] = td_w_fma(8.f, s, q) + m[5];                                            // q + 8 s + m5
}

// ---- activation of a finished output tile ---------------------------------------------------------------------------------------
// act is launch-uniform: ReLU (act 1) is ONE instruction per value, the IEEE-754-2019 maximum with -0 (gfx950: v_maximum3_f32).  td_activate
// gives 0 * v = -0 for v < 0 (-inf included), v otherwise, and passes a NaN on; this maximum orders -0 below +0 and returns a NaN for a
// NaN -- the same bits in every case (v_max_f32 would turn a NaN into -0).  The identity is nothing.  The leaky form (act 2) keeps
// td_activate and has kernel instances of its own (GEN), so the frame's kernels do not carry its code.
TD_DEV float td_w_relu(float v) { return __builtin_elementwise_maximum(v, -0.f); }
template <bool GEN> TD_DEV float td_w_act(float v, float slope) { return GEN ? td_activate(v, slope) : td_w_relu(v); }
template <bool GEN> TD_DEV f32x2 td_w_act(f32x2 v, float slope) { return f32x2{td_w_act<GEN>(v[0], slope), td_w_act<GEN>(v[1], slope)}; }
template <bool GEN> TD_DEV f32x2p td_w_act(f32x2p v, float slope) { return f32x2p{td_w_act<GEN>(v.lo, slope), td_w_act<GEN>(v.hi, slope)}; }
template <bool GEN, typename T, int N>
TD_DEV void td_wino_activate(T (&o)[N], int act) {
    if (GEN || act == 1) {                                            // wave-uniform
        const float slope = td_act_slope(act);
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = td_w_act<GEN>(o[i], slope);
    }
}
TD_HOSTDEV bool wino_act_general(int act) { return act == 2; }     // which instance a launch takes

// thread = (tile, 4 channels): 6x6 patch (stride = dilation) -> 36 planes of V.  All 36 loads first, then the columns, then each row of
// the intermediate is transformed and stored.  Offsets are 32-bit buffer offsets: a row term and a column term, each TD_BUF_OOB outside
// the image, added with saturation (two invalid terms must not wrap into the buffer); a store adds its plane's offset to the lane's.
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 2) k_wino4_in(WinoArgs p) {
    const int CV = p.C >> 2;
    const WinoBufs wb = td_wino_bufs(p);
    const unsigned plane = (unsigned)p.TP * (unsigned)p.C * 4u;
    const TdBuf vb = td_make_buf(p.V, 36u * plane);
    const long total = (long)p.T * CV;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cv = (int)(i % CV);
        const unsigned tile = (unsigned)(i / CV);
        int t = (int)tile;
        const int tx = t % p.TX; t /= p.TX;
        const int ty = t % p.TY; t /= p.TY;
        const int px = t % p.dil, py = t / p.dil;
        unsigned offy[6], offx[6], piy[6], pix[6];                        // byte offset = offy[r] + offx[c], 4 * pixel = piy[r] + pix[c]
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int y = py + p.dil * (4 * ty - 1 + r), x = px + p.dil * (4 * tx - 1 + r);
            const bool oky = (unsigned)y < (unsigned)p.H, okx = (unsigned)x < (unsigned)p.W;
            piy[r] = oky ? (unsigned)y * (unsigned)p.W * 4u : TD_BUF_OOB;
            pix[r] = okx ? (unsigned)x * 4u : TD_BUF_OOB;
            offy[r] = oky ? (unsigned)y * (unsigned)p.W * (unsigned)p.C * 4u : TD_BUF_OOB;
            offx[r] = okx ? ((unsigned)x * (unsigned)p.C + (unsigned)cv * 4u) * 4u : TD_BUF_OOB;
        }
        f32x2p dd[6][6];                                                  // [c][r]
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) dd[c][r] = td_w_split(td_buf_ld4(wb.in, __builtin_elementwise_add_sat(offy[r], offx[c]), 0u));
        if (p.ln_mean) {                                                  // uniform; outside the image gamma and beta read as 0: the element stays 0
            const f32x2p m4 = td_w_split(td_ld4(p.ln_mean + cv * 4)), r4 = td_w_split(td_ld4(p.ln_rstd + cv * 4));
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    const unsigned po = __builtin_elementwise_add_sat(piy[r], pix[c]);
                    dd[c][r] = td_w_ln(dd[c][r], m4, r4, td_buf_ld1(wb.g, po, 0u), td_buf_ld1(wb.b, po, 0u));
                }
        }
        f32x2p tm[6][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            f32x2p col[6];
            td_wino4_bt_t(dd[c], col);                                    // B^T d, one column
#pragma unroll
            for (int r = 0; r < 6; ++r) tm[r][c] = col[r];
        }
        const unsigned voff = (tile * (unsigned)p.C + (unsigned)cv * 4u) * 4u;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            f32x2p v[6];
            td_wino4_bt_t(tm[r], v);                                      // (.) B, one row
#pragma unroll
            for (int c = 0; c < 6; ++c) td_buf_st4(vb, voff + (unsigned)(r * 6 + c) * plane, td_w_join(v[c]));
        }
    }
}

// thread = (tile, 4 output channels): Y = A^T m A (4x4 pixels), + bias (+ residual), activation, scatter
template <bool GEN>
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 2) k_wino4_out(WinoArgs p) {
    const int CV = p.Cout >> 2;
    const WinoBufs wb = td_wino_bufs(p);
    const unsigned plane = (unsigned)p.TP * (unsigned)p.Cout * 4u;
    const TdBuf mb = td_make_buf(p.Mb, 36u * plane);
    const long total = (long)p.T * CV;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cv = (int)(i % CV);
        const unsigned tile = (unsigned)(i / CV);
        int t = (int)tile;
        const int tx = t % p.TX; t /= p.TX;
        const int ty = t % p.TY; t /= p.TY;
        const int px = t % p.dil, py = t / p.dil;
        // the 16 residual vectors first: they are in flight under the 36 plane loads and the transforms (a residual load, a wait and
        // a store per output pixel made this kernel latency-bound: 32.5 us average against 25 for the larger input transform)
        unsigned offy[4], offx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = py + p.dil * (4 * ty + r), x = px + p.dil * (4 * tx + r);
            offy[r] = y < p.H ? (unsigned)y * (unsigned)p.W * (unsigned)p.Cout * 4u : TD_BUF_OOB;
            offx[r] = x < p.W ? ((unsigned)x * (unsigned)p.Cout + (unsigned)cv * 4u) * 4u : TD_BUF_OOB;
        }
        f32x2p o[16];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) o[r * 4 + c] = td_w_split(td_buf_ld4(wb.resid, __builtin_elementwise_add_sat(offy[r], offx[c]), 0u));
        const unsigned moff = (tile * (unsigned)p.Cout + (unsigned)cv * 4u) * 4u;
        f32x2p mm[6][6];                                                  // [c][r]
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) mm[c][r] = td_w_split(td_buf_ld4(mb, moff, (unsigned)(r * 6 + c) * plane));
        const f32x2p b = td_w_split(td_ld4(p.bias + cv * 4));
        f32x2p sm[4][6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            f32x2p col[4];
            td_wino4_at_t(mm[c], col);                                    // A^T m, one column
#pragma unroll
            for (int r = 0; r < 4; ++r) sm[r][c] = col[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            f32x2p o4[4];
            td_wino4_at_t(sm[r], o4);                                     // (.) A, one row
#pragma unroll
            for (int c = 0; c < 4; ++c) o[r * 4 + c] = (o4[c] + b) + o[r * 4 + c];
        }
        td_wino_activate<GEN>(o, p.act);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) td_buf_st4(wb.out, __builtin_elementwise_add_sat(offy[r], offx[c]), td_w_join(o[r * 4 + c]));
    }
}


// ---- low-register, chunk-aware F(4x4) transforms -----------------------------------------------------------------------------
// Same arithmetic as k_wino4_in / k_wino4_out, element for element (results are bit-identical), laid out for CO-RESIDENCY with the
// persistent GEMM: that kernel holds 3 workgroups per CU for its whole life at 136 VGPRs per wave, which leaves 104 registers
// per SIMD -- the float4-per-lane transforms above need far more and could only start when a GEMM workgroup retires.  Here a
// WAVE owns (tile, slice of 64 * VW channels) and a lane VW channels (VW = 1: 60-odd VGPRs), so one transform wave fits beside
// three GEMM waves on every SIMD and the HBM-bound transform of one chunk runs UNDER the MFMA-bound GEMM of another.  The tile is
// wave-uniform, and so is everything about an access but the lane's channel offset: the tile's decode (divisions by TX, TY, dil), the
// six row and six column terms, the pixel offsets -- scalar work -- and whether the pixel is inside the image, which picks the buffer's
// SIZE (0 bytes = every lane out of range: zeros for a load, nothing for a store) instead of selecting a per-lane offset.  A load carries
// the uniform offset in the SGPR soffset.  A 16-byte buffer STORE must not (td_device.h td_buf_st4: the >64-bit store-data hazard the
// compiler does not see behind a register soffset), so every store gets a descriptor whose BASE is the uniform address -- scalar adds --
// and whose size is the tile's channel row: the lane offset is the channel offset alone, no VALU instruction per access.
TD_DEV TdBuf td_wino_row_buf(const float* base, unsigned off_bytes, unsigned bytes) {
    return td_make_buf(reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + off_bytes), bytes);
}
template <int VW> struct WinoVec;
template <> struct WinoVec<1> {
    typedef float T;
    TD_DEV_MEMBER T zero() { return 0.f; }
    TD_DEV_MEMBER T ld(TdBuf b, unsigned v, unsigned s) { return td_buf_ld1(b, v, s); }
    TD_DEV_MEMBER void st(TdBuf b, unsigned v, T x) { td_buf_st1(b, v, 0u, x); }
};
template <> struct WinoVec<2> {
    typedef f32x2 T;
    TD_DEV_MEMBER T zero() { return f32x2{0.f, 0.f}; }
    TD_DEV_MEMBER T ld(TdBuf b, unsigned v, unsigned s) { return td_buf_ld2(b, v, s); }
    TD_DEV_MEMBER void st(TdBuf b, unsigned v, T x) { td_buf_st2(b, v, 0u, x); }
};
template <> struct WinoVec<4> {
    typedef f32x2p T;
    TD_DEV_MEMBER T zero() { return f32x2p{f32x2{0.f, 0.f}, f32x2{0.f, 0.f}}; }
    TD_DEV_MEMBER T ld(TdBuf b, unsigned v, unsigned s) { return td_w_split(td_buf_ld4(b, v, s)); }
    TD_DEV_MEMBER void st(TdBuf b, unsigned v, T x) { td_buf_st4(b, v, td_w_join(x)); }
};
// (wave-uniform) unit wv of a chunk -> tile, channel slice, phase and tile coordinates
struct WinoTile { int tl, sl, py, px, ty, tx; };
TD_DEV WinoTile td_wino_unit_tile(const WinoArgs& p, int slices, int wv) {
    WinoTile w;
    w.tl = td_w_div(wv, p.mg_sl); w.sl = wv - w.tl * slices;
    const int t1 = td_w_div(w.tl, p.mg_tx), t2 = td_w_div(t1, p.mg_ty), t3 = td_w_div(t2, p.mg_pw);
    w.tx = w.tl - t1 * p.TX;
    w.ty = t1 - t2 * p.TY;
    w.px = p.nx * (t2 - t3 * p.pw) + p.cx;
    w.py = p.ny * t3 + p.cy;
    return w;
}

// One unit = one wave's work: (tile, slice of 64 VW channels) of the input transform.
template <int VW>
TD_DEV void td_wino4_in_unit(const WinoArgs& p, int wv) {
    typedef WinoVec<VW> X;
    typedef typename X::T T;
    const int slices = (p.C + 64 * VW - 1) / (64 * VW);
    const WinoTile w = td_wino_unit_tile(p, slices, wv);
    const int c0 = (w.sl * 64 + (int)(threadIdx.x & 63)) * VW;        // this lane's first channel
    const unsigned coff = c0 < p.C ? (unsigned)c0 * 4u : TD_BUF_OOB;  // lanes past C (C not a multiple of 64 VW): nothing read, nothing written
    const unsigned in_bytes = (unsigned)p.H * (unsigned)p.W * (unsigned)p.C * 4u;
    // Validity as ARITHMETIC on scalars (a compare and select of a wave-uniform value is handed to the VALU as soon as the mask is used as a number):
    // sy / sx: sign bit set = row / column inside the image (0 <= y < H; all sizes are below 2^30); my / mx: all ones / 0; pixel index = piy[r] + pix[c]
    unsigned sy[6], sx[6], my[6], mx[6], piy[6], pix[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const int y = w.py + p.dil * (4 * w.ty - 1 + r), x = w.px + p.dil * (4 * w.tx - 1 + r);
        sy[r] = ((unsigned)y - (unsigned)p.H) & ~(unsigned)y; sx[r] = ((unsigned)x - (unsigned)p.W) & ~(unsigned)x;
        my[r] = (unsigned)((int)sy[r] >> 31); mx[r] = (unsigned)((int)sx[r] >> 31);
        piy[r] = (unsigned)y * (unsigned)p.W; pix[r] = (unsigned)x;
    }
    T dd[6][6];                                                       // [c][r]
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const unsigned ok = my[r] & mx[c];
            dd[c][r] = X::ld(td_make_buf(p.in, in_bytes & ok), coff, ((piy[r] + pix[c]) & ok) * (unsigned)p.C * 4u);
        }
    if (p.ln_mean) {                                                  // uniform; the arithmetic of k_ln_apply, same order (the head conv only)
        const TdBuf mb = td_make_buf(p.ln_mean, (unsigned)p.C * 4u), rb = td_make_buf(p.ln_rstd, (unsigned)p.C * 4u);
        const T m4 = X::ld(mb, coff, 0u), r4 = X::ld(rb, coff, 0u);
        // A pixel's validity and index are stated ANEW here, from six row and six column terms of their own (gy / gx: the index term, 0 outside
        // the image, so the sum always is a pixel of the map; validity from the sign bits): restating the loads' expressions would keep their 72 values
        // in scalar registers from the loads to here, and they do not fit.
        unsigned gy[6], gx[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) { gy[r] = piy[r] & my[r]; gx[r] = pix[r] & mx[r]; }
        // gamma and beta of a pixel are the same for every lane: plain loads from a wave-uniform address are SCALAR loads -- no VALU, no
        // VGPR (they were 72 per-lane buffer loads).  Outside the image they read as 0 and the element stays 0.  One column at a time:
        // all 72 values at once do not fit the scalar registers.
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const unsigned ok = (unsigned)((int)(sy[r] & sx[c]) >> 31), pi = gy[r] + gx[c];
                const float g = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, p.ln_g[pi]) & ok);   // on the bits: scalar work (a float select is the VALU's)
                const float b = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, p.ln_b[pi]) & ok);
                dd[c][r] = td_w_ln_u(dd[c][r], m4, r4, g, b);
            }
            TD_SCHED_FENCE();
        }
    }
    T tm[6][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T col[6];
        td_wino4_bt_t(dd[c], col);                                    // B^T d, one column
#pragma unroll
        for (int r = 0; r < 6; ++r) tm[r][c] = col[r];
    }
    const unsigned plane = (unsigned)p.TP * (unsigned)p.C * 4u;
    const unsigned voff = (unsigned)w.tl * (unsigned)p.C * 4u;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        T v[6];
        TD_SCHED_FENCE();                                             // a row's six descriptors are made here, not 36 of them ahead of the arithmetic (72 scalar registers)
        td_wino4_bt_t(tm[r], v);                                      // (.) B, one row
#pragma unroll
        for (int c = 0; c < 6; ++c) X::st(td_wino_row_buf(p.V, (unsigned)(r * 6 + c) * plane + voff, (unsigned)p.C * 4u), coff, v[c]);
    }
}

template <int VW, bool GEN>
TD_DEV void td_wino4_out_unit(const WinoArgs& p, int wv) {
    typedef WinoVec<VW> X;
    typedef typename X::T T;
    const int slices = (p.Cout + 64 * VW - 1) / (64 * VW);
    const WinoTile w = td_wino_unit_tile(p, slices, wv);
    const int c0 = (w.sl * 64 + (int)(threadIdx.x & 63)) * VW;
    const unsigned coff = c0 < p.Cout ? (unsigned)c0 * 4u : TD_BUF_OOB;
    const unsigned res_bytes = p.resid ? (unsigned)p.H * (unsigned)p.W * (unsigned)p.Cout * 4u : 0u;
    unsigned offy[4], offx[4], my[4], mx[4];                          // all ones / 0: row, column inside the map
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = w.py + p.dil * (4 * w.ty + r), x = w.px + p.dil * (4 * w.tx + r);
        my[r] = (unsigned)((int)((unsigned)y - (unsigned)p.H) >> 31); mx[r] = (unsigned)((int)((unsigned)x - (unsigned)p.W) >> 31);   // y, x >= 0; as arithmetic: see td_wino4_in_unit
        offy[r] = (unsigned)y * (unsigned)p.W * (unsigned)p.Cout * 4u;
        offx[r] = (unsigned)x * (unsigned)p.Cout * 4u;
    }
    T o[16];                                                          // residual first: in flight under the 36 plane loads
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned ok = my[r] & mx[c];
            o[r * 4 + c] = X::ld(td_make_buf(p.resid, res_bytes & ok), coff, (offy[r] + offx[c]) & ok);
        }
    const unsigned plane = (unsigned)p.TP * (unsigned)p.Cout * 4u;
    const TdBuf mb = td_make_buf(p.Mb, 36u * plane);
    const unsigned moff = (unsigned)w.tl * (unsigned)p.Cout * 4u;
    T mm[6][6];                                                       // [c][r]
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int r = 0; r < 6; ++r) mm[c][r] = X::ld(mb, coff, (unsigned)(r * 6 + c) * plane + moff);
    const TdBuf bbuf = td_make_buf(p.bias, (unsigned)p.Cout * 4u);
    const T b = X::ld(bbuf, coff, 0u);
    T sm[4][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T col[4];
        td_wino4_at_t(mm[c], col);                                    // A^T m, one column
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[r][c] = col[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        T o4[4];
        td_wino4_at_t(sm[r], o4);                                     // (.) A, one row
#pragma unroll
        for (int c = 0; c < 4; ++c) o[r * 4 + c] = (o4[c] + b) + o[r * 4 + c];
    }
    td_wino_activate<GEN>(o, p.act);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned ok = my[r] & mx[c];
            X::st(td_wino_row_buf(p.out, (offy[r] + offx[c]) & ok, ((unsigned)p.Cout * 4u) & ok), coff, o[r * 4 + c]);
        }
}

template <int VW>
TD_KERNEL void TD_LAUNCH_BOUNDS(256, VW == 4 ? 2 : 4) k_wino4_in_c(WinoArgs p) {
    const int slices = (p.C + 64 * VW - 1) / (64 * VW);
    const int wv = TD_UNIFORM((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wv >= p.Tc * slices) return;
    td_wino4_in_unit<VW>(p, wv);
}
template <int VW, bool GEN>
TD_KERNEL void TD_LAUNCH_BOUNDS(256, VW == 4 ? 2 : 4) k_wino4_out_c(WinoArgs p) {
    const int slices = (p.Cout + 64 * VW - 1) / (64 * VW);
    const int wv = TD_UNIFORM((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wv >= p.Tc * slices) return;
    td_wino4_out_unit<VW, GEN>(p, wv);
}
// ---- the FCN head's output transform + its 1x1 classifier in one launch (round 6; td4_psp18.py:295-299: conv3x3 -> BN -> ReLU -> conv1x1 + bias) -------------
// A wave owns one tile = 16 pixels x ALL Cout = 64 VW channels of the head's hidden map (td4: 128, td2: 64): A^T m A + bias, ReLU as in td_wino4_out_unit, the
// 16 x Cout values go to LDS (rows padded by 4 floats: 16 lanes reading 16 rows hit 16 different 16-byte slots) instead of HBM, and lane i computes the outputs
// (pixel i & 15, class i >> 4), (.., + 4), .. with k_classifier's summation order -- four sequential fma chains over the channel quarters, added as
// ((s0 + s1) + s2) + s3 + bias -- so the low-resolution logits are bit-identical to the two-kernel form.  The hidden map (17 MB at 1024x2048) is never written.
struct ClsArgs { const float* w; const float* b; float* out; int NC; };   // classifier [NC][Cout], [NC]; out planar [NC][H * W]
template <int VW>
TD_KERNEL void TD_LAUNCH_BOUNDS(256, 2) k_wino4_out_cls(WinoArgs p, ClsArgs c) {
    typedef WinoVec<VW> X;
    typedef typename X::T T;
    constexpr int C = 64 * VW, ROW = C + 4;
    TD_DYN_LDS(smem);
    float* ws = reinterpret_cast<float*>(smem);                        // [NC][C]
    float* ys = ws + c.NC * C + (threadIdx.x >> 6) * (16 * ROW);       // this wave's [16 pixels][ROW]
    for (int i = threadIdx.x; i < c.NC * C; i += blockDim.x) ws[i] = c.w[i];
    __syncthreads();                                                   // the only workgroup barrier: waves past the last tile may leave after it
    const int wv = TD_UNIFORM((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (wv >= p.Tc) return;
    const int lane = threadIdx.x & 63;
    const WinoTile w = td_wino_unit_tile(p, 1, wv);
    const unsigned coff = (unsigned)(lane * VW) * 4u;
    const unsigned plane = (unsigned)p.TP * (unsigned)C * 4u;
    const TdBuf mb = td_make_buf(p.Mb, 36u * plane);
    const unsigned moff = (unsigned)w.tl * (unsigned)C * 4u;
    T mm[6][6];                                                       // [c][r]
#pragma unroll
    for (int cc = 0; cc < 6; ++cc)
#pragma unroll
        for (int r = 0; r < 6; ++r) mm[cc][r] = X::ld(mb, coff, (unsigned)(r * 6 + cc) * plane + moff);
    const TdBuf bbuf = td_make_buf(p.bias, (unsigned)C * 4u);
    const T b = X::ld(bbuf, coff, 0u);
    T sm[4][6];
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) {
        T col[4];
        td_wino4_at_t(mm[cc], col);                                   // A^T m, one column
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[r][cc] = col[r];
    }
    T o[16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        T o4[4];
        td_wino4_at_t(sm[r], o4);                                     // (.) A, one row
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) o[r * 4 + cc] = (o4[cc] + b) + X::zero();   // the zero residual of td_wino4_out_unit / k_wino4_out (-0 + 0 = +0: same bits)
    }
    td_wino_activate<false>(o, p.act);                                // the head's ReLU (or none): run_wino refuses the leaky form here
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float* dst = ys + i * ROW + lane * VW;
        if constexpr (VW == 1) dst[0] = o[i];
        else { dst[0] = o[i][0]; dst[1] = o[i][1]; }
    }
    td_wave_sync();
    const int CQ = C >> 2;
    for (int idx = lane; idx < 16 * c.NC; idx += 64) {
        const int px = idx & 15, k = idx >> 4;
        const float* yr = ys + px * ROW;
        const float* wr = ws + k * C;
        float s[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            float a = 0.f;
            for (int ch = 0; ch < CQ; ch += 4) {
                const f32x4 v = td_ld4(yr + qd * CQ + ch), u = td_ld4(wr + qd * CQ + ch);
                a = fmaf(v[0], u[0], a); a = fmaf(v[1], u[1], a); a = fmaf(v[2], u[2], a); a = fmaf(v[3], u[3], a);
            }
            s[qd] = a;
        }
        const int y = w.py + p.dil * (4 * w.ty + (px >> 2)), x = w.px + p.dil * (4 * w.tx + (px & 3));
        if (y < p.H && x < p.W) c.out[(size_t)k * p.H * p.W + (size_t)y * p.W + x] = (((s[0] + s[1]) + s[2]) + s[3]) + c.b[k];
    }
}
static inline bool wino_out_cls_supports(int Cout, int NC) { return (Cout == 64 || Cout == 128) && NC >= 1 && NC <= 32; }
static inline int wino_out_cls_lds(int Cout, int NC) { return (NC * Cout + 4 * 16 * (Cout + 4)) * 4; }

// grid of a chunked transform: one wave per (tile, channel slice)
static inline unsigned wino_chunk_grid(int Tc, int C, int VW) { return (unsigned)(((long)Tc * ((C + 64 * VW - 1) / (64 * VW)) + 3) / 4); }


// m = output tile edge (2 or 4)
static inline int wino_tiles_1d(int n, int dil, int m) { return ((n + dil - 1) / dil + m - 1) / m; }
static inline long wino_tiles(int H, int W, int dil, int m) { return (long)dil * dil * wino_tiles_1d(H, dil, m) * wino_tiles_1d(W, dil, m); }

// tile count for an output of M pixels whose shape is not at hand (layer setup): assume the 1:2 frames of the path
static inline long wino_tiles_estimate(long M, int dil, int m) {
    int H = 1;
    while ((long)H * H * 2 < M) ++H;
    const int W = (int)((M + H - 1) / H);
    return wino_tiles(H, W, dil, m);
}

// U = G g G^T (fp64) for every (co, ci): (m+2)^2 [Cout][Cin] matrices, matrix xi*(m+2)+nu first
static inline void wino_transform_weights(const float* w, int Cout, int Cin, int m, std::vector<std::vector<float>>& U) {
    static const double G4[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                    {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    const int n = m + 2;
    const double (*G)[3] = G4;                                        // m == 4 only
    U.assign((size_t)n * n, std::vector<float>((size_t)Cout * Cin));
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            const float* g = w + ((size_t)co * Cin + ci) * 9;
            double t[6][3];
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    U[(size_t)i * n + j][(size_t)co * Cin + ci] = (float)(t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2]);
        }
}
