// td_launch.h -- one host-side launch helper per operator of the frame (conv / Winograd conv / attention / plane LayerNorm / pyramid slice /
// stem / classifier) and per output form of its last launch + the per-launch profiling records.  Part of the td_model.hip translation unit.
#pragma once
#include "td_weights.h"

// ---------------------------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------------------------
// TIMING PROBE, compiled in only with -DTDNET_TIMING_PROBES (TDNET_EXTRA_CXXFLAGS of tdnet_amd/build.py; never in the shipped library): under
// TDNET_PROBE_SKIP=<mask> a handle leaves pieces of the frame OUT -- the results are garbage -- to measure what the frame costs without them:
//   1 = no Winograd transforms, 2 = no cache-only attention chain, 4 = no final attention, 8 = no Winograd GEMMs.  Upper bounds for what any
//   optimisation of that piece can return (DESIGN_experiments 8.6, profiles/r04z_frame_budget_*).
#ifdef TDNET_TIMING_PROBES
static int probe_skip() {
    static const int m = [] {
        const char* e = getenv("TDNET_PROBE_SKIP");
        const int v = e ? atoi(e) : 0;
        if (v) fprintf(stderr, "tdnet: TDNET_PROBE_SKIP=%d -- pieces of the frame are NOT computed, every result of this process is garbage (timing probe build)\n", v);
        return v;
    }();
    return m;
}
#else
static constexpr int probe_skip() { return 0; }
#endif
static void prof_begin(tdnet* n, int family, int dominant, double flops, hipStream_t s) {
    if (!n || !n->prof) return;
    if (n->nrec == n->recs.size()) {
        ProfRec r;
        hipEventCreate(&r.e0); hipEventCreate(&r.e1);
        n->recs.push_back(r);
    }
    ProfRec& r = n->recs[n->nrec];
    r.family = family; r.dominant = dominant; r.flops = flops;
    hipEventRecord(r.e0, s);
}
static void prof_end(tdnet* n, hipStream_t s) {
    if (!n || !n->prof) return;
    hipEventRecord(n->recs[n->nrec].e1, s);
    n->nrec++;
}

// plane LayerNorm applied to the conv's INPUT inside a Winograd input transform (td_wino.h WinoArgs.ln_*)
struct LnFuse { const float *mean, *rstd, *g, *b; };

// One row-parity / column-parity chunk of a Winograd conv (td_wino.h WinoArgs.Tc..cx): the tiles whose phase row is ny * i + cy and
// whose phase column is nx * j + cx.  {1, 0, 1, 0} = the whole conv.
struct WinoChunk { int ny = 1, cy = 0, nx = 1, cx = 0; };

template <int VW>
static void launch_wino4_c(bool out_side, WinoArgs wa, hipStream_t s) {
    wa.mg_sl = wino_magic(((out_side ? wa.Cout : wa.C) + 64 * VW - 1) / (64 * VW));
    if (out_side && wino_act_general(wa.act)) TD_LAUNCH((k_wino4_out_c<VW, true>), dim3(wino_chunk_grid(wa.Tc, wa.Cout, VW)), dim3(256), 0, s, wa);
    else if (out_side) TD_LAUNCH((k_wino4_out_c<VW, false>), dim3(wino_chunk_grid(wa.Tc, wa.Cout, VW)), dim3(256), 0, s, wa);
    else TD_LAUNCH((k_wino4_in_c<VW>), dim3(wino_chunk_grid(wa.Tc, wa.C, VW)), dim3(256), 0, s, wa);
}

// The launch arguments of layer L on an H x W input map / as one GEMM of `nbatch` x M rows
static ConvArgs conv_args(const ConvLayer& L, const float* in, int H, int W, const float* resid, float* out) {
    const int Ho = out_size(H, L.KS, L.stride, L.dil, L.pad), Wo = out_size(W, L.KS, L.stride, L.dil, L.pad);
    return ConvArgs{in, L.d_wp, L.d_bias, resid, out, H, W, L.Cin, Wo, L.Cout, L.CoutPad, L.stride, L.dil, L.pad, Ho * Wo, L.nsteps, L.act, 0, 1};
}
static GemmArgs gemm_args(const ConvLayer& L, const float* a, int M, int nbatch, const float* bias, const float* resid, float* out, int act) {
    GemmArgs ga;
    ga.a = a; ga.wp = L.d_wp; ga.bias = bias; ga.resid = resid; ga.out = out;
    ga.M = M; ga.N = L.Cout; ga.NPad = L.CoutPad; ga.K = L.Cin; ga.nbatch = nbatch; ga.act = act; ga.tiles_m = ga.tiles_n = 0; ga.MP = M;
    return ga;
}
// The GEMM(s) of a CR_WINO / CR_GEMM1X1 layer on the kernel it was planned for.  b3_grid: the split kernel's grid where the options force none (0: its own)
static void launch_gemm(const ConvLayer& L, const GemmArgs& ga, int b3_grid, hipStream_t s) {
    const int forced_grid = L.pers > 1 ? L.pers : 0;
    switch (L.gemm) {
    case GK_B3: gemm_b3_launch(ga, forced_grid ? forced_grid : b3_grid, s); break;
    case GK_DMA: gemm_dma_launch(ga, forced_grid, s); break;
    case GK_PERSISTENT: gemm_launch(ga, L.tile, forced_grid, s); break;
    case GK_CONV:                                                      // the same GEMMs as batched 1x1 convs over a 1 x M map, one tile per workgroup
        conv_launch(ConvArgs{ga.a, ga.wp, ga.bias, ga.resid, ga.out, 1, ga.M, ga.K, ga.M, ga.N, ga.NPad, 1, 1, 0, ga.M, L.nsteps, ga.act, 0, ga.nbatch}, L.tile, 1, false, s);
        break;
    }
}

// Winograd F(4x4) conv (or one chunk of it): input transform -> 36 batched GEMMs -> output transform, all on stream s.
// V / Mb: workspaces for THIS call ([nb][Tc + pad][C]); nullptr = the handle's (n->wino_v / wino_m) or, without a handle, temporary ones.
// cls != nullptr: the conv is the FCN head's 3x3 and its output transform also applies the 1x1 classifier (k_wino4_out_cls): `out` is not written
static int run_wino(tdnet* n, const ConvLayer& L, const float* in, int H, int W, const float* resid, float* out, hipStream_t s,
                    const LnFuse* lnf, const WinoChunk& ck, float* V, float* Mb, const ClsArgs* cls = nullptr) {
    const int TY = wino_tiles_1d(H, L.dil, L.wino), TX = wino_tiles_1d(W, L.dil, L.wino);
    const long T = (long)L.dil * L.dil * TY * TX;
    const bool chunked = ck.ny != 1 || ck.nx != 1;
    if (chunked && (!L.vw || L.dil % ck.ny || L.dil % ck.nx)) return td_fail("internal: this conv cannot run in chunks");
    const long Tc = (long)(L.dil / ck.ny) * (L.dil / ck.nx) * TY * TX;
    const int nb = (L.wino + 2) * (L.wino + 2);
    bool own = false;
    if (!V) {
        own = n == nullptr || n->wino_v_floats < (size_t)nb * Tc * L.Cin || n->wino_m_floats < (size_t)nb * Tc * L.Cout;
        if (own) {
            if (n) { n->failed = true; return td_fail("internal: Winograd workspace too small"); }
            if (dev_alloc(&V, (size_t)nb * Tc * L.Cin) || dev_alloc(&Mb, (size_t)nb * Tc * L.Cout)) return -1;
        } else { V = n->wino_v; Mb = n->wino_m; }
    }
    WinoArgs wa;
    wa.in = in; wa.V = V; wa.Mb = Mb; wa.bias = L.d_bias; wa.resid = resid; wa.out = out;
    wa.H = H; wa.W = W; wa.C = L.Cin; wa.Cout = L.Cout; wa.dil = L.dil; wa.TY = TY; wa.TX = TX; wa.T = (int)T; wa.act = L.act; wa.TP = (int)Tc;
    wa.ln_mean = lnf ? lnf->mean : nullptr; wa.ln_rstd = lnf ? lnf->rstd : nullptr; wa.ln_g = lnf ? lnf->g : nullptr; wa.ln_b = lnf ? lnf->b : nullptr;
    wa.Tc = (int)Tc; wa.ny = ck.ny; wa.cy = ck.cy; wa.nx = ck.nx; wa.cx = ck.cx;
    // the transforms address with 32-bit byte offsets below TD_BUF_OOB, and the wave-per-tile ones decode a tile with wino_magic() reciprocals
    const long cmax = L.Cin > L.Cout ? L.Cin : L.Cout;
    if ((long)nb * Tc * cmax * 4 >= (1l << 31) || (long)H * W * cmax * 4 >= (1l << 31) ||
        (L.vw && !(wino_magic_ok(Tc * ((cmax + 63) / 64), TX) && wino_magic_ok(0, TY) && wino_magic_ok(0, L.dil))))
        return td_fail("internal: this conv is too large for the Winograd transforms");
    wa.mg_sl = wino_magic(1); wa.mg_tx = wino_magic(TX); wa.mg_ty = wino_magic(TY); wa.pw = L.dil / ck.nx; wa.mg_pw = wino_magic(wa.pw);
    auto transform = [&](bool out_side) {
        if (n && (probe_skip() & 1)) return;
        prof_begin(n, 2, false, 0, s);
        const int C = out_side ? L.Cout : L.Cin;
        if (out_side && cls) {
            const unsigned grid = (unsigned)((Tc + 3) / 4);
            if (L.Cout == 128) TD_LAUNCH((k_wino4_out_cls<2>), dim3(grid), dim3(256), wino_out_cls_lds(128, cls->NC), s, wa, *cls);
            else TD_LAUNCH((k_wino4_out_cls<1>), dim3(grid), dim3(256), wino_out_cls_lds(64, cls->NC), s, wa, *cls);
        } else
        if (L.vw == 1) launch_wino4_c<1>(out_side, wa, s);
        else if (L.vw == 2 && C % 2 == 0) launch_wino4_c<2>(out_side, wa, s);
        else if (L.vw == 4 && C % 4 == 0) launch_wino4_c<4>(out_side, wa, s);
        else if (L.vw) launch_wino4_c<1>(out_side, wa, s);
        else if (out_side && wino_act_general(wa.act)) TD_LAUNCH((k_wino4_out<true>), dim3(td_grid_for(T * (L.Cout / 4), 256, 256 * 16)), dim3(256), 0, s, wa);
        else if (out_side) TD_LAUNCH((k_wino4_out<false>), dim3(td_grid_for(T * (L.Cout / 4), 256, 256 * 16)), dim3(256), 0, s, wa);
        else TD_LAUNCH(k_wino4_in, dim3(td_grid_for(T * (L.Cin / 4), 256, 256 * 16)), dim3(256), 0, s, wa);
        prof_end(n, s);
    };
    transform(false);
    prof_begin(n, 0, 2, 2.0 * nb * Tc * (double)L.Cin * L.Cout, s);
    // the split GEMM's persistent grid: 512 workgroups (two per CU); a row-parity CHUNK's GEMM -- two of them are in flight, one per chain -- takes 320: of
    // layer 4's 576 tiles 256 workgroups then walk two and the sibling's first workgroups find a free slot at once.  Frame with precision 2 at 1024x2048, by grid of the
    // chunks' GEMMs (profiles/r06ao_*): 512: 339.4, 288: 338.6, 320: 346.0, 352: 344.7, 384: 344.5, 448: 342.1 frames/s.
    // (the fp32 kernel keeps its 768 workgroups for the chunks too: 448 / 512 / 576 / 640 / 1024 gave 273.1 / 273.4 / 271.8 / 275.5 / 274.3 against 278.9 frames/s)
    if (!(n && (probe_skip() & 8))) launch_gemm(L, gemm_args(L, V, (int)Tc, nb, L.d_zero, nullptr, Mb, 0), chunked ? 320 : 0, s);   // (timing probe: no GEMMs)
    prof_end(n, s);
    transform(true);
    if (own) { TD_HIP(hipStreamSynchronize(s)); hipFree(V); hipFree(Mb); }
    return 0;
}

// The fp16 LDS-DMA conv of layer L on the arguments a: a cascade of kernel forms for the SAME tile, each falling back to the next when
// the conv does not qualify (not a 3x3 "same" conv, halo wider than the form's image buffer): narrow tiles -> loader waves -> row
// images (one LDS image per kernel ROW, k_conv_dma_h3) -> tap by tap.
static void launch_conv_dma_forms(const ConvLayer& L, const ConvArgs& a, hipStream_t s) {
    int rh = L.rh;
    bool done = false;
    const bool is192 = rh == CD_192_P || rh == CD_192_N;
    if (rh == CD_128_N || rh == CD_192_N) {                           // narrow tiles (rows x 64 channels) with loader waves (k_conv_dma_h3n)
        done = !L.rowimg_off && conv_launch_dma3n(a, rh, L.KS, L.out16, s);
        if (!done) rh = is192 ? CD_192_P : CD_128_P;
    }
    if (!done && (rh == CD_128_P || rh == CD_192_P)) {                // dedicated loader waves (k_conv_dma_h3p)
        done = !L.rowimg_off && conv_launch_dma3p(a, rh, L.KS, L.out16, s);
        if (!done) rh = is192 ? CD_192 : CD_128_8W;
    }
    if (!done && (L.rowimg_off || !conv_launch_dma3(a, rh, L.KS, L.out16, s))) conv_launch_dma(a, rh, L.KS, L.out16, s);
}

// out[Ho*Wo][Cout] = act(conv(in[H][W][Cin]) + bias (+ resid))
static int run_conv(tdnet* n, const ConvLayer& L, const float* in, int H, int W, const float* resid, float* out, hipStream_t s,
                    int* Ho_out = nullptr, int* Wo_out = nullptr, const LnFuse* lnf = nullptr, const ClsArgs* cls = nullptr) {
    if (lnf && !L.wino) return td_fail("internal: LayerNorm fusion needs a Winograd input transform");
    if (cls && (!L.wino || L.chunks > 1 || resid || wino_act_general(L.act))) return td_fail("internal: the classifier rides in a whole Winograd conv's output transform");
    const int Ho = out_size(H, L.KS, L.stride, L.dil, L.pad), Wo = out_size(W, L.KS, L.stride, L.dil, L.pad);
    if (L.wino) {
        if (Ho_out) *Ho_out = H;
        if (Wo_out) *Wo_out = W;
        if (L.chunks > 1 && (!n || !n->ws_ready)) {                    // operator tests and probes: the chunks one after the other on one stream
            for (int c = 0; c < L.chunks; ++c) {
                WinoChunk ck; ck.ny = L.chunks; ck.cy = c;
                TD_TRY(run_wino(n, L, in, H, W, resid, out, s, lnf, ck, nullptr, nullptr));
            }
            return 0;
        }
        return run_wino(n, L, in, H, W, resid, out, s, lnf, WinoChunk(), nullptr, nullptr, cls);
    }
    if (L.route == CR_WINO_F64 && !wino_f64_size_ok(H, W)) return td_fail("internal: this map is too large for the fused Winograd kernel");
    const ConvArgs a = conv_args(L, in, H, W, resid, out);
    // the fused F(4x4) kernel's record carries the executed FLOP (36 products per tile, channel pair: a quarter of the direct conv's)
    const double flops = L.route == CR_WINO_F64 ? 2.0 * 36 * (double)wino_tiles(H, W, 1, 4) * L.Cin * L.Cout : L.flops_per_pixel() * a.M;
    // dominant: bits 0-1 = 1 for the 128x128-tile / LDS-DMA 3x3 convs (the kernel set of rounds 3-4), bit 2 = EVERY 3x3 conv that reads an fp16 map
    // (the fixed set of the fp16 mode's roofline since round 5: routing a layer to another kernel does not change it)
    prof_begin(n, 0, (((L.tile == CT_128x128 || L.tile == CT_128x128_DEEP || L.rh) && L.KS == 3 && !L.stem) ? 1 : 0) | ((L.h16() && L.in16 && L.KS == 3 && !L.stem) ? 4 : 0), flops, s);
    switch (L.route) {
    case CR_STEM_H: conv_launch_stem_h(a, L.out16, s); break;
    case CR_CONV_DMA: launch_conv_dma_forms(L, a, s); break;
    case CR_CONV_H: conv_launch_h(a, L.tile, L.KS, L.in16, L.out16, s); break;
    case CR_ADIRECT_B3: conv_launch_adirect_b3(a, L.KS, 0, s); break;   // precision 2, narrow convs (incl. the stride-1 1x1 ones kept off the GEMM route)
    case CR_GEMM1X1: launch_gemm(L, gemm_args(L, in, a.M, 1, L.d_bias, resid, out, L.act), 0, s); break;
    case CR_ADIRECT_ROWS:
    case CR_ADIRECT_ROWS_B3: {                                         // the image is padded already: its own geometry, 3 channels, no padding taps
        ConvArgs r = a;
        r.H = stem_rows_hp(H); r.W = stem_rows_wp(W); r.Cin = 3; r.pad = 0;
        if (L.route == CR_ADIRECT_ROWS_B3) conv_launch_adirect_b3(r, L.KS, 2, s);
        else conv_launch_adirect(r, L.KS, 2, s);
        break;
    }
    case CR_ADIRECT: conv_launch_adirect(a, L.KS, L.stem ? 1 : 0, s); break;
    case CR_IGEMM: conv_launch(a, L.tile, L.KS, L.stem, s); break;
    case CR_WINO_F64: wino_f64_launch(in, L.d_wp, L.d_bias, resid, out, H, W, L.act, s); break;   // (size checked above)
    case CR_WINO: break;                                               // (ran above)
    }
    prof_end(n, s);
    if (Ho_out) *Ho_out = Ho;
    if (Wo_out) *Wo_out = Wo;
    return 0;
}

// A 1x1 conv with two operand sources (td_gemm.h / td_conv_ad.h SRC2): K steps 0 .. k_split - 1 from the map `in` (pixel stride ld floats) and the layer's packed
// weights, steps k_split .. nsteps - 1 from in2 (pixel stride ld2) and wp2.  k_split == nsteps: no second source -- the layer's own conv on the two-source kernel.
// Only the persistent fp32 GEMM and the fp32 direct 1x1 conv have the form; any other plan is an error here (plan_enc_fold keeps a frame away from it).
static int run_conv_src2(tdnet* n, const ConvLayer& L, const float* in, int ld, int k_split, int nsteps, const float* in2, int ld2, const float* wp2,
                         int H, int W, const float* resid, float* out, hipStream_t s) {
    if (L.KS != 1 || L.stem || L.wino) return td_fail("internal: two operand sources need a 1x1 conv");
    const ConvArgs a0 = conv_args(L, in, H, W, resid, out);
    prof_begin(n, 0, 0, 2.0 * L.Cout * 32.0 * nsteps * a0.M, s);      // the executed FLOP
    int rc = 0;
    if (L.route == CR_GEMM1X1 && L.gemm == GK_PERSISTENT) {
        GemmArgs ga = gemm_args(L, in, a0.M, 1, L.d_bias, resid, out, L.act);
        ga.K = 32 * nsteps; ga.k_split = k_split; ga.lda = ld; ga.a2 = in2; ga.lda2 = ld2; ga.wp2 = wp2;
        if (!gemm_src2_supports(ga)) rc = td_fail("internal: the persistent GEMM cannot take this second operand source");
        else launch_gemm(L, ga, 0, s);
    } else if (L.route == CR_ADIRECT) {
        ConvArgs a = a0;
        a.Cin = 32 * nsteps; a.nsteps = nsteps; a.k_split = k_split; a.ld = ld; a.in2 = in2; a.ld2 = ld2; a.wp2 = wp2;
        if (resid || !conv_adirect_src2_supports(a, L.KS, 0)) rc = td_fail("internal: the direct 1x1 conv cannot take this second operand source");
        else conv_launch_adirect(a, 1, 0, s);
    } else rc = td_fail("internal: this conv's kernel has no second operand source");
    prof_end(n, s);
    return rc;
}

struct ConvCall { const ConvLayer* L; const float* in; int H, W; float* out; };
// Up to three independent convs in one launch when they share a kernel form (fp16 mode: the register-staged k_conv_igemm_h on the same tile,
// kernel size and storage types; `fusion` bit 131072); otherwise one launch each, in order.
// The grouping decision: a function of the options and the planned layers alone (the tests' operator entry has no handle).
static bool conv_group_same_form(const tdnet_opts& o, const ConvCall* c, int ng) {
    bool same = (o.fusion & TDNET_FUSION_CONV_GROUPS) && ng >= 2 && ng <= 3;
    for (int g = 0; same && g < ng; ++g) {
        const ConvLayer& L = *c[g].L;
        const ConvLayer& L0 = *c[0].L;
        same = L.route == CR_CONV_H && L.in16 == L.out16 && L.in16 == L0.in16 && (g == 0 ? (L.KS == 1 || L.KS == 3) : L.KS == 1) &&
               conv_tile_dims(L.tile).BM == conv_tile_dims(L0.tile).BM && conv_tile_dims(L.tile).BN == conv_tile_dims(L0.tile).BN;
    }
    return same;
}
// grouped (tests): whether the grouped kernel ran (1) or the members one by one (0)
static int run_conv_group(tdnet* n, const tdnet_opts& o, const ConvCall* c, int ng, hipStream_t s, int* Ho_out = nullptr, int* Wo_out = nullptr,   // Ho / Wo: of c[0]
                          int* grouped = nullptr) {
    const bool same = conv_group_same_form(o, c, ng);
    if (grouped) *grouped = same ? 1 : 0;
    if (!same) {
        for (int g = 0; g < ng; ++g) TD_TRY(run_conv(n, *c[g].L, c[g].in, c[g].H, c[g].W, nullptr, c[g].out, s, g == 0 ? Ho_out : nullptr, g == 0 ? Wo_out : nullptr));
        return 0;
    }
    ConvArgs a[3];
    double flops = 0.0;
    for (int g = 0; g < ng; ++g) {
        const ConvLayer& L = *c[g].L;
        a[g] = conv_args(L, c[g].in, c[g].H, c[g].W, nullptr, c[g].out);
        flops += L.flops_per_pixel() * a[g].M;
        if (g == 0 && Ho_out) *Ho_out = out_size(c[0].H, L.KS, L.stride, L.dil, L.pad);
        if (g == 0 && Wo_out) *Wo_out = a[0].Wo;
    }
    // a 3x3 conv on an fp16 map stays in the fp16 roofline's fixed layer set: the record carries ITS FLOP only (the launch's time includes the 1x1 beside it)
    const bool dom = c[0].L->in16 && c[0].L->KS == 3;
    prof_begin(n, 0, dom ? 4 : 0, dom ? c[0].L->flops_per_pixel() * a[0].M : flops, s);
    conv_launch_h_group(a, ng, c[0].L->tile, c[0].L->KS, c[0].L->in16, c[0].L->out16, s);
    prof_end(n, s);
    return 0;
}

// ln_part != nullptr: the kernel also writes the plane-LayerNorm strip statistics of `out` (one strip per 32-row query tile)
// vt16 (or the handle's n->vt16): the operand buffer of the fp16-MFMA kernel (tdnet_opts.precision = 1) or, with b3, of the split kernel (precision 2:
// td_attn_b3.h; the handle uses it for the FINAL attention of a frame only -- the cached-frame steps are hidden on the side stream either way)
static int run_attention(tdnet* n, const float* q, const float* k, const float* vp, const float* bias, const float* resid,
                         int Lq, int Lk, int DV, float* out, hipStream_t s, int online = 0, float* ln_part = nullptr,
                         _Float16* vt16 = nullptr, bool slices = false, bool vt_ready = false, int b3 = 0) {   // b3: 1 = the split kernels (form by size), 2 / 3 = the 32- / 64-query form (tests)
    if (n && n->vt16 && (n->opts.precision == 1 || b3)) vt16 = n->vt16;
    AttnArgs a;
    a.q = q; a.k = k; a.vp = vp; a.bias = bias; a.resid = resid; a.out = out; a.Lq = Lq; a.Lk = Lk;
    a.scale_log2e = 1.4426950408889634f / 8.0f;                        // temperature = sqrt(d_k) = 8 (transformer.py:65)
    a.ln_part = ln_part; a.ln_nstr = 0;
    if (n && (probe_skip() & 4) && Lq > Lk) return 0;
    prof_begin(n, 1, false, 2.0 * Lq * (double)Lk * (64 + DV), s);
    const int rc = (vt16 && b3) ? attn_launch_b3(a, DV, reinterpret_cast<unsigned short*>(vt16), s, vt_ready, b3 - 1)
                 : vt16 ? attn_launch_h(a, DV, vt16, s, vt_ready) : attn_launch(a, DV, online, s, slices);   // vt16: the fp16-MFMA kernel (tdnet_opts.precision = 1)
    prof_end(n, s);
    if (rc) return td_fail("attention: unsupported d_v=%d (128 or a multiple of 512)", DV);
    return 0;
}

// Plane LayerNorm (td4_psp18.py:306-312) in up to three launches: strip statistics (skipped when the attention epilogue already
// wrote them: stats_nstr > 0 strips of 32 rows), their exact combination, and the normalisation (skipped when y == nullptr: the
// head's Winograd input transform applies it on the fly, run_conv's LnFuse).
static void run_layernorm(tdnet* n, const float* x, int HW, int C, const float* g, const float* b, float* part, float* mean,
                          float* rstd, float* y, hipStream_t s, int stats_nstr = 0, bool y16 = false) {
    const int CV = C / 4, threads = CV > 256 ? CV : 256, rows = threads / CV;                   // C = 2048 (td4 on ResNet-50): 512 threads, one row each
    int nstr = stats_nstr, per = 32;
    prof_begin(n, 2, false, 0, s);
    if (!stats_nstr) {
        nstr = (HW + rows - 1) / rows;
        if (nstr > 512) nstr = 512;
        per = (HW + nstr - 1) / nstr;                                                           // k_ln_stats' strip length
        TD_LAUNCH(k_ln_stats, dim3(nstr), dim3(threads), (rows + 1) * C * 4, s, x, part, HW, C);   // part: [2][nstr][C]
    }
    TD_LAUNCH(k_ln_finalize, dim3((C + 3) / 4), dim3(256), (256 + 32 + 4) * 4, s, (const float*)part, nstr, per, HW, C, 1e-5f, mean, rstd);
    if (y && y16) TD_LAUNCH(k_ln_apply_h, dim3(td_grid_for((long)HW * CV)), dim3(256), 0, s, x, (const float*)mean, (const float*)rstd, g, b, (_Float16*)y, HW, C);
    else if (y) TD_LAUNCH(k_ln_apply, dim3(td_grid_for((long)HW * CV)), dim3(256), 0, s, x, (const float*)mean, (const float*)rstd, g, b, y, HW, C);
    prof_end(n, s);
}

static void launch_ppm_assemble(const float* c4, const float* ppmfeat, float* z, int h, int w, int C, int xs_off, int XS, int FS, hipStream_t s) {
    TD_LAUNCH(k_ppm_assemble, dim3(td_grid_for((long)h * w * (C / 4))), dim3(256), 0, s, c4, ppmfeat, z, h, w, C, xs_off, XS, FS);
}
// The G launch of the fold for the three first layers of a path's Encoding (g: the handle's buffers, one per layer)
static PpmFoldArgs ppm_fold_args(const ConvLayer* const L[3], float* const g[3], const float* ppmfeat, int XS, int FS) {
    PpmFoldArgs a;
    a.nl = 3; a.feat = ppmfeat; a.XS = XS; a.FS = FS; a.first[0] = 0;
    for (int i = 0; i < 3; ++i) { a.wp[i] = L[i]->d_wp; a.g[i] = g[i]; a.NPad[i] = L[i]->CoutPad; a.first[i + 1] = a.first[i] + L[i]->CoutPad / 64; }
    return a;
}
// XS = channels of c4 kept (c/path_num, offset pid*XS), FS = channels kept of each pyramid conv (c/(4 path_num))
// fold != nullptr (fusion bit 2097152, plan_enc_fold): z is not assembled; the pooled features go through the Encoding's first-layer weights instead
// (k_ppm_fold_g -> the G rows the two-source convs read).  As many launches either way.
static void run_ppm(tdnet* n, const float* c4, int h, int w, int C, int XS, int FS, const float* wgt, const float* bias, int pid,
                    float* rowpart, float* pooled, float* ppmfeat, float* z, hipStream_t s, const PpmFoldArgs* fold = nullptr) {
    prof_begin(n, 2, false, 0, s);
    const PpmAtoms at = ppm_atoms(w);                                 // the row is read once: atoms between the bin edges of all four levels
    (void)pooled;
    TD_LAUNCH(k_ppm_rowbins, dim3(h * ((C + 511) / 512)), dim3(1024), at.n * 512 * 4, s, c4, rowpart, w, C, at);   // rowpart: [h][12][C] row bins
    TD_LAUNCH(k_ppm_pool_conv, dim3(50 * (FS / 64)), dim3(256), (256 + C) * 4, s, (const float*)rowpart, wgt, bias, ppmfeat, h, w, C, FS);
    if (fold) TD_LAUNCH(k_ppm_fold_g, dim3(TD_PPM_BINS * fold->first[fold->nl]), dim3(256), 256 * 4, s, *fold);
    else launch_ppm_assemble(c4, ppmfeat, z, h, w, C, pid * XS, XS, FS, s);
    prof_end(n, s);
}

// The image of a frame as the caller handed it over: fp32 NCHW [3][H][W] at the network size, or uint8 HWC [Hs][Ws][3] at the source size the
// handle was configured for (tdnet_set_input_u8; `u8` = that configuration), or the NV12 surface tdnet_set_input_nv12 described, or the frame of which tdnet_set_input_view described a rectangle.  Everything behind the stem's image buffer is the same frame.
enum { TD_IMG_F32 = 0, TD_IMG_U8 = 1 };                               // TD_IMG_U8: the handle's byte input (U8Input: packed pixels or an NV12 surface, whole or a rectangle)
struct FrameInput { const void* p; int kind; const U8Input* u8; };
static inline FrameInput frame_input_f32(const float* img) { return FrameInput{img, TD_IMG_F32, nullptr}; }
// rows: the packed-row image of the 7x7 stem (ConvLayer::stem_rows(); img4 then holds [H + 7][W + 8][3] with a zero border) instead of NHWC4
// the kernels' description of the frame a byte input is (td_ingest.h SrcLayout; td_handle.h surf_form, surf_coeffs): packed pixels use pitch and origin only; an
// NV12 surface or view is the NV12 row of the layout table (SurfForm's default) with both planes on one pitch
static SrcLayout src_layout(const U8Input& u) {
    const SurfForm f = u.surf ? surf_form(u.layout) : SurfForm();
    return SrcLayout{u.pitch, u.surf ? u.cpitch : u.pitch, (unsigned)(u.surf ? u.u_off : u.uv_offset), (unsigned)(u.surf ? u.v_off : u.uv_offset),
                     f.lstride, f.loff, f.cshift, f.cstep, f.uo, f.vo, u.surf ? f.planes : u.nv12 ? 1 : 0,
                     u.coef[0], f.wide ? 512 : 128, u.coef[1], u.coef[2], u.coef[3], u.coef[4], u.coef[5], u.oy, u.ox};
}
static void run_stem_pre(tdnet* n, const FrameInput& in, int H, int W, float* img4, hipStream_t s, bool rows = false) {
    prof_begin(n, 2, false, 0, s);
    switch (in.kind) {
    case TD_IMG_U8: {                                                  // resize + normalise (+ colour conversion) + layout in the same one launch (td_ingest.h)
        const U8Input& u = *in.u8;
        const SrcLayout l = src_layout(u);
        const IngestArgs a = {(const unsigned char*)in.p, img4, u.lut, u.xt, u.yt, u.Hs, u.Ws, H, W, u.Wt, rows ? stem_rows_wp(W) : 0, u.resize ? 1 : 0,
                              u.span, u.span_c, (unsigned)u.extent};
        const dim3 grid((W + 4 * u.threads - 1) / (4 * u.threads), H), block(u.threads);
        const int lds = TD_INGEST_LUT_BYTES + 2 * u.span + 2 * l.planes * u.span_c;
#define TD_INGEST(...) TD_LAUNCH((k_ingest<__VA_ARGS__>), grid, block, lds, s, a, l)
        if (u.surf && l.mid == 512) TD_INGEST(IngestYuv<true, YuvFormArgs>);   // a YUV surface: the layout is arguments, the sample width the instantiation
        else if (u.surf) TD_INGEST(IngestYuv<false, YuvFormArgs>);
        else if (u.nv12) TD_INGEST(IngestYuv<false, YuvFormNv12>);      // the NV12 row as constants
        else if (u.bpp == 3 && !u.swap) TD_INGEST(IngestPacked<3, false>);   // the format is the instantiation: RGB24 pays nothing for the others
        else if (u.bpp == 3) TD_INGEST(IngestPacked<3, true>);
        else if (!u.swap) TD_INGEST(IngestPacked<4, false>);
        else TD_INGEST(IngestPacked<4, true>);
#undef TD_INGEST
        break;
    }
    default: {
        const float* img = (const float*)in.p;
        if (rows)
            TD_LAUNCH(k_nchw3_to_rgbpad, dim3(td_grid_for((long)H * ((W + 3) / 4))), dim3(256), 0, s, img, img4, H, W, stem_rows_wp(W));
        else
            TD_LAUNCH(k_nchw3_to_nhwc4, dim3(td_grid_for((long)H * W)), dim3(256), 0, s, img, img4, H * W);
    }
    }
    prof_end(n, s);
}
// pool16: 0 = fp32 in / fp32 out; the fp16-activation mode's first map: 1 = fp32 in (the stem's output) / fp16 out, 2 = fp16 in (deep stem) / fp16 out
static void run_maxpool(tdnet* n, const float* in, int H, int W, int C, float* out, hipStream_t s, int pool16 = 0) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    prof_begin(n, 2, false, 0, s);
    if (pool16) {
        if (pool16 == 2) TD_LAUNCH((k_maxpool3s2_h<true>), dim3(td_grid_for((long)Ho * Wo * (C / 4))), dim3(256), 0, s, (const void*)in, (_Float16*)out, H, W, C, Ho, Wo);
        else TD_LAUNCH((k_maxpool3s2_h<false>), dim3(td_grid_for((long)Ho * Wo * (C / 4))), dim3(256), 0, s, (const void*)in, (_Float16*)out, H, W, C, Ho, Wo);
    } else
        TD_LAUNCH(k_maxpool3s2, dim3(td_grid_for((long)Ho * Wo * (C / 4))), dim3(256), 0, s, in, out, H, W, C, Ho, Wo);
    prof_end(n, s);
}
// Both cache entries of a frame in one launch (td_misc.h k_subsample2): q_out [hk][wk][C1] = q[::4, ::4], v_out [hk][wk][C2] = v[::4, ::4] of maps
// w pixels wide; a lane per float4 of either output, the grid capped by td_grid_for (grid-stride beyond 2048 workgroups).
static void launch_cache_subsample(const float* q, float* q_out, int C1, const float* v, float* v_out, int C2, int w, int hk, int wk, hipStream_t s) {
    TD_LAUNCH(k_subsample2, dim3(td_grid_for((long)hk * wk * (C1 / 4 + C2 / 4))), dim3(256), 0, s, q, q_out, C1, v, v_out, C2, w, hk, wk, 4);
}
static int run_classifier(tdnet* n, const float* x, int HW, int C, int NC, const float* wgt, const float* bias, float* out, hipStream_t s) {
    if (C % 16 || C < 16) return td_fail("classifier: C=%d is not a positive multiple of 16", C);
    if (NC < 1 || NC > 256) return td_fail("classifier: NC=%d must be in 1..256", NC);
    // NC <= 32: all [NC][C] weights and the [4][NC][64] reduction in one workgroup's LDS, which ends at a CU's 160 KiB (32 classes: C <= 1024)
    if (NC <= 32 && !classifier_supports(NC, C)) return td_fail("classifier: NC=%d x C=%d needs %ld bytes of LDS, above a CU's %d", NC, C, classifier_lds(NC, C), TD_CU_LDS_BYTES);
    prof_begin(n, 2, false, 0, s);
    const int grid = (HW + 63) / 64, lds = (int)classifier_lds(NC, C);
    if (NC <= 19) TD_LAUNCH((k_classifier<19>), dim3(grid), dim3(256), lds, s, x, wgt, bias, out, HW, C, NC);
    else if (NC <= 32) TD_LAUNCH((k_classifier<32>), dim3(grid), dim3(256), lds, s, x, wgt, bias, out, HW, C, NC);
    else {                                                             // 33 .. 256 classes: 32-class tiles, each tile's weights in LDS
        if (!classifier_ct_supports(C)) { prof_end(n, s); return td_fail("classifier: C=%d is above the class-tiled kernel's 512 channels", C); }
        TD_LAUNCH(k_classifier_ct, dim3((NC + 31) / 32, grid), dim3(256), classifier_ct_lds(C), s, x, wgt, bias, out, HW, C, NC);
    }
    prof_end(n, s);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the output stage (td_out.h, td_score.h, td_conf.h, td_matte.h): one launch function per output form on the raw sizes -- the tests' operator entries have no
// handle -- and emit_output, the last launch of a frame, on top of them
// ---------------------------------------------------------------------------------------------------------------
static void launch_upsample(const float* in, int C, int h, int w, int H, int W, float* out, hipStream_t s) {
    if (W % 4 == 0 && ((size_t)out & 15) == 0 && H <= 65535 && C <= 65535) TD_LAUNCH(k_upsample_x4, dim3((W / 4 + 255) / 256, H, C), dim3(256), 0, s, in, out, C, h, w, H, W);
    else if (H <= 65535 && C <= 65535) TD_LAUNCH(k_upsample_row, dim3((W / 4 + 2 + 255) / 256, H, C), dim3(256), 0, s, in, out, C, h, w, H, W);
    else TD_LAUNCH(k_upsample, dim3(td_grid_for((long)C * H * W, 256, 256 * 16)), dim3(256), 0, s, in, out, C, h, w, H, W);
}
static void launch_upsample_argmax(const float* in, int C, int h, int w, int H, int W, int32_t* labels, hipStream_t s) {
    TD_LAUNCH(k_upsample_argmax, dim3(td_grid_for((long)H * W)), dim3(256), 0, s, in, labels, C, h, w, H, W);
}
static void launch_argmax(const float* logits, int C, long HW, int32_t* labels, hipStream_t s) {
    TD_LAUNCH(k_argmax, dim3(td_grid_for(HW)), dim3(256), 0, s, logits, labels, C, HW);
}
// The byte forms share one geometry: a lane per 4 pixels of a row (+ the head and tail lanes of a row that starts at any address), a grid row
// per output row (`rows`: H, or the picture's out_height), or the HW pixels of a frame as ONE run; and one class range, a label being a byte.
static int out_check(const char* what, const char* rows_name, int rows, int C) {
    if (rows > 65535) return td_fail("%s: %s = %d is above the grid's 65535 rows", what, rows_name, rows);
    if (C < 1 || C > 256) return td_fail("%s: nclass = %d must be in 1..256", what, C);
    return 0;
}
static dim3 out_grid(int W, int rows) { return dim3((W / 4 + 2 + 255) / 256, rows); }
static dim3 out_grid_run(long HW) { return dim3((unsigned)((HW / 4 + 2 + 255) / 256)); }

// uint8 labels: the fused upsample + argmax, and the argmax of full-resolution logits
static int launch_upsample_argmax_u8(const float* in, int C, int h, int w, int H, int W, unsigned char* labels, hipStream_t s) {
    TD_TRY(out_check("uint8 labels", "H", H, C));
    TD_LAUNCH(k_upsample_argmax_u8, out_grid(W, H), dim3(256), 0, s, in, labels, C, h, w, H, W);
    return 0;
}
static int launch_argmax_u8(const float* logits, int C, long HW, unsigned char* labels, hipStream_t s) {
    TD_TRY(out_check("uint8 labels", "H", 1, C));
    TD_LAUNCH(k_argmax_u8, out_grid_run(HW), dim3(256), 0, s, logits, labels, C, HW);
    return 0;
}
// ---- pictures (td_out.h "pictures out"): the colour map and the overlay, into a contiguous block or a destination view ----
// ONE dispatch: every (source form, destination form, sample width) cell that exists, label-map and fused form of each.  R: k_picture_rows, B: k_picture_420.
// A frame with a destination in force reads a packed or NV12 source through the view reader (DESIGN.md 5.12 bounds the count that way): the tight forms
// exist for the contiguous block only.  YuvFormNv12 takes no surface source: behind one, the NV12 view goes through the argument form.
#define TD_PICTURE_CELLS(R, B) \
    R(NONE, RGB) R(P24T, RGB) R(P24, RGB) R(P32, RGB) R(NV12T, RGB) R(NV12, RGB) R(SURF8, RGB) R(SURF16, RGB) \
    R(NONE, P24) R(P24, P24) R(P32, P24) R(NV12, P24) R(SURF8, P24) R(SURF16, P24) \
    R(NONE, P32) R(P24, P32) R(P32, P32) R(NV12, P32) R(SURF8, P32) R(SURF16, P32) \
    B(NONE, NV12, false, YuvFormNv12) B(P24, NV12, false, YuvFormNv12) B(P32, NV12, false, YuvFormNv12) B(NV12, NV12, false, YuvFormNv12) \
    B(NONE, YUV420, false, YuvFormArgs) B(P24, YUV420, false, YuvFormArgs) B(P32, YUV420, false, YuvFormArgs) B(NV12, YUV420, false, YuvFormArgs) \
    B(SURF8, YUV420, false, YuvFormArgs) B(SURF16, YUV420, false, YuvFormArgs) \
    B(NONE, YUV420, true, YuvFormArgs) B(P24, YUV420, true, YuvFormArgs) B(P32, YUV420, true, YuvFormArgs) B(NV12, YUV420, true, YuvFormArgs) \
    B(SURF8, YUV420, true, YuvFormArgs) B(SURF16, YUV420, true, YuvFormArgs)
#define TD_PICTURE_KEY(src, dst, wide) (((src) * 8 + (dst)) * 2 + ((wide) ? 1 : 0))   // (launch_composite's own switch reuses the key with its third argument = the alpha mode)
// a.labels != NULL: the label-map form.  src, l: the overlay's source (TD_SRC_NONE: unused).  wide: a 4:2:0 destination of 16-bit samples.
static int launch_picture(const PicArgs& a, int src_form, const unsigned char* src, const SrcLayout& l, int dst_form, bool wide, const PicDst& d, hipStream_t s) {
    const bool labels = a.labels != nullptr;
    const dim3 rows = out_grid(a.ow, a.oh), blocks(((a.ow + 3) / 4 + 255) / 256, (a.oh + 1) / 2);
    switch (TD_PICTURE_KEY(src_form, dst_form, wide)) {
#define TD_R(SRC, DST) case TD_PICTURE_KEY(TD_SRC_##SRC, TD_DST_##DST, false): \
        if (labels) TD_LAUNCH((k_picture_rows<true, TD_SRC_##SRC, TD_DST_##DST>), rows, dim3(256), 0, s, a, src, l, d); \
        else TD_LAUNCH((k_picture_rows<false, TD_SRC_##SRC, TD_DST_##DST>), rows, dim3(256), 0, s, a, src, l, d); \
        return 0;
#define TD_B(SRC, DST, WIDE, F) case TD_PICTURE_KEY(TD_SRC_##SRC, TD_DST_##DST, WIDE): \
        if (labels) TD_LAUNCH((k_picture_420<true, TD_SRC_##SRC, WIDE, F>), blocks, dim3(256), 0, s, a, src, l, d); \
        else TD_LAUNCH((k_picture_420<false, TD_SRC_##SRC, WIDE, F>), blocks, dim3(256), 0, s, a, src, l, d); \
        return 0;
    TD_PICTURE_CELLS(TD_R, TD_B)
#undef TD_R
#undef TD_B
    }
    return td_fail("internal: no picture kernel for source form %d into destination form %d", src_form, dst_form);
}
// the source form of a byte input (`u`; td_out.h TD_SRC_*).  tight: the destination is the contiguous block, so the whole tight frame may take the form
// whose origin and pitch are constants; a VIEW is an origin, 4-byte pixels, or packed rows with a pitch
static int picture_src_form(const U8Input& u, bool tight) {
    if (u.surf) return surf_form(u.layout).wide ? TD_SRC_SURF16 : TD_SRC_SURF8;
    const bool view = !tight || u.oy || u.ox || u.bpp == 4 || (!u.nv12 && u.pitch != 3 * u.Ws);
    if (u.nv12) return view ? TD_SRC_NV12 : TD_SRC_NV12T;
    return u.bpp == 4 ? TD_SRC_P32 : view ? TD_SRC_P24 : TD_SRC_P24T;
}
static int overlay_check_tables(const OverlayOutput& o, const U8Input& u) {
    if (!o.Hs || o.Hs != u.Hs || o.Ws != u.Ws || o.H != u.H || o.W != u.W) return td_fail("overlay: the index tables of this source size are missing (their allocation failed)");
    if (o.swap != u.swap) return td_fail("overlay: the colour table is not in the source's colour order (its upload failed)");
    return 0;
}
// the colour map [oh][ow][3] of a frame (tdnet_set_output_rgb; `r` = that configuration) or its overlay [Hs][Ws][3] (tdnet_set_output_overlay; `o` = that
// configuration): from the low-resolution logits, evaluated at the sampled pixels only, or (labels != NULL) from a uint8 label map [H][W]
static PicArgs picture_args(const float* in, const unsigned char* labels, int C, int h, int w, const RgbOutput& r) {
    return PicArgs{in, labels, r.ys, r.xs, r.lut, C, h, w, r.H, r.W, r.oh, r.ow};
}
static PicArgs picture_args(const float* in, const unsigned char* labels, int C, int h, int w, const OverlayOutput& o) {
    return PicArgs{in, labels, o.ys, o.xs, o.lut, C, h, w, o.H, o.W, o.Hs, o.Ws};
}
static PicDst picture_block(unsigned char* out) { PicDst d = PicDst(); d.base = out; return d; }
static int launch_upsample_argmax_rgb(const float* in, int C, int h, int w, const RgbOutput& r, unsigned char* rgb, hipStream_t s) {
    TD_TRY(out_check("colour map", "out_height", r.oh, C));
    return launch_picture(picture_args(in, nullptr, C, h, w, r), TD_SRC_NONE, nullptr, SrcLayout(), TD_DST_RGB, false, picture_block(rgb), s);
}
static int launch_labels_rgb(const unsigned char* labels, const RgbOutput& r, unsigned char* rgb, hipStream_t s) {
    TD_TRY(out_check("colour map", "out_height", r.oh, 1));
    return launch_picture(picture_args(nullptr, labels, 0, 0, 0, r), TD_SRC_NONE, nullptr, SrcLayout(), TD_DST_RGB, false, picture_block(rgb), s);
}
// `u` = the byte input `src` is read by
static int launch_upsample_argmax_overlay(const float* in, int C, int h, int w, const OverlayOutput& o, const U8Input& u, const unsigned char* src,
                                          unsigned char* out, hipStream_t s) {
    TD_TRY(out_check("overlay", "src_height", o.Hs, C));
    TD_TRY(overlay_check_tables(o, u));
    return launch_picture(picture_args(in, nullptr, C, h, w, o), picture_src_form(u, true), src, src_layout(u), TD_DST_RGB, false, picture_block(out), s);
}
static int launch_labels_overlay(const unsigned char* labels, const OverlayOutput& o, const U8Input& u, const unsigned char* src, unsigned char* out, hipStream_t s) {
    TD_TRY(out_check("overlay", "src_height", o.Hs, 1));
    TD_TRY(overlay_check_tables(o, u));
    return launch_picture(picture_args(nullptr, labels, 0, 0, 0, o), picture_src_form(u, true), src, src_layout(u), TD_DST_RGB, false, picture_block(out), s);
}
// The picture into a destination view (tdnet_set_output_view / tdnet_set_output_surface; `d` = that configuration, `base` = the destination frame's base): the
// colour map (r != NULL) or the overlay (o, u, src), from the low-resolution logits (labels == NULL) or from a uint8 label map.  One launch, like the contiguous
// forms.  The picture's size must be the rectangle's: the frame entries check that before anything is enqueued (td_model.hip picture_dst_check), and here again.
static int launch_picture_dst(const float* in, int C, int h, int w, const unsigned char* labels, const RgbOutput* r, const OverlayOutput* o, const U8Input* u,
                              const unsigned char* src, const DstOutput& d, unsigned char* base, hipStream_t s) {
    const char* what = r ? "colour map" : "overlay";
    if (!r) TD_TRY(overlay_check_tables(*o, *u));
    const PicArgs a = r ? picture_args(in, labels, C, h, w, *r) : picture_args(in, labels, C, h, w, *o);
    TD_TRY(out_check(what, "height", a.oh, labels ? 1 : C));
    if (!d.set || a.oh != d.h || a.ow != d.w) return td_fail("%s: the picture %d x %d is not the destination rectangle %d x %d", what, a.oh, a.ow, d.h, d.w);
    const bool src_bgr = !r && u->swap;                                // the picture word's bytes are b g r: the overlay's table and source are
    const bool src_surf = !r && u->surf;
    const bool yuv = d.format == TDNET_PIX_NV12;                       // a 4:2:0 destination: the NV12 view, or a surface
    const SurfForm f = d.surf ? surf_form(d.layout) : SurfForm();      // the view: the NV12 row, both planes on one pitch
    PicDst pd = PicDst();
    pd.base = base; pd.pitch = d.pitch; pd.cpitch = d.surf ? d.cpitch : d.pitch;
    pd.u_off = (unsigned)(d.surf ? d.u_off : d.uv_offset); pd.v_off = (unsigned)(d.surf ? d.v_off : d.uv_offset);
    pd.oy = d.oy; pd.ox = d.ox; pd.swap = !yuv && d.swap != src_bgr;
    pd.cstep = f.cstep; pd.uo = f.uo; pd.vo = f.vo; pd.yoff = d.yoff;
    for (int i = 0; i < 3; ++i) {                                      // 4:2:0 behind a b g r picture: the r and b constants exchanged
        const int k = src_bgr ? 2 - i : i;
        pd.ky[i] = d.ky[k]; pd.ku[i] = d.ku[k]; pd.kv[i] = d.kv[k];
    }
    // An NV12 surface whose planes share one pitch IS the NV12 view: its layout is constants.  Every other surface, and any 4:2:0 destination behind a surface
    // source, takes its layout from the arguments.
    const bool plain_nv12 = !d.surf || (d.layout == TDNET_SURF_NV12 && d.cpitch == d.pitch);
    const int dst_form = !yuv ? (d.bpp == 4 ? TD_DST_P32 : TD_DST_P24) : (src_surf || !plain_nv12) ? TD_DST_YUV420 : TD_DST_NV12;
    return launch_picture(a, r ? TD_SRC_NONE : picture_src_form(*u, false), src, r ? SrcLayout() : src_layout(*u), dst_form, yuv && f.wide, pd, s);
}
// score out (td_score.h): cm[map[gt]][label] += 1 over a frame, labels from the low-resolution logits (optionally written too: labels may be
// NULL) or from a uint8 label map the caller holds.  A private LDS histogram per workgroup up to TD_SCORE_LDS_CLASSES classes, straight
// global atomics above.  The wave-uniform path is OFF in the library's entries until tools/score_probe.py has shown on the device that it
// pays on coherent input and costs nothing on noise (not measured yet); the tests' operator entry can run either form.
#define TD_SCORE_WAVE_UNIFORM false
static int score_lds_bins(int C) { return C <= TD_SCORE_LDS_CLASSES ? C * C : 0; }
static int launch_upsample_argmax_score(const float* in, int C, int h, int w, int H, int W, const unsigned char* gt, const unsigned char* map,
                                        unsigned char* labels, unsigned long long* cm, hipStream_t s, bool uniform = TD_SCORE_WAVE_UNIFORM) {
    TD_TRY(out_check("score", "H", H, C));
    const int bins = score_lds_bins(C);
    if (uniform) TD_LAUNCH((k_upsample_argmax_score<true>), out_grid(W, H), dim3(256), bins * sizeof(unsigned), s, in, gt, map, labels, cm, C, h, w, H, W, bins);
    else TD_LAUNCH((k_upsample_argmax_score<false>), out_grid(W, H), dim3(256), bins * sizeof(unsigned), s, in, gt, map, labels, cm, C, h, w, H, W, bins);
    return 0;
}
static int launch_labels_score(const unsigned char* labels, int C, int H, int W, const unsigned char* gt, const unsigned char* map, unsigned long long* cm,
                               hipStream_t s, bool uniform = TD_SCORE_WAVE_UNIFORM) {
    TD_TRY(out_check("score", "H", H, C));
    const int bins = score_lds_bins(C);
    if (uniform) TD_LAUNCH((k_labels_score<true>), out_grid(W, H), dim3(256), bins * sizeof(unsigned), s, labels, gt, map, cm, C, W, bins);
    else TD_LAUNCH((k_labels_score<false>), out_grid(W, H), dim3(256), bins * sizeof(unsigned), s, labels, gt, map, cm, C, W, bins);
    return 0;
}
// confidence out (td_conf.h): the label entries' last launch that also writes the confidence byte of every pixel and rejects labels below
// min_conf (labels may be NULL: confidence only), and the unfused form on full-resolution logits the caller holds.  TD_CONF_ONLINE: the
// one-pass form (running maximum, rescaled running sum: the gathers once) in the library's entries; the tests' operator entry can run
// either form (DESIGN.md 5.8 has the measurement).
#define TD_CONF_ONLINE true
static int conf_check(int C, int H, int min_conf, int reject) {
    TD_TRY(out_check("confidence", "H", H, C));
    if (min_conf < 0 || min_conf > 255 || reject < 0 || reject > 255) return td_fail("confidence: min_conf = %d and reject_label = %d must be in 0..255", min_conf, reject);
    return 0;
}
static int launch_upsample_argmax_conf_u8(const float* in, int C, int h, int w, int H, int W, unsigned char* labels, unsigned char* conf, int min_conf, int reject,
                                          hipStream_t s, bool online = TD_CONF_ONLINE) {
    TD_TRY(conf_check(C, H, min_conf, reject));
    if (online) TD_LAUNCH((k_upsample_argmax_conf_u8<true>), out_grid(W, H), dim3(256), 0, s, in, labels, conf, C, h, w, H, W, min_conf, reject);
    else TD_LAUNCH((k_upsample_argmax_conf_u8<false>), out_grid(W, H), dim3(256), 0, s, in, labels, conf, C, h, w, H, W, min_conf, reject);
    return 0;
}
static int launch_logits_conf_u8(const float* logits, int C, long HW, unsigned char* labels, unsigned char* conf, int min_conf, int reject, hipStream_t s,
                                 bool online = TD_CONF_ONLINE) {
    TD_TRY(conf_check(C, 1, min_conf, reject));
    if (online) TD_LAUNCH((k_logits_conf_u8<true>), out_grid_run(HW), dim3(256), 0, s, logits, labels, conf, C, HW, min_conf, reject);
    else TD_LAUNCH((k_logits_conf_u8<false>), out_grid_run(HW), dim3(256), 0, s, logits, labels, conf, C, HW, min_conf, reject);
    return 0;
}
// matte out (td_matte.h): the label entries' last launch that also writes the softmax mass of the class set `set` as a byte per pixel (labels may
// be NULL: matte only), and the unfused form on full-resolution logits the caller holds.  The set is a kernel argument: eight words by value.
static int launch_upsample_argmax_matte_u8(const float* in, int C, int h, int w, int H, int W, unsigned char* labels, unsigned char* matte, const MatteSet& set,
                                           hipStream_t s) {
    TD_TRY(out_check("matte", "H", H, C));
    TD_LAUNCH(k_upsample_argmax_matte_u8, out_grid(W, H), dim3(256), 0, s, in, labels, matte, C, h, w, H, W, set);
    return 0;
}
static int launch_logits_matte_u8(const float* logits, int C, long HW, unsigned char* labels, unsigned char* matte, const MatteSet& set, hipStream_t s) {
    TD_TRY(out_check("matte", "H", 1, C));
    TD_LAUNCH(k_logits_matte_u8, out_grid_run(HW), dim3(256), 0, s, logits, labels, matte, C, HW, set);
    return 0;
}
// The composite (td_matte.h k_composite_rows): the source frame through the matte at the source's size, from the low-resolution logits and the class
// set (map == NULL) or from a matte map [H][W] the caller holds.  `o`: the index tables of the pair (network size, source size); `u`: the byte input `src`
// is read by; `d`: the destination view in force, or one that is not set: the contiguous block [Hs][Ws][3] at `base`.
// 40 instantiations: 5 source forms (a view of 3- / 4-byte pixels, an NV12 view, a surface of 8- / 16-bit samples: a tight whole frame is a view with
// origin 0) x 4 destinations (the block, a 3-byte view, a 4-byte view, a 4-byte view with the matte as its x byte) x fused / from a map.
#define TD_COMPOSITE_SRCS(X, DST, ALPHA) X(P24, DST, ALPHA) X(P32, DST, ALPHA) X(NV12, DST, ALPHA) X(SURF8, DST, ALPHA) X(SURF16, DST, ALPHA)
#define TD_COMPOSITE_CELLS(X) TD_COMPOSITE_SRCS(X, RGB, false) TD_COMPOSITE_SRCS(X, P24, false) TD_COMPOSITE_SRCS(X, P32, false) TD_COMPOSITE_SRCS(X, P32, true)
// What the destination in force must be for the composite of byte input `u` in mode c.mode: ONE set of checks and messages, for the frame entries (on the
// host, before anything is enqueued: td_model.hip composite_args) and for the launch itself (the tests' operator entry has no handle).
static int composite_dst_check(const U8Input& u, const CompositeOutput& c, const DstOutput& d, const char* who) {
    static const char* const fmt[] = {"RGB24", "BGR24", "RGBA32", "BGRA32", "NV12"};
    if (d.set && d.format == TDNET_PIX_NV12)
        return td_fail("%s: the destination in force is %s: composite into 4:2:0 is not built (tdnet_set_output_view with a packed format, or NULL)", who,
                       d.surf ? "a 4:2:0 surface (tdnet_set_output_surface)" : "an NV12 view");
    if (c.mode == TDNET_COMPOSITE_ALPHA && !(d.set && d.bpp == 4))
        return td_fail("%s: TDNET_COMPOSITE_ALPHA writes the matte as the x byte of an RGBA32 / BGRA32 destination view, but the destination in force is %s", who,
                       d.set ? fmt[d.format] : "the contiguous [Hs][Ws][3] block (no tdnet_set_output_view)");
    if (d.set && (u.Hs != d.h || u.Ws != d.w))
        return td_fail("%s: the composite is %d x %d but the destination view's rectangle is %d x %d (tdnet_set_output_view: nothing is resized)", who, u.Hs, u.Ws, d.h, d.w);
    return 0;
}
// rf != NULL: `map` is a map at the SOURCE's size (the refined matte in rf's workspace), read through rf's identity tables with W = Ws: the same kernels.
static int launch_composite(const float* in, int C, int h, int w, const unsigned char* map, const MatteSet& set, const OverlayOutput& o, const U8Input& u,
                            const unsigned char* src, const CompositeOutput& c, const DstOutput& d, unsigned char* base, hipStream_t s, const RefineState* rf = nullptr) {
    if (!o.Hs || o.Hs != u.Hs || o.Ws != u.Ws || o.H != u.H || o.W != u.W) return td_fail("composite: the index tables of this source size are missing (their allocation failed)");
    TD_TRY(out_check("composite", "src_height", o.Hs, map ? 1 : C));
    TD_TRY(composite_dst_check(u, c, d, "composite"));
    const bool alpha = c.mode == TDNET_COMPOSITE_ALPHA;
    CompArgs a = CompArgs();
    a.in = in; a.map = map; a.ys = o.ys; a.xs = o.xs;
    a.C = C; a.h = h; a.w = w; a.H = o.H; a.W = o.W; a.oh = o.Hs; a.ow = o.Ws;
    if (rf) { a.ys = rf->idy; a.xs = rf->idx; a.H = rf->Hs; a.W = rf->Ws; }
    a.bg = u.swap ? (unsigned)c.bg[2] | ((unsigned)c.bg[1] << 8) | ((unsigned)c.bg[0] << 16)      // the picture word's bytes are the source's: b g r
                  : (unsigned)c.bg[0] | ((unsigned)c.bg[1] << 8) | ((unsigned)c.bg[2] << 16);
    a.set = set;
    PicDst pd = PicDst();
    pd.base = base;
    if (d.set) { pd.pitch = d.pitch; pd.oy = d.oy; pd.ox = d.ox; pd.swap = d.swap != u.swap; }
    const int dst_form = !d.set ? TD_DST_RGB : d.bpp == 4 ? TD_DST_P32 : TD_DST_P24;
    const int src_form = picture_src_form(u, false);
    const SrcLayout l = src_layout(u);
    const dim3 rows = out_grid(a.ow, a.oh);
    switch (TD_PICTURE_KEY(src_form, dst_form, alpha)) {
#define TD_C(SRC, DST, ALPHA) case TD_PICTURE_KEY(TD_SRC_##SRC, TD_DST_##DST, ALPHA): \
        if (map) TD_LAUNCH((k_composite_rows<true, TD_SRC_##SRC, TD_DST_##DST, ALPHA>), rows, dim3(256), 0, s, a, src, l, pd); \
        else TD_LAUNCH((k_composite_rows<false, TD_SRC_##SRC, TD_DST_##DST, ALPHA>), rows, dim3(256), 0, s, a, src, l, pd); \
        return 0;
    TD_COMPOSITE_CELLS(TD_C)
#undef TD_C
    }
    return td_fail("internal: no composite kernel for source form %d into destination form %d", src_form, dst_form);
}
// refined matte (td_refine.h): the guided filter of a matte byte map with a guide byte map of the same size, two launches.  The scratch holds the
// coefficient planes: b_q int32 [rows][cols], then a_q int16 [rows][cols] -- 6 bytes per pixel, 4-byte aligned.
static_assert(TD_RF_MAX_RADIUS == TDNET_REFINE_MAX_RADIUS && TD_RF_MIN_EPS == TDNET_REFINE_MIN_EPS && TD_RF_MAX_EPS == TDNET_REFINE_MAX_EPS && TDNET_REFINE_OP_LAUNCHES == 2 && TDNET_REFINE_LAUNCHES == 3,
              "td_refine.h and include/tdnet.h disagree");
static size_t refine_scratch_bytes(int rows, int cols) { return rows < 1 || cols < 1 ? 0 : (size_t)6 * (size_t)rows * (size_t)cols; }
static int refine_range_check(int radius, int eps, const char* who) {
    if (radius < 1 || radius > TD_RF_MAX_RADIUS) return td_fail("%s: radius = %d must be in 1..%d", who, radius, TD_RF_MAX_RADIUS);
    if (eps < TD_RF_MIN_EPS || eps > TD_RF_MAX_EPS) return td_fail("%s: eps = %d must be in %d..%d (squared byte units)", who, eps, TD_RF_MIN_EPS, TD_RF_MAX_EPS);
    return 0;
}
static int refine_size_check(int rows, int cols, const char* who) {
    if (rows < 1 || cols < 1 || rows > 65535 || cols > 65535 || (long)rows * cols > TD_RG_MAX_PIXELS)
        return td_fail("%s: a map of %d x %d is outside 1..65535 per side and 2^30 - 16 pixels", who, rows, cols);
    return 0;
}
static bool refine_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}
static size_t refine_extent(size_t pitch, int rows, int cols) { return (size_t)(rows - 1) * pitch + (size_t)cols; }
// every check of the operator, before anything is enqueued; want_out false: the coefficient launch alone (the tests' entry): no output, and the scratch may be NULL
static int refine_args_check(const unsigned char* guide, size_t gpitch, const unsigned char* matte, size_t mpitch, const unsigned char* out, size_t opitch, bool want_out,
                             int rows, int cols, int radius, int eps, const void* scratch, const char* who) {
    if (!guide || !matte || (want_out && (!out || !scratch))) return td_fail("%s: null argument", who);
    TD_TRY(refine_size_check(rows, cols, who));
    TD_TRY(refine_range_check(radius, eps, who));
    if (gpitch < (size_t)cols) return td_fail("%s: guide_pitch = %zu is below cols = %d", who, gpitch, cols);
    if (mpitch < (size_t)cols) return td_fail("%s: matte_pitch = %zu is below cols = %d", who, mpitch, cols);
    if (want_out && opitch < (size_t)cols) return td_fail("%s: out_pitch = %zu is below cols = %d", who, opitch, cols);
    if (!scratch) return 0;                                            // the tests' coefficient entry allocates its own behind these checks
    if ((size_t)scratch & 3u) return td_fail("%s: scratch_dev = %p is not 4-byte aligned", who, scratch);
    const size_t ng = refine_extent(gpitch, rows, cols), nm = refine_extent(mpitch, rows, cols), ns = refine_scratch_bytes(rows, cols);
    if (refine_overlap(scratch, ns, guide, ng)) return td_fail("%s: the scratch overlaps the guide (%zu bytes at %p against %zu bytes at %p)", who, ns, scratch, ng, (const void*)guide);
    if (refine_overlap(scratch, ns, matte, nm)) return td_fail("%s: the scratch overlaps the matte (%zu bytes at %p against %zu bytes at %p)", who, ns, scratch, nm, (const void*)matte);
    if (!want_out) return 0;
    const size_t no = refine_extent(opitch, rows, cols);
    if (refine_overlap(out, no, guide, ng)) return td_fail("%s: out overlaps the guide (%zu bytes at %p against %zu bytes at %p)", who, no, (const void*)out, ng, (const void*)guide);
    if (refine_overlap(out, no, matte, nm)) return td_fail("%s: out overlaps the matte (%zu bytes at %p against %zu bytes at %p)", who, no, (const void*)out, nm, (const void*)matte);
    if (refine_overlap(out, no, scratch, ns)) return td_fail("%s: out overlaps the scratch (%zu bytes at %p against %zu bytes at %p)", who, no, (const void*)out, ns, scratch);
    return 0;
}
static int* refine_bq(void* scratch) { return (int*)scratch; }
static short* refine_aq(void* scratch, int rows, int cols) { return (short*)((char*)scratch + (size_t)4 * rows * cols); }
// the arguments are checked (refine_args_check); radius and eps travel as kernel arguments: a captured graph replays those of capture time
static void launch_refine_coeff(const unsigned char* guide, size_t gpitch, const unsigned char* matte, size_t mpitch, int rows, int cols, int radius, int eps, void* scratch,
                                hipStream_t s) {
    TD_LAUNCH(k_refine_coeff, dim3((cols + TD_RF_TX - 1) / TD_RF_TX, (rows + TD_RF_CY - 1) / TD_RF_CY), dim3(256), td_rf_coeff_lds(radius), s, guide, gpitch, matte, mpitch,
              refine_aq(scratch, rows, cols), refine_bq(scratch), rows, cols, radius, eps);
}
static void launch_refine_apply(const unsigned char* guide, size_t gpitch, unsigned char* out, size_t opitch, int rows, int cols, int radius, void* scratch, hipStream_t s) {
    TD_LAUNCH(k_refine_apply, dim3((cols + TD_RF_TX - 1) / TD_RF_TX, (rows + TD_RF_AY - 1) / TD_RF_AY), dim3(256), td_rf_apply_lds(radius), s, guide, gpitch,
              (const short*)refine_aq(scratch, rows, cols), (const int*)refine_bq(scratch), out, opitch, rows, cols, radius);
}
// regions out (td_regions.h): the seven launches, from the low-resolution logits (in != NULL: the first launch is the frame's label launch too and writes the
// label bytes to labels_out, or to the workspace's map where the caller asks for none) or from a uint8 label map [H][W] the caller holds (labels_in, at any
// byte address).  ids: int32 [H][W] or NULL.  table: regions_table_bytes(r.max_regions) bytes, 8-byte aligned.  `r`: the workspace of this H x W and the
// configuration, read NOW (kernel arguments: a captured graph replays the ones it was captured with).  Only enqueues: every buffer is zeroed by a kernel.
static_assert(TD_REGIONS_LAUNCHES == TDNET_REGIONS_LAUNCHES && TD_RG_OVERFLOW == TDNET_REGIONS_OVERFLOW && TD_RG_BOUND == TDNET_REGIONS_BOUND &&
              sizeof(TdRegion) == sizeof(tdnet_region) && sizeof(TdRegionsHeader) == sizeof(tdnet_regions_header), "td_regions.h and include/tdnet.h disagree");
static int regions_table_check(const void* table, const char* who) {
    if (!table) return td_fail("%s: regions_dev is NULL", who);
    if ((size_t)table & 7u) return td_fail("%s: regions_dev = %p is not 8-byte aligned", who, table);
    return 0;
}
static int run_regions(const float* in, int C, int h, int w, int H, int W, const unsigned char* labels_in, unsigned char* labels_out, int32_t* ids, void* table,
                       const RegionsOutput& r, hipStream_t s, const char* who) {
    TD_TRY(regions_table_check(table, who));
    TD_TRY(regions_size_check(H, W, who));
    if (C < 1 || C > 256) return td_fail("%s: nclass = %d must be in 1..256", who, C);
    if (!r.parent || r.H != H || r.W != W) return td_fail("%s: internal: the regions workspace is not that of a %d x %d map", who, H, W);
    if (r.conn != 4 && r.conn != 8) return td_fail("%s: connectivity = %d must be 4 or 8", who, r.conn);
    if (r.max_regions < 1 || r.max_regions > 65536 || r.min_area < 1) return td_fail("%s: max_regions = %d must be in 1..65536 and min_area = %d at least 1", who, r.max_regions, r.min_area);
    RegionsArgs a = RegionsArgs();
    a.in = in; a.labels = in ? (labels_out ? labels_out : r.lab) : labels_in;
    a.ids = ids; a.table = (unsigned long long*)table;
    a.parent = r.parent; a.root = r.root; a.area = r.area; a.blk = r.blk; a.flag = r.flag;
    a.C = C; a.h = h; a.w = w; a.H = H; a.W = W;
    a.conn = r.conn; a.max_regions = r.max_regions; a.min_area = r.min_area;
    a.set = r.classes;
    a.zero = 0;                                                        // K2's read operand (td_regions.h td_rg_read): a zero the compiler cannot see
    const dim3 tiles((W + TD_RG_TW - 1) / TD_RG_TW, (H + TD_RG_TH - 1) / TD_RG_TH);
    const long words = (long)(regions_table_bytes(r.max_regions) / 8), nblk = regions_blocks(H, W);
    const long row_lanes = (long)((H - 1) / TD_RG_TH) * W, col_lanes = (long)((W - 1) / TD_RG_TW) * H, lanes = row_lanes + (r.conn == 8 ? 2 : 1) * col_lanes;
    const size_t tile_lds = 2 * TD_RG_TW * TD_RG_TH * sizeof(int);
    if (in) TD_LAUNCH((k_regions_tile<true>), tiles, dim3(256), tile_lds, s, a, words);
    else TD_LAUNCH((k_regions_tile<false>), tiles, dim3(256), tile_lds, s, a, words);
    TD_LAUNCH(k_regions_merge, dim3((unsigned)std::max<long>(1, (lanes + 255) / 256)), dim3(256), 0, s, a, row_lanes, col_lanes);
    TD_LAUNCH(k_regions_flatten, dim3((unsigned)nblk), dim3(256), 0, s, a);
    TD_LAUNCH(k_regions_count, dim3((unsigned)nblk), dim3(256), 4 * sizeof(int), s, a);
    TD_LAUNCH(k_regions_scan, dim3(1), dim3(256), 256 * sizeof(int), s, a, (int)nblk);
    TD_LAUNCH(k_regions_number, dim3((unsigned)nblk), dim3(256), 260 * sizeof(int), s, a);
    TD_LAUNCH(k_regions_stats, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return 0;
}
// tracks out (td_tracks.h): the four launches behind run_regions, on the id map and the regions table the same call wrote.  ids: the current id map (the
// caller's, or the state's own map where the caller asked for none).  table: tracks_table_bytes(max_regions) bytes, 8-byte aligned.  min_overlap is read
// NOW (a kernel argument).  Only enqueues: the state is zeroed by the kernels themselves.
static_assert(TD_TRACKS_LAUNCHES == TDNET_TRACKS_LAUNCHES && TD_TK_BOUND == TDNET_TRACKS_BOUND && sizeof(TdTrack) == sizeof(tdnet_track) &&
              sizeof(TdTracksHeader) == sizeof(tdnet_tracks_header), "td_tracks.h and include/tdnet.h disagree");
static int tracks_table_check(const void* table, const char* who) {
    if (!table) return td_fail("%s: tracks_dev is NULL", who);
    if ((size_t)table & 7u) return td_fail("%s: tracks_dev = %p is not 8-byte aligned", who, table);
    return 0;
}
static int run_tracks(int H, int W, const int32_t* ids, const void* rtable, int32_t* track_ids, void* table, const TracksState& st, int max_regions, int min_overlap,
                      hipStream_t s, const char* who) {
    TD_TRY(tracks_table_check(table, who));
    TD_TRY(regions_size_check(H, W, who));
    if (!st.words || !ids || !rtable) return td_fail("%s: internal: the track state is not allocated", who);
    if (min_overlap < 1) return td_fail("%s: min_overlap = %d must be at least 1", who, min_overlap);
    TracksArgs a = TracksArgs();
    a.st = st; a.ids = ids; a.rtable = (const td_u64*)rtable; a.table = (td_u64*)table; a.track_ids = track_ids;
    a.H = H; a.W = W; a.max_regions = max_regions; a.min_overlap = min_overlap;
    const long nblk = regions_blocks(H, W), cap = 1l << st.lg, words = (long)(tracks_table_bytes(max_regions) / 8);
    const long HW = (long)H * W;
    TD_LAUNCH(k_tracks_pairs, dim3((unsigned)nblk), dim3(256), 0, s, a);
    TD_LAUNCH(k_tracks_best, dim3((unsigned)std::max<long>(1, (cap + 255) / 256)), dim3(256), 0, s, a, words);
    TD_LAUNCH(k_tracks_resolve, dim3(1), dim3(TD_TK_WG), (TD_TK_WG + TD_TK_WG / 64) * sizeof(int), s, a);
    TD_LAUNCH(k_tracks_commit, dim3((unsigned)nblk), dim3(256), 0, s, a, (int)std::min<long>(TD_TK_MAX_REGIONS, HW));
    return 0;
}
// runs out (td_runs.h): the three launches behind a map the caller or the frame's label launch wrote -- uint8 [H][W] at any byte address (i32 false) or
// int32 [H][W], 4-byte aligned -- into a table of runs_table_bytes(max_runs) bytes, 8-byte aligned.  `r`: the workspace of this H x W; max_runs is read NOW
// (a kernel argument: a captured graph replays the one it was captured with).  Only enqueues: every word the table's contract names is stored by a kernel.
static_assert(TD_RUNS_LAUNCHES == TDNET_RUNS_LAUNCHES && TD_RUNS_DECODE_LAUNCHES == TDNET_RUNS_DECODE_LAUNCHES && TD_RN_OVERFLOW == TDNET_RUNS_OVERFLOW &&
              sizeof(TdRun) == sizeof(tdnet_run) && sizeof(TdRunsHeader) == sizeof(tdnet_runs_header), "td_runs.h and include/tdnet.h disagree");
static int runs_table_check(const void* table, const char* who) {
    if (!table) return td_fail("%s: runs_dev is NULL", who);
    if ((size_t)table & 7u) return td_fail("%s: runs_dev = %p is not 8-byte aligned", who, table);
    return 0;
}
static int runs_args_check(int H, int W, const void* map, bool i32, const void* table, const RunsState& r, int max_runs, const char* who) {
    TD_TRY(runs_table_check(table, who));
    TD_TRY(regions_size_check(H, W, who));
    if (!map) return td_fail("%s: the map is NULL", who);
    if (i32 && ((size_t)map & 3u)) return td_fail("%s: ids_dev = %p is not 4-byte aligned", who, map);
    if (!r.blk || r.H != H || r.W != W) return td_fail("%s: internal: the runs workspace is not that of a %d x %d map", who, H, W);
    if (max_runs < 1 || (long)max_runs > (long)H * W) return td_fail("%s: max_runs = %d must be in 1..%ld (H W)", who, max_runs, (long)H * W);
    return 0;
}
static int run_runs(int H, int W, const void* map, bool i32, void* table, const RunsState& r, int max_runs, hipStream_t s, const char* who) {
    TD_TRY(runs_args_check(H, W, map, i32, table, r, max_runs, who));
    RunsArgs a = RunsArgs();
    a.map = map; a.table = (unsigned long long*)table; a.blk = r.blk;
    a.H = H; a.W = W; a.max_runs = max_runs;
    const long nblk = runs_blocks(H, W);
    if (i32) TD_LAUNCH(k_runs_count<int>, dim3((unsigned)nblk), dim3(TD_RN_LANES), 4 * sizeof(int), s, a);
    else TD_LAUNCH(k_runs_count<unsigned char>, dim3((unsigned)nblk), dim3(TD_RN_LANES), 4 * sizeof(int), s, a);
    TD_LAUNCH(k_runs_scan, dim3(1), dim3(TD_RN_LANES), 4 * sizeof(int), s, a, (int)nblk);
    if (i32) TD_LAUNCH(k_runs_emit<int>, dim3((unsigned)nblk), dim3(TD_RN_LANES), 4 * sizeof(int), s, a);
    else TD_LAUNCH(k_runs_emit<unsigned char>, dim3((unsigned)nblk), dim3(TD_RN_LANES), 4 * sizeof(int), s, a);
    return 0;
}
// the way back: one launch; `out` uint8 [H][W] at any byte address or int32 [H][W], 4-byte aligned.  The kernel reads the table's stored from the device,
// clamped to max_runs.
static int run_runs_decode(int H, int W, const void* table, int fill, void* out, bool i32, const RunsState& r, int max_runs, hipStream_t s, const char* who) {
    TD_TRY(runs_args_check(H, W, out, i32, table, r, max_runs, who));
    RunsArgs a = RunsArgs();
    a.map = out; a.table = (unsigned long long*)const_cast<void*>(table); a.blk = nullptr;
    a.H = H; a.W = W; a.max_runs = max_runs;
    const long nblk = runs_blocks(H, W);
    if (i32) TD_LAUNCH(k_runs_decode<int>, dim3((unsigned)nblk), dim3(TD_RN_LANES), 0, s, a, fill);
    else TD_LAUNCH(k_runs_decode<unsigned char>, dim3((unsigned)nblk), dim3(TD_RN_LANES), 0, s, a, fill);
    return 0;
}

// The refined matte of a frame at the source's size (td_refine.h k_refine_gather, then the operator's two launches): from the low-resolution logits and the class
// set (map == NULL: the gather IS the frame's last launch) or from a matte map [H][W] the caller holds.  out: [Hs][Ws] bytes, rows opitch apart -- the caller's,
// or rf.refined for the composite.  radius and eps are read NOW.  10 instantiations: the composite's 5 source forms x fused / from a map.
#define TD_GATHER_SRCS(X) X(P24) X(P32) X(NV12) X(SURF8) X(SURF16)
static int refine_ready(const RefineState& rf, const U8Input& u, const char* who) {
    if (rf.radius < 1) return td_fail("%s: the matte refinement is not configured (call tdnet_set_matte_refine with a radius of 1..%d first)", who, TD_RF_MAX_RADIUS);
    if (!rf.luma || rf.Hs != u.Hs || rf.Ws != u.Ws) return td_fail("%s: the refined matte's workspace for this source size is missing (its allocation failed)", who);
    return 0;
}
static int launch_refine_gather(const GatherArgs& a, const U8Input& u, const unsigned char* src, hipStream_t s) {
    const int src_form = picture_src_form(u, false);
    const SrcLayout l = src_layout(u);
    const dim3 rows = out_grid(a.ow, a.oh);
    switch (src_form) {
#define TD_G(SRC) case TD_SRC_##SRC: \
        if (a.map) TD_LAUNCH((k_refine_gather<true, TD_SRC_##SRC>), rows, dim3(256), 0, s, a, src, l); \
        else TD_LAUNCH((k_refine_gather<false, TD_SRC_##SRC>), rows, dim3(256), 0, s, a, src, l); \
        return 0;
    TD_GATHER_SRCS(TD_G)
#undef TD_G
    }
    return td_fail("internal: no gather kernel for source form %d", src_form);
}
static int run_refine_frame(const float* in, int C, int h, int w, const unsigned char* map, const MatteSet& set, const OverlayOutput& o, const U8Input& u,
                            const unsigned char* src, const RefineState& rf, unsigned char* out, size_t opitch, hipStream_t s, const char* who) {
    if (!o.Hs || o.Hs != u.Hs || o.Ws != u.Ws || o.H != u.H || o.W != u.W) return td_fail("%s: the index tables of this source size are missing (their allocation failed)", who);
    TD_TRY(refine_ready(rf, u, who));
    TD_TRY(out_check("refined matte", "src_height", o.Hs, map ? 1 : C));
    GatherArgs a = GatherArgs();
    a.in = in; a.map = map; a.ys = o.ys; a.xs = o.xs;
    a.C = C; a.h = h; a.w = w; a.H = o.H; a.W = o.W; a.oh = o.Hs; a.ow = o.Ws;
    a.swap = u.swap ? 1 : 0; a.luma = rf.luma; a.msrc = rf.msrc; a.set = set;
    TD_TRY(launch_refine_gather(a, u, src, s));
    launch_refine_coeff(rf.luma, (size_t)rf.Ws, rf.msrc, (size_t)rf.Ws, rf.Hs, rf.Ws, rf.radius, rf.eps, rf.scratch, s);
    launch_refine_apply(rf.luma, (size_t)rf.Ws, out, opitch, rf.Hs, rf.Ws, rf.radius, rf.scratch, s);
    return 0;
}
// the composite through the refined matte: the three launches into the workspace's map, then the EXISTING composite kernel from that map
static int run_refined_composite(const float* in, int C, int h, int w, const unsigned char* map, const MatteSet& set, const OverlayOutput& o, const U8Input& u,
                                 const unsigned char* src, const CompositeOutput& c, const DstOutput& d, const RefineState& rf, unsigned char* base, hipStream_t s, const char* who) {
    TD_TRY(composite_dst_check(u, c, d, who));                         // before the first launch
    TD_TRY(run_refine_frame(in, C, h, w, map, set, o, u, src, rf, rf.refined, (size_t)rf.Ws, s, who));
    return launch_composite(nullptr, 0, 0, 0, rf.refined, set, o, u, src, c, d, base, s, &rf);
}

// What leaves a frame: the form and the pointers that form needs (device memory of the caller's)
enum OutKind { OUT_LOGITS, OUT_LABELS_I32, OUT_LABELS_U8, OUT_RGB, OUT_SCORE, OUT_CONF, OUT_OVERLAY, OUT_MATTE, OUT_COMPOSITE, OUT_REGIONS, OUT_TRACKS, OUT_RUNS, OUT_MATTE_REFINED };
struct FrameOutput {
    OutKind kind;
    void* dst;                     // fp32 logits [C][H][W] | int32 labels [H][W] | uint8 labels [H][W] (OUT_SCORE, OUT_CONF, OUT_MATTE: may be NULL) | rgb [oh][ow][3] | overlay, composite [Hs][Ws][3]
                                   // (the two pictures with a destination view in force: the destination frame's base)
    const unsigned char* gt;       // OUT_SCORE: ground truth [H][W]
    unsigned char* conf;           // OUT_CONF: confidence bytes [H][W]; OUT_MATTE: matte bytes [H][W]
    const unsigned char* src;      // OUT_OVERLAY, OUT_COMPOSITE: the source frame, read by the handle's byte-input configuration
    int32_t* ids;                  // OUT_REGIONS: the id map [H][W] (may be NULL; dst: the uint8 labels, may be NULL too)
    void* table;                   // OUT_REGIONS: the header and the records; OUT_RUNS: the runs table (dst: the uint8 labels, may be NULL)
    int32_t* track_ids;            // OUT_TRACKS (OUT_REGIONS' fields plus): the track map [H][W] (may be NULL)
    void* tracks;                  // OUT_TRACKS: the tracks table
};
// the handle-side precondition of a form: its tables exist
static int output_configured(const tdnet* n, OutKind kind, const char* who) {
    if (kind == OUT_RGB && !n->rgb.set) return td_fail("%s: the colour-map output is not configured (call tdnet_set_output_rgb first)", who);
    if (kind == OUT_SCORE && !n->score.set) return td_fail("%s: the score output is not configured (call tdnet_set_score first)", who);
    if ((kind == OUT_REGIONS || kind == OUT_TRACKS) && !n->regions.set) return td_fail("%s: the regions output is not configured (call tdnet_set_regions first)", who);
    if (kind == OUT_RUNS && !n->runs.set) return td_fail("%s: the runs output is not configured (call tdnet_set_runs first)", who);
    if (kind == OUT_TRACKS && !n->tracks.set) return td_fail("%s: the tracks output is not configured (call tdnet_set_tracks first)", who);
    if ((kind == OUT_MATTE || kind == OUT_COMPOSITE || kind == OUT_MATTE_REFINED) && !n->matte_set) return td_fail("%s: the class set of the matte is not configured (call tdnet_set_matte first)", who);
    if (kind == OUT_COMPOSITE && !n->comp.set) return td_fail("%s: the composite output is not configured (call tdnet_set_output_composite first)", who);
    if (kind == OUT_COMPOSITE && !n->u8.set)
        return td_fail("%s: the byte input is not configured (call tdnet_set_input_u8 or one of its siblings first): the composite is written at its source size", who);
    if (kind == OUT_MATTE_REFINED && !n->u8.set)
        return td_fail("%s: the byte input is not configured (call tdnet_set_input_u8 or one of its siblings first): the refined matte is written at its source size", who);
    if (kind == OUT_MATTE_REFINED) TD_TRY(refine_ready(n->refine, n->u8, who));
    if (kind == OUT_OVERLAY && !n->overlay.set) return td_fail("%s: the overlay output is not configured (call tdnet_set_output_overlay first)", who);
    if (kind == OUT_OVERLAY && !n->u8.set)
        return td_fail("%s: the byte input is not configured (call tdnet_set_input_u8 or tdnet_set_input_nv12 first): the overlay is written at its source size", who);
    return 0;
}
// The last launch of a frame: the handle's low-resolution logits leave in the form `o`.  Confidence takes the threshold, the matte the class set
// in force NOW (kernel arguments: a captured graph replays the ones it was captured with).
static int emit_output(tdnet* n, const FrameOutput& o, hipStream_t s, const char* who) {
    TD_TRY(output_configured(n, o.kind, who));
    const float* in = n->lowres;
    const int C = n->cfg.nclass, h = n->h, w = n->w, H = n->H, W = n->W;
    switch (o.kind) {
    case OUT_LOGITS: launch_upsample(in, C, h, w, H, W, (float*)o.dst, s); return 0;
    case OUT_LABELS_I32: launch_upsample_argmax(in, C, h, w, H, W, (int32_t*)o.dst, s); return 0;
    case OUT_LABELS_U8: return launch_upsample_argmax_u8(in, C, h, w, H, W, (unsigned char*)o.dst, s);
    case OUT_RGB:
        if (n->dst.set) return launch_picture_dst(in, C, h, w, nullptr, &n->rgb, nullptr, nullptr, nullptr, n->dst, (unsigned char*)o.dst, s);
        return launch_upsample_argmax_rgb(in, C, h, w, n->rgb, (unsigned char*)o.dst, s);
    case OUT_SCORE: return launch_upsample_argmax_score(in, C, h, w, H, W, o.gt, n->score.dmap, (unsigned char*)o.dst, n->score.cm, s);
    case OUT_CONF: return launch_upsample_argmax_conf_u8(in, C, h, w, H, W, (unsigned char*)o.dst, o.conf, n->min_conf, n->reject_label, s);
    case OUT_MATTE: return launch_upsample_argmax_matte_u8(in, C, h, w, H, W, (unsigned char*)o.dst, o.conf, n->matte, s);
    case OUT_COMPOSITE:
        if (n->refine.radius) return run_refined_composite(in, C, h, w, nullptr, n->matte, n->overlay, n->u8, o.src, n->comp, n->dst, n->refine, (unsigned char*)o.dst, s, who);
        return launch_composite(in, C, h, w, nullptr, n->matte, n->overlay, n->u8, o.src, n->comp, n->dst, (unsigned char*)o.dst, s);
    case OUT_MATTE_REFINED:
        return run_refine_frame(in, C, h, w, nullptr, n->matte, n->overlay, n->u8, o.src, n->refine, (unsigned char*)o.dst, (size_t)n->u8.Ws, s, who);
    case OUT_REGIONS: return run_regions(in, C, h, w, H, W, nullptr, (unsigned char*)o.dst, o.ids, o.table, n->regions, s, who);
    case OUT_TRACKS: {
        int32_t* ids = o.ids ? o.ids : n->tracks.st.cur;
        TD_TRY(tracks_table_check(o.tracks, who));
        TD_TRY(run_regions(in, C, h, w, H, W, nullptr, (unsigned char*)o.dst, ids, o.table, n->regions, s, who));
        return run_tracks(H, W, ids, o.table, o.track_ids, o.tracks, n->tracks.st, n->regions.max_regions, n->tracks.min_overlap, s, who);
    }
    case OUT_RUNS: {                                                   // the label launch as the label entries enqueue it, then the map it wrote
        unsigned char* lab = o.dst ? (unsigned char*)o.dst : n->runs.lab;
        TD_TRY(runs_args_check(H, W, lab, false, o.table, n->runs, n->runs.max_runs, who));
        TD_TRY(launch_upsample_argmax_u8(in, C, h, w, H, W, lab, s));
        return run_runs(H, W, lab, false, o.table, n->runs, n->runs.max_runs, s, who);
    }
    case OUT_OVERLAY:
        if (n->dst.set) return launch_picture_dst(in, C, h, w, nullptr, nullptr, &n->overlay, &n->u8, o.src, n->dst, (unsigned char*)o.dst, s);
        return launch_upsample_argmax_overlay(in, C, h, w, n->overlay, n->u8, o.src, (unsigned char*)o.dst, s);
    }
    return td_fail("internal: unknown output form");
}
