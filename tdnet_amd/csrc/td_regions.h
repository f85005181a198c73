// td_regions.h -- regions out: the connected components of a class set of a frame's labels, numbered in raster order of their first pixel, with
// area, box and coordinate sums per component -- on the device, behind (or instead of) the frame's label launch.
//
// The contract (include/tdnet.h "regions out"): L the label map the label entries give, S the class set.  A region is a maximal set of pixels with
// L in S connected (4 or 8 neighbours) through pixels of the SAME label; its key is its smallest raster index Y * W + X; regions below min_area are
// dropped, the others numbered 1, 2, ... by growing key.  Everything is an integer: the result does not depend on the launch geometry or on the
// order in which the atomics land.
//
// Seven launches (TD_REGIONS_LAUNCHES), every one a plain grid -- no workgroup ever waits for another:
//   K1 k_regions_tile     a workgroup per 64 x 16 tile (256 lanes x 4 pixels of a row): labels from the low-resolution logits (k_upsample_argmax_u8's
//                         expressions) or from the caller's bytes, union-find in LDS over the backward neighbours, parent[i] = raster index of the
//                         tile-local root (the tile-local component's smallest raster index; TD_RG_BG for background); zeroes area[] and the table
//   K2 k_regions_merge    a lane per pixel with a backward neighbour in ANOTHER tile: the lock-free min-root union on parent[]
//   K3 k_regions_flatten  root[i] = find(i) into a SECOND array; area[root] += 1
//   K4 k_regions_count    survivors (root[i] == i and area[i] >= min_area) per block of 1024 pixels
//   K5 k_regions_scan     one workgroup: exclusive scan of the block counts; the table's header
//   K6 k_regions_number   rank inside the block: num[i] of every root (0: dropped), written over parent[]; the root's lane fills its record's label,
//                         area, first pixel and the box's starting values
//   K7 k_regions_stats    every pixel: id = num[root]; the id map; sum_x, sum_y (add), x0 (min), x1, y1 (max) of its record
//
// Memory visibility.  K2 is the only launch in which a workgroup reads words another workgroup of the SAME launch writes (parent[]).  The XCDs' L2s
// are not coherent with each other and a CU's L1 is never refreshed by another CU's stores, so there EVERY access to parent[] is an agent-scope
// atomic read-modify-write: the link is td_rg_min, the read is td_rg_read, an atomic OR with a zero that arrives as a KERNEL ARGUMENT.  The operand must
// be opaque: an RMW the compiler can prove idempotent (a minimum with INT_MAX, an OR with a literal 0) is folded into an atomic LOAD, which the L2 of
// this XCD may serve from a line it still holds.  The compiled k_regions_merge has no load of parent[] (its only loads are the label bytes, which are
// read-only in that launch).  Everything else goes from one launch to the next.
// Bounded loops.  The invariant is parent[x] <= x, kept by every write (K1 stores a tile's smallest index, the link is a minimum with a smaller root).
// A union holds two indices a, b < H W.  Every step it counts -- a find step x = parent[x] < x, or the retry a = old < a behind a link another lane
// won -- strictly lowers one of them and raises neither (the swap only renames them), so a union takes fewer than a + b < 2 H W counted steps whatever
// the other lanes do, and a lone find fewer than H W.  The budgets are those bounds (td_rg_budget: 2 H W + 16; in LDS 4 * 1024 over indices below
// 1024): on a correct build they cannot run out, under any contention.  A loop that does run out sets TDNET_REGIONS_BOUND in the workspace's flag
// word, which K5 folds into the header, and leaves: a bug ends as a flagged wrong answer, not as a hang.
// Contention.  A region may be a third of the frame, and every pixel adding into one word serialises the chip.  K3 and K7 reduce across the wave first, in
// rounds by key (TD_RG_ROUNDS below): the flat raster geometry gives a wave 256 consecutive pixels of a row, so one region -- one round, one lane issuing
// the atomics -- is the common case; what is left after the rounds goes lane by lane, equal keys among a lane's 4 pixels merged.
//
// Written on the TD_* macros only (tests/emu runs this file unchanged): the wrappers below are the only build-dependent lines; plain C++, vector
// stores and HIP atomics, no inline assembly.
#pragma once
#include "td_device.h"
#include "td_out.h"      // td_up_classes / td_first_max / td_run_px / td_u8_store
#include "td_matte.h"    // MatteSet / td_matte_member: the class set as 256 membership bits in the kernel arguments

#define TD_RG_TW 64                                                    // tile: 16 lanes x 4 pixels wide,
#define TD_RG_TH 16                                                    // 16 rows: 256 lanes
#define TD_RG_BLOCK 1024                                               // pixels per workgroup of the flat launches K3 .. K7
#define TD_RG_BG (-1)                                                  // parent / root of a background pixel
#define TD_REGIONS_LAUNCHES 7
#define TD_RG_OVERFLOW 1u                                              // header status bits (include/tdnet.h TDNET_REGIONS_*)
#define TD_RG_BOUND 2u

struct TdRegion { int label, area, x0, y0, x1, y1, first_y, first_x; unsigned long long sum_x, sum_y; };   // 48 bytes
struct TdRegionsHeader { unsigned count, stored, status, reserved; };                                      // 16 bytes
typedef int td_i32x4 __attribute__((ext_vector_type(4)));

// What one enqueue of the pipeline works on: the maps, the workspace and the configuration in force when the entry enqueues.
struct RegionsArgs {
    const float* in;               // FROM_LOGITS: low-resolution logits [C][h][w]
    const unsigned char* labels;   // the label map [H][W] at any byte address: read by K1 (!FROM_LOGITS) and K2, K6; written by K1 (FROM_LOGITS)
    int* ids;                      // id map [H][W] or NULL
    unsigned long long* table;     // header + max_regions records, 8-byte aligned
    int *parent, *root, *area, *blk;   // workspace: three int32 [H][W] and the block counts [ceil(H W / 1024)]
    unsigned* flag;                // workspace: one word, zero between runs (K5 folds it into the header and clears it)
    int zero;                      // 0, handed to td_rg_read as a value the compiler cannot see through
    int C, h, w, H, W;
    int conn, max_regions, min_area;
    MatteSet set;
};

// ---- the build-dependent wrappers.  The emulator runs the fibers of a workgroup on one OS thread (LDS: plain operations are atomic there) and
// workgroups on several OS threads (global memory: real atomics there too).
TD_DEV int td_rg_lds_min(int* p, int v) {
#ifdef TD_EMU
    const int old = *p;
    if (v < old) *p = v;
    return old;
#else
    return atomicMin(p, v);
#endif
}
TD_DEV int td_rg_min(int* p, int v) {                                  // agent scope (HIP's default for global atomics); returns the old value
#ifdef TD_EMU
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
#else
    return atomicMin(p, v);
#endif
}
// A read that IS an atomic RMW: OR with `zero`, which is 0 but comes from the kernel arguments (RegionsArgs.zero), so the compiler cannot fold it to a load
TD_DEV int td_rg_read(int* p, int zero) {
#ifdef TD_EMU
    (void)zero;
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return atomicOr(p, zero);
#endif
}
TD_DEV void td_rg_max(int* p, int v) {
#ifdef TD_EMU
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
#else
    atomicMax(p, v);
#endif
}
TD_DEV void td_rg_add(int* p, int v) {
#ifdef TD_EMU
    __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#else
    atomicAdd(p, v);
#endif
}
TD_DEV void td_rg_add64(unsigned long long* p, unsigned long long v) {
#ifdef TD_EMU
    __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#else
    atomicAdd(p, v);
#endif
}
TD_DEV void td_rg_or(unsigned* p, unsigned v) {
#ifdef TD_EMU
    __atomic_fetch_or(p, v, __ATOMIC_RELAXED);
#else
    atomicOr(p, v);
#endif
}
// the value of lane ^ m (every lane of the wave calls it).  The emulator's one shuffle carries a float: two exact 16-bit halves.
TD_DEV unsigned td_rg_shfl_xor(unsigned v, int m) {
#ifdef TD_EMU
    const float lo = td_shfl_xor((float)(v & 0xffffu), m), hi = td_shfl_xor((float)(v >> 16), m);
    return ((unsigned)hi << 16) | (unsigned)lo;
#else
    return (unsigned)__shfl_xor((int)v, m, 64);
#endif
}
TD_DEV unsigned td_rg_wave_sum(unsigned v) {
    for (int m = 1; m < 64; m <<= 1) v += td_rg_shfl_xor(v, m);
    return v;
}
TD_DEV unsigned td_rg_wave_min(unsigned v) {
    for (int m = 1; m < 64; m <<= 1) { const unsigned o = td_rg_shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
TD_DEV unsigned td_rg_wave_max(unsigned v) { return ~td_rg_wave_min(~v); }

// ---- union-find -------------------------------------------------------------------------------------------------------------------------
// LDS, inside a tile: par[i] <= i always; the min-root union (the larger root is hung under the smaller with an atomic minimum; if another lane got
// there first, go on from what it wrote).  `budget` counts every step; false when it ran out.
TD_DEV int td_rg_lds_find(volatile int* par, int x, int& budget) {
    for (int p = par[x]; p != x && budget > 0; p = par[x]) { x = p; --budget; }
    return x;
}
TD_DEV bool td_rg_lds_union(int* par, int a, int b, int budget) {
    while (budget > 0) {
        a = td_rg_lds_find(par, a, budget);
        b = td_rg_lds_find(par, b, budget);
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = td_rg_lds_min(par + a, b);
        if (old == a) return true;
        a = old;
        --budget;
    }
    return false;
}
// Global, between tiles (K2): the same union with every access to parent[] an atomic RMW (zero: td_rg_read's opaque operand)
TD_DEV int td_rg_find_rmw(int* parent, int x, int& budget, int zero) {
    for (int p = td_rg_read(parent + x, zero); p != x && budget > 0; p = td_rg_read(parent + x, zero)) { x = p; --budget; }
    return x;
}
TD_DEV bool td_rg_union(int* parent, int a, int b, int budget, int zero) {
    while (budget > 0) {
        a = td_rg_find_rmw(parent, a, budget, zero);
        b = td_rg_find_rmw(parent, b, budget, zero);
        if (a == b) return true;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = td_rg_min(parent + a, b);
        if (old == a) return true;
        a = old;
        --budget;
    }
    return false;
}
#define TD_RG_MAX_PIXELS 0x3ffffff0L                                   // 2 H W + 16 is an int up to here (the host refuses larger maps)
TD_HOSTDEV int td_rg_budget(long HW) { return (int)(2 * HW + 16); }

// is label l (a byte, or an argmax index) a member: below nclass and in the set
TD_DEV bool td_rg_member(const MatteSet& set, int l, int C) { return l < C && td_matte_member(set, l); }

// ---- K1: tile-local labelling --------------------------------------------------------------------------------------------------------------
// grid = (ceil(W / 64), ceil(H / 16)), 256 lanes; LDS: int par[1024], int lab[1024] (-1: background or outside the map).  Lane t holds the pixels
// (ly = t / 16, lx = 4 (t % 16) .. + 3) of the tile.  FROM_LOGITS: a.labels is WRITTEN (k_upsample_argmax_u8's bytes), else read.  Also zeroes
// area[] over the tile and, grid-stride, the table's table_words 8-byte words.  No lane leaves before the last barrier.
template <bool FROM_LOGITS>
TD_KERNEL void k_regions_tile(RegionsArgs a, long table_words) {
    TD_DYN_LDS(smem);
    int* par = reinterpret_cast<int*>(smem);
    int* lab = par + TD_RG_TW * TD_RG_TH;
    const int t = threadIdx.x, ly = t >> 4, lx = (t & 15) * 4;
    const int Y = blockIdx.y * TD_RG_TH + ly, X0 = blockIdx.x * TD_RG_TW + lx;
    const long nthreads = (long)gridDim.x * gridDim.y * blockDim.x;
    for (long k = ((long)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + t; k < table_words; k += nthreads) a.table[k] = 0ull;
    const bool inside = Y < a.H && X0 < a.W;
    const long xb = X0 + 4 < a.W ? X0 + 4 : a.W;
    int l[4] = {-1, -1, -1, -1};
    if (inside) {
        unsigned char* row = const_cast<unsigned char*>(a.labels) + (size_t)Y * a.W;
        if (FROM_LOGITS) {
            float best[4] = {0.f, 0.f, 0.f, 0.f};
            int bi[4] = {0, 0, 0, 0};
            td_up_classes(a.in, a.C, a.h, a.w, a.H, a.W, Y, [&](int e) { return (int)td_run_px(X0, e, a.W); }, [&](int c, int e, float v) { td_first_max(c, v, best[e], bi[e]); });
            td_u8_store(row, X0, xb, bi);
#pragma unroll
            for (int e = 0; e < 4; ++e) l[e] = bi[e];
        } else if (xb - X0 == 4 && (((size_t)(row + X0)) & 3u) == 0) {
            const unsigned v = *reinterpret_cast<const unsigned*>(row + X0);
            l[0] = (int)(v & 255u); l[1] = (int)((v >> 8) & 255u); l[2] = (int)((v >> 16) & 255u); l[3] = (int)(v >> 24);
        } else {
            for (long X = X0; X < xb; ++X) l[X - X0] = row[X];
        }
    }
    const int li0 = ly * TD_RG_TW + lx;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool fg = inside && X0 + e < a.W && td_rg_member(a.set, l[e], a.C);
        l[e] = fg ? l[e] : -1;
        lab[li0 + e] = l[e];
        par[li0 + e] = li0 + e;
    }
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (l[e] < 0) continue;
        const int li = li0 + e, x = lx + e;
        const bool wsame = x > 0 && lab[li - 1] == l[e];
        const bool nsame = ly > 0 && lab[li - TD_RG_TW] == l[e];
        if (wsame) ok &= td_rg_lds_union(par, li, li - 1, 4 * TD_RG_TW * TD_RG_TH);
        if (nsame) ok &= td_rg_lds_union(par, li, li - TD_RG_TW, 4 * TD_RG_TW * TD_RG_TH);
        // 8 neighbours: with N in the region, NW and NE hang on N through their own W links; with W in it, NW hangs on W through W's N link
        if (a.conn == 8 && ly > 0 && !nsame) {
            if (x > 0 && !wsame && lab[li - TD_RG_TW - 1] == l[e]) ok &= td_rg_lds_union(par, li, li - TD_RG_TW - 1, 4 * TD_RG_TW * TD_RG_TH);
            if (x < TD_RG_TW - 1 && lab[li - TD_RG_TW + 1] == l[e]) ok &= td_rg_lds_union(par, li, li - TD_RG_TW + 1, 4 * TD_RG_TW * TD_RG_TH);
        }
    }
    __syncthreads();
    if (inside) {
        const long base = (long)Y * a.W;
        const int ty = blockIdx.y * TD_RG_TH, tx = blockIdx.x * TD_RG_TW;
        for (long X = X0; X < xb; ++X) {
            const int e = (int)(X - X0);
            int r = TD_RG_BG;
            if (l[e] >= 0) {
                int budget = 2 * TD_RG_TW * TD_RG_TH;
                const int lr = td_rg_lds_find(par, li0 + e, budget);
                ok &= budget > 0;
                r = (ty + lr / TD_RG_TW) * a.W + tx + lr % TD_RG_TW;
            }
            a.parent[base + X] = r;
            a.area[base + X] = 0;
        }
    }
    if (!ok) td_rg_or(a.flag, TD_RG_BOUND);
}

// ---- K2: border merge ------------------------------------------------------------------------------------------------------------------------
// A lane per pixel of: the top rows of the tile rows 1 .. (nr * W lanes), the left columns of the tile columns 1 .. (nc * H lanes) and, 8 neighbours,
// the right columns of the tile columns 0 .. nc - 1 (nc * H lanes).  Which of a pixel's backward links cross a tile border follows from where it
// sits; a link is skipped where the links of its neighbours already carry it: a vertical link at x when (y, x - 1) and (y - 1, x - 1) are in the
// region and x is not a tile's first column (by induction along the row: the tile's first column never skips), likewise a horizontal link along
// the column; a diagonal link when one of the two pixels beside it is in the region (two straight links then carry it).
TD_KERNEL void k_regions_merge(RegionsArgs a, long row_lanes, long col_lanes) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = a.W, H = a.H;
    int y, x, kind;                                                    // 0: top row of a tile, 1: left column, 2: right column
    if (q < row_lanes) { kind = 0; y = (int)(q / W + 1) * TD_RG_TH; x = (int)(q % W); }
    else if (q < row_lanes + col_lanes) { const long c = q - row_lanes; kind = 1; x = (int)(c / H + 1) * TD_RG_TW; y = (int)(c % H); }
    else if (q < row_lanes + 2 * col_lanes && a.conn == 8) { const long c = q - row_lanes - col_lanes; kind = 2; x = (int)(c / H + 1) * TD_RG_TW - 1; y = (int)(c % H); }
    else return;
    const unsigned char* lab = a.labels;
    const long p = (long)y * W + x;
    const int l = lab[p];
    if (!td_rg_member(a.set, l, a.C)) return;
    const int budget = td_rg_budget((long)H * W);
    const bool up = y > 0, tile_row = y % TD_RG_TH == 0, tile_col = x % TD_RG_TW == 0;
    const bool n = up && lab[p - W] == l, w = x > 0 && lab[p - 1] == l, nw = up && x > 0 && lab[p - W - 1] == l, ne = up && x < W - 1 && lab[p - W + 1] == l;
    bool ok = true;
    if (kind == 0) {
        if (n && !(w && nw && !tile_col)) ok &= td_rg_union(a.parent, (int)p, (int)(p - W), budget, a.zero);
        if (a.conn == 8 && !n) {
            if (nw && !w) ok &= td_rg_union(a.parent, (int)p, (int)(p - W - 1), budget, a.zero);
            if (ne) ok &= td_rg_union(a.parent, (int)p, (int)(p - W + 1), budget, a.zero);
        }
    } else if (kind == 1) {
        if (w && !(n && nw && !tile_row)) ok &= td_rg_union(a.parent, (int)p, (int)(p - 1), budget, a.zero);
        if (a.conn == 8 && !tile_row && nw && !n && !w) ok &= td_rg_union(a.parent, (int)p, (int)(p - W - 1), budget, a.zero);   // (a tile's top row: the row lane's)
    } else {
        if (!tile_row && ne && !n) ok &= td_rg_union(a.parent, (int)p, (int)(p - W + 1), budget, a.zero);
    }
    if (!ok) td_rg_or(a.flag, TD_RG_BOUND);
}

// ---- the flat launches K3 .. K7: a workgroup per 1024 consecutive pixels of the raster, a lane per 4 -----------------------------------------
// the lane's pixels [i0, i0 + n), n in 0 .. 4
TD_DEV long td_rg_quad(long HW, int* n) {
    const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    *n = i0 >= HW ? 0 : (HW - i0 < 4 ? (int)(HW - i0) : 4);
    return i0;
}
// 4 ints of a workspace map (16-byte aligned: a fresh allocation, i0 a multiple of 4); v[e] = fill beyond n
TD_DEV void td_rg_load4(const int* p, long i0, int n, int fill, int* v) {
    if (n == 4) {
        const td_i32x4 q = *reinterpret_cast<const td_i32x4*>(p + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < n ? p[i0 + e] : fill;
    }
}
TD_DEV void td_rg_store4(int* p, long i0, int n, const int* v) {
    if (n == 4 && (((size_t)(p + i0)) & 15u) == 0) {
        const td_i32x4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<td_i32x4*>(p + i0) = q;
    } else {
        for (int e = 0; e < n; ++e) p[i0 + e] = v[e];
    }
}
// The pre-reduction of K3 and K7 goes in rounds: every round takes the SMALLEST key any lane of the wave still holds (td_rg_wave_min over the lanes' own
// smallest; TD_RG_NONE when nothing is left -- a wave-uniform answer, so all lanes leave together), reduces what the wave's pixels of that key carry across
// the wave, and lane 0 issues the atomics for it.  A wave inside one region is done after one round; a wave of noise around a region that spans the map
// (whose key, its first pixel, is the smallest there) sheds that region's pixels in the first round.  What is left after TD_RG_ROUNDS goes lane by lane.
#define TD_RG_ROUNDS 2
#define TD_RG_NONE 0xffffffffu

// K3: root[i] = find(i), plain loads (parent[] was finished by the previous launch); area[root] += 1
TD_KERNEL void k_regions_flatten(RegionsArgs a) {
    const long HW = (long)a.H * a.W;
    int n;
    const long i0 = td_rg_quad(HW, &n);
    int p[4], r[4];
    td_rg_load4(a.parent, i0, n, TD_RG_BG, p);
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = p[e];
        if (p[e] < 0 || (e > 0 && p[e] == p[e - 1])) { if (p[e] >= 0) r[e] = r[e - 1]; continue; }
        int budget = td_rg_budget(HW), x = p[e];
        for (int q = a.parent[x]; q != x && budget > 0; q = a.parent[x]) { x = q; --budget; }
        ok &= budget > 0;
        r[e] = x;
    }
    if (!ok) td_rg_or(a.flag, TD_RG_BOUND);
    td_rg_store4(a.root, i0, n, r);
    bool left[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) left[e] = r[e] >= 0;
    for (int round = 0; round < TD_RG_ROUNDS; ++round) {
        unsigned mine = TD_RG_NONE;
#pragma unroll
        for (int e = 0; e < 4; ++e) mine = (left[e] && (unsigned)r[e] < mine) ? (unsigned)r[e] : mine;
        const unsigned key = td_rg_wave_min(mine);
        if (key == TD_RG_NONE) return;
        unsigned c = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (left[e] && (unsigned)r[e] == key) { ++c; left[e] = false; }
        const unsigned total = td_rg_wave_sum(c);
        if (td_lane() == 0) td_rg_add(a.area + key, (int)total);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                      // the rest: equal roots among the lane's own pixels merged
        if (!left[e]) continue;
        int c = 1;
#pragma unroll
        for (int f = e + 1; f < 4; ++f)
            if (left[f] && r[f] == r[e]) { ++c; left[f] = false; }
        td_rg_add(a.area + r[e], c);
    }
}

// does the root pixel i survive: a root of at least min_area pixels
TD_DEV int td_rg_survivors(const RegionsArgs& a, long i0, int n, int* flag) {
    int r[4], ar[4], c = 0;
    td_rg_load4(a.root, i0, n, TD_RG_BG, r);
    td_rg_load4(a.area, i0, n, 0, ar);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        flag[e] = (e < n && r[e] == (int)(i0 + e) && ar[e] >= a.min_area) ? ar[e] : 0;   // the area itself: > 0 for a survivor
        c += flag[e] != 0;
    }
    return c;
}
// K4: blk[b] = survivors among the block's pixels.  LDS: 4 ints.
TD_KERNEL void k_regions_count(RegionsArgs a) {
    TD_DYN_LDS(smem);
    int* wsum = reinterpret_cast<int*>(smem);
    int n, flag[4];
    const long i0 = td_rg_quad((long)a.H * a.W, &n);
    const unsigned c = td_rg_wave_sum((unsigned)td_rg_survivors(a, i0, n, flag));
    if (td_lane() == 0) wsum[threadIdx.x >> 6] = (int)c;
    __syncthreads();
    if (threadIdx.x == 0) a.blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// K5: ONE workgroup of 256 lanes: blk[] becomes its exclusive scan; the header.  LDS: 256 ints.
TD_KERNEL void k_regions_scan(RegionsArgs a, int nblk) {
    TD_DYN_LDS(smem);
    int* part = reinterpret_cast<int*>(smem);
    const int t = threadIdx.x, chunk = (nblk + 255) / 256, j0 = t * chunk, j1 = j0 + chunk < nblk ? j0 + chunk : nblk;
    int s = 0;
    for (int j = j0; j < j1; ++j) s += a.blk[j];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < 256; ++k) { const int v = part[k]; part[k] = run; run += v; }
        TdRegionsHeader* hd = reinterpret_cast<TdRegionsHeader*>(a.table);
        const unsigned count = (unsigned)run, maxr = (unsigned)a.max_regions;
        hd->count = count;
        hd->stored = count < maxr ? count : maxr;
        hd->status = (count > maxr ? TD_RG_OVERFLOW : 0u) | (*a.flag ? TD_RG_BOUND : 0u);
        hd->reserved = 0u;
        *a.flag = 0u;
    }
    __syncthreads();
    int run = part[t];
    for (int j = j0; j < j1; ++j) { const int v = a.blk[j]; a.blk[j] = run; run += v; }
}
// K6: num[i] (written over parent[]: nothing reads parent[] any more) = the region's number for a surviving root, 0 for every other pixel; the record's
// fields that the root's lane knows.  LDS: 256 + 4 ints.
TD_KERNEL void k_regions_number(RegionsArgs a) {
    TD_DYN_LDS(smem);
    int* cnt = reinterpret_cast<int*>(smem);
    int* wtot = cnt + 256;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int n, flag[4];
    const long i0 = td_rg_quad((long)a.H * a.W, &n);
    const int c = td_rg_survivors(a, i0, n, flag);
    cnt[t] = c;
    __syncthreads();
    int pre = 0;
    for (int j = t - lane; j < t; ++j) pre += cnt[j];
    if (lane == 63) wtot[wave] = pre + c;
    __syncthreads();
    for (int k = 0; k < wave; ++k) pre += wtot[k];
    int num[4] = {0, 0, 0, 0}, next = a.blk[blockIdx.x] + pre + 1;
    TdRegion* rec = reinterpret_cast<TdRegion*>(a.table + 2);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!flag[e]) continue;
        num[e] = next++;
        if (num[e] > a.max_regions) continue;
        const long i = i0 + e;
        const int y = (int)(i / a.W), x = (int)(i - (long)y * a.W);
        TdRegion* r = rec + (num[e] - 1);
        r->label = a.labels[i]; r->area = flag[e];
        r->x0 = x; r->y0 = y; r->x1 = x; r->y1 = y; r->first_y = y; r->first_x = x;
    }
    td_rg_store4(a.parent, i0, n, num);
}
// K7: id = num[root] of every pixel; the id map; the sums and the box of its record (id <= max_regions)
TD_KERNEL void k_regions_stats(RegionsArgs a) {
    const long HW = (long)a.H * a.W;
    int n, r[4], id[4];
    const long i0 = td_rg_quad(HW, &n);
    td_rg_load4(a.root, i0, n, TD_RG_BG, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) id[e] = r[e] < 0 ? 0 : (e > 0 && r[e] == r[e - 1]) ? id[e - 1] : a.parent[r[e]];
    if (a.ids) td_rg_store4(a.ids, i0, n, id);
    int px[4], py[4];
    bool left[4];
    {
        int y = (int)(i0 / a.W), x = (int)(i0 - (long)y * a.W);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            px[e] = x; py[e] = y;
            if (++x == a.W) { x = 0; ++y; }
            left[e] = id[e] > 0 && id[e] <= a.max_regions;             // beyond the table: an id, but no record
        }
    }
    TdRegion* rec = reinterpret_cast<TdRegion*>(a.table + 2);
    for (int round = 0; round < TD_RG_ROUNDS; ++round) {
        unsigned mine = TD_RG_NONE;
#pragma unroll
        for (int e = 0; e < 4; ++e) mine = (left[e] && (unsigned)id[e] < mine) ? (unsigned)id[e] : mine;
        const unsigned key = td_rg_wave_min(mine);
        if (key == TD_RG_NONE) return;
        unsigned sx = 0, sy = 0, x0 = 0x7fffffffu, x1 = 0, y1 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (left[e] && (unsigned)id[e] == key) {
                sx += (unsigned)px[e]; sy += (unsigned)py[e];
                x0 = (unsigned)px[e] < x0 ? (unsigned)px[e] : x0; x1 = (unsigned)px[e] > x1 ? (unsigned)px[e] : x1; y1 = (unsigned)py[e] > y1 ? (unsigned)py[e] : y1;
                left[e] = false;
            }
        sx = td_rg_wave_sum(sx); sy = td_rg_wave_sum(sy);
        x0 = td_rg_wave_min(x0); x1 = td_rg_wave_max(x1); y1 = td_rg_wave_max(y1);
        if (td_lane() == 0) {
            TdRegion* q = rec + (key - 1);
            td_rg_add64(&q->sum_x, sx); td_rg_add64(&q->sum_y, sy);
            td_rg_min(&q->x0, (int)x0); td_rg_max(&q->x1, (int)x1); td_rg_max(&q->y1, (int)y1);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                      // the rest: equal ids among the lane's own pixels merged
        if (!left[e]) continue;
        unsigned sx = (unsigned)px[e], sy = (unsigned)py[e];
        int x0 = px[e], x1 = px[e], y1 = py[e];
#pragma unroll
        for (int f = e + 1; f < 4; ++f)
            if (left[f] && id[f] == id[e]) {
                sx += (unsigned)px[f]; sy += (unsigned)py[f];
                x0 = px[f] < x0 ? px[f] : x0; x1 = px[f] > x1 ? px[f] : x1; y1 = py[f] > y1 ? py[f] : y1;
                left[f] = false;
            }
        TdRegion* q = rec + (id[e] - 1);
        td_rg_add64(&q->sum_x, sx); td_rg_add64(&q->sum_y, sy);
        td_rg_min(&q->x0, x0); td_rg_max(&q->x1, x1); td_rg_max(&q->y1, y1);
    }
}
