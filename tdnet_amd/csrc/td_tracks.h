// td_tracks.h -- tracks out: region identity across frames.  The regions of this frame (td_regions.h) are matched against those of the previous tracked
// frame by pixel overlap, on the device, behind the regions pipeline; a matched region keeps its track id, every other one is born with a new id.
//
// The contract (include/tdnet.h "tracks out"): n(p, c) = pixels with ids'[i] == p and ids[i] == c over regions that have a record on both sides and
// carry the same label; bp(c) / bc(p) the partner of largest n (ties: the smallest number); c continues p iff they choose each other and
// n >= min_overlap.  Everything is an integer: the result does not depend on the launch geometry, on where a pair lands in the pair table or on the
// order in which the atomics arrive.
//
// Four launches (TD_TRACKS_LAUNCHES), every one a plain grid -- no workgroup ever waits for another:
//   T1 k_tracks_pairs    a lane per 4 pixels of the flat raster (td_rg_quad): key = (p - 1) << 16 | (c - 1) of every pixel with a record on both sides,
//                        equal keys pre-reduced across the wave in rounds, then counted in an open-addressing table of 64-bit slots (key high, count low)
//   T2 k_tracks_best     a lane per slot: pairs of equal label raise best_prev[c] with n << 32 | ~p and best_cur[p] with n << 32 | ~c (64-bit maxima:
//                        the largest n, then the smallest partner); the slot is zeroed for the next run; the tracks table is zeroed, grid-stride
//   T3 k_tracks_resolve  ONE workgroup of 1024 lanes, 1024 regions a step: the mutual test, an exclusive scan of the birth flags, the ids from `next`, the
//                        records and the header
//   T4 k_tracks_commit   a lane per 4 pixels: the optional track map; the ids of regions with a record over the previous map; label, track and age of every
//                        region, stored' and the zeroed best arrays into the state
//
// Memory visibility.  T1 is the only launch in which a workgroup reads words another workgroup of the SAME launch writes (the pair table).  The XCDs' L2s
// are not coherent with each other (td_regions.h has the paragraph), so there EVERY access to the table is a returning agent-scope read-modify-write: the
// probe IS the compare-and-swap on an empty slot (its return value is the only way a slot's key is ever read), the count is an atomic add.  No slot is
// loaded in T1.  The maxima of T2 are atomics on words nothing reads in T2; everything else goes from one launch to the next.
// Bounded loops.  The table has cap >= 2 H W slots and a launch inserts at most H W distinct keys (a pixel has one key); slots are never released inside a
// launch.  A probe sequence visits the cap slots once each, so within cap probes it meets its own key or an empty slot, whatever the other lanes do:
// the budget is cap.  A loop that does run out sets the state's flag word, which T3 folds into the header as TD_TK_BOUND and clears: a bug ends as a
// flagged wrong answer, not as a hang.  T3's loop runs ceil(stored / 1024) <= 64 steps.
// Contention.  A region may be a third of the frame, and with the same region under it in the previous frame every one of its pixels carries ONE key.  T1
// reduces across the wave first, in rounds by key, exactly as td_regions.h K3 and K7 do: a wave of 256 consecutive pixels inside one object issues one
// atomic.  What is left after the rounds goes lane by lane, equal keys among a lane's 4 pixels merged.
//
// Written on the TD_* macros only (tests/emu runs this file unchanged): the wrappers below are the only build-dependent lines; plain C++, vector
// stores and HIP atomics, no inline assembly.
#pragma once
#include "td_regions.h"

#define TD_TRACKS_LAUNCHES 4
#define TD_TK_BOUND 1u                                                 // header status bit (include/tdnet.h TDNET_TRACKS_BOUND)
#define TD_TK_MAX_REGIONS 65536                                        // the ceiling of tdnet_set_regions' max_regions: p - 1 and c - 1 are 16 bits
#define TD_TK_WG 1024                                                  // lanes of T3's one workgroup

struct TdTrack { unsigned track, age, prev_region, overlap, origin_track, reserved; };   // 24 bytes
struct TdTracksHeader { unsigned count, matched, ended, status; };                        // 16 bytes
typedef unsigned long long td_u64;

// The state between frames and the scratch of one run, at fixed addresses inside one blob (td_handle.h tracks_layout).  All zero = the reset state.
struct TracksState {
    unsigned* words;               // [0] stored', [1] births so far (next - 1), [2] the bound flag (zero between runs), [3] reserved
    int* prev;                     // ids' [H][W]: the previous frame's ids of regions with a record, 0 elsewhere
    int* cur;                      // [H][W]: where a frame's ids go when the caller asks for none
    td_u64* hash;                  // the pair table: 1 << lg slots, zero between runs
    td_u64 *best_prev, *best_cur;  // [65536] each, indexed c - 1 / p - 1, zero between runs
    int* lab;                      // label'[p - 1]
    unsigned *track, *age;         // track'[p - 1], age'[p - 1]
    int lg;
};
struct TracksArgs {
    TracksState st;
    const int* ids;                // the current id map [H][W] (the caller's or st.cur)
    const td_u64* rtable;          // the regions table the same call wrote
    td_u64* table;                 // the tracks table: header + max_regions records, 8-byte aligned
    int* track_ids;                // track map [H][W] or NULL
    int H, W, max_regions, min_overlap;
};

// ---- the build-dependent wrappers (the emulator: workgroups on several OS threads, real atomics) ----
TD_DEV td_u64 td_tk_cas64(td_u64* p, td_u64 expect, td_u64 v) {        // agent scope (HIP's default for global atomics); returns the old value
#ifdef TD_EMU
    __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;
#else
    return atomicCAS(p, expect, v);
#endif
}
TD_DEV td_u64 td_tk_add64(td_u64* p, td_u64 v) {
#ifdef TD_EMU
    return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#else
    return atomicAdd(p, v);
#endif
}
TD_DEV void td_tk_max64(td_u64* p, td_u64 v) {
#ifdef TD_EMU
    td_u64 old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
#else
    atomicMax(p, v);
#endif
}

// 4 ints of a map the CALLER may hold (any int32 address); v[e] = 0 beyond n
TD_DEV void td_tk_load4(const int* p, long i0, int n, int* v) {
    if (n == 4 && (((size_t)(p + i0)) & 15u) == 0) {
        const td_i32x4 q = *reinterpret_cast<const td_i32x4*>(p + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < n ? p[i0 + e] : 0;
    }
}
TD_DEV unsigned td_tk_slot(unsigned key, int lg) {
    unsigned k = key * 0x9E3779B1u;
    k ^= k >> 15;
    k *= 0x85EBCA77u;
    return k >> (32 - lg);                                             // lg in 1 .. 31
}
// count `cnt` pixels of `key`: every access to the table is a returning RMW (see the head of this file); false when the budget of cap probes ran out
TD_DEV bool td_tk_insert(td_u64* hash, int lg, unsigned key, unsigned cnt) {
    const unsigned long cap = 1ul << lg, mask = cap - 1;
    unsigned long s = td_tk_slot(key, lg);
    const td_u64 want = ((td_u64)key << 32) | cnt;                     // cnt >= 1: a taken slot is never 0, also for key 0
    for (unsigned long k = 0; k < cap; ++k, s = (s + 1) & mask) {
        const td_u64 old = td_tk_cas64(hash + s, 0ull, want);
        if (old == 0ull) return true;
        if ((unsigned)(old >> 32) == key) { td_tk_add64(hash + s, cnt); return true; }
    }
    return false;
}

// ---- T1: pair count ----------------------------------------------------------------------------------------------------------------------------
// grid = ceil(H W / 1024), 256 lanes.  A pixel takes part when both ids have a record: 1 <= c <= stored, 1 <= p <= stored'.  The labels are compared in T2,
// once per pair instead of once per pixel.
TD_KERNEL void k_tracks_pairs(TracksArgs a) {
    const long HW = (long)a.H * a.W;
    int n, c[4], p[4];
    const long i0 = td_rg_quad(HW, &n);
    const int stored = (int)reinterpret_cast<const TdRegionsHeader*>(a.rtable)->stored, storedp = (int)a.st.words[0];
    td_tk_load4(a.ids, i0, n, c);
    td_tk_load4(a.st.prev, i0, n, p);
    unsigned key[4];
    bool left[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        left[e] = e < n && c[e] >= 1 && c[e] <= stored && p[e] >= 1 && p[e] <= storedp;
        key[e] = ((unsigned)(p[e] - 1) << 16) | ((unsigned)(c[e] - 1) & 0xffffu);
    }
    bool ok = true;
    for (int round = 0; round < TD_RG_ROUNDS; ++round) {
        unsigned mine = TD_RG_NONE;                                    // 0xffffffff is a key too (p = c = 65536): "nothing left" is asked separately
        bool have = false;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (left[e]) { have = true; mine = key[e] < mine ? key[e] : mine; }
        if (!td_any(have)) return;
        const unsigned k = td_rg_wave_min(mine);
        unsigned cnt = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (left[e] && key[e] == k) { ++cnt; left[e] = false; }
        const unsigned total = td_rg_wave_sum(cnt);
        if (td_lane() == 0 && !td_tk_insert(a.st.hash, a.st.lg, k, total)) td_rg_or(a.st.words + 2, TD_TK_BOUND);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                      // the rest: equal keys among the lane's own pixels merged
        if (!left[e]) continue;
        unsigned cnt = 1;
#pragma unroll
        for (int f = e + 1; f < 4; ++f)
            if (left[f] && key[f] == key[e]) { ++cnt; left[f] = false; }
        ok &= td_tk_insert(a.st.hash, a.st.lg, key[e], cnt);
    }
    if (!ok) td_rg_or(a.st.words + 2, TD_TK_BOUND);
}

// ---- T2: best partners ---------------------------------------------------------------------------------------------------------------------------
// grid = ceil(cap / 256), 256 lanes, a lane per slot (plain loads: the table was finished by the previous launch).  ~p in the low word: of equal n the
// SMALLEST partner is the maximum.  Also zeroes the tracks table's table_words 8-byte words, grid-stride (T3 writes the header and the records).
TD_KERNEL void k_tracks_best(TracksArgs a, long table_words) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long)gridDim.x * blockDim.x;
    for (long k = g; k < table_words; k += nthreads) a.table[k] = 0ull;
    if (g >= (1l << a.st.lg)) return;
    const td_u64 v = a.st.hash[g];
    if (v == 0ull) return;
    a.st.hash[g] = 0ull;
    const unsigned p1 = (unsigned)(v >> 48), c1 = (unsigned)(v >> 32) & 0xffffu;
    const td_u64 n = v & 0xffffffffull;
    const TdRegion* rec = reinterpret_cast<const TdRegion*>(a.rtable + 2);
    if (a.st.lab[p1] != rec[c1].label) return;                         // a track keeps its class: n(p, c) = 0
    td_tk_max64(a.st.best_prev + c1, (n << 32) | (td_u64)(~(p1 + 1u)));
    td_tk_max64(a.st.best_cur + p1, (n << 32) | (td_u64)(~(c1 + 1u)));
}

// ---- T3: resolve -----------------------------------------------------------------------------------------------------------------------------------
// ONE workgroup of TD_TK_WG lanes; LDS: TD_TK_WG + 16 ints.  Step by step over 1024 regions: lane t holds region c = base + t + 1.
TD_KERNEL void k_tracks_resolve(TracksArgs a) {
    TD_DYN_LDS(smem);
    int* cnt = reinterpret_cast<int*>(smem);
    int* wtot = cnt + TD_TK_WG;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned stored = reinterpret_cast<const TdRegionsHeader*>(a.rtable)->stored, storedp = a.st.words[0], born0 = a.st.words[1];
    TdTrack* rec = reinterpret_cast<TdTrack*>(a.table + 2);
    unsigned births = 0;
    for (unsigned base = 0; base < stored; base += TD_TK_WG) {         // wave-uniform and workgroup-uniform: every lane meets every barrier
        const unsigned c1 = base + t;
        const bool active = c1 < stored;
        unsigned bp = 0, n = 0;
        bool matched = false;
        if (active) {
            const td_u64 v = a.st.best_prev[c1];
            if (v != 0ull) {
                bp = ~(unsigned)v; n = (unsigned)(v >> 32);
                matched = ~(unsigned)a.st.best_cur[bp - 1] == c1 + 1 && n >= (unsigned)a.min_overlap;
            }
        }
        const int born = active && !matched;
        cnt[t] = born;
        __syncthreads();
        int pre = 0;
        for (int j = t - lane; j < t; ++j) pre += cnt[j];
        if (lane == 63) wtot[wave] = pre + born;
        __syncthreads();
        int total = 0;
        for (int k = 0; k < TD_TK_WG / 64; ++k) { if (k < wave) pre += wtot[k]; total += wtot[k]; }
        if (active) {
            TdTrack r;
            if (matched) { r.track = a.st.track[bp - 1]; r.age = a.st.age[bp - 1] + 1; r.prev_region = bp; r.overlap = n; r.origin_track = r.track; }
            else { r.track = born0 + births + (unsigned)pre + 1u; r.age = 1; r.prev_region = 0; r.overlap = 0; r.origin_track = bp ? a.st.track[bp - 1] : 0u; }
            r.reserved = 0;
            rec[c1] = r;
        }
        births += (unsigned)total;
        __syncthreads();                                               // cnt[] and wtot[] are written again in the next step
    }
    if (t == 0) {
        TdTracksHeader* hd = reinterpret_cast<TdTracksHeader*>(a.table);
        const unsigned matched = stored - births;                      // a match is mutual: the matched p are as many as the matched c
        hd->count = stored; hd->matched = matched; hd->ended = storedp - matched;
        hd->status = a.st.words[2] ? TD_TK_BOUND : 0u;
        a.st.words[1] = born0 + births;
        a.st.words[2] = 0u;
    }
}

// ---- T4: commit ------------------------------------------------------------------------------------------------------------------------------------
// grid = ceil(H W / 1024), 256 lanes.  nbest = min(65536, H W): no frame of this size stores more regions.
TD_KERNEL void k_tracks_commit(TracksArgs a, int nbest) {
    const long HW = (long)a.H * a.W;
    int n, c[4], tr[4];
    const long i0 = td_rg_quad(HW, &n);
    const int stored = (int)reinterpret_cast<const TdRegionsHeader*>(a.rtable)->stored;
    const TdTrack* trec = reinterpret_cast<const TdTrack*>(a.table + 2);
    td_tk_load4(a.ids, i0, n, c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        c[e] = (c[e] >= 1 && c[e] <= stored) ? c[e] : 0;
        tr[e] = c[e] == 0 ? 0 : (e > 0 && c[e] == c[e - 1]) ? tr[e - 1] : (int)trec[c[e] - 1].track;
    }
    td_rg_store4(a.st.prev, i0, n, c);
    if (a.track_ids) td_rg_store4(a.track_ids, i0, n, tr);
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long)gridDim.x * blockDim.x;
    const TdRegion* rrec = reinterpret_cast<const TdRegion*>(a.rtable + 2);
    for (long k = g; k < stored; k += nthreads) { a.st.lab[k] = rrec[k].label; a.st.track[k] = trec[k].track; a.st.age[k] = trec[k].age; }
    for (long k = g; k < nbest; k += nthreads) { a.st.best_prev[k] = 0ull; a.st.best_cur[k] = 0ull; }
    if (g == 0) a.st.words[0] = (unsigned)stored;
}

// tdnet_tracks_reset: one lane; stored' = 0 makes every previous pixel background, the next region is born as track 1
TD_KERNEL void k_tracks_reset(TracksState st) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { st.words[0] = 0u; st.words[1] = 0u; }
}
