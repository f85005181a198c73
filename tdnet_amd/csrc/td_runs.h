// td_runs.h -- runs out: a label map (uint8) or an id / track map (int32) as a table of horizontal runs, coded -- and decoded -- on the device.
//
// The contract (include/tdnet.h "runs out"): V[Y][X] a map of H x W, flat index i = Y W + X.  Pixel i starts a run iff X == 0 or V[i] != V[i - 1]; the
// runs are numbered 1, 2, ... by growing start; the table is a header {count, stored, status, reserved}, then stored records {start, value} and ONE
// closing record {start of run stored + 1, or H W; 0}.  Nothing behind the closing record is written.  Everything is an integer and every rank is a
// prefix sum over the raster: the result does not depend on the launch geometry, and no launch needs an atomic or waits for another workgroup.
//
// Three launches behind the map (TD_RUNS_LAUNCHES counts the frame's label launch, k_upsample_argmax_u8 unchanged, as the first), each a plain grid:
//   k_runs_count<T>   the start flags of a lane's (up to) 4 pixels, popcount, a wave reduction, one word per block of TD_RN_BLOCK lanes
//   k_runs_scan       ONE workgroup: the exclusive scan of the block counts in chunks of 256 with a carry; the header
//   k_runs_emit<T>    the flags again; rank = block offset + wave offsets (LDS) + the prefix inside the wave; a start with rank < max_runs stores its
//                     record with one 8-byte store; the start with rank == max_runs, or else the lane that owns the map's last pixel, the closing record
// and one for the way back:
//   k_runs_decode<T>  a binary search over the stored starts for the lane's first pixel, a walk over at most three further records, packed stores
//
// Lanes and pixels: the map is ONE run of H W elements (k_argmax_u8's split, td_out.h td_u8_run): lane 0 takes the elements in front of the first
// aligned group of 4 (4 bytes for uint8, 16 bytes for int32), lane q >= 1 the aligned group behind it, so every full group is one aligned load whatever
// the map's address.  The left neighbour of a lane's first pixel is one extra element.  X == 0 comes from one 32-bit remainder per lane (H W < 2^30).
//
// Written on the TD_* macros only (tests/emu runs this file unchanged): td_rn_prefix4 below is the only build-dependent code; plain C++ and vector
// stores, no inline assembly, no atomics.
#pragma once
#include "td_device.h"
#include "td_regions.h"  // td_rg_shfl_xor / td_rg_wave_sum / td_i32x4 / TD_RG_MAX_PIXELS: the same wave helpers, the same size limit

#define TD_RN_LANES 256                                                // lanes of a workgroup,
#define TD_RN_BLOCK (4 * TD_RN_LANES)                                  // pixels it covers (the first block: up to 3 fewer, the head lane)
#define TD_RUNS_LAUNCHES 4                                             // label launch + count + scan + emit
#define TD_RUNS_DECODE_LAUNCHES 1
#define TD_RN_OVERFLOW 1u                                              // header status bit (include/tdnet.h TDNET_RUNS_OVERFLOW)

struct TdRun { unsigned start; int value; };                          // 8 bytes
struct TdRunsHeader { unsigned count, stored, status, reserved; };    // 16 bytes
typedef unsigned td_u32x2 __attribute__((ext_vector_type(2)));

struct RunsArgs {
    const void* map;               // the map [H][W]: uint8 at any byte address, int32 at any 4-byte aligned address
    unsigned long long* table;     // header + max_runs + 1 records, 8-byte aligned
    int* blk;                      // workspace: the block counts [runs_blocks(H, W)], then their exclusive scan
    int H, W;
    int max_runs;
};

// The sum of v over the lanes of the wave below this one (every lane of the wave calls it), for any v whose wave sum fits 32 bits, on the xor shuffle
// alone: after the step of mask m a lane holds the total of its 2 m lanes, and a lane with bit m set has added the total of the m lanes below its half
TD_DEV unsigned td_rn_prefix(unsigned v) {
    const unsigned lane = (unsigned)td_lane();
    unsigned pre = 0;
    for (unsigned m = 1; m < 64; m <<= 1) {
        const unsigned o = td_rg_shfl_xor(v, (int)m);
        pre += (lane & m) ? o : 0u;
        v += o;
    }
    return pre;
}

// ---- the build-dependent wrapper: the same for c in 0 .. 4 from three ballots
TD_DEV unsigned td_rn_prefix4(unsigned c) {
#ifdef TD_EMU
    return td_rn_prefix(c);
#else
    unsigned pre = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(((c >> b) & 1u) != 0);
        pre += __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)) << b;
    }
    return pre;
#endif
}
// ---- the lane split and the loads ---------------------------------------------------------------------------------------------------------
// lane q's elements [pa, pb) of the HW elements at `base`: lane 0 those in front of the first 4 sizeof(T)-byte boundary, lane q >= 1 the aligned group
template <typename T>
TD_DEV void td_rn_run(const T* base, long q, long HW, long* pa, long* pb) {
    const unsigned A = 4u * (unsigned)sizeof(T);
    const long X0 = (long)(((A - (unsigned)((size_t)base & (A - 1u))) & (A - 1u)) / (unsigned)sizeof(T));
    *pa = q == 0 ? 0 : X0 + 4 * (q - 1);
    *pb = q == 0 ? (X0 < HW ? X0 : HW) : (*pa + 4 < HW ? *pa + 4 : HW);
    if (*pa > HW) *pa = HW;
}
// a full group starts at an aligned address by construction of the split (q >= 1): one 4-byte / 16-byte load
TD_DEV void td_rn_load(const unsigned char* p, long pa, long pb, bool full, int* v) {
    if (full) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p + pa);
        v[0] = (int)(w & 255u); v[1] = (int)((w >> 8) & 255u); v[2] = (int)((w >> 16) & 255u); v[3] = (int)(w >> 24);
    } else {
        for (long i = pa; i < pb; ++i) v[i - pa] = p[i];
    }
}
TD_DEV void td_rn_load(const int* p, long pa, long pb, bool full, int* v) {
    if (full) {
        const td_i32x4 w = *reinterpret_cast<const td_i32x4*>(p + pa);
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
        for (long i = pa; i < pb; ++i) v[i - pa] = p[i];
    }
}
TD_DEV void td_rn_store(unsigned char* p, long pa, long pb, bool full, const int* v) {
    if (full) *reinterpret_cast<unsigned*>(p + pa) = (unsigned)(v[0] & 255) | ((unsigned)(v[1] & 255) << 8) | ((unsigned)(v[2] & 255) << 16) | ((unsigned)(v[3] & 255) << 24);
    else for (long i = pa; i < pb; ++i) p[i] = (unsigned char)v[i - pa];
}
TD_DEV void td_rn_store(int* p, long pa, long pb, bool full, const int* v) {
    if (full) { const td_i32x4 w = {v[0], v[1], v[2], v[3]}; *reinterpret_cast<td_i32x4*>(p + pa) = w; }
    else for (long i = pa; i < pb; ++i) p[i] = v[i - pa];
}
// The lane's pixels, their values and start flags (bit e: pixel pa + e starts a run); returns the number of starts.  v[] must hold 4.
template <typename T>
TD_DEV unsigned td_rn_flags(const RunsArgs& a, long* pa, long* pb, int* v, unsigned* flags) {
    const long HW = (long)a.H * a.W, q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const T* map = reinterpret_cast<const T*>(a.map);
    td_rn_run(map, q, HW, pa, pb);
    unsigned f = 0;
    if (*pa < *pb) {
        td_rn_load(map, *pa, *pb, q > 0 && *pb - *pa == 4, v);
        int left = *pa > 0 ? (int)map[*pa - 1] : 0;
        unsigned x = (unsigned)*pa % (unsigned)a.W;                    // one remainder per lane; the pixels behind it count up
        const int n = (int)(*pb - *pa);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < n) {
                f |= (x == 0u || v[e] != left) ? 1u << e : 0u;
                left = v[e];
                if (++x == (unsigned)a.W) x = 0u;
            }
        }
    }
    *flags = f;
    return (unsigned)__builtin_popcount(f);
}

// ---- count: blk[b] = the run starts among block b's pixels.  LDS: 4 ints. ----------------------------------------------------------------
template <typename T>
TD_KERNEL void k_runs_count(RunsArgs a) {
    TD_DYN_LDS(smem);
    int* wsum = reinterpret_cast<int*>(smem);
    long pa, pb;
    int v[4];
    unsigned flags;
    const unsigned c = td_rg_wave_sum(td_rn_flags<T>(a, &pa, &pb, v, &flags));
    if (td_lane() == 0) wsum[threadIdx.x >> 6] = (int)c;
    __syncthreads();
    if (threadIdx.x == 0) a.blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// ---- scan: ONE workgroup of 256 lanes; blk[] becomes its exclusive scan, 256 counts at a time with a carry; the header.  LDS: 4 ints. --------
TD_KERNEL void k_runs_scan(RunsArgs a, int nblk) {
    TD_DYN_LDS(smem);
    int* wtot = reinterpret_cast<int*>(smem);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned carry = 0;
    for (int j0 = 0; j0 < nblk; j0 += TD_RN_LANES) {
        const int j = j0 + t;
        const unsigned v = j < nblk ? (unsigned)a.blk[j] : 0u;
        unsigned pre = td_rn_prefix(v);
        if (lane == 63) wtot[wave] = (int)(pre + v);
        __syncthreads();
        unsigned total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const unsigned w = (unsigned)wtot[k]; pre += k < wave ? w : 0u; total += w; }
        if (j < nblk) a.blk[j] = (int)(carry + pre);
        carry += total;
        __syncthreads();                                               // wtot[] is free for the next chunk
    }
    if (t == 0) {
        TdRunsHeader* hd = reinterpret_cast<TdRunsHeader*>(a.table);
        const unsigned maxr = (unsigned)a.max_runs;
        hd->count = carry;
        hd->stored = carry < maxr ? carry : maxr;
        hd->status = carry > maxr ? TD_RN_OVERFLOW : 0u;
        hd->reserved = 0u;
    }
}
// ---- emit: the records.  LDS: 4 ints. ---------------------------------------------------------------------------------------------------------
TD_DEV void td_rn_put(unsigned long long* table, unsigned j, unsigned start, int value) {
    const td_u32x2 r = {start, (unsigned)value};
    *reinterpret_cast<td_u32x2*>(table + 2 + j) = r;
}
template <typename T>
TD_KERNEL void k_runs_emit(RunsArgs a) {
    TD_DYN_LDS(smem);
    int* wtot = reinterpret_cast<int*>(smem);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long pa, pb;
    int v[4];
    unsigned flags;
    const unsigned c = td_rn_flags<T>(a, &pa, &pb, v, &flags);
    unsigned rank = td_rn_prefix4(c);
    if (lane == 63) wtot[wave] = (int)(rank + c);
    __syncthreads();
    for (int k = 0; k < wave; ++k) rank += (unsigned)wtot[k];
    rank += (unsigned)a.blk[blockIdx.x];
    const unsigned maxr = (unsigned)a.max_runs;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!((flags >> e) & 1u)) continue;
        if (rank < maxr) td_rn_put(a.table, rank, (unsigned)(pa + e), v[e]);
        else if (rank == maxr) td_rn_put(a.table, rank, (unsigned)(pa + e), 0);   // count > max_runs: the closing record is the start of run stored + 1
        ++rank;
    }
    const long HW = (long)a.H * a.W;
    if (pa < pb && pb == HW && rank <= maxr) td_rn_put(a.table, rank, (unsigned)HW, 0);   // the owner of the last pixel knows count: nothing starts behind it
}
// ---- decode: one launch; out[i] = the value of the run that holds i below the closing record's start, fill elsewhere ---------------------------------
// stored comes from the device header, clamped to max_runs: every record index read is <= max_runs whatever the table holds.
template <typename T>
TD_KERNEL void k_runs_decode(RunsArgs a, int fill) {
    const long HW = (long)a.H * a.W, q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    T* out = reinterpret_cast<T*>(const_cast<void*>(a.map));
    long pa, pb;
    td_rn_run(out, q, HW, &pa, &pb);
    if (pa >= pb) return;
    const TdRunsHeader* hd = reinterpret_cast<const TdRunsHeader*>(a.table);
    const TdRun* rec = reinterpret_cast<const TdRun*>(a.table + 2);
    const unsigned maxr = (unsigned)a.max_runs;
    const unsigned stored = hd->stored < maxr ? hd->stored : maxr;
    const unsigned end = rec[stored].start;
    unsigned lo = 0, hi = stored;                                      // the first record in [0, stored) that starts behind pa
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (rec[mid].start <= (unsigned)pa) lo = mid + 1; else hi = mid;
    }
    long j = (long)lo - 1;                                             // the run that holds pa (-1: none, an unwritten table)
    int val = j >= 0 ? rec[j].value : fill;
    int v[4] = {fill, fill, fill, fill};
    const int n = (int)(pb - pa);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e >= n) continue;
        const unsigned i = (unsigned)(pa + e);
        if (e > 0 && j + 1 < (long)stored) {                           // distinct starts: a pixel further is at most a record further
            const TdRun r = rec[j + 1];
            if (r.start <= i) { ++j; val = r.value; }
        }
        v[e] = (j >= 0 && i < end) ? val : fill;
    }
    td_rn_store(out, pa, pb, q > 0 && n == 4, v);
}
