// tools/copybench.hip -- which 16 B/lane copy shapes reach the HBM copy ceiling on MI355X (development aid).
//   hipcc --offload-arch=gfx950 -O3 -o gpurun_out/copybench tools/copybench.hip && gpurun_out/copybench [GiB]
//   ... copybench pieces: the read patterns of a count-free pass 1's output
//   ... copybench planes: word-plane layouts of its payload array
// Shapes: the scatter kernel's (one contiguous region per workgroup, 32 KiB tiles, next tile prefetched)
// against tile-interleaved and grid-stride copies, with and without nontemporal hints.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>

typedef unsigned long long u64;
typedef unsigned int u32;
struct __attribute__((aligned(16))) Tup { u64 key, payload; };

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <bool NT> __device__ __forceinline__ Tup ld(const Tup *p)
{
    if (NT) { Tup t; t.key = __builtin_nontemporal_load(&p->key); t.payload = __builtin_nontemporal_load(&p->payload); return t; }
    return *p;
}
template <bool NT> __device__ __forceinline__ void st(Tup *p, const Tup &t)
{
    if (NT) { __builtin_nontemporal_store(t.key, &p->key); __builtin_nontemporal_store(t.payload, &p->payload); }
    else *p = t;
}

// MODE 0: workgroup u copies the contiguous region [u*L, (u+1)*L) tile by tile (the scatter's shape)
// MODE 1: workgroup u copies tiles u, u+G, u+2G, ...
template <int THREADS, int TPT, int MODE, bool NTL, bool NTS, bool PREFETCH>
__global__ void __launch_bounds__(THREADS) k_copy(const Tup *__restrict__ in, Tup *__restrict__ out, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT;
    const u32 u = blockIdx.x, G = gridDim.x, tid = threadIdx.x;
    const u64 ntiles_unit = (MODE == 0) ? (L + TILE - 1) / TILE : (n / TILE + G - 1 - u) / G;
    auto base = [&](u64 j) -> u64 { return MODE == 0 ? (u64)u * L + j * TILE : (j * G + u) * TILE; };
    auto lim = [&](u64 j) -> u64 {
        if (MODE == 0) { u64 e = (u64)(u + 1) * L; return e < n ? e : n; }
        return n;
    };
    Tup a[TPT], b[TPT];
    auto load = [&](Tup (&t)[TPT], u64 j) {
        const u64 tb = base(j), e = lim(j);
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < e) t[k] = ld<NTL>(in + i); }
    };
    auto store = [&](Tup (&t)[TPT], u64 j) {
        const u64 tb = base(j), e = lim(j);
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < e) st<NTS>(out + i, t[k]); }
    };
    if (!PREFETCH) {
        for (u64 j = 0; j < ntiles_unit; j++) { load(a, j); store(a, j); }
        return;
    }
    u64 j = 0;
    if (j < ntiles_unit) load(a, j);
    while (j < ntiles_unit) {
        if (j + 1 < ntiles_unit) load(b, j + 1);
        store(a, j);
        if (++j >= ntiles_unit) break;
        if (j + 1 < ntiles_unit) load(a, j + 1);
        store(b, j);
        ++j;
    }
}

// read-only: sum of payloads (one atomic per workgroup)
template <int THREADS, int TPT, int MODE>
__global__ void __launch_bounds__(THREADS) k_read(const Tup *__restrict__ in, u64 *__restrict__ sink, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT;
    const u32 u = blockIdx.x, G = gridDim.x, tid = threadIdx.x;
    const u64 nt = (MODE == 0) ? (L + TILE - 1) / TILE : (n / TILE + G - 1 - u) / G;
    u64 acc = 0;
    for (u64 j = 0; j < nt; j++) {
        const u64 tb = MODE == 0 ? (u64)u * L + j * TILE : (j * G + u) * TILE;
        u64 e = MODE == 0 ? (u64)(u + 1) * L : n; if (e > n) e = n;
        Tup t[TPT];
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; t[k] = (i < e) ? in[i] : Tup{0, 0}; }
#pragma unroll
        for (int k = 0; k < TPT; k++) acc += t[k].payload ^ t[k].key;
    }
    if (acc == 0x1234567) atomicAdd(sink, acc);
}

// write-only
template <int THREADS, int TPT, int MODE>
__global__ void __launch_bounds__(THREADS) k_write(Tup *__restrict__ out, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT;
    const u32 u = blockIdx.x, G = gridDim.x, tid = threadIdx.x;
    const u64 nt = (MODE == 0) ? (L + TILE - 1) / TILE : (n / TILE + G - 1 - u) / G;
    for (u64 j = 0; j < nt; j++) {
        const u64 tb = MODE == 0 ? (u64)u * L + j * TILE : (j * G + u) * TILE;
        u64 e = MODE == 0 ? (u64)(u + 1) * L : n; if (e > n) e = n;
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < e) out[i] = Tup{i, j}; }
    }
}


// ---- narrow (12 B/tuple, structure of arrays) experiments -----------------------------------------------
// tuples/s is what matters here: AoS16 moves 32 B per tuple copied, SoA12 moves 24 B
// PAIR: a lane handles two adjacent tuples (16 B payload load + 8 B rowid load)
template <int THREADS, int TPT, bool PAIR>
__global__ void __launch_bounds__(THREADS) k_copy_soa(const u64 *__restrict__ inP, const u32 *__restrict__ inK,
                                                      u64 *__restrict__ outP, u32 *__restrict__ outK, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT;
    const u32 u = blockIdx.x, tid = threadIdx.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    for (u64 tb = beg; tb < end; tb += TILE) {
        if (PAIR) {
            ulonglong2 p[TPT / 2]; uint2 k2[TPT / 2];
#pragma unroll
            for (int k = 0; k < TPT / 2; k++) {
                const u64 i = tb + (u64)k * 2 * THREADS + 2 * tid;
                if (i < end) { p[k] = *reinterpret_cast<const ulonglong2 *>(inP + i); k2[k] = *reinterpret_cast<const uint2 *>(inK + i); }
            }
#pragma unroll
            for (int k = 0; k < TPT / 2; k++) {
                const u64 i = tb + (u64)k * 2 * THREADS + 2 * tid;
                if (i < end) { *reinterpret_cast<ulonglong2 *>(outP + i) = p[k]; *reinterpret_cast<uint2 *>(outK + i) = k2[k]; }
            }
        } else {
            u64 p[TPT]; u32 kk[TPT];
#pragma unroll
            for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < end) { p[k] = inP[i]; kk[k] = inK[i]; } }
#pragma unroll
            for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < end) { outP[i] = p[k]; outK[i] = kk[k]; } }
        }
    }
}

// AoS16 in -> scattered 8-tuple lines out (the write pattern of the scatter: 8 adjacent lanes own one line at a
// pseudo-random line index).  NARROW: line = 64 B of payloads + 32 B of rowids in two arrays; else one 128 B line.
template <int THREADS, int TPT, bool NARROW>
__global__ void __launch_bounds__(THREADS) k_scatter_lines(const Tup *__restrict__ in, Tup *__restrict__ out, u64 *__restrict__ outP,
                                                           u32 *__restrict__ outK, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT;
    const u32 u = blockIdx.x, tid = threadIdx.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    const u64 nlines = n / 8;
    for (u64 tb = beg; tb < end; tb += TILE) {
        Tup t[TPT];
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < end) t[k] = in[i]; }
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const u64 i = tb + (u64)k * THREADS + tid;
            if (i < end) {
                const u64 line = ((i >> 3) * 0x9E3779B97F4A7C15ull >> 20) % nlines;          // a permutation-ish map of lines
                const u64 o = line * 8 + (i & 7);
                if (NARROW) { outP[o] = t[k].payload; outK[o] = (u32)t[k].key; }
                else out[o] = t[k];
            }
        }
    }
}

// AoS16 in -> the scatter's real write pattern: 256 sequential streams per workgroup, each advancing by one chunk of GR
// tuples at a time.  NARROW: chunk = GR*8 B of payloads + GR*4 B of rowids in two arrays; else GR*16 B in one.
template <int THREADS, int TPT, bool NARROW, int GR, int MODE = 0>
__global__ void __launch_bounds__(THREADS) k_stream_lines(const Tup *__restrict__ in, Tup *__restrict__ out, u64 *__restrict__ outP,
                                                          u32 *__restrict__ outK, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT;
    const u32 u = blockIdx.x, tid = threadIdx.x, G = gridDim.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    const u64 cpud = (L / GR + 255) / 256, cpd = (u64)G * cpud;
    u64 j = 0;
    for (u64 tb = beg; tb < end; tb += TILE, j++) {
        Tup t[TPT];
        // MODE 1: the READ side is tile-interleaved over the workgroups (tile j of workgroup u = global tile j * G + u)
        const u64 rb = MODE == 0 ? tb : (j * G + u) * TILE;
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = rb + (u64)k * THREADS + tid; if (tb + (u64)k * THREADS + tid < end && i < n) t[k] = in[i]; }
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const u32 it = k * THREADS + tid;
            if (tb + it < end) {
                const u64 cg = j * (TILE / GR) + it / GR;
                const u64 o = ((cg & 255) * cpd + (u64)u * cpud + (cg >> 8)) * GR + it % GR;
                if (NARROW) { outP[o] = t[k].payload; outK[o] = (u32)t[k].key; }
                else out[o] = t[k];
            }
        }
    }
}

// AoS16 in -> SoA12 out, linear (the byte mix of a narrow-output pass without any scatter): T threads, tiles of T*TPT
template <int THREADS, int TPT>
__global__ void __launch_bounds__(THREADS) k_aos_to_soa(const Tup *__restrict__ in, u64 *__restrict__ outP, u32 *__restrict__ outK, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT;
    const u32 u = blockIdx.x, tid = threadIdx.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    for (u64 tb = beg; tb < end; tb += TILE) {
        Tup t[TPT];
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < end) t[k] = in[i]; }
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < end) { outP[i] = t[k].payload; outK[i] = (u32)t[k].key; } }
    }
}

// ---- count-free pass 1: what reading its output costs ------------------------------------
// Pass 1 without counts leaves bucket d's tuples as one piece per pass-1 unit u, in region (d * U + u) * cap of the
// payload / rowID arrays; a pass-2 unit (d, g) then reads PER consecutive pieces at stride cap instead of one run.
// len(d, u) = mean - spread/2 + (a hash of the region) % spread: not line-aligned, as the real pieces.
__host__ __device__ __forceinline__ u32 piece_len(u32 region, u32 mean, u32 spread)
{
    return mean - spread / 2 + (u32)(((u64)region * 0x9E3779B97F4A7C15ull) >> 40) % spread;
}
__global__ void k_fill_hash(u64 *__restrict__ p, u64 n)       // digits spread over all counters, as hashed join values are
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        u64 z = (i + 1) * 0x9E3779B97F4A7C15ull; z ^= z >> 29; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 32;
        p[i] = z;
    }
}
constexpr int PC_PER = 64;              // pieces per pass-2 unit (pass-1 units per group)

// (a) the pass-2 histogram: 8 B per tuple.  PIECES: every wavefront streams whole pieces (piece j of the unit goes to
// wavefront j % waves), eight loads in flight per lane; else the unit's tuples are ONE run (today's k_hist_units_n shape).
template <int THREADS, bool PIECES>
__global__ void __launch_bounds__(THREADS) k_hist_pieces(const u64 *__restrict__ inP, u32 cap, u32 mean, u32 spread, int shift,
                                                         u32 *__restrict__ hist)
{
    __shared__ u32 cnt[256];
    __shared__ u32 pre[PC_PER + 1];
    const u32 unit = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) cnt[tid] = 0;
    if (tid == 0) { u32 s = 0; for (int j = 0; j < PC_PER; j++) { pre[j] = s; s += piece_len(unit * PC_PER + j, mean, spread); } pre[PC_PER] = s; }
    __syncthreads();
    const u64 ubase = (u64)unit * PC_PER * cap;
    if (PIECES) {
        for (u32 j = wave; j < PC_PER; j += THREADS / 64) {
            const u64 *p = inP + ubase + (u64)j * cap;
            const u32 len = pre[j + 1] - pre[j];
            u32 i = lane;
            for (; i + 7u * 64u < len; i += 8u * 64u) {
                u64 v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = p[i + k * 64];
#pragma unroll
                for (int k = 0; k < 8; k++) atomicAdd(&cnt[(u32)(v[k] >> shift) & 255u], 1u);
            }
            for (; i < len; i += 64) atomicAdd(&cnt[(u32)(p[i] >> shift) & 255u], 1u);
        }
    } else {
        const u64 *p = inP + ubase;
        const u32 len = pre[PC_PER];
        u32 i = tid;
        for (; i + 7u * THREADS < len; i += 8u * THREADS) {
            u64 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = p[i + k * THREADS];
#pragma unroll
            for (int k = 0; k < 8; k++) atomicAdd(&cnt[(u32)(v[k] >> shift) & 255u], 1u);
        }
        for (; i < len; i += THREADS) atomicAdd(&cnt[(u32)(p[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 256) hist[(u64)unit * 256 + tid] = cnt[tid];
}

// (b) pass 2's byte mix: 8 + 4 B read per tuple in dense 4096-tuple tiles (slot t of the unit -> piece by a binary search of
// the prefix in LDS, next tile prefetched), 8 + 4 B written as 256 streams of 32-tuple lines per workgroup (k_stream_lines).
template <int THREADS, int TPT, bool PIECES, int LAYOUT = 0>
__global__ void __launch_bounds__(THREADS) k_pass2_pieces(const u64 *__restrict__ inP, const u32 *__restrict__ inK, u64 *__restrict__ outP,
                                                          u32 *__restrict__ outK, u32 cap, u32 mean, u32 spread, u32 cpud, u64 plane)
{
    constexpr u32 TILE = THREADS * TPT, GR = 32;
    __shared__ u32 pre[PC_PER + 1];
    const u32 unit = blockIdx.x, tid = threadIdx.x, G = gridDim.x;
    if (tid == 0) { u32 s = 0; for (int j = 0; j < PC_PER; j++) { pre[j] = s; s += piece_len(unit * PC_PER + j, mean, spread); } pre[PC_PER] = s; }
    __syncthreads();
    const u32 total = pre[PC_PER];
    const u64 ubase = (u64)unit * PC_PER * cap, cpd = (u64)G * cpud;
    auto addr = [&](u32 t) -> u64 {
        if (!PIECES) return ubase + t;
        u32 lo = 0;
#pragma unroll
        for (u32 s = PC_PER / 2; s > 0; s >>= 1) if (pre[lo + s] <= t) lo += s;
        return ubase + (u64)lo * cap + (t - pre[lo]);
    };
    auto load = [&](u64 (&p)[TPT], u32 (&kk)[TPT], u32 tb) {
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            u32 t = tb + k * THREADS + tid; t = t < total ? t : total - 1;
            const u64 a = addr(t);
            if (LAYOUT != 0) {                                               // (word planes: see k_hist_planes; 1 blocked, 2 separate)
                const u32 *W = reinterpret_cast<const u32 *>(inP);
                const u64 w = LAYOUT == 1 ? (((a >> 5) << 6) | (a & 31)) : a;
                p[k] = W[w] | (u64)W[w + (LAYOUT == 1 ? 32 : plane)] << 32;
            } else p[k] = inP[a];
            kk[k] = inK[a];
        }
    };
    auto store = [&](u64 (&p)[TPT], u32 (&kk)[TPT], u32 tb) {
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const u32 it = k * THREADS + tid;
            if (tb + it < total) {
                const u64 cg = (u64)(tb / TILE) * (TILE / GR) + it / GR;
                const u64 o = ((cg & 255) * cpd + (u64)unit * cpud + (cg >> 8)) * GR + it % GR;
                __builtin_nontemporal_store(p[k], &outP[o]); __builtin_nontemporal_store(kk[k], &outK[o]);
            }
        }
    };
    u64 pa[TPT], pb[TPT]; u32 ka[TPT], kb[TPT];
    u32 cur = 0;
    load(pa, ka, cur);
    while (cur < total) {
        u32 nxt = cur + TILE;
        load(pb, kb, nxt < total ? nxt : cur);
        store(pa, ka, cur);
        cur = nxt; if (cur >= total) break;
        nxt = cur + TILE;
        load(pa, ka, nxt < total ? nxt : cur);
        store(pb, kb, cur);
        cur = nxt;
    }
}


// ---- word planes for the count-free payload array -------------------------------------------
// The pass-2 digit lies in the low 32-bit word of a payload, so the histogram needs 4 of the 8 bytes.  BLOCKED: inside every
// 256-byte block of 32 slots the 32 low words come first, then the 32 high words: slot a -> word w(a) = ((a >> 5) << 6) | (a & 31),
// high word at w(a) + 32; the histogram reads every other 128-byte line.  Else a separate, dense array of low words.
// 16-byte loads: 8 lanes cover a line, a wavefront 256 tuples per load, eight loads in flight (clamped to the piece's last block).
template <int THREADS, bool BLOCKED>
__global__ void __launch_bounds__(THREADS) k_hist_planes(const u32 *__restrict__ W, u32 cap, u32 mean, u32 spread, int shift,
                                                         u32 *__restrict__ hist)
{
    __shared__ u32 cnt[256];
    __shared__ u32 pre[PC_PER + 1];
    const u32 unit = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) cnt[tid] = 0;
    if (tid == 0) { u32 s = 0; for (int j = 0; j < PC_PER; j++) { pre[j] = s; s += piece_len(unit * PC_PER + j, mean, spread); } pre[PC_PER] = s; }
    __syncthreads();
    const u64 ubase = (u64)unit * PC_PER * cap;
    const u32 sub = lane >> 3, off = (lane & 7) * 4;
    for (u32 j = wave; j < PC_PER; j += THREADS / 64) {
        const u32 *p = W + (ubase + (u64)j * cap) * (BLOCKED ? 2 : 1);
        const u32 len = pre[j + 1] - pre[j], nblk = (len + 31) / 32;
        for (u32 b0 = 0; b0 < nblk; b0 += 64) {
            uint4 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                u32 b = b0 + k * 8 + sub; b = b < nblk ? b : nblk - 1;
                v[k] = *reinterpret_cast<const uint4 *>(p + (u64)b * (BLOCKED ? 64 : 32) + off);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const u32 t = (b0 + k * 8 + sub) * 32 + off;                 // (beyond the clamp: t >= len)
                if (t + 0 < len) atomicAdd(&cnt[(v[k].x >> shift) & 255u], 1u);
                if (t + 1 < len) atomicAdd(&cnt[(v[k].y >> shift) & 255u], 1u);
                if (t + 2 < len) atomicAdd(&cnt[(v[k].z >> shift) & 255u], 1u);
                if (t + 3 < len) atomicAdd(&cnt[(v[k].w >> shift) & 255u], 1u);
            }
        }
    }
    __syncthreads();
    if (tid < 256) hist[(u64)unit * 256 + tid] = cnt[tid];
}

// pass 1's write pattern (k_stream_lines, narrow, 32-tuple chunks, nontemporal).  LAYOUT 0: 256 + 128 bytes into two arrays
// (today's), 1: the same bytes with the payload words in blocked planes, 2: 128 + 128 + 128 bytes into three arrays.
template <int THREADS, int TPT, int LAYOUT>
__global__ void __launch_bounds__(THREADS) k_stream_planes(const Tup *__restrict__ in, u64 *__restrict__ outP, u32 *__restrict__ outK,
                                                           u64 plane, u64 n, u64 L)
{
    constexpr u64 TILE = (u64)THREADS * TPT, GR = 32;
    const u32 u = blockIdx.x, tid = threadIdx.x, G = gridDim.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    const u64 cpud = (L / GR + 255) / 256, cpd = (u64)G * cpud;
    u32 *W = reinterpret_cast<u32 *>(outP);
    u64 j = 0;
    for (u64 tb = beg; tb < end; tb += TILE, j++) {
        Tup t[TPT];
#pragma unroll
        for (int k = 0; k < TPT; k++) { const u64 i = tb + (u64)k * THREADS + tid; if (i < end) t[k] = in[i]; }
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const u32 it = k * THREADS + tid;
            if (tb + it < end) {
                const u64 cg = j * (TILE / GR) + it / GR;
                const u64 o = ((cg & 255) * cpd + (u64)u * cpud + (cg >> 8)) * GR + it % GR;
                const u64 v = t[k].payload;
                if (LAYOUT == 0) __builtin_nontemporal_store(v, &outP[o]);
                else {
                    const u64 w = LAYOUT == 1 ? (((o >> 5) << 6) | (o & 31)) : o, hi = LAYOUT == 1 ? 32 : plane;
                    __builtin_nontemporal_store((u32)v, &W[w]); __builtin_nontemporal_store((u32)(v >> 32), &W[w + hi]);
                }
                __builtin_nontemporal_store((u32)t[k].key, &outK[o]);
            }
        }
    }
}

template <typename F> static double time_ms(F f, int reps = 5)
{
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    f(); CK(hipDeviceSynchronize());
    std::vector<float> ms;
    for (int r = 0; r < reps; r++) {
        CK(hipEventRecord(e0, 0)); f(); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        float m; CK(hipEventElapsedTime(&m, e0, e1)); ms.push_back(m);
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

// copybench pieces: the two read patterns of a count-free pass 1's output at 10^9 tuples (256 buckets x 1024 pass-1 units,
// mean piece 3824 tuples in regions of cap = 4448), each against its contiguous form, plus the 16-byte read they replace.
static int run_pieces()
{
    const u32 nb1 = 256, U = 1024, mean = 3824, spread = 257, cap = 4448, units2 = nb1 * U / PC_PER;
    const u64 regions = (u64)nb1 * U, slots = regions * cap;
    u64 ntup = 0; u32 lmax = 0;
    for (u32 r = 0; r < regions; r++) { const u32 l = piece_len(r, mean, spread); ntup += l; lmax = l > lmax ? l : lmax; }
    if (lmax > cap) { fprintf(stderr, "piece above cap\n"); return 1; }
    const u32 cpud = ((u32)PC_PER * lmax / 32 + 1 + 255) / 256;                  // 32-tuple chunks per (unit, stream)
    const u64 out_slots = 256ull * units2 * cpud * 32;                           // one past the largest index written
    u64 *inP, *outP; u32 *inK, *outK, *hist; Tup *aos; u64 *sink;
    CK(hipMalloc(&inP, slots * 8)); CK(hipMalloc(&inK, slots * 4)); CK(hipMalloc(&outP, out_slots * 8)); CK(hipMalloc(&outK, out_slots * 4));
    CK(hipMalloc(&hist, (size_t)units2 * 256 * 4)); CK(hipMalloc(&aos, ntup * 16)); CK(hipMalloc(&sink, 8));
    hipLaunchKernelGGL(k_fill_hash, dim3(4096), dim3(256), 0, 0, inP, slots); CK(hipDeviceSynchronize()); CK(hipMemset(inK, 1, slots * 4)); CK(hipMemset(aos, 1, ntup * 16)); CK(hipMemset(sink, 0, 8));
    printf("# %llu tuples in %llu pieces (mean %u, max %u, cap %u); times scaled to 10^9 tuples\n", (unsigned long long)ntup,
           (unsigned long long)regions, mean, lmax, cap);
    auto rep = [&](const char *name, double ms) { printf("%-74s %8.3f ms\n", name, ms * 1e9 / (double)ntup); fflush(stdout); };
    for (int round = 0; round < 2; round++) {
        {
            const int G = 1024; const u64 L = ((ntup + G - 1) / G + 2047) / 2048 * 2048;
            rep("16 B AoS read T=512 tpt=4 contiguous G=1024 (the histogram's)",
                time_ms([&] { hipLaunchKernelGGL((k_read<512, 4, 0>), dim3(G), dim3(512), 0, 0, aos, sink, ntup, L); }));
        }
        rep("(a) 8 B hist, one run per unit, T=512", time_ms([&] { hipLaunchKernelGGL((k_hist_pieces<512, false>), dim3(units2), dim3(512), 0, 0, inP, cap, mean, spread, 8, hist); }));
        rep("(a) 8 B hist, 64 pieces at stride cap, wavefront per piece, T=512", time_ms([&] { hipLaunchKernelGGL((k_hist_pieces<512, true>), dim3(units2), dim3(512), 0, 0, inP, cap, mean, spread, 8, hist); }));
        rep("(a) 8 B hist, 64 pieces at stride cap, wavefront per piece, T=1024", time_ms([&] { hipLaunchKernelGGL((k_hist_pieces<1024, true>), dim3(units2), dim3(1024), 0, 0, inP, cap, mean, spread, 8, hist); }));
        rep("(b) 12 + 12 B, one run per unit, T=1024 lds=150K", time_ms([&] { hipLaunchKernelGGL((k_pass2_pieces<1024, 4, false>), dim3(units2), dim3(1024), 150 << 10, 0, inP, inK, outP, outK, cap, mean, spread, cpud, (u64)0); }));
        rep("(b) 12 + 12 B, 64 pieces at stride cap, dense tiles, T=1024 lds=150K", time_ms([&] { hipLaunchKernelGGL((k_pass2_pieces<1024, 4, true>), dim3(units2), dim3(1024), 150 << 10, 0, inP, inK, outP, outK, cap, mean, spread, cpud, (u64)0); }));
    }
    return 0;
}

// copybench planes: the same geometry as `pieces`; what the word-plane layouts of the count-free payload array cost and save.
// Each line stands against the `pieces` figure it would replace (printed first in every round).
static int run_planes()
{
    const u32 nb1 = 256, U = 1024, mean = 3824, spread = 257, cap = 4448, units2 = nb1 * U / PC_PER;
    const u64 regions = (u64)nb1 * U, slots = regions * cap;
    u64 ntup = 0; u32 lmax = 0;
    for (u32 r = 0; r < regions; r++) { const u32 l = piece_len(r, mean, spread); ntup += l; lmax = l > lmax ? l : lmax; }
    if (lmax > cap || cap % 32) { fprintf(stderr, "piece above cap\n"); return 1; }
    const u32 cpud = ((u32)PC_PER * lmax / 32 + 1 + 255) / 256;
    const u64 out_slots = 256ull * units2 * cpud * 32;
    const int G1 = 1024;                                                          // pass 1: 1024 units, 256 streams each
    const u64 n1 = ntup - (32ull << 20), L1 = ((n1 + G1 - 1) / G1 + 4095) / 4096 * 4096;
    const u64 top1 = 256ull * G1 * ((L1 / 32 + 255) / 256) * 32;                  // one past the largest index pass 1's pattern writes
    if (top1 > out_slots) { fprintf(stderr, "stream test would overrun: %llu > %llu\n", (unsigned long long)top1, (unsigned long long)out_slots); return 1; }
    u64 *inP, *outP; u32 *inK, *outK, *hist; Tup *aos;
    CK(hipMalloc(&inP, slots * 8)); CK(hipMalloc(&inK, slots * 4)); CK(hipMalloc(&outP, out_slots * 8)); CK(hipMalloc(&outK, out_slots * 4));
    CK(hipMalloc(&hist, (size_t)units2 * 256 * 4)); CK(hipMalloc(&aos, ntup * 16));
    hipLaunchKernelGGL(k_fill_hash, dim3(4096), dim3(256), 0, 0, inP, slots); CK(hipDeviceSynchronize()); CK(hipMemset(inK, 1, slots * 4)); CK(hipMemset(aos, 1, ntup * 16));
    printf("# %llu tuples in %llu pieces (mean %u, max %u, cap %u); times scaled to 10^9 tuples\n", (unsigned long long)ntup,
           (unsigned long long)regions, mean, lmax, cap);
    auto rep = [&](const char *name, double ms, u64 n) { printf("%-78s %8.3f ms\n", name, ms * 1e9 / (double)n); fflush(stdout); };
    const u32 *W = reinterpret_cast<const u32 *>(inP);
    for (int round = 0; round < 3; round++) {
        rep("pieces (a) 8 B hist, wavefront per piece, T=512 (today)", time_ms([&] { hipLaunchKernelGGL((k_hist_pieces<512, true>), dim3(units2), dim3(512), 0, 0, inP, cap, mean, spread, 8, hist); }), ntup);
        rep("(a) 4 B hist, blocked planes (every other line), 16 B loads, T=512", time_ms([&] { hipLaunchKernelGGL((k_hist_planes<512, true>), dim3(units2), dim3(512), 0, 0, W, cap, mean, spread, 8, hist); }), ntup);
        rep("(a) 4 B hist, blocked planes (every other line), 16 B loads, T=1024", time_ms([&] { hipLaunchKernelGGL((k_hist_planes<1024, true>), dim3(units2), dim3(1024), 0, 0, W, cap, mean, spread, 8, hist); }), ntup);
        rep("(b) 4 B hist, separate low-word array (dense), 16 B loads, T=512", time_ms([&] { hipLaunchKernelGGL((k_hist_planes<512, false>), dim3(units2), dim3(512), 0, 0, W, cap, mean, spread, 8, hist); }), ntup);
        rep("(b) 4 B hist, separate low-word array (dense), 16 B loads, T=1024", time_ms([&] { hipLaunchKernelGGL((k_hist_planes<1024, false>), dim3(units2), dim3(1024), 0, 0, W, cap, mean, spread, 8, hist); }), ntup);
        rep("pass-1 writes, 256 streams/WG of 256 + 128 B, T=1024 lds=150K (today)", time_ms([&] { hipLaunchKernelGGL((k_stream_planes<1024, 4, 0>), dim3(G1), dim3(1024), 150 << 10, 0, aos, outP, outK, (u64)0, n1, L1); }), n1);
        rep("    the same bytes, payload words in blocked planes", time_ms([&] { hipLaunchKernelGGL((k_stream_planes<1024, 4, 1>), dim3(G1), dim3(1024), 150 << 10, 0, aos, outP, outK, (u64)0, n1, L1); }), n1);
        rep("(c) pass-1 writes, 256 streams/WG of 128 + 128 + 128 B into three arrays", time_ms([&] { hipLaunchKernelGGL((k_stream_planes<1024, 4, 2>), dim3(G1), dim3(1024), 150 << 10, 0, aos, outP, outK, out_slots, n1, L1); }), n1);
        rep("pieces (b) 12 + 12 B, 64 pieces at stride cap, dense tiles, T=1024 lds=150K (today)", time_ms([&] { hipLaunchKernelGGL((k_pass2_pieces<1024, 4, true>), dim3(units2), dim3(1024), 150 << 10, 0, inP, inK, outP, outK, cap, mean, spread, cpud, (u64)0); }), ntup);
        rep("(d) the same, payloads read through the blocked index", time_ms([&] { hipLaunchKernelGGL((k_pass2_pieces<1024, 4, true, 1>), dim3(units2), dim3(1024), 150 << 10, 0, inP, inK, outP, outK, cap, mean, spread, cpud, (u64)0); }), ntup);
        rep("(d) the same, payloads read from two separate word arrays", time_ms([&] { hipLaunchKernelGGL((k_pass2_pieces<1024, 4, true, 2>), dim3(units2), dim3(1024), 150 << 10, 0, inP, inK, outP, outK, cap, mean, spread, cpud, slots); }), ntup);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "planes")) return run_planes();
    if (argc > 1 && !strcmp(argv[1], "pieces")) return run_pieces();
    const double gib = argc > 1 ? atof(argv[1]) : 14.9;
    const u64 n = (u64)(gib * (1ull << 30) / 16) / 8192 * 8192;
    Tup *in, *out; u64 *sink;
    CK(hipMalloc(&in, n * 16)); CK(hipMalloc(&out, n * 16)); CK(hipMalloc(&sink, 8));
    CK(hipMemset(in, 1, n * 16)); CK(hipMemset(out, 0, n * 16)); CK(hipMemset(sink, 0, 8));
    auto report = [&](const char *name, double ms, double bytes) {
        printf("%-58s %8.3f ms  %7.0f GB/s\n", name, ms, bytes / ms / 1e6); fflush(stdout);
    };
    report("hipMemcpyDtoD", time_ms([&] { CK(hipMemcpyAsync(out, in, n * 16, hipMemcpyDeviceToDevice, 0)); }), 32.0 * n);

#define RUN_COPY(T, P, M, NL, NS, PF, G, LDS)                                                                     \
    {                                                                                                                \
        const u64 L = ((n + (G) - 1) / (G) + (T) * (P) - 1) / ((T) * (P)) * ((T) * (P));                          \
        char nm[128];                                                                                                \
        snprintf(nm, sizeof nm, "copy T=%d tpt=%d %s ntl=%d nts=%d pf=%d G=%d lds=%dK", T, P,                     \
                 M ? "interleaved" : "contiguous", NL, NS, PF, (int)(G), (int)((LDS) >> 10));                      \
        report(nm, time_ms([&] { hipLaunchKernelGGL((k_copy<T, P, M, NL, NS, PF>), dim3(G), dim3(T), LDS, 0, in, out, n, L); }), \
               32.0 * n);                                                                                            \
    }
    // the scatter's shape: 512 threads, 4 x 16 B, 2 WGs/CU (LDS-limited), 2048 units
    RUN_COPY(512, 4, 0, false, false, true, 2048, 76 << 10)
    RUN_COPY(512, 4, 0, false, false, true, 512, 76 << 10)
    RUN_COPY(512, 4, 1, false, false, true, 2048, 76 << 10)
    RUN_COPY(512, 4, 1, false, false, true, 512, 76 << 10)
    RUN_COPY(512, 4, 0, true, true, true, 2048, 76 << 10)
    RUN_COPY(512, 4, 1, true, true, true, 2048, 76 << 10)
    RUN_COPY(512, 4, 0, false, true, true, 2048, 76 << 10)
    RUN_COPY(512, 4, 0, true, false, true, 2048, 76 << 10)
    RUN_COPY(512, 4, 0, false, false, false, 2048, 76 << 10)
    RUN_COPY(512, 4, 1, false, false, false, 2048, 76 << 10)
    // occupancy: no LDS cap
    RUN_COPY(512, 4, 0, false, false, true, 2048, 0)
    RUN_COPY(512, 4, 1, false, false, true, 2048, 0)
    RUN_COPY(256, 4, 1, false, false, false, 4096, 0)
    RUN_COPY(256, 1, 1, false, false, false, 8192, 0)
    RUN_COPY(256, 4, 1, true, true, false, 4096, 0)
    RUN_COPY(1024, 4, 0, false, false, true, 2048, 150 << 10)
    RUN_COPY(1024, 4, 1, false, false, true, 2048, 150 << 10)
    RUN_COPY(1024, 2, 0, false, false, true, 2048, 150 << 10)
    RUN_COPY(512, 8, 0, false, false, true, 2048, 76 << 10)
    RUN_COPY(512, 2, 0, false, false, true, 2048, 76 << 10)
    RUN_COPY(256, 4, 0, false, false, true, 2048, 38 << 10)
    RUN_COPY(256, 8, 0, false, false, true, 2048, 38 << 10)

#define RUN_RW(T, P, M, G, LDS)                                                                                   \
    {                                                                                                                \
        const u64 L = ((n + (G) - 1) / (G) + (T) * (P) - 1) / ((T) * (P)) * ((T) * (P));                          \
        char nm[128];                                                                                                \
        snprintf(nm, sizeof nm, "read  T=%d tpt=%d %s G=%d lds=%dK", T, P, M ? "interleaved" : "contiguous", (int)(G), (int)((LDS) >> 10)); \
        report(nm, time_ms([&] { hipLaunchKernelGGL((k_read<T, P, M>), dim3(G), dim3(T), LDS, 0, in, sink, n, L); }), 16.0 * n); \
        snprintf(nm, sizeof nm, "write T=%d tpt=%d %s G=%d lds=%dK", T, P, M ? "interleaved" : "contiguous", (int)(G), (int)((LDS) >> 10)); \
        report(nm, time_ms([&] { hipLaunchKernelGGL((k_write<T, P, M>), dim3(G), dim3(T), LDS, 0, out, n, L); }), 16.0 * n); \
    }
    RUN_RW(512, 4, 0, 2048, 76 << 10)
    RUN_RW(512, 4, 1, 2048, 76 << 10)
    RUN_RW(512, 4, 0, 2048, 0)
    RUN_RW(512, 4, 1, 2048, 0)
    RUN_RW(256, 4, 1, 8192, 0)
    {   // narrow experiments: reuse the two buffers as (P, K) pairs
        u64 *inP = reinterpret_cast<u64 *>(in), *outP = reinterpret_cast<u64 *>(out);
        u32 *inK = reinterpret_cast<u32 *>(inP + n), *outK = reinterpret_cast<u32 *>(outP + n);
        const int G = 2048;
        const u64 L = ((n + G - 1) / G + 2047) / 2048 * 2048;
        auto rep = [&](const char *name, double ms) { printf("%-58s %8.3f ms  %7.2f Gtuples/s\n", name, ms, n / ms / 1e6); fflush(stdout); };
        rep("AoS16 copy T=512 tpt=4 contiguous (reference point)",
            time_ms([&] { hipLaunchKernelGGL((k_copy<512, 4, 0, false, false, true>), dim3(G), dim3(512), 76 << 10, 0, in, out, n, L); }));
        rep("SoA12 copy T=512 tpt=4 single", time_ms([&] { hipLaunchKernelGGL((k_copy_soa<512, 4, false>), dim3(G), dim3(512), 76 << 10, 0, inP, inK, outP, outK, n, L); }));
        rep("SoA12 copy T=512 tpt=8 single", time_ms([&] { hipLaunchKernelGGL((k_copy_soa<512, 8, false>), dim3(G), dim3(512), 76 << 10, 0, inP, inK, outP, outK, n, L); }));
        rep("SoA12 copy T=512 tpt=4 pair", time_ms([&] { hipLaunchKernelGGL((k_copy_soa<512, 4, true>), dim3(G), dim3(512), 76 << 10, 0, inP, inK, outP, outK, n, L); }));
        rep("SoA12 copy T=512 tpt=8 pair", time_ms([&] { hipLaunchKernelGGL((k_copy_soa<512, 8, true>), dim3(G), dim3(512), 76 << 10, 0, inP, inK, outP, outK, n, L); }));
        rep("AoS16 -> scattered 128 B lines", time_ms([&] { hipLaunchKernelGGL((k_scatter_lines<512, 4, false>), dim3(G), dim3(512), 76 << 10, 0, in, out, outP, outK, n, L); }));
        rep("AoS16 -> scattered 64 B + 32 B lines (narrow)", time_ms([&] { hipLaunchKernelGGL((k_scatter_lines<512, 4, true>), dim3(G), dim3(512), 76 << 10, 0, in, out, outP, outK, n, L); }));
#define RUN_SL(NARROW, GR)                                                                                          \
    {                                                                                                                \
        const u64 n2 = n - (64ull << 20), L2 = ((n2 + G - 1) / G + 2047) / 2048 * 2048;                              \
        const u64 top = 256ull * G * ((L2 / GR + 255) / 256) * GR;             /* one past the largest index written */ \
        if (top > n) { fprintf(stderr, "stream test would overrun: %llu > %llu\n", top, n); exit(1); }               \
        rep("AoS16 -> 256 streams/WG, " #NARROW " GR=" #GR, time_ms([&] { hipLaunchKernelGGL((k_stream_lines<512, 4, NARROW, GR>), dim3(G), dim3(512), 76 << 10, 0, in, out, outP, outK, n2, L2); }) * (double)n / (double)n2); \
    }
        rep("AoS16 -> SoA12 linear T=512 tpt=4 lds=76K", time_ms([&] { hipLaunchKernelGGL((k_aos_to_soa<512, 4>), dim3(G), dim3(512), 76 << 10, 0, in, outP, outK, n, L); }));
        rep("AoS16 -> SoA12 linear T=1024 tpt=4 lds=150K", time_ms([&] { hipLaunchKernelGGL((k_aos_to_soa<1024, 4>), dim3(G), dim3(1024), 150 << 10, 0, in, outP, outK, n, L); }));
        rep("AoS16 -> SoA12 linear T=256 tpt=4 lds=0", time_ms([&] { hipLaunchKernelGGL((k_aos_to_soa<256, 4>), dim3(G * 4), dim3(256), 0, 0, in, outP, outK, n, (L + 3) / 4 / 1024 * 1024 + 1024); }));
#define RUN_SLM(T, MODE)                                                                                             \
    {                                                                                                                \
        const u64 n2 = n - (64ull << 20), L2 = ((n2 + G - 1) / G + 4095) / 4096 * 4096;                              \
        const u64 top = 256ull * G * ((L2 / 32 + 255) / 256) * 32;                                                   \
        if (top > n) { fprintf(stderr, "stream test would overrun\n"); exit(1); }                                    \
        rep("AoS16 -> 256 streams/WG narrow GR=32, T=" #T " lds=150K, read " #MODE, time_ms([&] { hipLaunchKernelGGL((k_stream_lines<T, 4, true, 32, MODE>), dim3(G), dim3(T), 150 << 10, 0, in, out, outP, outK, n2, L2); }) * (double)n / (double)n2); \
    }
        RUN_SLM(1024, 0) RUN_SLM(1024, 1) RUN_SLM(1024, 0) RUN_SLM(1024, 1)
        RUN_SL(false, 8) RUN_SL(false, 4) RUN_SL(false, 16) RUN_SL(true, 8) RUN_SL(true, 16) RUN_SL(true, 32)
    }
    return 0;
}
