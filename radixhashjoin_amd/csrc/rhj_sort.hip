// rhj_sort.hip -- the sort entry (include/rhj.h, "sort"): a stable least-significant-digit radix sort of one 64-bit key
// column with rowIDs.  A range probe, then per 8-bit digit three launches ordered on the context's stream -- histogram per unit and
// digit, scan, stable scatter -- the launch shape of the exact-cursor partition passes.  No workgroup ever waits on another.
// Behind it the top-k entries (include/rhj.h, "top-k"): a most-significant-digit radix select on the same sort key, a
// stable compaction, and the sort above over what is left.
#include "rhj_ordered.h"

#include <atomic>

namespace {

constexpr int TILE = SORT_TILE, BINS = 1 << SORT_DIGIT_BITS;
constexpr u32 DMASK = BINS - 1;
constexpr u32 SORT_MAX_UNITS = 2048;             // ~8 units per CU, as PART_TARGET_UNITS ("sort.max_units": fewer)
constexpr int PROBE_THREADS = 256;
constexpr u32 PROBE_MAX_GRID = 2048;
constexpr int HIST_UNROLL = 4;
static_assert(BINS == 256 && BINS <= ST && ST % 64 == 0 && TILE == ST * TPT, "k_sort_scatter's geometry");

// the order transform: key = t(v) - t(min) ascending, t(max) - t(v) descending, t(v) = v ^ bias (bias: 1 << 63 for the int64 view).
// Both are < 2^w, both keep ties, and ascending order of `key` is the order asked for.
struct KeyXf {
    u64 bias, base;
    u32 desc;
    __device__ __forceinline__ u64 fwd(u64 v) const { const u64 t = v ^ bias; return desc ? base - t : t - base; }
    __device__ __forceinline__ u64 inv(u64 k) const { return (desc ? base - k : k + base) ^ bias; }
};

// ---- k_sort_probe: one launch over the column ------------------------------------------------------------------------------------
// The four words: {min, AND, max, OR}, set to {~0, ~0, 0, 0} by two memsets.  MODE 0: out[0] / out[2] = min / max of v ^ bias.
// MODE 1: out[1] / out[3] = AND / OR of the sort keys: a digit in which OR and AND agree is the same in every key, and its pass is
// skipped.  8-byte loads at the caller's stride (1: a column, 2: the payload word of 16-byte tuples); waves reduce, then the
// workgroup, then thread 0 issues its two atomics -- only where a plain load, however stale, says they would still change something:
// the words only ever move one way, and after the first workgroups nearly every one skips both (as k_keys_range).
template <int MODE>
__global__ void __launch_bounds__(PROBE_THREADS)
k_sort_probe(const u64 *__restrict__ keys, u64 stride, u64 n, KeyXf xf, u64 *__restrict__ out)
{
    __shared__ u64 sa[PROBE_THREADS / 64], sb[PROBE_THREADS / 64];
    u64 a = ~0ull, b = 0;                                            // a: min / AND, b: max / OR
    const u64 step = (u64)gridDim.x * PROBE_THREADS;
    for (u64 i0 = (u64)blockIdx.x * PROBE_THREADS + threadIdx.x; i0 < n; i0 += HIST_UNROLL * step) {
        u64 v[HIST_UNROLL];
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            const u64 i = i0 + j * step;
            v[j] = i < n ? keys[i * stride] : 0;
        }
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            if (i0 + j * step >= n) continue;
            if (MODE == 0) {
                const u64 t = v[j] ^ xf.bias;
                a = t < a ? t : a;
                b = t > b ? t : b;
            } else {
                const u64 k = xf.fwd(v[j]);
                a &= k;
                b |= k;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 oa = __shfl_xor(a, off, 64), ob = __shfl_xor(b, off, 64);
        if (MODE == 0) {
            a = oa < a ? oa : a;
            b = ob > b ? ob : b;
        } else {
            a &= oa;
            b |= ob;
        }
    }
    if ((threadIdx.x & 63) == 0) { sa[threadIdx.x >> 6] = a; sb[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < PROBE_THREADS / 64; w++) {
        if (MODE == 0) {
            a = sa[w] < a ? sa[w] : a;
            b = sb[w] > b ? sb[w] : b;
        } else {
            a &= sa[w];
            b |= sb[w];
        }
    }
    unsigned long long *w = (unsigned long long *)out;
    const volatile unsigned long long *seen = w;
    if (MODE == 0) {                                                 // (a workgroup that saw no row holds the identities: no atomic)
        if (a < seen[0]) atomicMin(w + 0, (unsigned long long)a);
        if (b > seen[2]) atomicMax(w + 2, (unsigned long long)b);
    } else {
        if (~a & seen[1]) atomicAnd(w + 1, (unsigned long long)a);
        if (b & ~seen[3]) atomicOr(w + 3, (unsigned long long)b);
    }
}

// ---- k_sort_copy: width 0 -- every key is the same word, so the input order is the sorted order -----------------------------------
__global__ void __launch_bounds__(PROBE_THREADS)
k_sort_copy(const u64 *__restrict__ keys, u64 kstride, const u64 *__restrict__ rows, u64 rstride, u64 n, u64 *__restrict__ okeys,
            u64 okstride, u64 *__restrict__ orows, u64 orstride)
{
    for (u64 i = (u64)blockIdx.x * PROBE_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * PROBE_THREADS) {
        if (okeys) okeys[i * okstride] = keys[i * kstride];
        if (orows) orows[i * orstride] = rows ? rows[i * rstride] : i;
    }
}

// exclusive scan of one value per thread over the workgroup; wsum: NW words of LDS, free again when the call returns
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T *wsum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T wb = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) wb += w < wave ? wsum[w] : (T)0;
    __syncthreads();
    return wb + inc - v;
}

// ---- k_sort_hist: hist[d * U + u] = rows of unit u whose digit is d ---------------------------------------------------------------
// One workgroup per unit (L rows, a multiple of the tile).  Per-wave bins in LDS; a wave whose rows all hold one digit -- a column of
// few values, a digit above the data -- adds its count once instead of queueing 64 atomics on one word.
template <bool FIRST>
__global__ void __launch_bounds__(ST)
k_sort_hist(const u64 *__restrict__ keys, u64 stride, u64 n, u64 L, u32 U, int shift, KeyXf xf, u32 *__restrict__ hist)
{
    __shared__ u32 h[NW * BINS];
    const u32 tid = threadIdx.x, wave = tid >> 6, u = blockIdx.x;
    for (u32 i = tid; i < NW * BINS; i += ST) h[i] = 0;
    __syncthreads();
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    for (u64 i0 = beg; i0 < end; i0 += HIST_UNROLL * ST) {              // HIST_UNROLL independent loads in flight per lane
        u64 v[HIST_UNROLL];
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            const u64 i = i0 + (u64)j * ST + tid;
            v[j] = i < end ? keys[i * stride] : 0;
        }
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            const bool valid = i0 + (u64)j * ST + tid < end;
            const u32 d = (u32)((FIRST ? xf.fwd(v[j]) : v[j]) >> shift) & DMASK;
            const u64 live = __ballot(valid);
            if (live == 0) continue;
            const u32 d0 = __shfl(d, __ffsll((long long)live) - 1, 64);
            if (__ballot(valid && d == d0) == live) {
                if (valid && (u32)__builtin_amdgcn_mbcnt_hi((u32)(live >> 32), __builtin_amdgcn_mbcnt_lo((u32)live, 0)) == 0)
                    atomicAdd(&h[wave * BINS + d0], (u32)__popcll(live));
            } else if (valid) {
                atomicAdd(&h[wave * BINS + d], 1u);
            }
        }
    }
    __syncthreads();
    if (tid < BINS) {
        u32 s = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) s += h[w * BINS + tid];
        hist[(u64)tid * U + u] = s;
    }
}

// ---- k_sort_scan: per digit, the exclusive prefix of its unit counts, and its total -----------------------------------------------
// Workgroup d scans row d of the table; the prefix over the digits' totals is 256 words and every scatter workgroup does it itself.
__global__ void __launch_bounds__(ST)
k_sort_scan(const u32 *__restrict__ hist, u32 U, u64 *__restrict__ rel, u64 *__restrict__ total)
{
    __shared__ u64 wsum[NW];
    __shared__ u64 last;
    const u32 tid = threadIdx.x, d = blockIdx.x;
    const u32 per = (U + ST - 1) / ST;
    const u64 row = (u64)d * U;
    const u32 beg = tid * per < U ? tid * per : U, end = beg + per < U ? beg + per : U;
    u64 s = 0;
    for (u32 u = beg; u < end; u++) s += hist[row + u];
    u64 off = block_excl_scan<u64>(s, wsum);
    if (tid == ST - 1) last = off + s;
    for (u32 u = beg; u < end; u++) {
        rel[row + u] = off;
        off += hist[row + u];
    }
    __syncthreads();
    if (tid == 0) total[d] = last;
}

// ---- k_sort_scatter<FORM, FIRST, LAST>: the stable scatter of one pass -------------------------------------------------------------
// FORM 0: keys only; 1: narrow -- positions carried as 4 bytes between passes, implicit in the first pass, widened in the last;
// 2: wide -- 8-byte rows, explicit or (in_rows null, first pass) implicit.  FIRST: the keys are the caller's words at in_kstride and
// get the order transform; LAST: the outputs are the caller's, the key words restored, at out_kstride / out_rstride.
//
// One workgroup per unit, tile by tile.  Wave w of a tile owns rows [w * 64 * TPT, (w + 1) * 64 * TPT) of it, lane l of round r the
// row w * 64 * TPT + r * 64 + l: input order is (wave, round, lane).  Rank of a row among the rows of its digit:
//   in its round -- the lanes below it that match all eight digit bits (one ballot per bit, mbcnt under the match mask);
//   in its wave -- plus the wave's running count of the digit, a wave-private LDS word that the first matching lane advances
//                  after all matching lanes have read it (one wave: the LDS executes its accesses in program order);
//   in its tile -- plus the counts of the waves before it (a prefix over NW words per digit, thread d's);
//   in its unit -- the digit's running cursor, advanced by the tile's count after the tile;
//   in the pass -- the cursor starts at (rows of smaller digits) + (rows of this digit in earlier units): the scan's table.
// Every term counts rows that come earlier in the input, so equal digits keep their input order.
// The ranked tile is laid out in LDS by (digit, rank) and stored from there: consecutive lanes store consecutive words of a run, so
// a run is written as whole lines except for its two ends.
struct SortPass {
    const u64 *in_keys;
    u64 in_kstride;
    const void *in_rows;
    u64 in_rstride;
    u64 *out_keys;
    u64 out_kstride;
    void *out_rows;
    u64 out_rstride;
    u64 n, L;
    u32 U;
    int shift;
    KeyXf xf;
    const u64 *rel, *total;
};

template <int FORM> struct RowWord { typedef u64 type; };
template <> struct RowWord<1> { typedef u32 type; };

constexpr size_t sort_lds_bytes(int form)
{
    return (size_t)8 * (TILE + BINS + NW) + (size_t)4 * (NW * BINS + 2 * BINS + NW) + (size_t)(form == 0 ? 0 : form == 1 ? 4 : 8) * TILE;
}
static_assert(2 * sort_lds_bytes(2) <= 160 * 1024 && (4 * (NW * BINS + 2 * BINS + NW)) % 8 == 0, "two scatter workgroups per CU");

template <int FORM, bool FIRST, bool LAST>
__global__ void __launch_bounds__(ST)
k_sort_scatter(SortPass a)
{
    typedef typename RowWord<FORM>::type RowT;
    extern __shared__ __align__(16) unsigned char sort_lds[];
    u64 *skey = (u64 *)sort_lds;                 // TILE: the ranked tile
    u64 *cur = skey + TILE;                      // BINS: the unit's digit cursors
    u64 *wsum64 = cur + BINS;                    // NW
    u32 *wcnt = (u32 *)(wsum64 + NW);            // NW x BINS: per-wave digit counts, then the prefix over the waves
    u32 *tot = wcnt + NW * BINS;                 // BINS: the tile's digit counts
    u32 *lstart = tot + BINS;                    // BINS: ... and their prefix
    u32 *wsum32 = lstart + BINS;                 // NW
    RowT *srow = (RowT *)(wsum32 + NW);          // TILE (FORM != 0)

    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const int shift = a.shift;
    {
        const u64 t = tid < BINS ? a.total[tid] : 0;
        const u64 ds = block_excl_scan<u64>(t, wsum64);
        if (tid < BINS) cur[tid] = ds + a.rel[(u64)tid * a.U + u];
    }
    __syncthreads();
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    volatile u32 *wc = wcnt + wave * BINS;
    for (u64 tb = beg; tb < end; tb += TILE) {
        const u32 tn = end - tb < (u64)TILE ? (u32)(end - tb) : (u32)TILE;
#pragma unroll
        for (int j = 0; j < BINS / 64; j++) wc[lane + 64 * j] = 0;
        u64 key[TPT];
        RowT row[TPT];
        u32 rk[TPT];
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            const u64 gi = tb + li;
            key[r] = 0;
            row[r] = 0;
            if (li < tn) {
                const u64 v = a.in_keys[gi * a.in_kstride];
                key[r] = FIRST ? a.xf.fwd(v) : v;
                if (FORM != 0) {
                    if (FIRST) row[r] = (RowT)(a.in_rows ? ((const u64 *)a.in_rows)[gi * a.in_rstride] : gi);
                    else row[r] = ((const RowT *)a.in_rows)[gi];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const bool valid = wave * (64 * TPT) + r * 64 + lane < tn;
            const u32 d = (u32)(key[r] >> shift) & DMASK;
            u64 m = __ballot(valid);
#pragma unroll
            for (int b = 0; b < SORT_DIGIT_BITS; b++) {
                const bool bit = (d >> b) & 1;
                const u64 bb = __ballot(bit);
                m &= bit ? bb : ~bb;
            }
            const u32 below = (u32)__builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0));
            const u32 old = valid ? wc[d] : 0;
            rk[r] = old + below;
            __builtin_amdgcn_wave_barrier();
            if (valid && below == 0) wc[d] = old + (u32)__popcll(m);
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        u32 s = 0;
        if (tid < BINS) {
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const u32 c = wcnt[w * BINS + tid];
                wcnt[w * BINS + tid] = s;
                s += c;
            }
            tot[tid] = s;
        }
        const u32 ls = block_excl_scan<u32>(s, wsum32);
        if (tid < BINS) lstart[tid] = ls;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            if (wave * (64 * TPT) + r * 64 + lane < tn) {
                const u32 d = (u32)(key[r] >> shift) & DMASK;
                const u32 p = lstart[d] + wcnt[wave * BINS + d] + rk[r];
                if (p < (u32)TILE) {                                  // (always: the ranks of a tile are a permutation of its slots)
                    skey[p] = key[r];
                    if (FORM != 0) srow[p] = row[r];
                }
            }
        }
        __syncthreads();
        for (u32 p = tid; p < tn; p += ST) {
            const u64 k = skey[p];
            const u32 d = (u32)(k >> shift) & DMASK;
            const u64 g = cur[d] + (p - lstart[d]);
            if (g >= a.n) continue;                                   // (never, with the histogram of the same rows: nothing is stored out of bounds)
            if (!LAST || a.out_keys) a.out_keys[g * a.out_kstride] = LAST ? a.xf.inv(k) : k;
            if (FORM != 0) {
                if (LAST) ((u64 *)a.out_rows)[g * a.out_rstride] = (u64)srow[p];
                else ((RowT *)a.out_rows)[g] = srow[p];
            }
        }
        __syncthreads();
        if (tid < BINS) cur[tid] += tot[tid];
    }
}

u32 bits_of(u64 x) { u32 b = 0; while (x) { b++; x >>= 1; } return b; }          // 64 - clz(x), 0 for 0

unsigned probe_grid(u64 n)
{
    u64 g = (n + PROBE_THREADS - 1) / PROBE_THREADS;
    if (g > PROBE_MAX_GRID) g = PROBE_MAX_GRID;
    return (unsigned)(g ? g : 1);
}

// the scatter of one pass; the kernel's LDS size is allowed once per instantiation and device
template <int FORM, bool FIRST, bool LAST>
hipError_t launch_scatter_t(hipStream_t st, const SortPass &a)
{
    static std::atomic<bool> allowed[64];        // (zero-initialised; setting the attribute twice is harmless, a torn flag is not)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!allowed[dev].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sort_scatter<FORM, FIRST, LAST>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds_bytes(FORM));
        if (e != hipSuccess) return e;
        allowed[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL((k_sort_scatter<FORM, FIRST, LAST>), dim3(a.U), dim3(ST), sort_lds_bytes(FORM), st, a);
    return hipSuccess;
}

template <int FORM>
hipError_t launch_scatter_f(hipStream_t st, const SortPass &a, bool first, bool last)
{
    if (first) return last ? launch_scatter_t<FORM, true, true>(st, a) : launch_scatter_t<FORM, true, false>(st, a);
    return last ? launch_scatter_t<FORM, false, true>(st, a) : launch_scatter_t<FORM, false, false>(st, a);
}

hipError_t launch_scatter(hipStream_t st, int form, const SortPass &a, bool first, bool last)
{
    return form == 0 ? launch_scatter_f<0>(st, a, first, last) : form == 1 ? launch_scatter_f<1>(st, a, first, last) : launch_scatter_f<2>(st, a, first, last);
}

// the range probe, one launch and one 32-byte read-back: h_w[0] / h_w[2] = the minimum / maximum of v ^ bias over the column
int probe_range(rhj_ctx *ctx, hipStream_t st, const std::string &me, const u64 *keys, u64 kstride, u64 n, const KeyXf &xf, u64 *d_w, u64 *h_w)
{
    int rc;
    hipError_t e = hipMemsetAsync(d_w, 0xFF, 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_w + 2, 0, 16, st);
    if (e != hipSuccess) return hip_fail(ctx, (me + ": probe words").c_str(), e);
    if ((rc = launch(ctx, RHJ_K_AUX, "k_sort_probe", k_sort_probe<0>, probe_grid(n), PROBE_THREADS, st, keys, kstride, n, xf, d_w)) != RHJ_OK) return rc;
    e = hipMemcpyAsync(h_w, d_w, 4 * sizeof(u64), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(ctx, "k_sort_probe", e);
    return RHJ_OK;
}

// units: L rows each, a whole number of tiles, at most "sort.max_units" of them
void sort_units(rhj_ctx *ctx, u64 n, u64 *L, u32 *U)
{
    const int want_units = rhj_internal_sort_max_units(ctx);
    const u64 max_units = want_units >= 1 && (u32)want_units <= SORT_MAX_UNITS ? (u64)want_units : SORT_MAX_UNITS;
    const u64 tiles = (n + TILE - 1) / TILE, tpu = (tiles + max_units - 1) / max_units;
    *L = tpu * TILE;
    *U = (u32)((n + *L - 1) / *L);
}

// the sort proper.  keys / rows / okeys / orows at strides of 1 (columns) or 2 (the words of 16-byte tuples), in words.
int sort_run(rhj_ctx *ctx, const char *who, const u64 *keys, u64 kstride, const u64 *rows, u64 rstride, u64 n, u32 flags, u64 *okeys,
             u64 okstride, u64 *orows, u64 orstride)
{
    const std::string me(who);
    if (flags & ~(RHJ_SORT_I64 | RHJ_SORT_DESC)) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": unknown flags").c_str());
    if (n == 0) return RHJ_OK;
    if (!keys) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": null keys with a non-zero row count").c_str());
    if (!okeys && !orows) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": both outputs are null").c_str());
    hipStream_t st = rhj_internal_stream(ctx);
    hipError_t e;
    int rc;
    KeyXf xf;
    xf.bias = (flags & RHJ_SORT_I64) ? BIAS : 0;
    xf.base = 0;
    xf.desc = (flags & RHJ_SORT_DESC) ? 1 : 0;

    // 1. the probe: minimum and maximum in the view, one launch
    u64 *d_w = (u64 *)rhj_internal_counters(ctx);
    if (!d_w) return RHJ_E_NOMEM;
    u64 h_w[4];
    if ((rc = probe_range(ctx, st, me, keys, kstride, n, xf, d_w, h_w)) != RHJ_OK) return rc;
    const u32 w = bits_of(h_w[2] - h_w[0]);
    xf.base = xf.desc ? h_w[2] : h_w[0];

    // 2. width 0: the outputs are copies
    if (w == 0) {
        if ((rc = launch(ctx, RHJ_K_AUX, "k_sort_copy", k_sort_copy, probe_grid(n), PROBE_THREADS, st, keys, kstride, rows, rstride, n, okeys, okstride, orows,
                         orstride)) != RHJ_OK)
            return rc;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_sort_copy", e);
        rhj_internal_sort_report(ctx, 0, 0, 0);
        return RHJ_OK;
    }

    // 3. the passes: every digit below the width in which the keys differ
    int shifts[64 / SORT_DIGIT_BITS], np = 0;
    if (w <= SORT_DIGIT_BITS) {
        shifts[np++] = 0;
    } else {
        if ((rc = launch(ctx, RHJ_K_AUX, "k_sort_probe", k_sort_probe<1>, probe_grid(n), PROBE_THREADS, st, keys, kstride, n, xf, d_w)) != RHJ_OK) return rc;
        e = hipMemcpyAsync(h_w, d_w, sizeof h_w, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(ctx, "k_sort_probe", e);
        const u64 differ = h_w[1] ^ h_w[3];
        for (int s = 0; s < (int)w; s += SORT_DIGIT_BITS)
            if ((differ >> s) & DMASK) shifts[np++] = s;
        if (np == 0) shifts[np++] = 0;                                    // (unreachable: max != min, so some bit differs)
    }

    // 4. geometry, tables, ping-pong buffers
    const int form = !orows ? 0 : (!rows && n <= (1ull << 32)) ? 1 : 2;
    u64 L;
    u32 U;
    sort_units(ctx, n, &L, &U);
    const size_t rowb = form == 0 ? 0 : form == 1 ? 4 : 8;
    const size_t hist_b = up256((size_t)U * BINS * 4), rel_b = up256((size_t)U * BINS * 8), tot_b = up256((size_t)BINS * 8);
    const size_t kb = up256((size_t)n * 8), rb = up256((size_t)n * rowb);
    // set 0 always lives in the workspace; set 1 is the caller's outputs where they are plain arrays, else the workspace too
    const bool need0 = np >= 2, need1 = np >= 3;
    const bool k1_ws = need1 && !(okeys && okstride == 1), r1_ws = need1 && form != 0 && !(orows && orstride == 1);
    const size_t bytes = hist_b + rel_b + tot_b + (need0 ? kb + rb : 0) + (k1_ws ? kb : 0) + (r1_ws ? rb : 0);
    void *ws = nullptr;
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_SORT, bytes, &ws)) != RHJ_OK) return rc;
    unsigned char *p = (unsigned char *)ws;
    u32 *d_hist = (u32 *)p; p += hist_b;
    u64 *d_rel = (u64 *)p; p += rel_b;
    u64 *d_tot = (u64 *)p; p += tot_b;
    u64 *tk[2] = {nullptr, nullptr};
    void *tr[2] = {nullptr, nullptr};
    if (need0) { tk[0] = (u64 *)p; p += kb; tr[0] = p; p += rb; }
    if (need1) {
        if (k1_ws) { tk[1] = (u64 *)p; p += kb; } else tk[1] = okeys;
        if (r1_ws) { tr[1] = p; p += rb; } else tr[1] = orows;
    }

    for (int i = 0; i < np; i++) {
        const bool first = i == 0, last = i == np - 1;
        SortPass a = {};
        a.n = n; a.L = L; a.U = U; a.shift = shifts[i]; a.xf = xf; a.rel = d_rel; a.total = d_tot;
        if (first) { a.in_keys = keys; a.in_kstride = kstride; a.in_rows = rows; a.in_rstride = rstride; }
        else { const int src = (np - 1 - i) & 1; a.in_keys = tk[src]; a.in_kstride = 1; a.in_rows = tr[src]; a.in_rstride = 1; }
        if (last) { a.out_keys = okeys; a.out_kstride = okstride; a.out_rows = orows; a.out_rstride = orstride; }
        else { const int dst = (np - 2 - i) & 1; a.out_keys = tk[dst]; a.out_kstride = 1; a.out_rows = tr[dst]; a.out_rstride = 1; }
        rc = first ? launch(ctx, RHJ_K_HIST, "k_sort_hist", k_sort_hist<true>, U, ST, st, a.in_keys, a.in_kstride, n, L, U, a.shift, xf, d_hist)
                   : launch(ctx, RHJ_K_HIST, "k_sort_hist", k_sort_hist<false>, U, ST, st, a.in_keys, a.in_kstride, n, L, U, a.shift, xf, d_hist);
        if (rc != RHJ_OK) return rc;
        if ((rc = launch(ctx, RHJ_K_SCAN, "k_sort_scan", k_sort_scan, BINS, ST, st, d_hist, U, d_rel, d_tot)) != RHJ_OK) return rc;
        {
            Span s(ctx, RHJ_K_SCATTER);
            e = launch_scatter(st, form, a, first, last);
        }
        if (e != hipSuccess) return hip_fail(ctx, "k_sort_scatter: dynamic LDS", e);
        if ((rc = check(ctx, "k_sort_scatter")) != RHJ_OK) return rc;
    }
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_sort_scatter", e);
    rhj_internal_sort_report(ctx, (int)w, np, (int)U);
    return RHJ_OK;
}

// ==== top-k and k-th value (include/rhj.h, "top-k") =====================================================================
// A most-significant-digit radix select on the sort key, a stable in-order compaction of what survives, and sort_run over that.
// The select state, four device words: {P, r, M, c} -- P the threshold's digits found so far (the bits below them 0), r the wanted
// rank among the rows whose upper digits equal P's (the candidates), M the rows whose upper digits are smaller (sure to be in the
// result), c the candidates.  The host reads the state after each digit; the next histogram reads it from the device.
constexpr int TS_PREFIX = 0, TS_RANK = 1, TS_SURE = 2, TS_CAND = 3, TS_WORDS = 4;

// ---- k_topk_hist: ghist[d] += candidates of unit u whose digit at `shift` is d -----------------------------------------------------
// k_sort_hist's shape -- units, per-wave LDS bins, HIST_UNROLL loads in flight, the one-digit-wave shortcut -- over the rows whose
// digits above `shift` equal the threshold's.  A wave in which no lane is a candidate touches no LDS, and a workgroup without one
// adds nothing: after the first digit that is nearly all of them.  The 256 global words take integer atomics: exact in any order.
__global__ void __launch_bounds__(ST)
k_topk_hist(const u64 *__restrict__ keys, u64 stride, u64 n, u64 L, int shift, KeyXf xf, const u64 *__restrict__ state,
            unsigned long long *__restrict__ ghist)
{
    __shared__ u32 h[NW * BINS];
    const u32 tid = threadIdx.x, wave = tid >> 6, u = blockIdx.x;
    for (u32 i = tid; i < NW * BINS; i += ST) h[i] = 0;
    __syncthreads();
    const int up = shift + SORT_DIGIT_BITS;
    const bool all = up >= 64;                                          // the top digit of a 57 .. 64 bit key: no digit above it
    const u64 want = all ? 0 : state[TS_PREFIX] >> (up & 63);
    int used = 0;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    for (u64 i0 = beg; i0 < end; i0 += HIST_UNROLL * ST) {
        u64 v[HIST_UNROLL];
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            const u64 i = i0 + (u64)j * ST + tid;
            v[j] = i < end ? keys[i * stride] : 0;
        }
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            const u64 key = xf.fwd(v[j]);
            const bool hit = i0 + (u64)j * ST + tid < end && (all || (key >> (up & 63)) == want);
            const u32 d = (u32)(key >> shift) & DMASK;
            const u64 live = __ballot(hit);
            if (live == 0) continue;
            used = 1;
            const u32 d0 = __shfl(d, __ffsll((long long)live) - 1, 64);
            if (__ballot(hit && d == d0) == live) {
                if (hit && (u32)__builtin_amdgcn_mbcnt_hi((u32)(live >> 32), __builtin_amdgcn_mbcnt_lo((u32)live, 0)) == 0)
                    atomicAdd(&h[wave * BINS + d0], (u32)__popcll(live));
            } else if (hit) {
                atomicAdd(&h[wave * BINS + d], 1u);
            }
        }
    }
    if (!__syncthreads_or(used)) return;
    if (tid < BINS) {
        u32 s = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) s += h[w * BINS + tid];
        if (s) atomicAdd(&ghist[tid], (unsigned long long)s);
    }
}

// ---- k_topk_pick: one workgroup -- the digit in which the wanted rank falls ---------------------------------------------------------
// Extends P by that digit, takes the candidates of smaller digits off r and adds them to M, sets c to the digit's count; zeroes
// the histogram for the next digit.
__global__ void __launch_bounds__(ST)
k_topk_pick(unsigned long long *__restrict__ ghist, u64 *__restrict__ state, int shift)
{
    __shared__ u64 wsum[NW];
    const u32 tid = threadIdx.x;
    const u64 t = tid < BINS ? ghist[tid] : 0;
    const u64 rank = state[TS_RANK], sure = state[TS_SURE], prefix = state[TS_PREFIX];
    const u64 below = block_excl_scan<u64>(t, wsum);                    // (its barriers stand between the loads above and the stores below)
    if (tid >= BINS) return;
    ghist[tid] = 0;
    if (below <= rank && rank < below + t) {                            // exactly one digit while r < c
        state[TS_PREFIX] = prefix | ((u64)tid << shift);
        state[TS_RANK] = rank - below;
        state[TS_SURE] = sure + below;
        state[TS_CAND] = t;
    }
}

// What count and compact keep.  A row is SURE when fwd(key) >> shift is below `want`, a CANDIDATE when equal.  Kept: the sure rows
// (keep_sure) and the candidates whose index among the candidates, in input order, is in [lo, hi).
struct TopkKeep {
    const u64 *keys;
    u64 kstride, n, L;
    u32 U;
    int shift;
    KeyXf xf;
    u64 want;
    u32 keep_sure;
    u64 lo, hi;
};

// ---- k_topk_count: cnt[0 * U + u] / cnt[1 * U + u] = the sure rows / the candidates of unit u ----------------------------------------
__global__ void __launch_bounds__(ST)
k_topk_count(TopkKeep a, u32 *__restrict__ cnt)
{
    __shared__ u32 ws[NW], wc[NW];
    const u32 tid = threadIdx.x, u = blockIdx.x;
    u32 ns = 0, nc = 0;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    for (u64 i0 = beg; i0 < end; i0 += HIST_UNROLL * ST) {
        u64 v[HIST_UNROLL];
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            const u64 i = i0 + (u64)j * ST + tid;
            v[j] = i < end ? a.keys[i * a.kstride] : 0;
        }
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) {
            const bool valid = i0 + (u64)j * ST + tid < end;
            const u64 p = a.xf.fwd(v[j]) >> a.shift;
            ns += valid && p < a.want;
            nc += valid && p == a.want;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ns += __shfl_xor(ns, off, 64);
        nc += __shfl_xor(nc, off, 64);
    }
    if ((tid & 63) == 0) { ws[tid >> 6] = ns; wc[tid >> 6] = nc; }
    __syncthreads();
    if (tid != 0) return;
    u32 s = 0, c = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) { s += ws[w]; c += wc[w]; }
    cnt[u] = s;
    cnt[(u64)a.U + u] = c;
}

// ---- k_topk_compact: the kept rows, key words and 64-bit rows, in INPUT ORDER --------------------------------------------------------
// One workgroup per unit, tile by tile, in the scatter's row order (wave, round, lane).  The position of a kept row is the number of
// kept rows before it in the input, and that follows from two counts: the sure rows before it, and the candidates before it --
//   in its round -- the lanes below it in the ballot of the class (mbcnt);
//   in its wave  -- plus the wave's count over the earlier rounds (a wave-uniform register);
//   in its tile  -- plus the counts of the waves before it (a prefix over NW words);
//   in its unit  -- plus the running cursors, advanced by the tile's counts after the tile;
//   in the call  -- the cursors start at the counts of the earlier units: the scan's table.
// Of x candidates before a row, min(max(x, lo), hi) - lo are kept.  No position comes from an atomic.
__global__ void __launch_bounds__(ST)
k_topk_compact(TopkKeep a, const u64 *__restrict__ rows, u64 rstride, const u64 *__restrict__ rel, u64 *__restrict__ okeys,
               u64 *__restrict__ orows, u64 cap)
{
    __shared__ u32 ws[NW], wc[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    u64 s0 = rel[u], c0 = rel[(u64)a.U + u];
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    for (u64 tb = beg; tb < end; tb += TILE) {
        const u32 tn = end - tb < (u64)TILE ? (u32)(end - tb) : (u32)TILE;
        u64 v[TPT];
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            v[r] = li < tn ? a.keys[(tb + li) * a.kstride] : 0;
        }
        u32 sb[TPT], cb[TPT], sure = 0, cand = 0, ns = 0, nc = 0;       // sure / cand: one bit per round
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const bool valid = wave * (64 * TPT) + r * 64 + lane < tn;
            const u64 p = a.xf.fwd(v[r]) >> a.shift;
            const bool is_s = valid && p < a.want, is_c = valid && p == a.want;
            const u64 bs = __ballot(is_s), bc = __ballot(is_c);
            sb[r] = ns + (u32)__builtin_amdgcn_mbcnt_hi((u32)(bs >> 32), __builtin_amdgcn_mbcnt_lo((u32)bs, 0));
            cb[r] = nc + (u32)__builtin_amdgcn_mbcnt_hi((u32)(bc >> 32), __builtin_amdgcn_mbcnt_lo((u32)bc, 0));
            ns += (u32)__popcll(bs);
            nc += (u32)__popcll(bc);
            sure |= (u32)is_s << r;
            cand |= (u32)is_c << r;
        }
        if (lane == 0) { ws[wave] = ns; wc[wave] = nc; }
        __syncthreads();
        u32 ps = 0, pc = 0, ts = 0, tc = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const u32 x = ws[w], y = wc[w];
            ps += (u32)w < wave ? x : 0;
            pc += (u32)w < wave ? y : 0;
            ts += x;
            tc += y;
        }
        if (ts + tc != 0) {
#pragma unroll
            for (int r = 0; r < TPT; r++) {
                if (!((sure | cand) >> r & 1)) continue;
                const u64 sbefore = a.keep_sure ? s0 + ps + sb[r] : 0, cbefore = c0 + pc + cb[r];
                const u64 ckept = (cbefore < a.lo ? a.lo : cbefore > a.hi ? a.hi : cbefore) - a.lo;
                const bool keep = (sure >> r & 1) ? a.keep_sure != 0 : (cbefore >= a.lo && cbefore < a.hi);
                const u64 g = sbefore + ckept;
                if (!keep || g >= cap) continue;                          // (g < cap always: cap is the count of kept rows)
                const u64 gi = tb + wave * (64 * TPT) + r * 64 + lane;
                okeys[g] = v[r];
                if (orows) orows[g] = rows ? rows[gi * rstride] : gi;
            }
        }
        s0 += ts;
        c0 += tc;
        __syncthreads();
    }
}

int read_words(rhj_ctx *ctx, hipStream_t st, const char *what, u64 *dst, const u64 *d_src, int words)
{
    hipError_t e = hipMemcpyAsync(dst, d_src, (size_t)words * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? RHJ_OK : hip_fail(ctx, what, e);
}

// the k-th tuple: its key word from d_key, its row word from d_row (null: the row is `implicit`)
int read_kth(rhj_ctx *ctx, hipStream_t st, const u64 *d_key, const u64 *d_row, u64 implicit, u64 *out_kth)
{
    hipError_t e = hipMemcpyAsync(out_kth, d_key, 8, hipMemcpyDeviceToHost, st);
    if (d_row) { if (e == hipSuccess) e = hipMemcpyAsync(out_kth + 1, d_row, 8, hipMemcpyDeviceToHost, st); }
    else out_kth[1] = implicit;
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? RHJ_OK : hip_fail(ctx, "the k-th tuple", e);
}

int topk_run(rhj_ctx *ctx, const char *who, const u64 *keys, u64 kstride, const u64 *rows, u64 rstride, u64 n, u64 k, u32 flags,
             u64 *okeys, u64 okstride, u64 *orows, u64 orstride, u64 *out_kth)
{
    const std::string me(who);
    if (flags & ~(RHJ_SORT_I64 | RHJ_SORT_DESC)) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": unknown flags").c_str());
    if (n == 0 || k == 0) return RHJ_OK;
    if (!keys) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": null keys with a non-zero row count").c_str());
    if (!okeys && !orows && !out_kth) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": both outputs and out_kth are null").c_str());
    hipStream_t st = rhj_internal_stream(ctx);
    hipError_t e;
    int rc;
    const u64 m = k < n ? k : n;
    const bool pure = !okeys && !orows;
    const bool both = okeys && orows;

    // k >= n: the sort (the k-th tuple can be read from its outputs when both are there; otherwise the selection below finds it)
    if (k >= n && !pure && (!out_kth || both)) {
        if ((rc = sort_run(ctx, who, keys, kstride, rows, rstride, n, flags, okeys, okstride, orows, orstride)) != RHJ_OK) return rc;
        return out_kth ? read_kth(ctx, st, okeys + (n - 1) * okstride, orows + (n - 1) * orstride, 0, out_kth) : RHJ_OK;
    }

    // 1. the sort's probe
    KeyXf xf;
    xf.bias = (flags & RHJ_SORT_I64) ? BIAS : 0;
    xf.base = 0;
    xf.desc = (flags & RHJ_SORT_DESC) ? 1 : 0;
    u64 *d_w = (u64 *)rhj_internal_counters(ctx);
    if (!d_w) return RHJ_E_NOMEM;
    u64 h_w[4];
    if ((rc = probe_range(ctx, st, me, keys, kstride, n, xf, d_w, h_w)) != RHJ_OK) return rc;
    const u32 w = bits_of(h_w[2] - h_w[0]);
    xf.base = xf.desc ? h_w[2] : h_w[0];

    // width 0: every key is the same word, the first m rows of the input are the answer
    if (w == 0) {
        if (!pure) {
            if ((rc = launch(ctx, RHJ_K_AUX, "k_sort_copy", k_sort_copy, probe_grid(m), PROBE_THREADS, st, keys, kstride, rows, rstride, m, okeys, okstride,
                             orows, orstride)) != RHJ_OK)
                return rc;
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_sort_copy", e);
        }
        rhj_internal_topk_report(ctx, 0, 0, n, 0);
        return out_kth ? read_kth(ctx, st, keys + (m - 1) * kstride, rows ? rows + (m - 1) * rstride : nullptr, m - 1, out_kth) : RHJ_OK;
    }

    // 2. select: from the top digit of w downward, until few enough candidates are left or the digits are
    const int64_t opt = rhj_internal_topk_max_candidates(ctx);
    const u64 max_cand = opt >= 1 ? (u64)opt : (m > (u64)TOPK_AUTO_CANDIDATES ? m : (u64)TOPK_AUTO_CANDIDATES);
    u64 L;
    u32 U;
    sort_units(ctx, n, &L, &U);
    const size_t state_b = 256, ghist_b = up256((size_t)BINS * 8), cnt_b = up256((size_t)U * 2 * 4), rel_b = up256((size_t)U * 2 * 8);
    const size_t head_b = state_b + ghist_b + cnt_b + rel_b + 256;
    u64 sel[TS_WORDS] = {0, m - 1, 0, n};
    int passes = 0, shift = 0;
    if (sel[TS_CAND] > max_cand) {
        void *ws = nullptr;
        if ((rc = rhj_internal_workspace(ctx, RHJ_WS_TOPK, head_b, &ws)) != RHJ_OK) return rc;
        u64 *d_state = (u64 *)ws;
        unsigned long long *d_ghist = (unsigned long long *)((unsigned char *)ws + state_b);
        e = hipMemcpyAsync(d_state, sel, sizeof sel, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_ghist, 0, (size_t)BINS * 8, st);
        if (e != hipSuccess) return hip_fail(ctx, (me + ": select state").c_str(), e);
        for (shift = (int)((w - 1) / SORT_DIGIT_BITS) * SORT_DIGIT_BITS;; shift -= SORT_DIGIT_BITS) {
            if ((rc = launch(ctx, RHJ_K_HIST, "k_topk_hist", k_topk_hist, U, ST, st, keys, kstride, n, L, shift, xf, d_state, d_ghist)) != RHJ_OK) return rc;
            if ((rc = launch(ctx, RHJ_K_SCAN, "k_topk_pick", k_topk_pick, 1, ST, st, d_ghist, d_state, shift)) != RHJ_OK) return rc;
            if ((rc = read_words(ctx, st, "k_topk_pick", sel, d_state, TS_WORDS)) != RHJ_OK) return rc;
            passes++;
            if (sel[TS_CAND] <= max_cand || shift == 0) break;
        }
        if (sel[TS_CAND] == 0 || sel[TS_RANK] >= sel[TS_CAND] || sel[TS_SURE] + sel[TS_RANK] != m - 1)
            return rhj_internal_fail(ctx, RHJ_E_HIP, (me + ": the selection lost its rank").c_str());      // (never: the histogram counts every candidate)
    }
    const bool ran_out = passes > 0 && shift == 0;                       // every candidate holds the threshold key itself
    const u64 M = sel[TS_SURE], r = sel[TS_RANK], c = sel[TS_CAND];

    // 3. keep: the sure rows and the candidates -- when the digits ran out only the first r + 1 of them, in a pure selection no sure
    //    row and of such a run only the candidate of index r
    const bool keep_sure = !pure;
    const u64 lo = ran_out && pure ? r : 0, hi = ran_out ? r + 1 : c;
    const u64 kept = (keep_sure ? M : 0) + (hi - lo);
    const u64 at = pure ? (ran_out ? 0 : r) : m - 1;                     // where the k-th tuple stands among the sorted kept rows
    const bool need_keys = okeys || out_kth, need_rows = orows || out_kth;
    const bool direct = kept == m && !pure && (!out_kth || both);        // the inner sort writes the caller's arrays
    const size_t kb = up256((size_t)kept * 8);
    const u64 *in_k = keys, *in_r = rows;
    u64 in_ks = kstride, in_rs = rstride, *out_k = nullptr, *out_r = nullptr;
    void *ws = nullptr;
    const size_t bytes = head_b + (passes ? kb + (need_rows ? kb : 0) : 0) + (direct ? 0 : (need_keys ? kb : 0) + (need_rows ? kb : 0));
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_TOPK, bytes, &ws)) != RHJ_OK) return rc;
    {
        unsigned char *p = (unsigned char *)ws + state_b + ghist_b;
        u32 *d_cnt = (u32 *)p; p += cnt_b;
        u64 *d_rel = (u64 *)p; p += rel_b;
        u64 *d_tot = (u64 *)p; p += 256;
        if (passes) {
            u64 *kk = (u64 *)p; p += kb;
            u64 *kr = nullptr;
            if (need_rows) { kr = (u64 *)p; p += kb; }
            TopkKeep a = {};
            a.keys = keys; a.kstride = kstride; a.n = n; a.L = L; a.U = U; a.shift = shift; a.xf = xf; a.want = sel[TS_PREFIX] >> shift;
            a.keep_sure = keep_sure; a.lo = lo; a.hi = hi;
            if ((rc = launch(ctx, RHJ_K_HIST, "k_topk_count", k_topk_count, U, ST, st, a, d_cnt)) != RHJ_OK) return rc;
            if ((rc = launch(ctx, RHJ_K_SCAN, "k_sort_scan", k_sort_scan, 2, ST, st, d_cnt, U, d_rel, d_tot)) != RHJ_OK) return rc;
            if ((rc = launch(ctx, RHJ_K_SCATTER, "k_topk_compact", k_topk_compact, U, ST, st, a, rows, rstride, d_rel, kk, kr, kept)) != RHJ_OK) return rc;
            in_k = kk; in_r = kr; in_ks = in_rs = 1;
        }
        if (!direct) {
            if (need_keys) { out_k = (u64 *)p; p += kb; }
            if (need_rows) { out_r = (u64 *)p; p += kb; }
        }
    }

    // 4. order: the sort over the kept rows, then the first m of them
    if (direct) rc = sort_run(ctx, who, in_k, in_ks, in_r, in_rs, kept, flags, okeys, okstride, orows, orstride);
    else rc = sort_run(ctx, who, in_k, in_ks, need_rows ? in_r : nullptr, in_rs, kept, flags, out_k, 1, out_r, 1);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_report(ctx, 0, 0, 0);                              // "last.sort_*" speak of the sort entries only
    rhj_internal_topk_report(ctx, (int)w, passes, c, kept);
    if (!direct && !pure) {
        if ((rc = launch(ctx, RHJ_K_AUX, "k_sort_copy", k_sort_copy, probe_grid(m), PROBE_THREADS, st, out_k, (u64)1, out_r, (u64)1, m, okeys, okstride, orows,
                         orstride)) != RHJ_OK)
            return rc;
        if (!out_kth && (e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_sort_copy", e);
    }
    if (!out_kth) return RHJ_OK;
    if (direct) return read_kth(ctx, st, okeys + at * okstride, orows + at * orstride, 0, out_kth);
    return read_kth(ctx, st, out_k + at, out_r + at, 0, out_kth);
}

}  // namespace

// hooks for rhj_window.hip: the sort proper on plain columns, under the caller's entry name and "last.*", and the unit
// geometry its passes use
int rhj_internal_sort_run(rhj_ctx *ctx, const char *who, const u64 *keys, const u64 *rows, u64 n, u32 flags, u64 *okeys, u64 *orows)
{
    return sort_run(ctx, who, keys, 1, rows, 1, n, flags, okeys, 1, orows, 1);
}
void rhj_internal_sort_units(rhj_ctx *ctx, u64 n, u64 *L, u32 *U) { sort_units(ctx, n, L, U); }

extern "C" {

int rhj_sort_cols_dev(rhj_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_rows, uint64_t n, uint32_t flags,
                      uint64_t *d_out_keys, uint64_t *d_out_rows)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    return sort_run(ctx, "rhj_sort_cols_dev", (const u64 *)d_keys, 1, (const u64 *)d_rows, 1, n, flags, (u64 *)d_out_keys, 1, (u64 *)d_out_rows, 1);
}

int rhj_sort_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t n, uint32_t flags, rhj_tuple *d_out)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    const u64 *in = (const u64 *)d_R;
    u64 *out = (u64 *)d_out;
    // value = .payload (word 1), rowID = .key (word 0)
    return sort_run(ctx, "rhj_sort_dev", in ? in + 1 : nullptr, 2, in, 2, n, flags, out ? out + 1 : nullptr, 2, out, 2);
}

int rhj_topk_cols_dev(rhj_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_rows, uint64_t n, uint64_t k, uint32_t flags,
                      uint64_t *d_out_keys, uint64_t *d_out_rows, uint64_t *out_kth)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    return topk_run(ctx, "rhj_topk_cols_dev", (const u64 *)d_keys, 1, (const u64 *)d_rows, 1, n, k, flags, (u64 *)d_out_keys, 1, (u64 *)d_out_rows, 1,
                    (u64 *)out_kth);
}

int rhj_topk_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t n, uint64_t k, uint32_t flags, rhj_tuple *d_out, uint64_t *out_kth)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    const u64 *in = (const u64 *)d_R;
    u64 *out = (u64 *)d_out;
    return topk_run(ctx, "rhj_topk_dev", in ? in + 1 : nullptr, 2, in, 2, n, k, flags, out ? out + 1 : nullptr, 2, out, 2, (u64 *)out_kth);
}

}  // extern "C"
