// rhj_range.hip -- the range join entries (include/rhj.h, "range join"): for every row of R the rows of S of its
// partition whose `on` word lies in the row's interval, as a CSR result over S in sorted order and as ordered pairs -- JOIN .. ON r.by =
// s.by AND s.t BETWEEN r.lo AND r.hi, the band join, the point-in-interval join.  The lower bounds of R and the `on` words of S are
// concatenated in the workspace and ordered by (by, word, concatenated position) with the stable sort of rhj_sort.hip, as the as-of
// entry does.  In that order the partners of a row of R are the rows of S between its own position p and the first position q whose
// word is past its upper bound: a run of rowsS, the rows of S in sorted order, that starts at srank[p], the number of rows of S
// before p.  What is new here: the rank scan -- a plain exclusive sum on the sort's units, a reduce per unit, a one-workgroup carry,
// an apply per unit --, the galloping search for q, the same scan over the counts in row order, and the expansion of the CSR result
// into pairs, balanced over pairs and not over rows.  No workgroup ever waits on another, and no position, count or value comes from
// an atomic.
#include "rhj_ordered.h"

namespace {

constexpr int TILE = RANGE_TILE;
constexpr int EX_THREADS = 256, EX_SPT = RANGE_EXPAND_TILE / EX_THREADS;   // the expansion: slots per thread
static_assert(TILE == SORT_TILE, "k_rj_apply's geometry is the sort's (rhj_ordered.h)");
static_assert(RANGE_EXPAND_TILE == EX_THREADS * EX_SPT && EX_THREADS >= 128, "k_rj_expand's geometry");

// The concatenation is [first ; second]: [R ; S], under RHJ_RANGE_LO_OPEN [S ; R].  Concatenated index c belongs to R when
// (c < nfirst) == r_first; its row is c or c - nfirst.
// What a scan sums.  RANK: 1 at every sorted position that holds a row of S -- out[p] = srank[p], and rowsS[srank[p]] = the row at
// such a position.  OFFS: cnt[i] in row order -- out[i] = offsets[i], and the last row stores the total behind it.
constexpr int RANK = 0, OFFS = 1;
struct RjScan {
    const u64 *src;                              // RANK: perm, n words by sorted position; OFFS: cnt, n words by row
    u64 *out;                                    // n words (OFFS: n + 1)
    u64 *rows;                                   // RANK: nS words, or null
    u64 n, L, nfirst, nS;
    u32 r_first;
    u64 *usum;                                   // per unit: its sum
    u64 *carry;                                  // per unit: the sum of the units before it
};

template <int MODE>
__device__ __forceinline__ u64 rj_value(const RjScan &a, u64 w)
{
    return MODE == RANK ? (u64)((w < a.nfirst) != (a.r_first != 0)) : w;
}

// ---- k_rj_concat: the order words and, when given, the `by` words of both tables in one column each --------------------------------
// R's word is its lower bound: lo[i], or under RHJ_RANGE_BAND x - below in the view, saturated at the view's minimum, as the word
// whose view it is (bias: 1 << 63 in the int64 view -- the sort's transform, its own inverse).
__global__ void __launch_bounds__(FLAT_THREADS)
k_rj_concat(const u64 *__restrict__ loR, const u64 *__restrict__ onS, const u64 *__restrict__ byR, const u64 *__restrict__ byS, u64 nR, u64 nS,
            u32 r_first, u32 band, u64 bias, u64 below, u64 *__restrict__ con, u64 *__restrict__ cby)
{
    const u64 n = nR + nS, nfirst = r_first ? nR : nS;
    for (u64 c = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; c < n; c += (u64)gridDim.x * FLAT_THREADS) {
        const bool isR = (c < nfirst) == (r_first != 0);
        const u64 row = c < nfirst ? c : c - nfirst;
        u64 w;
        if (isR) {
            w = loR[row];
            if (band) {
                const u64 x = w ^ bias;
                w = (x >= below ? x - below : 0) ^ bias;
            }
        } else {
            w = onS[row];
        }
        con[c] = w;
        if (cby) cby[c] = isR ? byR[row] : byS[row];
    }
}

// ---- k_rj_fill: a[0 .. na) = 0 and b[0 .. nb) = 0 (S is empty: the offsets and the firsts) -------------------------------------------
__global__ void __launch_bounds__(FLAT_THREADS)
k_rj_fill(u64 *__restrict__ a, u64 na, u64 *__restrict__ b, u64 nb)
{
    for (u64 i = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; i < na + nb; i += (u64)gridDim.x * FLAT_THREADS) {
        if (i < na) a[i] = 0;
        else b[i - na] = 0;
    }
}

// ---- k_rj_reduce<MODE>: per unit its sum ---------------------------------------------------------------------------------------------
// One workgroup per unit; the threads stride over the unit, the lanes are summed with shuffles and the waves through LDS.
template <int MODE>
__global__ void __launch_bounds__(ST)
k_rj_reduce(RjScan a)
{
    __shared__ u64 ws[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    u64 s = 0;
    for (u64 p = beg + tid; p < end; p += ST) s += rj_value<MODE>(a, a.src[p]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) ws[wave] = s;
    __syncthreads();
    if (tid != 0) return;
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) t += ws[w];
    a.usum[u] = t;
}

// ---- k_rj_carry: one workgroup -- the exclusive sum of at most 2048 unit sums ---------------------------------------------------------
// Thread t folds its run of ceil(U / 512) consecutive units, the runs are scanned over the workgroup (wave scan, per-wave totals
// through LDS), and the thread walks its run again from its carry-in.
__global__ void __launch_bounds__(ST)
k_rj_carry(const u64 *__restrict__ usum, u32 U, u64 *__restrict__ carry)
{
    __shared__ u64 ws[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 per = (U + ST - 1) / ST;
    const u32 b = tid * per < U ? tid * per : U, e = b + per < U ? b + per : U;
    u64 s = 0;
    for (u32 u = b; u < e; u++) s += usum[u];
    u64 inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up(inc, off, 64);
        if (lane >= (u32)off) inc += o;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    u64 cur = inc - s;
#pragma unroll
    for (int w = 0; w < NW; w++)
        if ((u32)w < wave) cur += ws[w];
    for (u32 u = b; u < e; u++) {
        carry[u] = cur;
        cur += usum[u];
    }
}

// ---- k_rj_apply<MODE>: the scan itself ---------------------------------------------------------------------------------------------
// One workgroup per unit, tile by tile, in the sort's position order (wave, round, lane): wave w of a tile owns positions [w * 64 *
// TPT, (w + 1) * 64 * TPT) of it.  Per round a wave scan continued from the wave's running sum; per tile the waves' totals through
// LDS, added to the tile's carry-in -- the unit's from k_rj_carry, then the running one.
template <int MODE>
__global__ void __launch_bounds__(ST)
k_rj_apply(RjScan a)
{
    __shared__ u64 ws[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    u64 cv = a.carry[u];
    for (u64 tb = beg; tb < end; tb += TILE) {
        const u32 tn = end - tb < (u64)TILE ? (u32)(end - tb) : (u32)TILE;
        u64 w[TPT], x[TPT], v[TPT];
        u64 run = 0;
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            w[r] = 0;
            x[r] = 0;
            if (li < tn) {
                w[r] = a.src[tb + li];
                x[r] = rj_value<MODE>(a, w[r]);
            }
            u64 inc = x[r];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const u64 o = __shfl_up(inc, off, 64);
                if (lane >= (u32)off) inc += o;
            }
            v[r] = run + inc - x[r];                                     // exclusive, inside the wave's part
            run += __shfl(inc, 63, 64);
        }
        if (lane == 0) ws[wave] = run;
        __syncthreads();
        u64 pre = cv, tot = cv;
#pragma unroll
        for (int k = 0; k < NW; k++) {
            if ((u32)k == wave) pre = tot;
            tot += ws[k];
        }
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            if (li >= tn) continue;
            const u64 p = tb + li, ex = pre + v[r];
            a.out[p] = ex;
            if (MODE == RANK) {
                if (x[r] != 0 && a.rows) {
                    const u64 row = w[r] < a.nfirst ? w[r] : w[r] - a.nfirst;
                    if (ex < a.nS && row < a.nS) a.rows[ex] = row;       // (always: the rank of a row of S among the rows of S)
                }
            } else {
                if (p + 1 == a.n) a.out[a.n] = ex + x[r];                // the total behind the last row's offset
            }
        }
        cv = tot;
        __syncthreads();
    }
}

// ---- k_rj_search: first[i] and cnt[i] of every row of R ----------------------------------------------------------------------------
// One thread per sorted position; a position of S has nothing to do.  At a position p of R with row i: hi in the view (gathered, or
// under BAND x + above saturated at the view's maximum), then the first position q of [p, n] at which "the `by` word is p's and the
// word is <= hi (HI_OPEN: < hi)" fails.  Positions are ordered by (by, word), so the test is monotone from p on: gallop in doubling
// steps while it holds, then bisect the bracket -- about 2 log2(q - p) dependent loads.  Every index read lies in [p, n).
struct RjSearch {
    const u64 *perm, *vs, *sp, *srank;           // by sorted position: concatenated index, order word, `by` word (or null), rows of S before it
    const u64 *loR, *hiR;                        // by row of R (BAND: loR holds x, hiR is null)
    u64 *first, *cnt;                            // by row of R
    u64 n, nfirst, nR, nS, bias, above;
    u32 r_first, band, hi_open;
};

__device__ __forceinline__ bool rj_in(const RjSearch &s, u64 t, u64 byw, u64 hv)
{
    if (s.sp && s.sp[t] != byw) return false;
    const u64 v = s.vs[t] ^ s.bias;
    return s.hi_open ? v < hv : v <= hv;
}

__global__ void __launch_bounds__(FLAT_THREADS)
k_rj_search(RjSearch s)
{
    for (u64 p = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; p < s.n; p += (u64)gridDim.x * FLAT_THREADS) {
        const u64 c = s.perm[p];
        if ((c < s.nfirst) != (s.r_first != 0)) continue;               // a row of S
        const u64 i = c < s.nfirst ? c : c - s.nfirst;
        if (c >= s.n || i >= s.nR) continue;                             // (never: perm is a permutation, and the position is a row of R)
        u64 hv;
        if (s.band) {
            const u64 x = s.loR[i] ^ s.bias;
            hv = s.above > ~x ? ~0ull : x + s.above;
        } else {
            hv = s.hiR[i] ^ s.bias;
        }
        const u64 byw = s.sp ? s.sp[p] : 0;
        u64 l = p, h = s.n, step = 1;                                    // q lies in [l, h]; every position of [p, l) passes, h fails (or is n)
        while (l < h) {
            const u64 t = l + (step - 1);
            if (t >= h) break;
            if (rj_in(s, t, byw, hv)) {
                l = t + 1;
                step <<= 1;
            } else {
                h = t;
                break;
            }
        }
        while (l < h) {
            const u64 mid = l + ((h - l) >> 1);
            if (rj_in(s, mid, byw, hv)) l = mid + 1;
            else h = mid;
        }
        const u64 a = s.srank[p], b = l < s.n ? s.srank[l] : s.nS;
        s.first[i] = a;
        s.cnt[i] = b >= a ? b - a : 0;                                   // (b >= a always: srank does not decrease)
    }
}

// ---- k_rj_validate: a caller's CSR arrays before rhj_range_expand_dev expands them -----------------------------------------------
// One thread per row: offsets[0] == 0, offsets[i] <= offsets[i + 1], first[i] + cnt[i] <= nS wherever cnt[i] > 0.  res[0] (zero before
// the launch) is set to 1 by every thread that finds a violation -- plain stores of one value --, res[1] receives offsets[nR].
__global__ void __launch_bounds__(FLAT_THREADS)
k_rj_validate(const u64 *__restrict__ offsets, const u64 *__restrict__ first, u64 nR, u64 nS, u64 *__restrict__ res)
{
    for (u64 i = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; i < nR; i += (u64)gridDim.x * FLAT_THREADS) {
        const u64 a = offsets[i], b = offsets[i + 1];
        bool bad = (i == 0 && a != 0) || a > b;
        if (!bad && b > a) {
            const u64 f = first[i];
            bad = f > nS || b - a > nS - f;
        }
        if (bad) res[0] = 1;
        if (i + 1 == nR) res[1] = b;
    }
}

// ---- k_rj_expand: the pairs of output slots [0, limit) -------------------------------------------------------------------------------
// One workgroup per RANGE_EXPAND_TILE slots.  Two threads find the rows that cover the tile's first and last slot -- the last row i
// with offsets[i] <= slot, a binary search over the nR offsets; rows without partners share their successor's offset and are never the
// last such row --, every thread then finds the row of each of its slots between those two in the same way and stores {i,
// rowsS[first[i] + slot - offsets[i]]} as one 16-byte word.  A slot at or past limit = min(total, capacity) is not written.
__device__ __forceinline__ u64 rj_row_of(const u64 *__restrict__ offsets, u64 a, u64 b, u64 k)
{
    while (a < b) {                                                      // the answer lies in [a, b]
        const u64 mid = a + ((b - a + 1) >> 1);
        if (offsets[mid] <= k) a = mid;
        else b = mid - 1;
    }
    return a;
}

__global__ void __launch_bounds__(EX_THREADS)
k_rj_expand(const u64 *__restrict__ offsets, const u64 *__restrict__ first, const u64 *__restrict__ rowsS, u64 nR, u64 nS, u64 limit,
            ulonglong2 *__restrict__ out)
{
    __shared__ u64 rng[2];
    const u32 tid = threadIdx.x;
    const u64 s0 = (u64)blockIdx.x * RANGE_EXPAND_TILE;
    if (s0 >= limit || nR == 0) return;                                  // (never: the grid is ceil(limit / tile))
    const u64 s1 = s0 + RANGE_EXPAND_TILE < limit ? s0 + RANGE_EXPAND_TILE : limit;
    if (tid == 0) rng[0] = rj_row_of(offsets, 0, nR - 1, s0);
    if (tid == 64) rng[1] = rj_row_of(offsets, 0, nR - 1, s1 - 1);
    __syncthreads();
    const u64 ra = rng[0], rb = rng[1];
#pragma unroll
    for (int j = 0; j < EX_SPT; j++) {
        const u64 k = s0 + (u64)j * EX_THREADS + tid;
        if (k >= s1) continue;
        const u64 i = rj_row_of(offsets, ra, rb, k);
        const u64 o = offsets[i];
        const u64 at = first[i] + (k - o);
        if (k < o || at >= nS) continue;                                 // (never: the arrays are the scan's, or passed k_rj_validate)
        out[k] = make_ulonglong2(i, rowsS[at]);
    }
}

// the exclusive sum over n words in three launches: a.src, a.out, a.rows and the sides are the caller's
template <int MODE>
int scan(rhj_ctx *ctx, hipStream_t st, RjScan a, u64 L, u32 U, const char *what)
{
    int rc;
    a.L = L;
    if ((rc = launch(ctx, RHJ_K_HIST, what, k_rj_reduce<MODE>, U, ST, st, a)) != RHJ_OK) return rc;
    if ((rc = launch(ctx, RHJ_K_SCAN, what, k_rj_carry, 1, ST, st, a.usum, U, a.carry)) != RHJ_OK) return rc;
    return launch(ctx, RHJ_K_SCATTER, what, k_rj_apply<MODE>, U, ST, st, a);
}

// step 6 of both entries: the first min(total, capacity) pairs; tiles: the workgroups it took
int expand(rhj_ctx *ctx, hipStream_t st, const u64 *offsets, const u64 *first, const u64 *rowsS, u64 nR, u64 nS, u64 total, rhj_pair *d_out,
           u64 capacity, u64 *tiles)
{
    const u64 limit = total < capacity ? total : capacity;
    *tiles = 0;
    if (limit == 0 || !d_out) return RHJ_OK;
    const u64 g = (limit + RANGE_EXPAND_TILE - 1) / RANGE_EXPAND_TILE;
    if (g > 0x7FFFFFFFull) return rhj_internal_fail(ctx, RHJ_E_INVALID, "range join: more than 2^31 - 1 expansion tiles in one call -- slice R");
    *tiles = g;
    return launch(ctx, RHJ_K_JOIN, "k_rj_expand", k_rj_expand, (unsigned)g, EX_THREADS, st, offsets, first, rowsS, nR, nS, limit, (ulonglong2 *)d_out);
}

int range_run(rhj_ctx *ctx, const u64 *d_byR, const u64 *d_loR, const u64 *d_hiR, u64 nR, const u64 *d_byS, const u64 *d_onS, u64 nS, u32 flags,
              u64 below, u64 above, u64 *d_offsets, u64 *d_first, u64 *d_rowsS, rhj_pair *d_out, u64 capacity, u64 *out_count)
{
    const std::string me("rhj_range_join_cols_dev");
    const bool band = (flags & RHJ_RANGE_BAND) != 0;
    if (flags & ~(RHJ_RANGE_I64 | RHJ_RANGE_LO_OPEN | RHJ_RANGE_HI_OPEN | RHJ_RANGE_BAND))
        return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": unknown flags").c_str());
    if (nR > 0 && !d_loR) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_loR is null with a non-zero nR").c_str());
    if (nS > 0 && !d_onS) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_onS is null with a non-zero nS").c_str());
    if (!band && nR > 0 && !d_hiR) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_hiR is null with a non-zero nR and without RHJ_RANGE_BAND").c_str());
    if (band && d_hiR) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_hiR must be null under RHJ_RANGE_BAND").c_str());
    if (nR > 0 && nS > 0 && !d_byR != !d_byS)
        return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + (d_byR ? ": d_byS is null but d_byR is not" : ": d_byR is null but d_byS is not") +
                                                      ": `by` is given for both tables or for neither").c_str());
    if (!d_out && capacity != 0) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_out is null with a non-zero out_capacity").c_str());

    hipStream_t st = rhj_internal_stream(ctx);
    hipError_t e;
    int rc;
    if (nR == 0) {
        if (d_offsets) {
            if ((e = hipMemsetAsync(d_offsets, 0, 8, st)) != hipSuccess) return hip_fail(ctx, me.c_str(), e);
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, me.c_str(), e);
        }
        if (out_count) *out_count = 0;
        return RHJ_OK;
    }
    if (nS == 0) {
        if (d_offsets || d_first) {
            if ((rc = launch(ctx, RHJ_K_AUX, "k_rj_fill", k_rj_fill, flat_grid(nR + 1), FLAT_THREADS, st, d_offsets, d_offsets ? nR + 1 : 0, d_first,
                             d_first ? nR : 0)) != RHJ_OK)
                return rc;
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_rj_fill", e);
        }
        if (out_count) *out_count = 0;
        return RHJ_OK;
    }

    const u64 n = nR + nS;
    const bool by = d_byR != nullptr, lo_open = (flags & RHJ_RANGE_LO_OPEN) != 0;
    const u64 bias = (flags & RHJ_RANGE_I64) ? BIAS : 0;
    u64 L, LR;
    u32 U, UR;
    rhj_internal_sort_units(ctx, n, &L, &U);
    rhj_internal_sort_units(ctx, nR, &LR, &UR);
    if (U == 0 || U > ORD_MAX_UNITS || UR == 0 || UR > ORD_MAX_UNITS)
        return rhj_internal_fail(ctx, RHJ_E_HIP, (me + ": unit geometry").c_str());   // (never: the sort's own bound)

    // 1. the workspace: the concatenation, the permutation, the order words by position (with `by`: the sorted `by` words and the two
    //    buffers between the sorts, the second of which then takes the order words), the ranks, the counts, a stand-in for every CSR
    //    output the caller left out, the unit tables, the total
    const size_t nb = up256((size_t)n * 8), rb = up256((size_t)(nR + 1) * 8), sb = up256((size_t)nS * 8), ub = up256((size_t)(U > UR ? U : UR) * 8);
    const size_t bytes = (by ? 6 : 4) * nb + rb + (d_offsets ? 0 : rb) + (d_first ? 0 : rb) + (d_rowsS ? 0 : sb) + 2 * ub + 256;
    void *ws = nullptr;
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_RANGE, bytes, &ws)) != RHJ_OK) return rc;
    unsigned char *p = (unsigned char *)ws;
    u64 *con = (u64 *)p; p += nb;
    u64 *perm = (u64 *)p; p += nb;
    u64 *srank = (u64 *)p; p += nb;
    u64 *vs = (u64 *)p; p += nb;                                         // (with `by`: bufB first)
    u64 *cby = nullptr, *bufA = nullptr;
    if (by) { cby = (u64 *)p; p += nb; bufA = (u64 *)p; p += nb; }
    u64 *cnt = (u64 *)p; p += rb;
    u64 *offsets = d_offsets, *first = d_first, *rowsS = d_rowsS;
    if (!offsets) { offsets = (u64 *)p; p += rb; }
    if (!first) { first = (u64 *)p; p += rb; }
    if (!rowsS) { rowsS = (u64 *)p; p += sb; }
    u64 *d_usum = (u64 *)p; p += ub;
    u64 *d_carry = (u64 *)p; p += ub;

    // 2. the concatenation: [R ; S], under LO_OPEN [S ; R] -- among equal words the stable sort then puts the rows of S behind the row
    //    of R exactly when equality qualifies at the lower end
    const u32 r_first = lo_open ? 0u : 1u;
    const u64 nfirst = r_first ? nR : nS;
    const unsigned fg = flat_grid(n);
    if ((rc = launch(ctx, RHJ_K_AUX, "k_rj_concat", k_rj_concat, fg, FLAT_THREADS, st, d_loR, d_onS, d_byR, d_byS, nR, nS, r_first, band ? 1u : 0u, bias, below,
                     con, cby)) != RHJ_OK)
        return rc;

    // 3. the order (by, word, concatenated position), as the as-of entry's: the words argsorted in the view, then `by` gathered through
    //    that permutation and stable-sorted with the permutation as its rows; the order words by sorted position are the sorted keys
    //    after one sort, one gather after two
    const u32 sflags = (flags & RHJ_RANGE_I64) ? RHJ_SORT_I64 : 0;
    Ordered ord;
    if ((rc = order_rows(ctx, st, me.c_str(), cby, con, n, sflags, bufA, vs, cby, vs, perm, &ord)) != RHJ_OK) return rc;
    if (by && (rc = launch(ctx, RHJ_K_AUX, "k_ord_gather", k_ord_gather<u64>, fg, FLAT_THREADS, st, con, perm, n, vs)) != RHJ_OK) return rc;

    // 4. the rank scan: srank[p] = the rows of S before sorted position p, and rowsS
    RjScan a = {};
    a.src = perm; a.out = srank; a.rows = rowsS; a.n = n; a.nfirst = nfirst; a.nS = nS; a.r_first = r_first; a.usum = d_usum; a.carry = d_carry;
    if ((rc = scan<RANK>(ctx, st, a, L, U, "the rank scan")) != RHJ_OK) return rc;

    // 5. the searches: first and cnt by row of R
    RjSearch s = {};
    s.perm = perm; s.vs = vs; s.sp = ord.sp; s.srank = srank; s.loR = d_loR; s.hiR = d_hiR; s.first = first; s.cnt = cnt;
    s.n = n; s.nfirst = nfirst; s.nR = nR; s.nS = nS; s.bias = bias; s.above = above;
    s.r_first = r_first; s.band = band ? 1 : 0; s.hi_open = (flags & RHJ_RANGE_HI_OPEN) ? 1 : 0;
    if ((rc = launch(ctx, RHJ_K_TASKS, "k_rj_search", k_rj_search, fg, FLAT_THREADS, st, s)) != RHJ_OK) return rc;

    // 6. the offsets: the same scan over the counts in row order; the host reads the total
    RjScan o = {};
    o.src = cnt; o.out = offsets; o.n = nR; o.usum = d_usum; o.carry = d_carry;
    if ((rc = scan<OFFS>(ctx, st, o, LR, UR, "the offsets scan")) != RHJ_OK) return rc;
    u64 total = 0;
    e = hipMemcpyAsync(&total, offsets + nR, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(ctx, me.c_str(), e);

    // 7. the pairs
    u64 tiles = 0;
    if ((rc = expand(ctx, st, offsets, first, rowsS, nR, nS, total, d_out, capacity, &tiles)) != RHJ_OK) return rc;
    if (tiles && (e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_rj_expand", e);
    if (out_count) *out_count = total;
    rhj_internal_range_report(ctx, (int)U, by ? 2 : 1, total, tiles);
    if (total > capacity && (d_out || capacity != 0))
        return rhj_internal_fail(ctx, RHJ_E_OVERFLOW, (me + ": out_capacity is smaller than the result; *out_count holds its size").c_str());
    return RHJ_OK;
}

int expand_run(rhj_ctx *ctx, const u64 *d_offsets, const u64 *d_first, u64 nR, const u64 *d_rowsS, u64 nS, rhj_pair *d_out, u64 capacity, u64 *out_count,
               int units, int sorts)
{
    const std::string me("rhj_range_expand_dev");
    if (!d_offsets) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_offsets is null").c_str());
    if (nR > 0 && !d_first) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_first is null with a non-zero nR").c_str());
    if (nS > 0 && !d_rowsS) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_rowsS is null with a non-zero nS").c_str());
    if (!d_out && capacity != 0) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_out is null with a non-zero out_capacity").c_str());

    hipStream_t st = rhj_internal_stream(ctx);
    hipError_t e;
    int rc;
    void *ws = nullptr;
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_RANGE, 256, &ws)) != RHJ_OK) return rc;
    u64 *d_res = (u64 *)ws;
    u64 res[2] = {0, 0};
    if ((e = hipMemsetAsync(d_res, 0, 16, st)) != hipSuccess) return hip_fail(ctx, me.c_str(), e);
    if (nR > 0) {
        if ((rc = launch(ctx, RHJ_K_AUX, "k_rj_validate", k_rj_validate, flat_grid(nR), FLAT_THREADS, st, d_offsets, d_first, nR, nS, d_res)) != RHJ_OK) return rc;
        e = hipMemcpyAsync(res, d_res, 16, hipMemcpyDeviceToHost, st);
    } else {
        e = hipMemcpyAsync(res, d_offsets, 8, hipMemcpyDeviceToHost, st);   // offsets[0], which must be 0
        res[1] = 0;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(ctx, me.c_str(), e);
    if (res[0] != 0)
        return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_offsets / d_first are no CSR result over nS rows: offsets[0] != 0, an offset below its "
                                                      "predecessor, or first[i] + cnt[i] > nS").c_str());
    const u64 total = res[1];
    u64 tiles = 0;
    if ((rc = expand(ctx, st, d_offsets, d_first, d_rowsS, nR, nS, total, d_out, capacity, &tiles)) != RHJ_OK) return rc;
    if (tiles && (e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_rj_expand", e);
    if (out_count) *out_count = total;
    rhj_internal_range_report(ctx, units, sorts, total, tiles);
    if (total > capacity && (d_out || capacity != 0))
        return rhj_internal_fail(ctx, RHJ_E_OVERFLOW, (me + ": out_capacity is smaller than the result; *out_count holds its size").c_str());
    return RHJ_OK;
}

}  // namespace

extern "C" {

int rhj_range_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_byR, const uint64_t *d_loR, const uint64_t *d_hiR, uint64_t nR,
                            const uint64_t *d_byS, const uint64_t *d_onS, uint64_t nS, uint32_t flags, uint64_t below, uint64_t above,
                            uint64_t *d_out_offsets, uint64_t *d_out_first, uint64_t *d_out_rowsS,
                            rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    return range_run(ctx, (const u64 *)d_byR, (const u64 *)d_loR, (const u64 *)d_hiR, nR, (const u64 *)d_byS, (const u64 *)d_onS, nS, flags, below, above,
                     (u64 *)d_out_offsets, (u64 *)d_out_first, (u64 *)d_out_rowsS, d_out, out_capacity, (u64 *)out_count);
}

int rhj_range_expand_dev(rhj_ctx *ctx, const uint64_t *d_offsets, const uint64_t *d_first, uint64_t nR,
                         const uint64_t *d_rowsS, uint64_t nS, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    int units = 0, sorts = 0;
    rhj_internal_range_last(ctx, &units, &sorts);                        // no sort runs here: the two names keep speaking of the call that made the arrays
    rhj_internal_sort_begin(ctx);
    rhj_internal_range_report(ctx, units, sorts, 0, 0);
    return expand_run(ctx, (const u64 *)d_offsets, (const u64 *)d_first, nR, (const u64 *)d_rowsS, nS, d_out, out_capacity, (u64 *)out_count, units, sorts);
}

}  // extern "C"
