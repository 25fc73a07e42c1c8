// rhj_asof.hip -- the as-of join entry (include/rhj.h, "as-of join"): for every row of R the nearest row of S of its
// partition at or before it (or at or after it), aligned with R -- pandas.merge_asof, ASOF JOIN.  The two tables are concatenated in the
// workspace and ordered by (by, on, concatenated position) with the stable sort of rhj_sort.hip, reached through
// rhj_internal_sort_run; in that order the partner of a row of R is the last row of S before it in its partition.  What is new here
// is the heads kernel that knows which side a sorted position came from, and the scan of "the last row of S seen" that restarts at
// every partition head: three launches ordered on the context's stream -- a reduce per unit, a one-workgroup carry over the unit
// summaries, an apply per unit -- on the sort's unit geometry.  No workgroup ever waits on another, and no position, value or count
// comes from an atomic.
#include "../../include/rhj.h"
#include "rhj_internal.h"

#include <string>
#include <vector>

// provided by rhj_api.hip
int rhj_internal_use_device(rhj_ctx *ctx);
hipStream_t rhj_internal_stream(rhj_ctx *ctx);
int rhj_internal_fail(rhj_ctx *ctx, int code, const char *msg);
void rhj_internal_sort_begin(rhj_ctx *ctx);     // the start of a call: timings and "last.*" as prof_reset leaves them, "last.join_kernel" -1
void rhj_internal_sort_report(rhj_ctx *ctx, int bits, int passes, int units);
int rhj_internal_asof_workspace(rhj_ctx *ctx, size_t bytes, void **out);        // the as-of entry's own buffer (the inner sorts regrow the sort's), grown to >= bytes
void rhj_internal_asof_report(rhj_ctx *ctx, int units, int sorts, u64 matched);   // "last.asof_units" / "last.asof_sorts" / "last.asof_matched"
void *rhj_internal_span_open(rhj_ctx *ctx, int kind);
void rhj_internal_span_close(void *span);
// provided by rhj_sort.hip
int rhj_internal_sort_run(rhj_ctx *ctx, const char *who, const u64 *keys, const u64 *rows, u64 n, u32 flags, u64 *okeys, u64 *orows);
void rhj_internal_sort_units(rhj_ctx *ctx, u64 n, u64 *L, u32 *U);              // units of L rows, a whole number of tiles, under "sort.max_units"

namespace {

constexpr u64 BIAS = 1ull << 63;
constexpr int ST = SORT_THREADS, TPT = SORT_TPT, TILE = ASOF_TILE, NW = ST / 64;
constexpr u32 ASOF_MAX_UNITS = 2048;             // the sort's: what one carry workgroup scans
constexpr int RED_UNROLL = 4;
constexpr int FLAT_THREADS = 256;
constexpr u32 FLAT_MAX_GRID = 4096;
// the flag byte of a sorted position: it heads a partition / it is a row of S / it is a row of S that the scan may land on -- backward
// every row of S, forward the head of a run of rows of S with one `on` word (the smallest index of the run: the sort is stable)
constexpr u32 F_PART = 1, F_S = 2, F_RUN = 4;
static_assert(TILE == ST * TPT && ST % 64 == 0 && TILE % (NW * 64 * RED_UNROLL) == 0, "k_asof_reduce's and k_asof_apply's geometry");
static_assert(TPT <= 32, "k_asof_apply keeps one bit per round in a u32");

// ---- the scan's algebra ------------------------------------------------------------------------------------------------------------
// An element is (f, v): f -- a partition head stands here, v = (F_RUN ? position + 1 : 0).  (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 :
// max(v1, v2)), the later element on the right: DESIGN 4.27's algebra with max as the op, so the fold of a range's pieces in order is
// "1 + the last landing position since the last partition head, 0 when there is none", whatever the pieces: lanes, rounds, waves,
// tiles, units.
__device__ __forceinline__ u64 comb(u64 a, u64 b) { return b > a ? b : a; }
__device__ __forceinline__ u64 asof_value(u64 p, u32 fl) { return (fl & F_RUN) ? p + 1 : 0; }

// inclusive scan of (f, v) over the wave's lanes: __shfl_up with the head flag carried along
__device__ __forceinline__ void wave_seg_scan(u32 &f, u64 &v, u32 lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 ov = __shfl_up(v, off, 64);
        const u32 of = __shfl_up(f, off, 64);
        if (lane >= (u32)off) {
            v = f ? v : comb(ov, v);
            f |= of;
        }
    }
}

// The concatenation is [first ; second]: [S ; R], under RHJ_ASOF_STRICT [R ; S].  Concatenated index c belongs to S when
// (c < nfirst) == s_first; its row is c or c - nfirst.
struct AsofScan {
    const unsigned char *flags;                  // n flag bytes, by sorted position
    const u64 *perm;                             // perm[p] = the concatenated index at sorted position p
    const u64 *con;                              // the concatenated `on` words (the tolerance test)
    u64 *out;                                    // nR words, by row of R
    u64 n, L, nfirst, nR, nS;
    u32 U;
    u32 s_first;                                 // 1: the concatenation starts with S
    u32 use_tol, forward;
    u64 bias, tol;                               // 1 << 63 in the int64 view: the order transform of both `on` words
    u64 *usum_v;                                 // per unit: the aggregate since the unit's last head (the whole unit without one)
    u32 *usum_f;                                 // ... and whether it has a head
    u64 *carry;                                  // per unit: the aggregate since the last head before the unit
    u64 *ucnt;                                   // per unit: the rows of R that found a partner
};

// ---- k_asof_concat: dst[i] = i < na ? a[i] : b[i - na], for the `on` words and, when given, the `by` words -----------------------
__global__ void __launch_bounds__(FLAT_THREADS)
k_asof_concat(const u64 *__restrict__ on_a, const u64 *__restrict__ on_b, const u64 *__restrict__ by_a, const u64 *__restrict__ by_b, u64 na, u64 n,
              u64 *__restrict__ con, u64 *__restrict__ cby)
{
    for (u64 i = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * FLAT_THREADS) {
        const bool a = i < na;
        con[i] = a ? on_a[i] : on_b[i - na];
        if (cby) cby[i] = a ? by_a[i] : by_b[i - na];
    }
}

// ---- k_asof_gather: dst[i] = src[idx[i]] -- the `by` words in the order of the first inner sort -----------------------------------
__global__ void __launch_bounds__(FLAT_THREADS)
k_asof_gather(const u64 *__restrict__ src, const u64 *__restrict__ idx, u64 n, u64 *__restrict__ dst)
{
    for (u64 i = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * FLAT_THREADS) {
        const u64 r = idx[i];
        dst[i] = r < n ? src[r] : 0;                                  // (r < n always: idx is a permutation of 0 .. n - 1)
    }
}

// ---- k_asof_fill: every output RHJ_NO_ROW (S is empty) -----------------------------------------------------------------------------
__global__ void __launch_bounds__(FLAT_THREADS)
k_asof_fill(u64 *__restrict__ out, u64 n)
{
    for (u64 i = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * FLAT_THREADS) out[i] = RHJ_NO_ROW;
}

// ---- k_asof_heads: the flag byte of every sorted position --------------------------------------------------------------------------
// A position heads a partition when its sorted `by` word differs from its predecessor's (position 0 always does; without `by` only
// position 0).  Its side follows from its concatenated index.  con == null (backward): every row of S is a landing position.  con
// given (forward): a row of S is one when it heads its partition, follows a row of R, or its `on` word differs from its
// predecessor's -- rows of S with one (by, on) are adjacent in the sorted order, whichever table the concatenation starts with.  Each
// lane takes its predecessor's words from the lane below; lane 0 loads them.
__global__ void __launch_bounds__(ST)
k_asof_heads(const u64 *__restrict__ sp, const u64 *__restrict__ perm, const u64 *__restrict__ con, u64 n, u64 L, u64 nfirst, u32 s_first,
             unsigned char *__restrict__ flags)
{
    const u32 tid = threadIdx.x, lane = tid & 63, u = blockIdx.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    for (u64 p0 = beg; p0 < end; p0 += ST) {
        const u64 p = p0 + tid;
        const bool valid = p < end;
        u64 cp = 0, co = 0;
        u32 cs = 0;
        if (valid) {
            const u64 c = perm[p];
            if (sp) cp = sp[p];
            cs = (c < nfirst) == (s_first != 0);
            if (con) co = c < n ? con[c] : 0;                         // (c < n always: perm is a permutation)
        }
        u64 pp = __shfl_up(cp, 1, 64), po = __shfl_up(co, 1, 64);
        u32 ps = __shfl_up(cs, 1, 64);
        if (valid && lane == 0 && p > 0) {
            const u64 c = perm[p - 1];
            if (sp) pp = sp[p - 1];
            ps = (c < nfirst) == (s_first != 0);
            if (con) po = c < n ? con[c] : 0;
        }
        if (valid) {
            const bool ph = p == 0 || (sp && cp != pp);
            const bool run = cs && (!con || ph || !ps || co != po);
            flags[p] = (unsigned char)((ph ? F_PART : 0) | (cs ? F_S : 0) | (run ? F_RUN : 0));
        }
    }
}

// ---- k_asof_reduce: per unit "has a head" and the aggregate since the unit's last head ---------------------------------------------
// One workgroup per unit.  Wave w walks the w-th eighth of the unit (L is a whole number of tiles, so an eighth is a whole number of
// rounds) 64 positions at a time, RED_UNROLL rounds of loads in flight.  A round with a head keeps only the lanes from its last head
// on and replaces the wave's running aggregate; one without adds to it.  The eight wave summaries are folded in order.
__global__ void __launch_bounds__(ST)
k_asof_reduce(AsofScan a)
{
    __shared__ u64 wv[NW];
    __shared__ u32 wf[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    const u64 chunk = a.L / NW;
    u64 wb = beg + wave * chunk;
    if (wb > end) wb = end;
    const u64 we = wb + chunk < end ? wb + chunk : end;
    u32 rf = 0;
    u64 rv = 0;
    for (u64 p0 = wb; p0 < we; p0 += 64 * RED_UNROLL) {
        u32 fl[RED_UNROLL];
#pragma unroll
        for (int j = 0; j < RED_UNROLL; j++) {
            const u64 p = p0 + (u64)j * 64 + lane;
            fl[j] = p < we ? a.flags[p] : 0;
        }
#pragma unroll
        for (int j = 0; j < RED_UNROLL; j++) {
            const u64 p = p0 + (u64)j * 64 + lane;
            const u64 hb = __ballot((fl[j] & F_PART) != 0);
            u64 x = asof_value(p, fl[j]);
            if (hb != 0 && lane < (u32)(63 - __clzll((long long)hb))) x = 0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x = comb(x, __shfl_xor(x, off, 64));
            rv = hb != 0 ? x : comb(rv, x);
            rf |= hb != 0;
        }
    }
    if (lane == 0) { wv[wave] = rv; wf[wave] = rf; }
    __syncthreads();
    if (tid != 0) return;
    u32 f = 0;
    u64 v = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        v = wf[w] ? wv[w] : comb(v, wv[w]);
        f |= wf[w];
    }
    a.usum_v[u] = v;
    a.usum_f[u] = f;
}

// ---- k_asof_carry: one workgroup -- the exclusive scan of at most 2048 unit summaries ----------------------------------------------
// Thread t folds its run of ceil(U / 512) consecutive units, the runs are scanned over the workgroup (wave scan, per-wave totals
// through LDS with the flag carried along), and the thread walks its run again from its carry-in.
__global__ void __launch_bounds__(ST)
k_asof_carry(const u64 *__restrict__ usum_v, const u32 *__restrict__ usum_f, u32 U, u64 *__restrict__ carry)
{
    __shared__ u64 wv[NW];
    __shared__ u32 wf[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 per = (U + ST - 1) / ST;
    const u32 b = tid * per < U ? tid * per : U, e = b + per < U ? b + per : U;
    u32 sf = 0;
    u64 sv = 0;
    for (u32 u = b; u < e; u++) {
        const u32 fu = usum_f[u];
        const u64 vu = usum_v[u];
        sv = fu ? vu : comb(sv, vu);
        sf |= fu;
    }
    wave_seg_scan(sf, sv, lane);
    if (lane == 63) { wv[wave] = sv; wf[wave] = sf; }
    __syncthreads();
    u64 pv = 0;
#pragma unroll
    for (int w = 0; w < NW; w++)
        if ((u32)w < wave) pv = wf[w] ? wv[w] : comb(pv, wv[w]);
    u64 ev = __shfl_up(sv, 1, 64);
    u32 ef = __shfl_up(sf, 1, 64);
    if (lane == 0) { ev = 0; ef = 0; }
    u64 cur = ef ? ev : comb(pv, ev);
    for (u32 u = b; u < e; u++) {
        carry[u] = cur;
        const u32 fu = usum_f[u];
        const u64 vu = usum_v[u];
        cur = fu ? vu : comb(cur, vu);
    }
}

// ---- k_asof_apply: the scan itself, and out[row of R] ------------------------------------------------------------------------------
// One workgroup per unit, tile by tile, in the sort's position order (wave, round, lane): wave w of a tile owns positions [w * 64 *
// TPT, (w + 1) * 64 * TPT) of it.  Per round a wave scan, continued from the wave's running aggregate (lane 63 of the round before);
// per tile the waves' totals through LDS, folded onto the tile's carry-in -- the unit's from k_asof_carry, then the running one.  A
// position behind a head of its own wave is final after the wave's rounds; any other takes the fold of the carry and the waves before.
// A position of R with the value s stores: s == 0 RHJ_NO_ROW, else the row of S at sorted position s - 1 -- one gathered load of the
// permutation, and under the tolerance flag the two `on` words.  Every position of R stores.  The matches are counted per lane,
// summed over the wave with shuffles and over the waves through LDS: one word per unit, which the host adds up.
__global__ void __launch_bounds__(ST)
k_asof_apply(AsofScan a)
{
    __shared__ u64 wv[NW];
    __shared__ u32 wf[NW];
    __shared__ u64 wc[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    u64 cv = a.carry[u];
    u64 cnt = 0;
    for (u64 tb = beg; tb < end; tb += TILE) {
        const u32 tn = end - tb < (u64)TILE ? (u32)(end - tb) : (u32)TILE;
        u64 v[TPT], c[TPT];
        u32 hd = 0;                                                      // one bit per round: a head at or before this position, in its wave's part
        u32 sd = 0;                                                      // one bit per round: the position is a row of S (or past the tile's end)
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            const u64 p = tb + li;
            v[r] = 0;
            c[r] = ~0ull;
            if (li < tn) {
                const u32 fl = a.flags[p];
                c[r] = a.perm[p];
                hd |= ((fl & F_PART) ? 1u : 0u) << r;
                sd |= ((fl & F_S) ? 1u : 0u) << r;
                v[r] = asof_value(p, fl);
            } else {
                sd |= 1u << r;
            }
        }
        u32 rf = 0;
        u64 rv = 0;
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            u32 f = (hd >> r) & 1;
            u64 x = v[r];
            wave_seg_scan(f, x, lane);
            x = f ? x : comb(rv, x);
            f |= rf;
            v[r] = x;
            hd = (hd & ~(1u << r)) | (f << r);
            rv = __shfl(x, 63, 64);
            rf = __shfl(f, 63, 64);
        }
        if (lane == 0) { wv[wave] = rv; wf[wave] = rf; }
        __syncthreads();
        u64 pre = cv, tot = cv;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            tot = wf[w] ? wv[w] : comb(tot, wv[w]);
            if ((u32)w < wave) pre = tot;
        }
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            if ((sd >> r) & 1) continue;
            const u64 rowR = a.s_first ? c[r] - a.nfirst : c[r];
            if (c[r] >= a.n || rowR >= a.nR) continue;                   // (never: perm is a permutation, and the position is a row of R)
            const u64 s = ((hd >> r) & 1) ? v[r] : comb(pre, v[r]);
            u64 res = RHJ_NO_ROW;
            if (s != 0 && s <= a.n) {                                    // (s <= n always: a landing position + 1)
                const u64 cs = a.perm[s - 1];
                const u64 rowS = a.s_first ? cs : cs - a.nfirst;
                if (cs < a.n && rowS < a.nS) {                           // (always: a landing position is a row of S)
                    res = rowS;
                    if (a.use_tol) {
                        const u64 x = a.con[c[r]] ^ a.bias, y = a.con[cs] ^ a.bias;
                        if ((a.forward ? y - x : x - y) > a.tol) res = RHJ_NO_ROW;
                    }
                }
            }
            a.out[rowR] = res;
            cnt += res != RHJ_NO_ROW;
        }
        cv = tot;
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) wc[wave] = cnt;
    __syncthreads();
    if (tid != 0) return;
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) t += wc[w];
    a.ucnt[u] = t;
}

int hip_fail(rhj_ctx *ctx, const char *what, hipError_t e)
{
    (void)hipGetLastError();
    return rhj_internal_fail(ctx, e == hipErrorOutOfMemory ? RHJ_E_NOMEM : RHJ_E_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

int check(rhj_ctx *ctx, const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RHJ_OK : hip_fail(ctx, what, e);
}

struct Span {
    void *s;
    Span(rhj_ctx *ctx, int kind) : s(rhj_internal_span_open(ctx, kind)) {}
    ~Span() { rhj_internal_span_close(s); }
};

unsigned flat_grid(u64 n)
{
    u64 g = (n + FLAT_THREADS - 1) / FLAT_THREADS;
    if (g > FLAT_MAX_GRID) g = FLAT_MAX_GRID;
    return (unsigned)(g ? g : 1);
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

int asof_run(rhj_ctx *ctx, const u64 *d_byR, const u64 *d_onR, u64 nR, const u64 *d_byS, const u64 *d_onS, u64 nS, u32 flags, u64 tolerance,
             u64 *d_out, u64 *out_matched)
{
    const std::string me("rhj_asof_cols_dev");
    if (flags & ~(RHJ_ASOF_I64 | RHJ_ASOF_FORWARD | RHJ_ASOF_STRICT | RHJ_ASOF_TOLERANCE))
        return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": unknown flags").c_str());
    if (nR > 0 && !d_onR) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_onR is null with a non-zero nR").c_str());
    if (nS > 0 && !d_onS) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_onS is null with a non-zero nS").c_str());
    if (nR > 0 && !d_out) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_out_rowS is null with a non-zero nR").c_str());
    if (nR > 0 && nS > 0 && !d_byR != !d_byS)
        return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + (d_byR ? ": d_byS is null but d_byR is not" : ": d_byR is null but d_byS is not") +
                                                      ": `by` is given for both tables or for neither").c_str());
    if (out_matched) *out_matched = 0;
    if (nR == 0) return RHJ_OK;

    hipStream_t st = rhj_internal_stream(ctx);
    hipError_t e;
    int rc;
    if (nS == 0) {
        {
            Span s(ctx, RHJ_K_AUX);
            hipLaunchKernelGGL(k_asof_fill, dim3(flat_grid(nR)), dim3(FLAT_THREADS), 0, st, d_out, nR);
        }
        if ((rc = check(ctx, "k_asof_fill")) != RHJ_OK) return rc;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_asof_fill", e);
        return RHJ_OK;
    }

    const u64 n = nR + nS;
    const bool by = d_byR != nullptr, strict = (flags & RHJ_ASOF_STRICT) != 0, forward = (flags & RHJ_ASOF_FORWARD) != 0;
    u64 L;
    u32 U;
    rhj_internal_sort_units(ctx, n, &L, &U);
    if (U == 0 || U > ASOF_MAX_UNITS) return rhj_internal_fail(ctx, RHJ_E_HIP, (me + ": unit geometry").c_str());   // (never: the sort's own bound)

    // 1. the workspace: two n-word arrays, five with `by`, the flag bytes, the unit tables
    const size_t nb = up256((size_t)n * 8), ub = up256((size_t)U * 8);
    const size_t bytes = (by ? 5 : 2) * nb + up256((size_t)n) + 4 * ub;
    void *ws = nullptr;
    if ((rc = rhj_internal_asof_workspace(ctx, bytes, &ws)) != RHJ_OK) return rc;
    unsigned char *p = (unsigned char *)ws;
    u64 *con = (u64 *)p; p += nb;
    u64 *perm = (u64 *)p; p += nb;
    u64 *cby = nullptr, *bufA = nullptr, *bufB = nullptr;
    if (by) { cby = (u64 *)p; p += nb; bufA = (u64 *)p; p += nb; bufB = (u64 *)p; p += nb; }
    unsigned char *d_flags = p; p += up256((size_t)n);
    u64 *d_usum_v = (u64 *)p; p += ub;
    u32 *d_usum_f = (u32 *)p; p += ub;
    u64 *d_carry = (u64 *)p; p += ub;
    u64 *d_ucnt = (u64 *)p; p += ub;

    // 2. the concatenation: [S ; R], under STRICT [R ; S] -- among equal `on` words the stable sort then puts the rows of S in front of
    //    the rows of R exactly when they are candidates
    const u64 nfirst = strict ? nR : nS;
    {
        Span s(ctx, RHJ_K_AUX);
        hipLaunchKernelGGL(k_asof_concat, dim3(flat_grid(n)), dim3(FLAT_THREADS), 0, st, strict ? d_onR : d_onS, strict ? d_onS : d_onR,
                           strict ? d_byR : d_byS, strict ? d_byS : d_byR, nfirst, n, con, cby);
    }
    if ((rc = check(ctx, "k_asof_concat")) != RHJ_OK) return rc;

    // 3. the order (by, on, concatenated position): `on` argsorted in the view, descending for FORWARD, then `by` gathered through that
    //    permutation and stable-sorted with the permutation as its rows (its sorted words land on the concatenated `by`, which is done)
    const u32 sflags = ((flags & RHJ_ASOF_I64) ? RHJ_SORT_I64 : 0) | (forward ? RHJ_SORT_DESC : 0);
    const u64 *sp = nullptr;
    if (by) {
        if ((rc = rhj_internal_sort_run(ctx, me.c_str(), con, nullptr, n, sflags, nullptr, bufA)) != RHJ_OK) return rc;
        {
            Span s(ctx, RHJ_K_AUX);
            hipLaunchKernelGGL(k_asof_gather, dim3(flat_grid(n)), dim3(FLAT_THREADS), 0, st, (const u64 *)cby, (const u64 *)bufA, n, bufB);
        }
        if ((rc = check(ctx, "k_asof_gather")) != RHJ_OK) return rc;
        if ((rc = rhj_internal_sort_run(ctx, me.c_str(), bufB, bufA, n, 0, cby, perm)) != RHJ_OK) return rc;
        sp = cby;
    } else {
        if ((rc = rhj_internal_sort_run(ctx, me.c_str(), con, nullptr, n, sflags, nullptr, perm)) != RHJ_OK) return rc;
    }
    rhj_internal_sort_report(ctx, 0, 0, 0);                              // "last.sort_*" speak of the sort entries only

    // 4. heads
    {
        Span s(ctx, RHJ_K_AUX);
        hipLaunchKernelGGL(k_asof_heads, dim3(U), dim3(ST), 0, st, sp, (const u64 *)perm, forward ? (const u64 *)con : (const u64 *)nullptr, n, L, nfirst,
                           strict ? 0u : 1u, d_flags);
    }
    if ((rc = check(ctx, "k_asof_heads")) != RHJ_OK) return rc;

    // 5. the scan: reduce, carry, apply, ordered by the stream
    AsofScan a = {};
    a.flags = d_flags; a.perm = perm; a.con = con; a.out = d_out; a.n = n; a.L = L; a.nfirst = nfirst; a.nR = nR; a.nS = nS; a.U = U;
    a.s_first = strict ? 0 : 1; a.use_tol = (flags & RHJ_ASOF_TOLERANCE) ? 1 : 0; a.forward = forward ? 1 : 0;
    a.bias = (flags & RHJ_ASOF_I64) ? BIAS : 0; a.tol = tolerance;
    a.usum_v = d_usum_v; a.usum_f = d_usum_f; a.carry = d_carry; a.ucnt = d_ucnt;
    {
        Span s(ctx, RHJ_K_HIST);
        hipLaunchKernelGGL(k_asof_reduce, dim3(U), dim3(ST), 0, st, a);
    }
    if ((rc = check(ctx, "k_asof_reduce")) != RHJ_OK) return rc;
    {
        Span s(ctx, RHJ_K_SCAN);
        hipLaunchKernelGGL(k_asof_carry, dim3(1), dim3(ST), 0, st, (const u64 *)d_usum_v, (const u32 *)d_usum_f, U, d_carry);
    }
    if ((rc = check(ctx, "k_asof_carry")) != RHJ_OK) return rc;
    {
        Span s(ctx, RHJ_K_SCATTER);
        hipLaunchKernelGGL(k_asof_apply, dim3(U), dim3(ST), 0, st, a);
    }
    if ((rc = check(ctx, "k_asof_apply")) != RHJ_OK) return rc;

    // 6. matched: the apply's per-unit counts, summed on the host
    std::vector<u64> cnt(U);
    e = hipMemcpyAsync(cnt.data(), d_ucnt, (size_t)U * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(ctx, "rhj_asof_cols_dev", e);
    u64 matched = 0;
    for (u32 u = 0; u < U; u++) matched += cnt[u];
    if (out_matched) *out_matched = matched;
    rhj_internal_asof_report(ctx, (int)U, by ? 2 : 1, matched);
    return RHJ_OK;
}

}  // namespace

extern "C" {

int rhj_asof_cols_dev(rhj_ctx *ctx, const uint64_t *d_byR, const uint64_t *d_onR, uint64_t nR,
                      const uint64_t *d_byS, const uint64_t *d_onS, uint64_t nS, uint32_t flags, uint64_t tolerance,
                      uint64_t *d_out_rowS, uint64_t *out_matched)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    return asof_run(ctx, (const u64 *)d_byR, (const u64 *)d_onR, nR, (const u64 *)d_byS, (const u64 *)d_onS, nS, flags, tolerance, (u64 *)d_out_rowS,
                    (u64 *)out_matched);
}

}  // extern "C"
