// rhj_asof.hip -- the as-of join entry (include/rhj.h, "as-of join"): for every row of R the nearest row of S of its
// partition at or before it (or at or after it), aligned with R -- pandas.merge_asof, ASOF JOIN.  The two tables are concatenated in the
// workspace and ordered by (by, on, concatenated position) with the stable sort of rhj_sort.hip, reached through
// rhj_internal_sort_run; in that order the partner of a row of R is the last row of S before it in its partition.  What is new here
// is the heads kernel that knows which side a sorted position came from, and the scan of "the last row of S seen" that restarts at
// every partition head: three launches ordered on the context's stream -- a reduce per unit, a one-workgroup carry over the unit
// summaries, an apply per unit -- on the sort's unit geometry.  No workgroup ever waits on another, and no position, value or count
// comes from an atomic.
#include "rhj_ordered.h"

namespace {

constexpr int TILE = ASOF_TILE;
// the flag byte of a sorted position: it heads a partition / it is a row of S / it is a row of S that the scan may land on -- backward
// every row of S, forward the head of a run of rows of S with one `on` word (the smallest index of the run: the sort is stable)
constexpr u32 F_PART = 1, F_S = 2, F_RUN = 4;
static_assert(TILE == SORT_TILE, "k_asof_reduce's and k_asof_apply's geometry is the sort's (rhj_ordered.h)");

// ---- the scan's algebra ------------------------------------------------------------------------------------------------------------
// An element is (f, v): f -- a partition head stands here, v = (F_RUN ? position + 1 : 0), folded with rhj_ordered.h's algebra under
// OP_MAX: (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : max(v1, v2)), the later element on the right.  The fold of a range's pieces in
// order is "1 + the last landing position since the last partition head, 0 when there is none", whatever the pieces: lanes, rounds,
// waves, tiles, units.
__device__ __forceinline__ u64 asof_value(u64 p, u32 fl) { return (fl & F_RUN) ? p + 1 : 0; }

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
            for (int off = 32; off > 0; off >>= 1) x = comb<OP_MAX>(x, __shfl_xor(x, off, 64));
            rv = hb != 0 ? x : comb<OP_MAX>(rv, x);
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
        v = wf[w] ? wv[w] : comb<OP_MAX>(v, wv[w]);
        f |= wf[w];
    }
    a.usum_v[u] = v;
    a.usum_f[u] = f;
}

// ---- k_asof_apply: the scan itself, and out[row of R] ------------------------------------------------------------------------------
// One workgroup per unit, tile by tile, in the sort's position order (wave, round, lane): wave w of a tile owns positions [w * 64 *
// TPT, (w + 1) * 64 * TPT) of it.  Per round a wave scan, continued from the wave's running aggregate (lane 63 of the round before);
// per tile the waves' totals through LDS, folded onto the tile's carry-in -- the unit's from k_ord_carry, then the running one.  A
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
            wave_seg_scan<OP_MAX>(f, x, lane);
            x = f ? x : comb<OP_MAX>(rv, x);
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
            tot = wf[w] ? wv[w] : comb<OP_MAX>(tot, wv[w]);
            if ((u32)w < wave) pre = tot;
        }
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            if ((sd >> r) & 1) continue;
            const u64 rowR = a.s_first ? c[r] - a.nfirst : c[r];
            if (c[r] >= a.n || rowR >= a.nR) continue;                   // (never: perm is a permutation, and the position is a row of R)
            const u64 s = ((hd >> r) & 1) ? v[r] : comb<OP_MAX>(pre, v[r]);
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
        if ((rc = launch(ctx, RHJ_K_AUX, "k_asof_fill", k_asof_fill, flat_grid(nR), FLAT_THREADS, st, d_out, nR)) != RHJ_OK) return rc;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, "k_asof_fill", e);
        return RHJ_OK;
    }

    const u64 n = nR + nS;
    const bool by = d_byR != nullptr, strict = (flags & RHJ_ASOF_STRICT) != 0, forward = (flags & RHJ_ASOF_FORWARD) != 0;
    u64 L;
    u32 U;
    rhj_internal_sort_units(ctx, n, &L, &U);
    if (U == 0 || U > ORD_MAX_UNITS) return rhj_internal_fail(ctx, RHJ_E_HIP, (me + ": unit geometry").c_str());   // (never: the sort's own bound)

    // 1. the workspace: two n-word arrays, five with `by`, the flag bytes, the unit tables
    const size_t nb = up256((size_t)n * 8), ub = up256((size_t)U * 8);
    const size_t bytes = (by ? 5 : 2) * nb + up256((size_t)n) + 4 * ub;
    void *ws = nullptr;
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_ASOF, bytes, &ws)) != RHJ_OK) return rc;
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
    if ((rc = launch(ctx, RHJ_K_AUX, "k_asof_concat", k_asof_concat, flat_grid(n), FLAT_THREADS, st, strict ? d_onR : d_onS, strict ? d_onS : d_onR,
                     strict ? d_byR : d_byS, strict ? d_byS : d_byR, nfirst, n, con, cby)) != RHJ_OK)
        return rc;

    // 3. the order (by, on, concatenated position): `on` argsorted in the view, descending for FORWARD, then `by` gathered through that
    //    permutation and stable-sorted with the permutation as its rows (its sorted words land on the concatenated `by`, which is done)
    const u32 sflags = ((flags & RHJ_ASOF_I64) ? RHJ_SORT_I64 : 0) | (forward ? RHJ_SORT_DESC : 0);
    Ordered o;
    if ((rc = order_rows(ctx, st, me.c_str(), cby, con, n, sflags, bufA, bufB, cby, nullptr, perm, &o)) != RHJ_OK) return rc;

    // 4. heads
    if ((rc = launch(ctx, RHJ_K_AUX, "k_asof_heads", k_asof_heads, U, ST, st, o.sp, perm, forward ? con : nullptr, n, L, nfirst, strict ? 0u : 1u,
                     d_flags)) != RHJ_OK)
        return rc;

    // 5. the scan: reduce, carry, apply, ordered by the stream
    AsofScan a = {};
    a.flags = d_flags; a.perm = perm; a.con = con; a.out = d_out; a.n = n; a.L = L; a.nfirst = nfirst; a.nR = nR; a.nS = nS; a.U = U;
    a.s_first = strict ? 0 : 1; a.use_tol = (flags & RHJ_ASOF_TOLERANCE) ? 1 : 0; a.forward = forward ? 1 : 0;
    a.bias = (flags & RHJ_ASOF_I64) ? BIAS : 0; a.tol = tolerance;
    a.usum_v = d_usum_v; a.usum_f = d_usum_f; a.carry = d_carry; a.ucnt = d_ucnt;
    if ((rc = launch(ctx, RHJ_K_HIST, "k_asof_reduce", k_asof_reduce, U, ST, st, a)) != RHJ_OK) return rc;
    if ((rc = launch(ctx, RHJ_K_SCAN, "k_ord_carry", k_ord_carry<OP_MAX>, 1, ST, st, d_usum_v, d_usum_f, U, d_carry)) != RHJ_OK) return rc;
    if ((rc = launch(ctx, RHJ_K_SCATTER, "k_asof_apply", k_asof_apply, U, ST, st, a)) != RHJ_OK) return rc;

    // 6. matched: the apply's per-unit counts, summed on the host
    u64 matched = 0;
    if ((rc = unit_total(ctx, st, me.c_str(), d_ucnt, U, &matched)) != RHJ_OK) return rc;
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
