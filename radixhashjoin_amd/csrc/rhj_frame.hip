// rhj_frame.hip -- the frame entry (include/rhj.h, "framed window aggregates"): a value per row from the ROWS frame
// [q - preceding, q + following] around it in its partition -- COUNT, SUM, MIN / MAX, the frame's first / last row.  The order
// (partition, order key, input position) comes from the stable sort of rhj_sort.hip, as in rhj_window.hip.  What is new here: scans
// that are stored BY SORTED POSITION, run forward or backward (the same fold over the mirrored position n - 1 - p), and restart at
// the starts of blocks of w consecutive positions beside the partition heads -- so that a sliding minimum or maximum of width w is
// the fold of at most two stored words, whatever w (van Herk, Gil-Werman) --, and one emit launch that reads them at the frame's two
// ends and stores out[perm[p]].  Per scan three launches ordered on the context's stream: a reduce per unit, a one-workgroup carry
// over the unit summaries, an apply per unit.  No workgroup ever waits on another, and no position, value or count comes from an
// atomic.
// The RANGE entry (include/rhj.h, "RANGE frames") stands behind it in this file and runs on the same kernels: its frames
// are value distances on the order key, found by two searches per row in the order words by sorted position.
#include "rhj_ordered.h"

namespace {

constexpr int TILE = WINDOW_TILE;
static_assert(TILE == SORT_TILE, "k_frm_reduce's and k_frm_apply's geometry is the sort's (rhj_ordered.h)");

// ---- the scan's algebra ------------------------------------------------------------------------------------------------------------
// rhj_ordered.h's (f, v) fold.  It is associative wherever the heads stand, so heads at block starts beside the
// partition heads change nothing in the argument, and neither does the direction: a backward scan is this fold over the index
// m = n - 1 - p, in which a partition's tail and a block's end are the heads.
enum { VS_COL = 0, VS_POS = 1 };                 // the value: a column word through the permutation; head ? position : the identity

struct FrmScan {
    const unsigned char *flags;                  // n bytes, by sorted position: non-zero where a partition starts
    const u64 *perm;                             // perm[p] = the row at sorted position p; null: the identity
    const u64 *col;                              // VS_COL: the caller's column, by row
    u64 *out;                                    // BY SORTED POSITION p, in both directions
    u64 n, L;
    u32 U;
    u64 bias;                                    // VS_COL: 1 << 63 for the signed minimum / maximum; the stored words keep it, k_frm_emit takes it off
    u64 w, s64, stile;                           // BLK: the block length (1 <= w < n), 64 % w and TILE % w
    u64 *usum_v;                                 // per unit: the aggregate since the unit's last head (the whole unit without one)
    u32 *usum_f;                                 // ... and whether it has a head
    u64 *carry;                                  // per unit: the aggregate since the last head before the unit
};

// The scans run over the index m: the position itself forward, n - 1 - p backward.  The block counter c(m) is m forward and n - m
// (= p + 1) backward; a block head stands where c % w == 0: at a block's first position forward, at its last one backward.  A thread
// takes ONE 64-bit remainder per launch and steps it by 64 % w per round and TILE % w per tile (both from the host): x, s < w <
// n < 2^63, so nothing wraps.
template <bool BACK> __device__ __forceinline__ u64 frm_pos(const FrmScan &a, u64 m) { return BACK ? a.n - 1 - m : m; }
template <bool BACK> __device__ __forceinline__ u64 frm_rem0(const FrmScan &a, u64 m) { return m < a.n ? (BACK ? a.n - m : m) % a.w : 0; }
template <bool BACK> __device__ __forceinline__ u64 frm_step(u64 x, u64 s, u64 w)
{
    if (BACK) return x >= s ? x - s : x + (w - s);
    x += s;
    return x >= w ? x - w : x;
}
// the partition head at m (m < n): position 0 or a flagged one forward; backward the last position, or one whose successor is flagged
template <bool BACK> __device__ __forceinline__ u32 frm_head(const FrmScan &a, u64 m, u64 p)
{
    if (m == 0) return 1;
    return a.flags[BACK ? p + 1 : p] ? 1 : 0;
}
template <int OP, int VS, bool BACK> __device__ __forceinline__ u64 frm_value(const FrmScan &a, u64 p, u32 head)
{
    if (VS == VS_POS) return head ? p : ident<OP>();
    const u64 row = a.perm ? a.perm[p] : p;
    return row < a.n ? a.col[row] ^ a.bias : ident<OP>();                 // (row < n always: perm is a permutation)
}

// ---- k_frm_heads: one flag byte per sorted position, and the partition heads per unit ----------------------------------------------
// A position heads a partition when its sorted partition word differs from its predecessor's; position 0 always does.  Each lane
// takes its predecessor's word from the lane below; lane 0 loads it.
__global__ void __launch_bounds__(ST)
k_frm_heads(const u64 *__restrict__ sp, u64 n, u64 L, unsigned char *__restrict__ flags, u64 *__restrict__ ucnt)
{
    __shared__ u64 ws[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, u = blockIdx.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    u64 cnt = 0;
    for (u64 p0 = beg; p0 < end; p0 += ST) {
        const u64 p = p0 + tid;
        const bool valid = p < end;
        u64 cp = 0;
        if (valid && sp) cp = sp[p];
        u64 pp = __shfl_up(cp, 1, 64);
        if (valid && lane == 0 && p > 0 && sp) pp = sp[p - 1];
        if (valid) {
            const bool ph = p == 0 || (sp && cp != pp);
            flags[p] = ph ? 1 : 0;
            cnt += ph;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) ws[tid >> 6] = cnt;
    __syncthreads();
    if (tid != 0) return;
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) s += ws[w];
    ucnt[u] = s;
}

// ---- k_frm_reduce<OP, VS, BACK, BLK>: per unit "has a head" and the aggregate since the unit's last head --------------------------
// One workgroup per unit of the index m.  Wave w walks the w-th eighth of the unit 64 indices at a time, RED_UNROLL rounds of loads
// in flight.  A round with a head keeps only the lanes from its last head on and replaces the wave's running aggregate; one without
// adds to it.  The eight wave summaries are folded in order.
template <int OP, int VS, bool BACK, bool BLK>
__global__ void __launch_bounds__(ST)
k_frm_reduce(FrmScan a)
{
    __shared__ u64 wv[NW];
    __shared__ u32 wf[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    const u64 chunk = a.L / NW;
    u64 wb = beg + wave * chunk;
    if (wb > end) wb = end;
    const u64 we = wb + chunk < end ? wb + chunk : end;
    u64 rem = BLK ? frm_rem0<BACK>(a, wb + lane) : 1;
    u32 rf = 0;
    u64 rv = ident<OP>();
    for (u64 m0 = wb; m0 < we; m0 += 64 * RED_UNROLL) {
        u32 fl[RED_UNROLL];
        u64 v[RED_UNROLL];
#pragma unroll
        for (int j = 0; j < RED_UNROLL; j++) {
            const u64 m = m0 + (u64)j * 64 + lane;
            fl[j] = 0;
            v[j] = ident<OP>();
            if (m < we) {
                const u64 p = frm_pos<BACK>(a, m);
                const u32 ph = frm_head<BACK>(a, m, p);
                fl[j] = ph | (BLK && rem == 0 ? 1u : 0u);
                v[j] = frm_value<OP, VS, BACK>(a, p, ph);
            }
            if (BLK) rem = frm_step<BACK>(rem, a.s64, a.w);
        }
#pragma unroll
        for (int j = 0; j < RED_UNROLL; j++) {
            const u64 hb = __ballot(fl[j] != 0);
            u64 x = v[j];
            if (hb != 0 && lane < (u32)(63 - __clzll((long long)hb))) x = ident<OP>();
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x = comb<OP>(x, __shfl_xor(x, off, 64));
            rv = hb != 0 ? x : comb<OP>(rv, x);
            rf |= hb != 0;
        }
    }
    if (lane == 0) { wv[wave] = rv; wf[wave] = rf; }
    __syncthreads();
    if (tid != 0) return;
    u32 f = 0;
    u64 v = ident<OP>();
#pragma unroll
    for (int w = 0; w < NW; w++) {
        v = wf[w] ? wv[w] : comb<OP>(v, wv[w]);
        f |= wf[w];
    }
    a.usum_v[u] = v;
    a.usum_f[u] = f;
}

// ---- k_frm_apply<OP, VS, BACK, BLK>: the scan itself, stored by position -------------------------------------------------------------
// One workgroup per unit, tile by tile, in the order (wave, round, lane): wave w of a tile owns the indices [w * 64 * TPT, (w + 1) *
// 64 * TPT) of it.  Per round a wave scan, continued from the wave's running aggregate (lane 63 of the round before); per tile the
// waves' totals through LDS, folded onto the tile's carry-in -- the unit's from k_ord_carry, then the running one.  An index behind a
// head of its own wave is final after the wave's rounds; any other takes the fold of the carry and the waves before.
template <int OP, int VS, bool BACK, bool BLK>
__global__ void __launch_bounds__(ST)
k_frm_apply(FrmScan a)
{
    __shared__ u64 wv[NW];
    __shared__ u32 wf[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    u64 rem_t = BLK ? frm_rem0<BACK>(a, beg + wave * (64 * TPT) + lane) : 1;     // of this thread's first index of the tile
    u64 cv = a.carry[u];
    for (u64 tb = beg; tb < end; tb += TILE) {
        const u32 tn = end - tb < (u64)TILE ? (u32)(end - tb) : (u32)TILE;
        u64 v[TPT];
        u32 hd = 0;                                                      // one bit per round: a head at or before this index, in its wave's part
        u64 rem = rem_t;
        const u64 pb = frm_pos<BACK>(a, tb + wave * (64 * TPT) + lane);     // the position of this thread's first index of the tile; round r is r * 64 further on
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            v[r] = ident<OP>();
            if (li < tn) {
                const u64 p = BACK ? pb - (u64)(r * 64) : pb + (u64)(r * 64);
                const u32 ph = frm_head<BACK>(a, tb + li, p);
                hd |= (ph | (BLK && rem == 0 ? 1u : 0u)) << r;
                v[r] = frm_value<OP, VS, BACK>(a, p, ph);
            }
            if (BLK) rem = frm_step<BACK>(rem, a.s64, a.w);
        }
        if (BLK) rem_t = frm_step<BACK>(rem_t, a.stile, a.w);
        u32 rf = 0;
        u64 rv = ident<OP>();
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            u32 f = (hd >> r) & 1;
            u64 x = v[r];
            wave_seg_scan<OP>(f, x, lane);
            x = f ? x : comb<OP>(rv, x);
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
            tot = wf[w] ? wv[w] : comb<OP>(tot, wv[w]);
            if ((u32)w < wave) pre = tot;
        }
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            if (li >= tn) continue;                                      // (tb + li < end <= n: the store below is inside out[0 .. n))
            a.out[BACK ? pb - (u64)(r * 64) : pb + (u64)(r * 64)] = ((hd >> r) & 1) ? v[r] : comb<OP>(pre, v[r]);
        }
        cv = tot;
        __syncthreads();
    }
}

// ---- k_frm_emit: every op's answer from the by-position arrays, and out[perm[p]] ------------------------------------------------------
// pstart[p] / pend[p]: the first / last sorted position of p's partition (null: not needed by any op of the call -- every preceding /
// following is 0 --, and p stands in).  lo = max(pstart, p - preceding), hi = min(pend, p + following), without wrap-around.
//   COUNT hi - lo + 1;  FIRST_ROW perm[lo];  LAST_ROW perm[hi];  SUM S[hi] - (lo > pstart ? S[lo - 1] : 0)
//   MIN / MAX  M_FWD: F[hi] (lo is the partition's start);  M_BACK: B[lo] (hi is its end);  M_BOTH: with bs the start of hi's block
//              (0 without blocks) -- lo == max(bs, pstart): F[hi]; else lo >= bs: B[lo] (hi is the partition's end); else the two
//              blocks are neighbours and the answer is op(B[lo], F[hi])  
// One sweep of the positions per op (the bounds and the permutation are read again: 8 .. 24 coalesced bytes per row and op).
enum { M_FWD = 0, M_BACK = 1, M_BOTH = 2 };
struct FrmEmit {
    u32 nops;
    u32 op[RHJ_FRAME_MAX_OPS], mode[RHJ_FRAME_MAX_OPS];
    u64 prec[RHJ_FRAME_MAX_OPS], fol[RHJ_FRAME_MAX_OPS];
    u64 w[RHJ_FRAME_MAX_OPS], sgrid[RHJ_FRAME_MAX_OPS];               // M_BOTH with blocks: the block length and (grid stride) % w; w == 0: one block
    u64 bias[RHJ_FRAME_MAX_OPS];
    const u64 *F[RHJ_FRAME_MAX_OPS];                                  // SUM: S
    const u64 *B[RHJ_FRAME_MAX_OPS];
    u64 *out[RHJ_FRAME_MAX_OPS];
};

// one op over every position: its parameters stay uniform words for the length of its sweep, and the block offset p % w is ONE 64-bit
// remainder per thread, stepped by (grid stride) % w
__device__ __forceinline__ void frm_emit_op(const u64 *__restrict__ pstart, const u64 *__restrict__ pend, const u64 *__restrict__ perm, u64 n,
                                            u32 op, u32 mode, u64 prec, u64 fol, u64 w, u64 sgrid, u64 bias, const u64 *__restrict__ F,
                                            const u64 *__restrict__ B, u64 *__restrict__ out)
{
    const u64 p0 = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x;
    const bool mn = op == RHJ_FRAME_MIN_U64 || op == RHJ_FRAME_MIN_I64;
    u64 rem = w != 0 ? p0 % w : 0;
    for (u64 p = p0; p < n; p += (u64)gridDim.x * FLAT_THREADS) {
        const u64 row = perm ? perm[p] : p;
        u64 ps = pstart ? pstart[p] : p, pe = pend ? pend[p] : p;
        if (ps > p) ps = p;                                              // (never: pstart <= p <= pend < n; the guards keep every index below inside [0, n))
        if (pe < p || pe >= n) pe = p;
        const u64 lo = prec >= p - ps ? ps : p - prec;
        const u64 hi = fol >= pe - p ? pe : p + fol;
        u64 val;
        if (op == RHJ_FRAME_COUNT) {
            val = hi - lo + 1;
        } else if (op == RHJ_FRAME_FIRST_ROW) {
            val = perm ? perm[lo] : lo;
        } else if (op == RHJ_FRAME_LAST_ROW) {
            val = perm ? perm[hi] : hi;
        } else if (op == RHJ_FRAME_SUM) {
            val = F[hi] - (lo > ps ? F[lo - 1] : 0);
        } else {
            if (mode == M_FWD) {
                val = F[hi];
            } else if (mode == M_BACK) {
                val = B[lo];
            } else {
                u64 bs = 0;                                              // the start of hi's block: p's own, or the next one
                if (w != 0) bs = hi - p < w - rem ? p - rem : p - rem + w;
                if (lo == (bs > ps ? bs : ps)) {
                    val = F[hi];
                } else if (lo >= bs) {
                    val = B[lo];
                } else {
                    const u64 x = B[lo], y = F[hi];
                    val = mn ? (y < x ? y : x) : (y > x ? y : x);
                }
            }
            val ^= bias;
        }
        if (row < n) out[row] = val;                                     // (row < n always: perm is a permutation)
        if (w != 0) {
            rem += sgrid;
            if (rem >= w) rem -= w;
        }
    }
}

__global__ void __launch_bounds__(FLAT_THREADS)
k_frm_emit(const u64 *__restrict__ pstart, const u64 *__restrict__ pend, const u64 *__restrict__ perm, u64 n, FrmEmit e)
{
#pragma unroll
    for (u32 j = 0; j < RHJ_FRAME_MAX_OPS; j++) {
        if (j >= e.nops) break;
        frm_emit_op(pstart, pend, perm, n, e.op[j], e.mode[j], e.prec[j], e.fol[j], e.w[j], e.sgrid[j], e.bias[j], e.F[j], e.B[j], e.out[j]);
    }
}

// one scan: reduce, carry, apply, ordered by the stream
template <int OP, int VS, bool BACK, bool BLK>
int scan_t(rhj_ctx *ctx, hipStream_t st, const FrmScan &a)
{
    int rc;
    if ((rc = launch(ctx, RHJ_K_HIST, "k_frm_reduce", k_frm_reduce<OP, VS, BACK, BLK>, a.U, ST, st, a)) != RHJ_OK) return rc;
    if ((rc = launch(ctx, RHJ_K_SCAN, "k_ord_carry", k_ord_carry<OP>, 1, ST, st, a.usum_v, a.usum_f, a.U, a.carry)) != RHJ_OK) return rc;
    return launch(ctx, RHJ_K_SCATTER, "k_frm_apply", k_frm_apply<OP, VS, BACK, BLK>, a.U, ST, st, a);
}

template <int OP>
int scan_col(rhj_ctx *ctx, hipStream_t st, const FrmScan &a, bool back, bool blk)
{
    if (back) return blk ? scan_t<OP, VS_COL, true, true>(ctx, st, a) : scan_t<OP, VS_COL, true, false>(ctx, st, a);
    return blk ? scan_t<OP, VS_COL, false, true>(ctx, st, a) : scan_t<OP, VS_COL, false, false>(ctx, st, a);
}

bool is_col_op(u32 op) { return op >= RHJ_FRAME_SUM && op <= RHJ_FRAME_MAX_I64; }
bool is_minmax(u32 op) { return op >= RHJ_FRAME_MIN_U64 && op <= RHJ_FRAME_MAX_I64; }

// what both entries ask of their flags and op lists, in this order; order_err: the entry's own complaint about d_order (null: none),
// max_nops / last_op: the entry's bounds on nops and ops[j] (both entries pass RHJ_FRAME_MAX_OPS and RHJ_FRAME_LAST_ROW, which the
// two texts name: an entry with other bounds needs its own words there)
int check_ops(rhj_ctx *ctx, const std::string &me, u32 flags, const char *order_err, u32 max_nops, u32 last_op, const u32 *ops,
              const u64 *const *d_cols, u32 nops, u64 *const *d_outs, u64 n)
{
    if (flags & ~(RHJ_SORT_I64 | RHJ_SORT_DESC)) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": unknown flags").c_str());
    if (order_err) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + order_err).c_str());
    if (nops == 0 || nops > max_nops) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": nops must be 1 .. RHJ_FRAME_MAX_OPS").c_str());
    if (!ops) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": ops is null").c_str());
    if (!d_outs) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_outs is null").c_str());
    for (u32 j = 0; j < nops; j++) {
        const std::string at = "[" + std::to_string(j) + "]";
        if (ops[j] > last_op) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": ops" + at + " is not an RHJ_FRAME_* op").c_str());
        if (!d_outs[j]) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_outs" + at + " is null").c_str());
        if (is_col_op(ops[j]) && n > 0 && (!d_cols || !d_cols[j]))
            return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_cols" + at + " is null for a column op with a non-zero row count").c_str());
    }
    return RHJ_OK;
}

int frame_run(rhj_ctx *ctx, const u64 *d_part, const u64 *d_order, u64 n, u32 flags, const u32 *ops, const u64 *preceding,
              const u64 *following, const u64 *const *d_cols, u32 nops, u64 *const *d_outs, u64 *out_partitions)
{
    const std::string me("rhj_frame_cols_dev");
    int rc = check_ops(ctx, me, flags, flags && !d_order ? ": flags without d_order: they say how the order column is read" : nullptr, RHJ_FRAME_MAX_OPS,
                       RHJ_FRAME_LAST_ROW, ops, d_cols, nops, d_outs, n);
    if (rc != RHJ_OK) return rc;
    if (out_partitions) *out_partitions = 0;
    if (n == 0) return RHJ_OK;

    hipStream_t st = rhj_internal_stream(ctx);
    u64 L;
    u32 U;
    rhj_internal_sort_units(ctx, n, &L, &U);
    if (U == 0 || U > ORD_MAX_UNITS) return rhj_internal_fail(ctx, RHJ_E_HIP, (me + ": unit geometry").c_str());   // (never: the sort's own bound)

    // 1. the plan of every op: its frame, and for MIN / MAX which scans it needs.  A side that reaches n - 1 positions reaches every
    //    partition's edge from every row: it is unbounded.  With preceding unbounded lo is the partition's start and F alone answers;
    //    else with following unbounded hi is its end and B alone does; else w = preceding + following + 1 <= 2n - 3 does not wrap,
    //    and blocks of w positions apply when w < n (with w >= n the one block needs no heads of its own)
    FrmEmit em = {};
    em.nops = nops;
    bool need_ps = false, need_pe = false;
    int scans = 0, arrays = 0;
    const unsigned eg = flat_grid(n);
    for (u32 j = 0; j < nops; j++) {
        const u64 pr = preceding ? preceding[j] : RHJ_FRAME_UNBOUNDED, fo = following ? following[j] : 0;
        em.op[j] = ops[j];
        em.prec[j] = pr;
        em.fol[j] = fo;
        em.out[j] = d_outs[j];
        need_pe |= fo != 0;
        need_ps |= pr != 0 || ops[j] == RHJ_FRAME_SUM;
        if (ops[j] == RHJ_FRAME_SUM) { scans += 1; arrays += 1; }
        if (!is_minmax(ops[j])) continue;
        em.bias[j] = (ops[j] == RHJ_FRAME_MIN_I64 || ops[j] == RHJ_FRAME_MAX_I64) ? BIAS : 0;
        if (pr >= n - 1) {
            em.mode[j] = M_FWD;
        } else if (fo >= n - 1) {
            em.mode[j] = M_BACK;
        } else {
            em.mode[j] = M_BOTH;
            const u64 w = pr + fo + 1;
            if (w < n) { em.w[j] = w; em.sgrid[j] = ((u64)eg * FLAT_THREADS) % w; }
            need_ps = true;
        }
        scans += em.mode[j] == M_BOTH ? 2 : 1;
        arrays += em.mode[j] == M_BOTH ? 2 : 1;
    }

    // 2. the workspace: the sorted words and the permutation, two arrays for the first of two sorts (then the two bounds), one array
    //    per value scan, the flag bytes, the unit tables
    const int sorts = (d_part ? 1 : 0) + (d_order ? 1 : 0);
    const size_t nb = up256((size_t)n * 8), ub = up256((size_t)U * 8);
    const bool need_ab = sorts == 2 || need_ps || need_pe;
    const size_t bytes = (need_ab ? 2 * nb : 0) + (sorts ? 2 * nb : 0) + (size_t)arrays * nb + up256((size_t)n) + 4 * ub;
    void *ws = nullptr;
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_FRAME, bytes, &ws)) != RHJ_OK) return rc;
    unsigned char *p = (unsigned char *)ws;
    u64 *bufA = nullptr, *bufB = nullptr, *skey = nullptr, *perm = nullptr;
    if (need_ab) { bufA = (u64 *)p; p += nb; bufB = (u64 *)p; p += nb; }
    if (sorts) { skey = (u64 *)p; p += nb; perm = (u64 *)p; p += nb; }
    u64 *d_arr = (u64 *)p; p += (size_t)arrays * nb;
    unsigned char *d_flags = p; p += up256((size_t)n);
    u64 *d_usum_v = (u64 *)p; p += ub;
    u32 *d_usum_f = (u32 *)p; p += ub;
    u64 *d_carry = (u64 *)p; p += ub;
    u64 *d_ucnt = (u64 *)p; p += ub;

    // 3. the order (partition, order key, input position)
    Ordered o;
    if ((rc = order_rows(ctx, st, me.c_str(), d_part, d_order, n, flags, bufA, bufB, skey, skey, perm, &o)) != RHJ_OK) return rc;

    // 4. heads
    if ((rc = launch(ctx, RHJ_K_AUX, "k_frm_heads", k_frm_heads, U, ST, st, o.sp, n, L, d_flags, d_ucnt)) != RHJ_OK) return rc;

    FrmScan a = {};
    a.flags = d_flags; a.perm = perm; a.n = n; a.L = L; a.U = U; a.usum_v = d_usum_v; a.usum_f = d_usum_f; a.carry = d_carry;

    // 5. the bounds: pstart the forward maximum scan of (head ? p : 0), pend the backward minimum scan of (tail ? p : all ones)
    if (need_ps) {
        FrmScan b = a;
        b.out = bufA;
        if ((rc = scan_t<OP_MAX, VS_POS, false, false>(ctx, st, b)) != RHJ_OK) return rc;
    }
    if (need_pe) {
        FrmScan b = a;
        b.out = bufB;
        if ((rc = scan_t<OP_MIN, VS_POS, true, false>(ctx, st, b)) != RHJ_OK) return rc;
    }

    // 6. the value scans, by position
    u64 *next = d_arr;
    for (u32 j = 0; j < nops; j++) {
        if (!is_col_op(ops[j])) continue;
        FrmScan b = a;
        b.col = d_cols[j];
        b.bias = em.bias[j];
        if (ops[j] == RHJ_FRAME_SUM) {
            b.out = next; next += nb / 8;
            em.F[j] = b.out;
            if ((rc = scan_t<OP_SUM, VS_COL, false, false>(ctx, st, b)) != RHJ_OK) return rc;
            continue;
        }
        const bool mn = ops[j] == RHJ_FRAME_MIN_U64 || ops[j] == RHJ_FRAME_MIN_I64, blk = em.w[j] != 0;
        if (blk) { b.w = em.w[j]; b.s64 = 64 % b.w; b.stile = (u64)TILE % b.w; }
        if (em.mode[j] != M_BACK) {
            b.out = next; next += nb / 8;
            em.F[j] = b.out;
            if ((rc = mn ? scan_col<OP_MIN>(ctx, st, b, false, blk) : scan_col<OP_MAX>(ctx, st, b, false, blk)) != RHJ_OK) return rc;
        }
        if (em.mode[j] != M_FWD) {
            b.out = next; next += nb / 8;
            em.B[j] = b.out;
            if ((rc = mn ? scan_col<OP_MIN>(ctx, st, b, true, blk) : scan_col<OP_MAX>(ctx, st, b, true, blk)) != RHJ_OK) return rc;
        }
    }

    // 7. every op's answer, by row
    if ((rc = launch(ctx, RHJ_K_AUX, "k_frm_emit", k_frm_emit, eg, FLAT_THREADS, st, need_ps ? bufA : nullptr, need_pe ? bufB : nullptr, perm, n, em)) != RHJ_OK)
        return rc;

    // 8. the partitions: the heads' per-unit counts, summed on the host
    u64 parts = 0;
    if ((rc = unit_total(ctx, st, me.c_str(), d_ucnt, U, &parts)) != RHJ_OK) return rc;
    if (out_partitions) *out_partitions = parts;
    rhj_internal_frame_report(ctx, (int)U, sorts, scans, parts);
    return RHJ_OK;
}

// ==== the RANGE entry (include/rhj.h, "RANGE frames") ====================================================================
// The frame of a row is a VALUE distance on the order key: every row of the partition whose order value lies in [t - preceding, t +
// following].  The order, the heads and the two bounds are frame_run's.  New: the order words by sorted position, read through ONE
// transform v (unsigned, non-decreasing along a partition in all four views), two galloping searches per row and distinct frame for
// lo / hi, and for MIN / MAX -- a frame has no fixed width here -- the scans of above at the FIXED block length 64 with a sparse table
// over the whole blocks' summaries between them.
constexpr u64 RB = 64;                           // the block length of the MIN / MAX scans
constexpr int RB_SHIFT = 6;

// ---- k_frr_level: one level of the sparse table over the block summaries ---------------------------------------------------------
// half == 0: dst[k] = F[64 k + 63], the summary of whole block k (valid where no partition head stands inside the block: the only
// ones k_frr_emit reads).  Else dst[k] = op(src[k], src[k + half]), half = 2^(l - 1): blocks k .. k + 2^l - 1.
__global__ void __launch_bounds__(FLAT_THREADS)
k_frr_level(const u64 *__restrict__ src, u64 src_n, u64 cnt, u64 half, u32 mn, u64 *__restrict__ dst)
{
    for (u64 k = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; k < cnt; k += (u64)gridDim.x * FLAT_THREADS) {
        if (half == 0) {
            const u64 at = k * RB + (RB - 1);
            dst[k] = at < src_n ? src[at] : 0;                            // (at < n always: cnt = n / 64)
            continue;
        }
        if (k + half >= src_n) continue;                                 // (never: cnt + half is the length of the level below)
        const u64 x = src[k], y = src[k + half];
        dst[k] = mn ? (y < x ? y : x) : (y > x ? y : x);
    }
}

struct FrrEmit {
    u32 nops, nframes, levels, desc;
    u64 flip;                                                         // 1 << 63 under RHJ_SORT_I64
    u64 tstride, tcnt;                                                // words between two levels of a table; the whole blocks n / 64
    u64 prec[RHJ_FRAME_MAX_OPS], fol[RHJ_FRAME_MAX_OPS];              // per distinct FRAME
    u32 op[RHJ_FRAME_MAX_OPS], mode[RHJ_FRAME_MAX_OPS], frame[RHJ_FRAME_MAX_OPS];
    u64 bias[RHJ_FRAME_MAX_OPS];
    const u64 *F[RHJ_FRAME_MAX_OPS];                                  // SUM: S
    const u64 *B[RHJ_FRAME_MAX_OPS];
    const u64 *V[RHJ_FRAME_MAX_OPS];                                  // the column by sorted position
    const u64 *T[RHJ_FRAME_MAX_OPS];                                  // M_BOTH: the table, level l at T + l * tstride
    u64 *out[RHJ_FRAME_MAX_OPS];
};

__device__ __forceinline__ u64 frr_view(u64 word, u64 flip, u32 desc)
{
    const u64 v = word ^ flip;
    return desc ? ~v : v;
}

// lo: the first position of [ps, p] whose v is >= tl (v[p] is).  Gallop away from p in doubling steps while the probe still
// qualifies, then bisect the bracket: about 2 log2(p - lo) dependent loads.  Every index stays inside [ps, p].
__device__ __forceinline__ u64 frr_search_lo(const u64 *__restrict__ vs, u64 flip, u32 desc, u64 ps, u64 p, u64 tl)
{
    u64 l = ps, b = p, step = 1;
    while (b - l >= step) {
        const u64 c = b - step;
        if (frr_view(vs[c], flip, desc) >= tl) {
            b = c;
            step <<= 1;
        } else {
            l = c + 1;
            break;
        }
    }
    while (l < b) {
        const u64 mid = l + ((b - l) >> 1);
        if (frr_view(vs[mid], flip, desc) >= tl) b = mid;
        else l = mid + 1;
    }
    return b;
}

// hi: the last position of [p, pe] whose v is <= th (v[p] is): the mirror of frr_search_lo.  Every index stays inside [p, pe].
__device__ __forceinline__ u64 frr_search_hi(const u64 *__restrict__ vs, u64 flip, u32 desc, u64 p, u64 pe, u64 th)
{
    u64 g = p, h = pe, step = 1;
    while (h - g >= step) {
        const u64 c = g + step;
        if (frr_view(vs[c], flip, desc) <= th) {
            g = c;
            step <<= 1;
        } else {
            h = c - 1;
            break;
        }
    }
    while (g < h) {
        const u64 mid = g + ((h - g + 1) >> 1);
        if (frr_view(vs[mid], flip, desc) <= th) g = mid;
        else h = mid - 1;
    }
    return g;
}

// ---- k_frr_emit: the searches and every op's answer, out[perm[p]] -----------------------------------------------------------------
// Per position: v = the order word in the transformed view; per distinct frame lo = first position with v_r >= max(0, v - preceding),
// hi = last position with v_r <= min(2^64 - 1, v + following) (an all-ones side: the partition's edge, no search).  COUNT, FIRST_ROW,
// LAST_ROW, SUM as k_frm_emit.  MIN / MAX: M_FWD F[hi], M_BACK B[lo]; M_BOTH with bl = lo / 64, bh = hi / 64 --
//   bl == bh: lo at the block's or partition's start F[hi]; hi at the block's or partition's end B[lo]; else the walk V[lo .. hi]
//   (at most 62 words);  bl < bh: op(B[lo], F[hi]), and with c = bh - bl - 1 >= 1 interior blocks, l = floor(log2 c), also
//   op(T_l[bl + 1], T_l[bh - 2^l]).  Interior blocks lie inside the frame, so inside one partition: their summaries are valid.
__global__ void __launch_bounds__(FLAT_THREADS)
k_frr_emit(const u64 *__restrict__ pstart, const u64 *__restrict__ pend, const u64 *__restrict__ perm, const u64 *__restrict__ vs, u64 n, FrrEmit e)
{
    for (u64 p = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; p < n; p += (u64)gridDim.x * FLAT_THREADS) {
        const u64 row = perm[p];
        u64 ps = pstart[p], pe = pend[p];
        if (ps > p) ps = p;                                              // (never: pstart <= p <= pend < n; the guards keep every index below inside [0, n))
        if (pe < p || pe >= n) pe = p;
        const u64 v = frr_view(vs[p], e.flip, e.desc);
        u64 lo[RHJ_FRAME_MAX_OPS], hi[RHJ_FRAME_MAX_OPS];
#pragma unroll
        for (u32 f = 0; f < RHJ_FRAME_MAX_OPS; f++) {
            lo[f] = ps;
            hi[f] = pe;
            if (f >= e.nframes) continue;
            const u64 pr = e.prec[f], fo = e.fol[f];
            if (pr != RHJ_FRAME_UNBOUNDED) lo[f] = frr_search_lo(vs, e.flip, e.desc, ps, p, v >= pr ? v - pr : 0);
            if (fo != RHJ_FRAME_UNBOUNDED) hi[f] = frr_search_hi(vs, e.flip, e.desc, p, pe, fo > ~v ? ~0ull : v + fo);
        }
#pragma unroll
        for (u32 j = 0; j < RHJ_FRAME_MAX_OPS; j++) {
            if (j >= e.nops) continue;
            const u32 fr = e.frame[j], op = e.op[j];
            u64 l = lo[0], h = hi[0];
#pragma unroll
            for (u32 f = 1; f < RHJ_FRAME_MAX_OPS; f++)
                if (fr == f) { l = lo[f]; h = hi[f]; }
            u64 val;
            if (op == RHJ_FRAME_COUNT) {
                val = h - l + 1;
            } else if (op == RHJ_FRAME_FIRST_ROW) {
                val = perm[l];
            } else if (op == RHJ_FRAME_LAST_ROW) {
                val = perm[h];
            } else if (op == RHJ_FRAME_SUM) {
                val = e.F[j][h] - (l > ps ? e.F[j][l - 1] : 0);
            } else {
                const bool mn = op == RHJ_FRAME_MIN_U64 || op == RHJ_FRAME_MIN_I64;
                const u64 *__restrict__ F = e.F[j], *__restrict__ B = e.B[j];
                if (e.mode[j] == M_FWD) {
                    val = F[h];
                } else if (e.mode[j] == M_BACK) {
                    val = B[l];
                } else {
                    const u64 bl = l >> RB_SHIFT, bh = h >> RB_SHIFT;
                    if (bl == bh) {
                        const u64 bs = bl << RB_SHIFT, be = bs + (RB - 1);
                        if (l == (bs > ps ? bs : ps)) {
                            val = F[h];
                        } else if (h == (be < pe ? be : pe)) {
                            val = B[l];
                        } else {
                            val = e.V[j][l] ^ e.bias[j];
                            for (u64 q = l + 1; q <= h; q++) {
                                const u64 y = e.V[j][q] ^ e.bias[j];
                                val = mn ? (y < val ? y : val) : (y > val ? y : val);
                            }
                        }
                    } else {
                        const u64 x = B[l], y = F[h];
                        val = mn ? (y < x ? y : x) : (y > x ? y : x);
                        const u64 c = bh - bl - 1;
                        if (c != 0) {
                            const u32 lv = 63 - (u32)__clzll((long long)c);
                            const u64 i0 = bl + 1, i1 = bh - (1ull << lv);
                            if (lv < e.levels && i1 < e.tcnt && i0 <= i1) {       // (always: the levels reach floor(log2((n - 1) / 64 - 1)))
                                const u64 *__restrict__ t = e.T[j] + (u64)lv * e.tstride;
                                const u64 x2 = t[i0], y2 = t[i1];
                                const u64 z = mn ? (y2 < x2 ? y2 : x2) : (y2 > x2 ? y2 : x2);
                                val = mn ? (z < val ? z : val) : (z > val ? z : val);
                            }
                        }
                    }
                }
                val ^= e.bias[j];
            }
            if (row < n) e.out[j][row] = val;                            // (row < n always: perm is a permutation)
        }
    }
}

// the sparse-table levels a call with a two-sided MIN / MAX builds: T_0 .. T_floor(log2 c), c = (n - 1) / 64 - 1 the most interior
// blocks a frame can hold; 0 when no frame can hold one
int range_levels(u64 n)
{
    const u64 last = (n - 1) >> RB_SHIFT;
    if (last < 2) return 0;
    int l = 0;
    while ((2ull << l) <= last - 1) l++;
    return l + 1;
}

int range_run(rhj_ctx *ctx, const u64 *d_part, const u64 *d_order, u64 n, u32 flags, const u32 *ops, const u64 *preceding,
              const u64 *following, const u64 *const *d_cols, u32 nops, u64 *const *d_outs, u64 *out_partitions)
{
    const std::string me("rhj_frame_range_cols_dev");
    int rc = check_ops(ctx, me, flags, !d_order && (n > 0 || flags) ? ": d_order is null: a value distance needs a value" : nullptr, RHJ_FRAME_MAX_OPS,
                       RHJ_FRAME_LAST_ROW, ops, d_cols, nops, d_outs, n);
    if (rc != RHJ_OK) return rc;
    if (out_partitions) *out_partitions = 0;
    if (n == 0) return RHJ_OK;

    hipStream_t st = rhj_internal_stream(ctx);
    u64 L;
    u32 U;
    rhj_internal_sort_units(ctx, n, &L, &U);
    if (U == 0 || U > ORD_MAX_UNITS) return rhj_internal_fail(ctx, RHJ_E_HIP, (me + ": unit geometry").c_str());   // (never: the sort's own bound)

    // 1. the plan: the distinct frames (one pair of searches each), the distinct columns (one gather each), and per MIN / MAX the
    //    scans: an all-ones preceding makes lo the partition's start and F alone answers, an all-ones following B alone; else both, in
    //    blocks of 64 when n > 64, and the table when a frame can hold a whole block between its two ends
    FrrEmit em = {};
    em.nops = nops;
    em.flip = (flags & RHJ_SORT_I64) ? BIAS : 0;
    em.desc = (flags & RHJ_SORT_DESC) ? 1 : 0;
    const bool blk = n > RB;
    int scans = 0, arrays = 0, nboth = 0, ncols = 0;
    const u64 *ucol[RHJ_FRAME_MAX_OPS] = {};
    u32 colof[RHJ_FRAME_MAX_OPS] = {};
    for (u32 j = 0; j < nops; j++) {
        const u64 pr = preceding ? preceding[j] : RHJ_FRAME_UNBOUNDED, fo = following ? following[j] : 0;
        u32 f = 0;
        while (f < em.nframes && (em.prec[f] != pr || em.fol[f] != fo)) f++;
        if (f == em.nframes) { em.prec[f] = pr; em.fol[f] = fo; em.nframes++; }
        em.frame[j] = f;
        em.op[j] = ops[j];
        em.out[j] = d_outs[j];
        if (!is_col_op(ops[j])) continue;
        u32 c = 0;
        while (c < (u32)ncols && ucol[c] != d_cols[j]) c++;
        if (c == (u32)ncols) ucol[ncols++] = d_cols[j];
        colof[j] = c;
        if (ops[j] == RHJ_FRAME_SUM) { scans += 1; arrays += 1; continue; }
        em.bias[j] = (ops[j] == RHJ_FRAME_MIN_I64 || ops[j] == RHJ_FRAME_MAX_I64) ? BIAS : 0;
        em.mode[j] = pr == RHJ_FRAME_UNBOUNDED ? M_FWD : fo == RHJ_FRAME_UNBOUNDED ? M_BACK : M_BOTH;
        nboth += em.mode[j] == M_BOTH;
        scans += em.mode[j] == M_BOTH ? 2 : 1;
        arrays += em.mode[j] == M_BOTH ? 2 : 1;
    }
    const int levels = nboth ? range_levels(n) : 0;
    const u64 nblk = n >> RB_SHIFT;

    // 2. the workspace: the two bounds, the sorted words and the permutation, the order words by position after two sorts, one array
    //    per distinct column and per value scan, the tables, the flag bytes, the unit tables
    const int sorts = (d_part ? 1 : 0) + 1;
    const size_t nb = up256((size_t)n * 8), ub = up256((size_t)U * 8), tb = up256((size_t)nblk * 8);
    const size_t bytes = 4 * nb + (sorts == 2 ? nb : 0) + (size_t)(ncols + arrays) * nb + (size_t)nboth * levels * tb + up256((size_t)n) + 4 * ub;
    void *ws = nullptr;
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_FRAME, bytes, &ws)) != RHJ_OK) return rc;
    unsigned char *p = (unsigned char *)ws;
    u64 *bufA = (u64 *)p; p += nb;
    u64 *bufB = (u64 *)p; p += nb;
    u64 *skey = (u64 *)p; p += nb;
    u64 *perm = (u64 *)p; p += nb;
    u64 *vs = skey;
    if (sorts == 2) { vs = (u64 *)p; p += nb; }
    u64 *d_V = (u64 *)p; p += (size_t)ncols * nb;
    u64 *d_arr = (u64 *)p; p += (size_t)arrays * nb;
    u64 *d_tab = (u64 *)p; p += (size_t)nboth * levels * tb;
    unsigned char *d_flags = p; p += up256((size_t)n);
    u64 *d_usum_v = (u64 *)p; p += ub;
    u32 *d_usum_f = (u32 *)p; p += ub;
    u64 *d_carry = (u64 *)p; p += ub;
    u64 *d_ucnt = (u64 *)p; p += ub;
    em.tstride = tb / 8;
    em.tcnt = nblk;
    em.levels = (u32)levels;

    // 3. the order (partition, order key, input position), and the order words by sorted position
    const unsigned fg = flat_grid(n);
    Ordered o;
    if ((rc = order_rows(ctx, st, me.c_str(), d_part, d_order, n, flags, bufA, bufB, skey, skey, perm, &o)) != RHJ_OK) return rc;
    if (sorts == 2 && (rc = launch(ctx, RHJ_K_AUX, "k_ord_gather", k_ord_gather<u64>, fg, FLAT_THREADS, st, d_order, perm, n, vs)) != RHJ_OK) return rc;

    // 4. heads, and the two bounds
    if ((rc = launch(ctx, RHJ_K_AUX, "k_frm_heads", k_frm_heads, U, ST, st, o.sp, n, L, d_flags, d_ucnt)) != RHJ_OK) return rc;
    FrmScan a = {};
    a.flags = d_flags; a.n = n; a.L = L; a.U = U; a.usum_v = d_usum_v; a.usum_f = d_usum_f; a.carry = d_carry;
    {
        FrmScan b = a;
        b.out = bufA;
        if ((rc = scan_t<OP_MAX, VS_POS, false, false>(ctx, st, b)) != RHJ_OK) return rc;
        b.out = bufB;
        if ((rc = scan_t<OP_MIN, VS_POS, true, false>(ctx, st, b)) != RHJ_OK) return rc;
    }

    // 5. every distinct column by sorted position: the scans below and the walk read it in place (a.perm stays null)
    for (int c = 0; c < ncols; c++) {
        if ((rc = launch(ctx, RHJ_K_AUX, "k_ord_gather", k_ord_gather<u64>, fg, FLAT_THREADS, st, ucol[c], perm, n, d_V + (size_t)c * (nb / 8))) != RHJ_OK) return rc;
    }

    // 6. the value scans, and the tables
    u64 *next = d_arr, *tnext = d_tab;
    for (u32 j = 0; j < nops; j++) {
        if (!is_col_op(ops[j])) continue;
        FrmScan b = a;
        b.col = d_V + (size_t)colof[j] * (nb / 8);
        b.bias = em.bias[j];
        em.V[j] = b.col;
        if (ops[j] == RHJ_FRAME_SUM) {
            b.out = next; next += nb / 8;
            em.F[j] = b.out;
            if ((rc = scan_t<OP_SUM, VS_COL, false, false>(ctx, st, b)) != RHJ_OK) return rc;
            continue;
        }
        const bool mn = ops[j] == RHJ_FRAME_MIN_U64 || ops[j] == RHJ_FRAME_MIN_I64, both = em.mode[j] == M_BOTH, bk = both && blk;
        if (bk) { b.w = RB; b.s64 = 0; b.stile = (u64)TILE % RB; }
        if (em.mode[j] != M_BACK) {
            b.out = next; next += nb / 8;
            em.F[j] = b.out;
            if ((rc = mn ? scan_col<OP_MIN>(ctx, st, b, false, bk) : scan_col<OP_MAX>(ctx, st, b, false, bk)) != RHJ_OK) return rc;
        }
        if (em.mode[j] != M_FWD) {
            b.out = next; next += nb / 8;
            em.B[j] = b.out;
            if ((rc = mn ? scan_col<OP_MIN>(ctx, st, b, true, bk) : scan_col<OP_MAX>(ctx, st, b, true, bk)) != RHJ_OK) return rc;
        }
        if (!both || levels == 0) continue;
        em.T[j] = tnext;
        for (int l = 0; l < levels; l++) {
            const u64 half = l ? 1ull << (l - 1) : 0, cnt = nblk - (1ull << l) + 1;
            const u64 *src = l ? tnext + (size_t)(l - 1) * em.tstride : em.F[j];
            const u64 src_n = l ? nblk - half + 1 : n;
            if ((rc = launch(ctx, RHJ_K_TASKS, "k_frr_level", k_frr_level, flat_grid(cnt), FLAT_THREADS, st, src, src_n, cnt, half, (u32)(mn ? 1 : 0),
                             tnext + (size_t)l * em.tstride)) != RHJ_OK)
                return rc;
        }
        tnext += (size_t)levels * em.tstride;
    }

    // 7. the searches and every op's answer, by row
    if ((rc = launch(ctx, RHJ_K_JOIN, "k_frr_emit", k_frr_emit, fg, FLAT_THREADS, st, bufA, bufB, perm, vs, n, em)) != RHJ_OK) return rc;

    // 8. the partitions: the heads' per-unit counts, summed on the host
    u64 parts = 0;
    if ((rc = unit_total(ctx, st, me.c_str(), d_ucnt, U, &parts)) != RHJ_OK) return rc;
    if (out_partitions) *out_partitions = parts;
    rhj_internal_frame_range_report(ctx, (int)U, sorts, scans, levels, parts);
    return RHJ_OK;
}

}  // namespace

extern "C" {

int rhj_frame_range_cols_dev(rhj_ctx *ctx, const uint64_t *d_part, const uint64_t *d_order, uint64_t n, uint32_t flags,
                             const uint32_t *ops, const uint64_t *preceding, const uint64_t *following,
                             const uint64_t *const *d_cols, uint32_t nops, uint64_t *const *d_outs, uint64_t *out_partitions)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    return range_run(ctx, (const u64 *)d_part, (const u64 *)d_order, n, flags, ops, (const u64 *)preceding, (const u64 *)following,
                     (const u64 *const *)d_cols, nops, (u64 *const *)d_outs, (u64 *)out_partitions);
}

int rhj_frame_cols_dev(rhj_ctx *ctx, const uint64_t *d_part, const uint64_t *d_order, uint64_t n, uint32_t flags,
                       const uint32_t *ops, const uint64_t *preceding, const uint64_t *following,
                       const uint64_t *const *d_cols, uint32_t nops, uint64_t *const *d_outs, uint64_t *out_partitions)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    return frame_run(ctx, (const u64 *)d_part, (const u64 *)d_order, n, flags, ops, (const u64 *)preceding, (const u64 *)following,
                     (const u64 *const *)d_cols, nops, (u64 *const *)d_outs, (u64 *)out_partitions);
}

}  // extern "C"
