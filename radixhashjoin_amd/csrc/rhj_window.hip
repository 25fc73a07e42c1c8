// rhj_window.hip -- the window entry (include/rhj.h, "window functions"): a value per row from the rows before it in its
// partition -- ROW_NUMBER / RANK / DENSE_RANK, LAG / LEAD rows, running SUM / MIN / MAX.  The order (partition, order key, input
// position) comes from the stable sort of rhj_sort.hip, reached through rhj_internal_sort_run; what is new here is the scan over
// that order which restarts at every partition head.  Per scan three launches ordered on the context's stream -- a reduce per unit,
// a one-workgroup carry over the unit summaries, an apply per unit -- on the sort's unit geometry.  No workgroup ever waits on
// another, and no position or value comes from an atomic.
#include "rhj_ordered.h"

namespace {

constexpr int TILE = WINDOW_TILE;
constexpr u32 F_PART = 1, F_PEER = 2;            // the flag byte of a sorted position: it heads a partition / a run of peers
static_assert(TILE == SORT_TILE, "k_win_reduce's and k_win_apply's geometry is the sort's (rhj_ordered.h)");

// The scans fold rhj_ordered.h's (f, v) algebra; what makes v:
enum { VS_COL = 0, VS_PEER = 1, VS_POS = 2 };    // the value: a column word through the permutation; the peer-head bit; head ? position : 0

struct WinScan {
    const unsigned char *flags;                  // n flag bytes, by sorted position
    const u64 *perm;                             // perm[p] = the row at sorted position p; null: the identity
    const u64 *col;                              // VS_COL: the caller's column, by row
    u64 *out;                                    // by row (through perm)
    u64 n, L;
    u32 U;
    u32 hbit, vbit;                              // the flag bit at which the scan restarts; VS_PEER / VS_POS: the bit that makes the value
    u64 bias;                                    // VS_COL: 1 << 63 for the signed minimum / maximum, on the way in and out
    u64 *usum_v;                                 // per unit: the aggregate since the unit's last head (the whole unit without one)
    u32 *usum_f;                                 // ... and whether it has a head
    u64 *carry;                                  // per unit: the aggregate since the last head before the unit
};

template <int OP, int VS> __device__ __forceinline__ u64 win_value(const WinScan &a, u64 p, u32 fl, u64 row)
{
    if (VS == VS_COL) return row < a.n ? a.col[row] ^ a.bias : ident<OP>();
    if (VS == VS_PEER) return (fl & a.vbit) ? 1 : 0;
    return (fl & a.vbit) ? p : 0;
}

// ---- k_win_heads: the flag byte of every sorted position, and the partition heads per unit -----------------------------------------
// A position heads a partition when its sorted partition word differs from its predecessor's (position 0 always does), and a run of
// peers when it heads a partition or its order word differs -- without an order column every row is its own peer.  The order word
// comes from the sorted column (one inner sort) or through the permutation (two).  Each lane takes its predecessor's words from the
// lane below; lane 0 loads them.
__global__ void __launch_bounds__(ST)
k_win_heads(const u64 *__restrict__ sp, const u64 *__restrict__ so, const u64 *__restrict__ ord, const u64 *__restrict__ perm, u64 n, u64 L,
            unsigned char *__restrict__ flags, u64 *__restrict__ ucnt)
{
    __shared__ u64 ws[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, u = blockIdx.x;
    const u64 beg = (u64)u * L, end = beg + L < n ? beg + L : n;
    const bool ordered = so || ord;
    u64 cnt = 0;
    for (u64 p0 = beg; p0 < end; p0 += ST) {
        const u64 p = p0 + tid;
        const bool valid = p < end;
        u64 cp = 0, co = 0;
        if (valid) {
            if (sp) cp = sp[p];
            if (so) co = so[p];
            else if (ord) { const u64 r = perm[p]; co = r < n ? ord[r] : 0; }
        }
        u64 pp = __shfl_up(cp, 1, 64), po = __shfl_up(co, 1, 64);
        if (valid && lane == 0 && p > 0) {
            if (sp) pp = sp[p - 1];
            if (so) po = so[p - 1];
            else if (ord) { const u64 r = perm[p - 1]; po = r < n ? ord[r] : 0; }
        }
        if (valid) {
            const bool ph = p == 0 || (sp && cp != pp);
            const bool qh = ph || !ordered || co != po;
            flags[p] = (unsigned char)((ph ? F_PART : 0) | (qh ? F_PEER : 0));
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

// ---- k_win_reduce<OP, VS>: per unit "has a head" and the aggregate since the unit's last head -------------------------------------
// One workgroup per unit.  Wave w walks the w-th eighth of the unit (L is a whole number of tiles, so an eighth is a whole number of
// rounds) 64 positions at a time, RED_UNROLL rounds of loads in flight.  A round with a head keeps only the lanes from its last head
// on and replaces the wave's running aggregate; one without adds to it.  The eight wave summaries are folded in order.
template <int OP, int VS>
__global__ void __launch_bounds__(ST)
k_win_reduce(WinScan a)
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
    u64 rv = ident<OP>();
    for (u64 p0 = wb; p0 < we; p0 += 64 * RED_UNROLL) {
        u32 fl[RED_UNROLL];
        u64 v[RED_UNROLL];
#pragma unroll
        for (int j = 0; j < RED_UNROLL; j++) {
            const u64 p = p0 + (u64)j * 64 + lane;
            fl[j] = 0;
            v[j] = ident<OP>();
            if (p < we) {
                fl[j] = a.flags[p];
                const u64 row = VS == VS_COL ? (a.perm ? a.perm[p] : p) : 0;
                v[j] = win_value<OP, VS>(a, p, fl[j], row);
            }
        }
#pragma unroll
        for (int j = 0; j < RED_UNROLL; j++) {
            const u64 hb = __ballot((fl[j] & a.hbit) != 0);
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

// ---- k_win_apply<OP, VS>: the scan itself, and out[perm[p]] ------------------------------------------------------------------------
// One workgroup per unit, tile by tile, in the sort's position order (wave, round, lane): wave w of a tile owns positions [w * 64 *
// TPT, (w + 1) * 64 * TPT) of it.  Per round a wave scan, continued from the wave's running aggregate (lane 63 of the round before);
// per tile the waves' totals through LDS, folded onto the tile's carry-in -- the unit's from k_ord_carry, then the running one.  A
// position behind a head of its own wave is final after the wave's rounds; any other takes the fold of the carry and the waves before.
template <int OP, int VS>
__global__ void __launch_bounds__(ST)
k_win_apply(WinScan a)
{
    __shared__ u64 wv[NW];
    __shared__ u32 wf[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const u64 beg = (u64)u * a.L, end = beg + a.L < a.n ? beg + a.L : a.n;
    u64 cv = a.carry[u];
    for (u64 tb = beg; tb < end; tb += TILE) {
        const u32 tn = end - tb < (u64)TILE ? (u32)(end - tb) : (u32)TILE;
        u64 v[TPT], row[TPT];
        u32 hd = 0;                                                      // one bit per round: a head at or before this position, in its wave's part
#pragma unroll
        for (int r = 0; r < TPT; r++) {
            const u32 li = wave * (64 * TPT) + r * 64 + lane;
            const u64 p = tb + li;
            v[r] = ident<OP>();
            row[r] = ~0ull;
            if (li < tn) {
                const u32 fl = a.flags[p];
                row[r] = a.perm ? a.perm[p] : p;
                hd |= ((fl & a.hbit) ? 1u : 0u) << r;
                v[r] = win_value<OP, VS>(a, p, fl, row[r]);
            }
        }
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
            if (wave * (64 * TPT) + r * 64 + lane >= tn || row[r] >= a.n) continue;     // (row < n always: perm is a permutation)
            const u64 res = ((hd >> r) & 1) ? v[r] : comb<OP>(pre, v[r]);
            a.out[row[r]] = VS == VS_COL ? res ^ a.bias : res;
        }
        cv = tot;
        __syncthreads();
    }
}

// ---- k_win_rows: ROW_NUMBER, RANK, LAG_ROW and LEAD_ROW from the two starts ----------------------------------------------------------
// pstart[p] / qstart[p]: the sorted position at which p's partition / p's run of peers starts.  q = p - pstart[p] is the position in
// the partition; a start names its partition, so position p + off lies in p's partition exactly when its start is p's.
struct WinRows {
    u32 nops;
    u32 op[RHJ_WINDOW_MAX_OPS];
    u64 off[RHJ_WINDOW_MAX_OPS];
    u64 *out[RHJ_WINDOW_MAX_OPS];
};

__global__ void __launch_bounds__(FLAT_THREADS)
k_win_rows(const u64 *__restrict__ pstart, const u64 *__restrict__ qstart, const u64 *__restrict__ perm, u64 n, WinRows w)
{
    for (u64 p = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; p < n; p += (u64)gridDim.x * FLAT_THREADS) {
        const u64 ps = pstart[p], row = perm ? perm[p] : p;
        if (row >= n) continue;                                          // (never: perm is a permutation)
#pragma unroll
        for (u32 j = 0; j < RHJ_WINDOW_MAX_OPS; j++) {
            if (j >= w.nops) break;
            const u64 off = w.off[j];
            u64 val;
            if (w.op[j] == RHJ_WIN_ROW_NUMBER) {
                val = p - ps + 1;
            } else if (w.op[j] == RHJ_WIN_RANK) {
                val = qstart[p] - ps + 1;
            } else if (w.op[j] == RHJ_WIN_LAG_ROW) {
                val = RHJ_NO_ROW;
                if (off <= p - ps) val = perm ? perm[p - off] : p - off;
            } else {
                val = RHJ_NO_ROW;
                if (off < n - p && pstart[p + off] == ps) val = perm ? perm[p + off] : p + off;
            }
            w.out[j][row] = val;
        }
    }
}

// one scan: reduce, carry, apply, ordered by the stream
template <int OP, int VS>
int scan_t(rhj_ctx *ctx, hipStream_t st, const WinScan &a)
{
    int rc;
    if ((rc = launch(ctx, RHJ_K_HIST, "k_win_reduce", k_win_reduce<OP, VS>, a.U, ST, st, a)) != RHJ_OK) return rc;
    if ((rc = launch(ctx, RHJ_K_SCAN, "k_ord_carry", k_ord_carry<OP>, 1, ST, st, a.usum_v, a.usum_f, a.U, a.carry)) != RHJ_OK) return rc;
    return launch(ctx, RHJ_K_SCATTER, "k_win_apply", k_win_apply<OP, VS>, a.U, ST, st, a);
}

bool is_row_op(u32 op) { return op == RHJ_WIN_ROW_NUMBER || op == RHJ_WIN_RANK || op == RHJ_WIN_LAG_ROW || op == RHJ_WIN_LEAD_ROW; }
bool is_col_op(u32 op) { return op >= RHJ_WIN_CUMSUM && op <= RHJ_WIN_CUMMAX_I64; }

int window_run(rhj_ctx *ctx, const u64 *d_part, const u64 *d_order, u64 n, u32 flags, const u32 *ops, const u64 *args,
               const u64 *const *d_cols, u32 nops, u64 *const *d_outs, u64 *out_partitions)
{
    const std::string me("rhj_window_cols_dev");
    if (flags & ~(RHJ_SORT_I64 | RHJ_SORT_DESC)) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": unknown flags").c_str());
    if (flags && !d_order) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": flags without d_order: they say how the order column is read").c_str());
    if (nops == 0 || nops > RHJ_WINDOW_MAX_OPS) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": nops must be 1 .. RHJ_WINDOW_MAX_OPS").c_str());
    if (!ops) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": ops is null").c_str());
    if (!d_outs) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_outs is null").c_str());
    bool any_row = false, any_rank = false;
    for (u32 j = 0; j < nops; j++) {
        const std::string at = "[" + std::to_string(j) + "]";
        if (ops[j] > RHJ_WIN_CUMMAX_I64) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": ops" + at + " is not an RHJ_WIN_* op").c_str());
        if ((ops[j] == RHJ_WIN_LAG_ROW || ops[j] == RHJ_WIN_LEAD_ROW) && args && args[j] == 0)
            return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": args" + at + ": a lag / lead offset must be >= 1").c_str());
        if (!d_outs[j]) return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_outs" + at + " is null").c_str());
        if (is_col_op(ops[j]) && n > 0 && (!d_cols || !d_cols[j]))
            return rhj_internal_fail(ctx, RHJ_E_INVALID, (me + ": d_cols" + at + " is null for a column op with a non-zero row count").c_str());
        any_row |= is_row_op(ops[j]);
        any_rank |= ops[j] == RHJ_WIN_RANK;
    }
    if (out_partitions) *out_partitions = 0;
    if (n == 0) return RHJ_OK;

    hipStream_t st = rhj_internal_stream(ctx);
    int rc;
    u64 L;
    u32 U;
    rhj_internal_sort_units(ctx, n, &L, &U);
    if (U == 0 || U > ORD_MAX_UNITS) return rhj_internal_fail(ctx, RHJ_E_HIP, (me + ": unit geometry").c_str());   // (never: the sort's own bound)

    // 1. the workspace: four n-word arrays at most, the flag bytes, the unit tables
    const int sorts = (d_part ? 1 : 0) + (d_order ? 1 : 0);
    const size_t nb = up256((size_t)n * 8), ub = up256((size_t)U * 8);
    const bool need_ab = sorts == 2 || any_row;                          // A, B: the first sort's outputs, then the two starts
    const size_t bytes = (need_ab ? 2 * nb : 0) + (sorts ? 2 * nb : 0) + up256((size_t)n) + 4 * ub;
    void *ws = nullptr;
    if ((rc = rhj_internal_workspace(ctx, RHJ_WS_WINDOW, bytes, &ws)) != RHJ_OK) return rc;
    unsigned char *p = (unsigned char *)ws;
    u64 *bufA = nullptr, *bufB = nullptr, *skey = nullptr, *perm = nullptr;
    if (need_ab) { bufA = (u64 *)p; p += nb; bufB = (u64 *)p; p += nb; }
    if (sorts) { skey = (u64 *)p; p += nb; perm = (u64 *)p; p += nb; }
    unsigned char *d_flags = p; p += up256((size_t)n);
    u64 *d_usum_v = (u64 *)p; p += ub;
    u32 *d_usum_f = (u32 *)p; p += ub;
    u64 *d_carry = (u64 *)p; p += ub;
    u64 *d_ucnt = (u64 *)p; p += ub;

    // 2. the order (partition, order key, input position); after two sorts the order words are read through the permutation
    Ordered o;
    if ((rc = order_rows(ctx, st, me.c_str(), d_part, d_order, n, flags, bufA, bufB, skey, skey, perm, &o)) != RHJ_OK) return rc;
    const u64 *ord = sorts == 2 ? d_order : nullptr;

    // 3. heads
    if ((rc = launch(ctx, RHJ_K_AUX, "k_win_heads", k_win_heads, U, ST, st, o.sp, o.so, ord, perm, n, L, d_flags, d_ucnt)) != RHJ_OK) return rc;

    WinScan a = {};
    a.flags = d_flags; a.perm = perm; a.n = n; a.L = L; a.U = U; a.usum_v = d_usum_v; a.usum_f = d_usum_f; a.carry = d_carry;

    // 4. the two starts, once per call, and the ops that follow from them in one launch
    if (any_row) {
        WinScan b = a;
        b.perm = nullptr; b.hbit = b.vbit = F_PART; b.out = bufA;
        if ((rc = scan_t<OP_MAX, VS_POS>(ctx, st, b)) != RHJ_OK) return rc;
        if (any_rank) {
            b.hbit = b.vbit = F_PEER; b.out = bufB;
            if ((rc = scan_t<OP_MAX, VS_POS>(ctx, st, b)) != RHJ_OK) return rc;
        }
        WinRows w = {};
        for (u32 j = 0; j < nops; j++) {
            if (!is_row_op(ops[j])) continue;
            w.op[w.nops] = ops[j];
            w.off[w.nops] = args ? args[j] : 1;
            w.out[w.nops] = d_outs[j];
            w.nops++;
        }
        if ((rc = launch(ctx, RHJ_K_AUX, "k_win_rows", k_win_rows, flat_grid(n), FLAT_THREADS, st, bufA, bufB, perm, n, w)) != RHJ_OK) return rc;
    }

    // 5. one scan per remaining op
    for (u32 j = 0; j < nops; j++) {
        if (is_row_op(ops[j])) continue;
        WinScan b = a;
        b.out = d_outs[j];
        b.hbit = F_PART;
        if (ops[j] == RHJ_WIN_DENSE_RANK) {
            b.vbit = F_PEER;
            rc = scan_t<OP_SUM, VS_PEER>(ctx, st, b);
        } else {
            b.col = d_cols[j];
            b.bias = (ops[j] == RHJ_WIN_CUMMIN_I64 || ops[j] == RHJ_WIN_CUMMAX_I64) ? BIAS : 0;
            if (ops[j] == RHJ_WIN_CUMSUM) rc = scan_t<OP_SUM, VS_COL>(ctx, st, b);
            else if (ops[j] == RHJ_WIN_CUMMIN_U64 || ops[j] == RHJ_WIN_CUMMIN_I64) rc = scan_t<OP_MIN, VS_COL>(ctx, st, b);
            else rc = scan_t<OP_MAX, VS_COL>(ctx, st, b);
        }
        if (rc != RHJ_OK) return rc;
    }

    // 6. the partitions: the heads' per-unit counts, summed on the host
    u64 parts = 0;
    if ((rc = unit_total(ctx, st, me.c_str(), d_ucnt, U, &parts)) != RHJ_OK) return rc;
    if (out_partitions) *out_partitions = parts;
    rhj_internal_window_report(ctx, (int)U, sorts, parts);
    return RHJ_OK;
}

}  // namespace

extern "C" {

int rhj_window_cols_dev(rhj_ctx *ctx, const uint64_t *d_part, const uint64_t *d_order, uint64_t n, uint32_t flags,
                        const uint32_t *ops, const uint64_t *args, const uint64_t *const *d_cols, uint32_t nops,
                        uint64_t *const *d_outs, uint64_t *out_partitions)
{
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    rhj_internal_sort_begin(ctx);
    return window_run(ctx, (const u64 *)d_part, (const u64 *)d_order, n, flags, ops, (const u64 *)args, (const u64 *const *)d_cols, nops, (u64 *const *)d_outs,
                      (u64 *)out_partitions);
}

}  // extern "C"
