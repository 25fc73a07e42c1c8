// rhj_ordered.h -- what the sort-based operators share (rhj_sort.hip, rhj_window.hip, rhj_asof.hip, rhj_frame.hip, rhj_range.hip;
// DESIGN 4.25 .. 4.31): the unit and tile geometry, the host helpers around a launch, the algebra of a scan that restarts at heads
// with its one-workgroup carry kernel, the gather kernel, the order step (partition, order key, input position) over
// rhj_internal_sort_run, and the read-back of per-unit counts.  Only those five files include it; each is its own code object, and
// everything here is a template or lives in the anonymous namespace.  What an operator loads and stores per row -- its reduce, apply,
// heads, concat, search, emit and expand kernels and their argument structs -- stays in its own file.
#pragma once
#include "../../include/rhj.h"
#include "rhj_internal.h"

#include <string>
#include <vector>

namespace {

constexpr u64 BIAS = 1ull << 63;
constexpr int ST = SORT_THREADS, TPT = SORT_TPT, NW = ST / 64;
constexpr u32 ORD_MAX_UNITS = 2048;              // the sort's: what one carry workgroup scans
constexpr int RED_UNROLL = 4;
constexpr int FLAT_THREADS = 256;
constexpr u32 FLAT_MAX_GRID = 4096;
static_assert(SORT_TILE == ST * TPT && ST % 64 == 0 && SORT_TILE % (NW * 64 * RED_UNROLL) == 0, "the reduce and apply kernels' geometry");
static_assert(TPT <= 32, "the apply kernels keep one bit per round in a u32");

// ---- the host helpers --------------------------------------------------------------------------------------------------------------
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

// one launch inside a profiling span of `kind` (RHJ_K_*); the last error is read after the span has closed, under the name `what`
template <typename K, typename... A>
int launch(rhj_ctx *ctx, int kind, const char *what, K kernel, unsigned grid, unsigned block, hipStream_t st, A... args)
{
    {
        Span s(ctx, kind);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, args...);
    }
    return check(ctx, what);
}

// ---- the scan's algebra ------------------------------------------------------------------------------------------------------------
// An element is (f, v): f -- a head stands here, v -- its value.  (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2), the later
// element on the right, + the op.  It is associative wherever the heads stand, so the aggregate "since the last head" of a range is
// the fold of its pieces in order, whatever the pieces: lanes, rounds, waves, tiles, units.
enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2 };

template <int OP> __device__ __forceinline__ u64 ident() { return OP == OP_MIN ? ~0ull : 0ull; }
template <int OP> __device__ __forceinline__ u64 comb(u64 a, u64 b)
{
    return OP == OP_SUM ? a + b : OP == OP_MIN ? (b < a ? b : a) : (b > a ? b : a);
}

// inclusive scan of (f, v) over the wave's lanes: __shfl_up with the head flag carried along
template <int OP> __device__ __forceinline__ void wave_seg_scan(u32 &f, u64 &v, u32 lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 ov = __shfl_up(v, off, 64);
        const u32 of = __shfl_up(f, off, 64);
        if (lane >= (u32)off) {
            v = f ? v : comb<OP>(ov, v);
            f |= of;
        }
    }
}

// ---- k_ord_carry<OP>: one workgroup -- the exclusive scan of at most ORD_MAX_UNITS unit summaries -----------------------------------
// Thread t folds its run of ceil(U / 512) consecutive units, the runs are scanned over the workgroup (wave scan, per-wave totals
// through LDS: block_excl_scan's shape with the flag carried along), and the thread walks its run again from its carry-in.
template <int OP>
__global__ void __launch_bounds__(ST)
k_ord_carry(const u64 *__restrict__ usum_v, const u32 *__restrict__ usum_f, u32 U, u64 *__restrict__ carry)
{
    __shared__ u64 wv[NW];
    __shared__ u32 wf[NW];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 per = (U + ST - 1) / ST;
    const u32 b = tid * per < U ? tid * per : U, e = b + per < U ? b + per : U;
    u32 sf = 0;
    u64 sv = ident<OP>();
    for (u32 u = b; u < e; u++) {
        const u32 fu = usum_f[u];
        const u64 vu = usum_v[u];
        sv = fu ? vu : comb<OP>(sv, vu);
        sf |= fu;
    }
    wave_seg_scan<OP>(sf, sv, lane);
    if (lane == 63) { wv[wave] = sv; wf[wave] = sf; }
    __syncthreads();
    u64 pv = ident<OP>();
#pragma unroll
    for (int w = 0; w < NW; w++)
        if ((u32)w < wave) pv = wf[w] ? wv[w] : comb<OP>(pv, wv[w]);
    u64 ev = __shfl_up(sv, 1, 64);
    u32 ef = __shfl_up(sf, 1, 64);
    if (lane == 0) { ev = ident<OP>(); ef = 0; }
    u64 cur = ef ? ev : comb<OP>(pv, ev);
    for (u32 u = b; u < e; u++) {
        carry[u] = cur;
        const u32 fu = usum_f[u];
        const u64 vu = usum_v[u];
        cur = fu ? vu : comb<OP>(cur, vu);
    }
}

// ---- k_ord_gather<W>: dst[i] = src[idx[i]] -- a column of words W in the order of a permutation --------------------------------------
// (a template, so that only a file that gathers carries it in its code object: rhj_sort.hip does not)
template <typename W>
__global__ void __launch_bounds__(FLAT_THREADS)
k_ord_gather(const W *__restrict__ src, const u64 *__restrict__ idx, u64 n, W *__restrict__ dst)
{
    for (u64 i = (u64)blockIdx.x * FLAT_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * FLAT_THREADS) {
        const u64 r = idx[i];
        dst[i] = r < n ? src[r] : 0;                                  // (r < n always: idx is a permutation of 0 .. n - 1)
    }
}

// ---- the order step: (part, order, input position) ------------------------------------------------------------------------------------
// The order column argsorted under flags, then the partition column gathered through that permutation (bufA -> bufB) and stable-sorted
// with the permutation as its rows; one column alone is sorted as it stands, neither leaves perm untouched.  The sorted partition
// words land in spart; sorder takes the sorted order words where the order column is sorted alone (null: not wanted; after two sorts
// they exist only through perm).  "last.sort_*" speak of the sort entries only, so they are zeroed behind the inner sorts.
struct Ordered {
    const u64 *sp, *so;                          // the sorted partition words, the sorted order words: null where the step has none
};

// (A template on the columns' word type, u64 at every call, for the reason k_ord_gather is one: a file that does not order rows this
// way -- rhj_sort.hip -- instantiates neither.)
template <typename W>
int order_rows(rhj_ctx *ctx, hipStream_t st, const char *who, const W *part, const W *order, u64 n, u32 flags, u64 *bufA, u64 *bufB,
               u64 *spart, u64 *sorder, u64 *perm, Ordered *o)
{
    int rc;
    o->sp = o->so = nullptr;
    if (part && order) {
        if ((rc = rhj_internal_sort_run(ctx, who, order, nullptr, n, flags, nullptr, bufA)) != RHJ_OK) return rc;
        if ((rc = launch(ctx, RHJ_K_AUX, "k_ord_gather", k_ord_gather<W>, flat_grid(n), FLAT_THREADS, st, part, bufA, n, bufB)) != RHJ_OK) return rc;
        if ((rc = rhj_internal_sort_run(ctx, who, bufB, bufA, n, 0, spart, perm)) != RHJ_OK) return rc;
        o->sp = spart;
    } else if (part) {
        if ((rc = rhj_internal_sort_run(ctx, who, part, nullptr, n, 0, spart, perm)) != RHJ_OK) return rc;
        o->sp = spart;
    } else if (order) {
        if ((rc = rhj_internal_sort_run(ctx, who, order, nullptr, n, flags, sorder, perm)) != RHJ_OK) return rc;
        o->so = sorder;
    }
    rhj_internal_sort_report(ctx, 0, 0, 0);
    return RHJ_OK;
}

// the U per-unit counts a kernel left at d_ucnt, read back and summed on the host; `who` is the entry in the error text
int unit_total(rhj_ctx *ctx, hipStream_t st, const char *who, const u64 *d_ucnt, u32 U, u64 *total)
{
    std::vector<u64> cnt(U);
    hipError_t e = hipMemcpyAsync(cnt.data(), d_ucnt, (size_t)U * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(ctx, who, e);
    *total = 0;
    for (u32 u = 0; u < U; u++) *total += cnt[u];
    return RHJ_OK;
}

}  // namespace
