// rhj_keys.hip -- composite keys (include/rhj.h, "composite keys"): up to four key columns per relation packed into
// one exact 64-bit surrogate key column, and back.  Three streaming kernels (range probe, pack, unpack) and the host rule that
// chooses a layout; the dense ids of a column that does not fit come from the engine's own group-by with ids.
#include "../../include/rhj.h"
#include "rhj_internal.h"

#include <string>
#include <vector>

static_assert(RHJ_KEYS_MAX_COLS == 4 && RHJ_KEYS_MAX_FOLDS == 2 && RHJ_KEYS_FOLD0 == RHJ_KEYS_MAX_COLS, "the fold shapes below");

// the plan: the layout, and what the layout's fields need to be read back
struct rhj_keyplan {
    rhj_keys_layout_t lay;
    u64 *dict[RHJ_KEYS_MAX_COLS] = {};          // DICT column j: dict_size[j] words in HBM (null: packed with RHJ_KEYS_NO_UNPACK)
    u64 *fold_dict[RHJ_KEYS_MAX_FOLDS] = {};    // fold f: fold_size[f] packed words of its two inputs
    bool no_unpack = false;
};

namespace {

constexpr u64 BIAS = 1ull << 63;
constexpr int KEYS_THREADS = 256;
constexpr u32 KEYS_MAX_GRID = 2048;

// ---- k_keys_range: per column, over both sides, min / max of v and of v ^ BIAS ------------------------------------------------
// blockIdx.y = 2 * column + side.  Two rows per lane by 16-byte loads over the 16-byte aligned body of the column; its at most two
// odd words (a misaligned first, a last) are lane 0 of block 0's.  A wave reduces, then issues four 64-bit atomics into the
// column's four words {min v, max v, min v ^ BIAS, max v ^ BIAS} (set to {~0, 0, ~0, 0} by the host).
struct RangeArgs { const u64 *col[2 * RHJ_KEYS_MAX_COLS]; u64 n[2 * RHJ_KEYS_MAX_COLS]; };

struct MinMax4 {
    u64 lo = ~0ull, hi = 0, blo = ~0ull, bhi = 0;
    __device__ __forceinline__ void take(u64 v)
    {
        const u64 b = v ^ BIAS;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        blo = b < blo ? b : blo;
        bhi = b > bhi ? b : bhi;
    }
};

__global__ void __launch_bounds__(KEYS_THREADS)
k_keys_range(RangeArgs a, u64 *__restrict__ mm)
{
    const u32 y = blockIdx.y;
    const u64 *__restrict__ p = a.col[y];
    const u64 n = a.n[y];
    if (n == 0) return;
    const u64 head = ((uintptr_t)p & 8) ? 1 : 0;
    const ulonglong2 *__restrict__ p2 = (const ulonglong2 *)(p + head);
    const u64 n2 = (n - head) / 2;
    MinMax4 m;
    for (u64 i = (u64)blockIdx.x * KEYS_THREADS + threadIdx.x; i < n2; i += (u64)gridDim.x * KEYS_THREADS) {
        const ulonglong2 v = p2[i];
        m.take(v.x);
        m.take(v.y);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head) m.take(p[0]);
        if ((n - head) & 1) m.take(p[n - 1]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 lo = __shfl_xor(m.lo, off, 64), hi = __shfl_xor(m.hi, off, 64);
        const u64 blo = __shfl_xor(m.blo, off, 64), bhi = __shfl_xor(m.bhi, off, 64);
        m.lo = lo < m.lo ? lo : m.lo;
        m.hi = hi > m.hi ? hi : m.hi;
        m.blo = blo < m.blo ? blo : m.blo;
        m.bhi = bhi > m.bhi ? bhi : m.bhi;
    }
    if ((threadIdx.x & 63) == 0 && m.lo <= m.hi) {           // (a wave that saw no row has nothing to say)
        // The four words only ever move one way, so a plain load -- however stale -- that already holds a value as good as this
        // wave's means the atomic would change nothing: after the first waves nearly every wave skips all four, and thousands of
        // waves do not queue up on one address (DESIGN 4.21 has the pack's time with every atomic issued and with this check).
        unsigned long long *w = (unsigned long long *)mm + 4 * (y >> 1);
        const volatile unsigned long long *seen = w;
        if (m.lo < seen[0]) atomicMin(w + 0, (unsigned long long)m.lo);
        if (m.hi > seen[1]) atomicMax(w + 1, (unsigned long long)m.hi);
        if (m.blo < seen[2]) atomicMin(w + 2, (unsigned long long)m.blo);
        if (m.bhi > seen[3]) atomicMax(w + 3, (unsigned long long)m.bhi);
    }
}

// ---- k_keys_pack<K>: out[i] = OR over k < K of (src[k][i] - base[k]) << shift[k] ------------------------------------------------
// One pass, (K + 1) * 8 bytes per row, no LDS.  src[k] is the caller's column (base: the probe's) or an id array (base 0); every
// term is below 2^width of its field by construction, so nothing is masked.  VEC: every pointer is 16-byte aligned -- two rows
// per lane by 16-byte loads and one 16-byte store; otherwise the same two rows by 8-byte accesses.  An odd last row: block 0's.
struct PackArgs { const u64 *src[RHJ_KEYS_MAX_COLS]; u64 base[RHJ_KEYS_MAX_COLS]; u32 shift[RHJ_KEYS_MAX_COLS]; };

template <int K, bool VEC>
__global__ void __launch_bounds__(KEYS_THREADS)
k_keys_pack(PackArgs a, u64 *__restrict__ out, u64 n)
{
    const u64 n2 = n / 2;
    for (u64 i = (u64)blockIdx.x * KEYS_THREADS + threadIdx.x; i < n2; i += (u64)gridDim.x * KEYS_THREADS) {
        u64 w0 = 0, w1 = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            u64 x, y;
            if (VEC) {
                const ulonglong2 v = ((const ulonglong2 *)a.src[k])[i];
                x = v.x;
                y = v.y;
            } else {
                x = a.src[k][2 * i];
                y = a.src[k][2 * i + 1];
            }
            w0 |= (x - a.base[k]) << a.shift[k];
            w1 |= (y - a.base[k]) << a.shift[k];
        }
        if (VEC) {
            ((ulonglong2 *)out)[i] = make_ulonglong2(w0, w1);
        } else {
            out[2 * i] = w0;
            out[2 * i + 1] = w1;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        u64 w = 0;
#pragma unroll
        for (int k = 0; k < K; k++) w |= (a.src[k][n - 1] - a.base[k]) << a.shift[k];
        out[n - 1] = w;
    }
}

// ---- k_keys_unpack: packed word -> the key columns ------------------------------------------------------------------------------
// The plan by value.  The rule fixes the shape (rhj.h): no fold -- field i is column i; one fold -- field 0 is fold 0 {column 0,
// column 1}, fields 1.. are columns 2..; two folds -- field 0 is fold 1 {fold 0, column 2}, field 1 is column 3.  An id is compared
// with its dictionary's size before it is an index; one that fails raises *bad and the row's columns are not written.
struct UnpackPlan {
    u32 nkeys, nfolds;
    u32 fshift[RHJ_KEYS_MAX_COLS];              // of the final word's fields (0 for a field of width 0)
    u64 fmask[RHJ_KEYS_MAX_COLS];
    u32 fold_shift[RHJ_KEYS_MAX_FOLDS];         // width of a fold's low input
    u64 fold_mask[RHJ_KEYS_MAX_FOLDS];          // ... as a mask
    const u64 *fold_dict[RHJ_KEYS_MAX_FOLDS];
    u64 fold_size[RHJ_KEYS_MAX_FOLDS];
    const u64 *dict[RHJ_KEYS_MAX_COLS];         // null: a RANGE column
    u64 dict_size[RHJ_KEYS_MAX_COLS];
    u64 base[RHJ_KEYS_MAX_COLS];
    u64 *out[RHJ_KEYS_MAX_COLS];
};

__global__ void __launch_bounds__(KEYS_THREADS)
k_keys_unpack(UnpackPlan p, const u64 *__restrict__ packed, u64 n, u32 *__restrict__ bad)
{
    for (u64 i = (u64)blockIdx.x * KEYS_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * KEYS_THREADS) {
        const u64 w = packed[i];
        u64 f[RHJ_KEYS_MAX_COLS], v[RHJ_KEYS_MAX_COLS];
#pragma unroll
        for (int k = 0; k < RHJ_KEYS_MAX_COLS; k++) f[k] = (w >> p.fshift[k]) & p.fmask[k];
        bool ok = true;
        if (p.nfolds == 0) {
#pragma unroll
            for (int k = 0; k < RHJ_KEYS_MAX_COLS; k++) v[k] = f[k];
        } else {
            u64 id0 = f[0];
            if (p.nfolds == 2) {
                ok = id0 < p.fold_size[1];
                const u64 w1 = ok ? p.fold_dict[1][id0] : 0;
                id0 = w1 & p.fold_mask[1];
                v[2] = w1 >> p.fold_shift[1];
                v[3] = f[1];
            } else {
                v[2] = f[1];
                v[3] = f[2];
            }
            ok = ok && id0 < p.fold_size[0];
            const u64 w0 = ok ? p.fold_dict[0][id0] : 0;
            v[0] = w0 & p.fold_mask[0];
            v[1] = w0 >> p.fold_shift[0];
        }
#pragma unroll
        for (int j = 0; j < RHJ_KEYS_MAX_COLS; j++)
            if (j < (int)p.nkeys && p.dict[j]) ok = ok && v[j] < p.dict_size[j];
        if (!ok) {
            atomicOr(bad, 1u);
            continue;
        }
#pragma unroll
        for (int j = 0; j < RHJ_KEYS_MAX_COLS; j++)
            if (j < (int)p.nkeys) p.out[j][i] = p.dict[j] ? p.dict[j][v[j]] : v[j] + p.base[j];
    }
}

unsigned grid_for(u64 work)
{
    u64 g = (work + KEYS_THREADS - 1) / KEYS_THREADS;
    if (g > KEYS_MAX_GRID) g = KEYS_MAX_GRID;
    if (g == 0) g = 1;
    return (unsigned)g;
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

// Allocations of a pack call that do not outlive it: blocks of their own from rhj_dev_alloc, never the context's workspace (the
// group-by inside the call and the operator after it reuse that).  rhj_dev_free keeps a released block for the next request of its
// size -- every temporary here is nR + nS words -- so a call's encoding steps, and the next call, mostly meet memory that is already
// mapped: with fresh hipMalloc blocks most packs of 2 * 10^8 rows took 0.4 - 1.4 s instead of 25 ms.  Work on the context's
// stream is ordered, so a block handed out again is never still being read.
struct Temps {
    rhj_ctx *ctx;
    std::vector<void *> blocks;
    explicit Temps(rhj_ctx *c) : ctx(c) {}
    ~Temps() { for (void *b : blocks) (void)rhj_dev_free(ctx, b); }
    int get(u64 words, u64 **out)
    {
        void *p = nullptr;
        const int rc = rhj_dev_alloc(ctx, (words ? words : 1) * 8, &p);
        if (rc != RHJ_OK) return rc;
        blocks.push_back(p);
        *out = (u64 *)p;
        return RHJ_OK;
    }
    void drop(void *p)
    {
        for (size_t i = 0; i < blocks.size(); i++)
            if (blocks[i] == p) { blocks.erase(blocks.begin() + i); (void)rhj_dev_free(ctx, p); return; }
    }
};

void free_plan(rhj_ctx *ctx, rhj_keyplan *plan)
{
    if (!plan) return;
    for (u64 *d : plan->dict) if (d) (void)rhj_dev_free(ctx, d);
    for (u64 *d : plan->fold_dict) if (d) (void)rhj_dev_free(ctx, d);
    delete plan;
}

u32 bits_of(u64 x) { u32 b = 0; while (x) { b++; x >>= 1; } return b; }          // 64 - clz(x), 0 for 0

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// one pack launch over n rows: the fields of `a` that have a width
template <int K> void launch_pack_k(hipStream_t st, const PackArgs &a, u64 *out, u64 n, bool vec)
{
    const unsigned g = grid_for(n / 2);
    if (vec) hipLaunchKernelGGL((k_keys_pack<K, true>), dim3(g), dim3(KEYS_THREADS), 0, st, a, out, n);
    else hipLaunchKernelGGL((k_keys_pack<K, false>), dim3(g), dim3(KEYS_THREADS), 0, st, a, out, n);
}

int launch_pack(rhj_ctx *ctx, hipStream_t st, const PackArgs &a, u32 k, u64 *out, u64 n)
{
    if (n == 0) return RHJ_OK;
    if (k == 0) {                                   // every field has width 0: all rows agree
        const hipError_t e = hipMemsetAsync(out, 0, (size_t)n * 8, st);
        return e == hipSuccess ? RHJ_OK : hip_fail(ctx, "rhj_keys_pack_dev: memset", e);
    }
    bool vec = aligned16(out);
    for (u32 i = 0; i < k; i++) vec = vec && aligned16(a.src[i]);
    switch (k) {
    case 1: launch_pack_k<1>(st, a, out, n, vec); break;
    case 2: launch_pack_k<2>(st, a, out, n, vec); break;
    case 3: launch_pack_k<3>(st, a, out, n, vec); break;
    default: launch_pack_k<4>(st, a, out, n, vec); break;
    }
    return check(ctx, "k_keys_pack");
}

// what a field of the pack is read from, per side: the caller's column and its base, or an id array over the concatenation
struct FieldSrc { const u64 *R = nullptr, *S = nullptr; u64 base = 0; };

// packs the given fields (source, width) of both sides, fields in order from bit 0; outR / outS: nR / nS words
int pack_fields(rhj_ctx *ctx, hipStream_t st, const FieldSrc *src, const u32 *width, u32 nf, u64 nR, u64 nS, u64 *outR, u64 *outS)
{
    PackArgs aR = {}, aS = {};
    u32 k = 0, shift = 0;
    for (u32 i = 0; i < nf; i++) {
        if (width[i]) {
            aR.src[k] = src[i].R; aS.src[k] = src[i].S;
            aR.base[k] = aS.base[k] = src[i].base;
            aR.shift[k] = aS.shift[k] = shift;
            k++;
        }
        shift += width[i];
    }
    int rc = launch_pack(ctx, st, aR, k, outR, nR);
    if (rc != RHJ_OK) return rc;
    return launch_pack(ctx, st, aS, k, outS, nS);
}

// dense ids of the n words at d_vals (device) by the engine's group-by with ids: ids[i] = index of d_vals[i] among the *G distinct
// values; d_dict (may be null: count only, no dictionary) receives them, n words of room.  Synchronises.
int dense_ids(rhj_ctx *ctx, const u64 *d_vals, u64 n, u64 *d_dict, u64 *d_ids, uint64_t *G)
{
    return rhj_group_agg_ids_cols_dev(ctx, (const uint64_t *)d_vals, nullptr, n, nullptr, nullptr, 0, 0, nullptr, (uint64_t *)d_dict,
                                      nullptr, nullptr, d_dict ? n : 0, G, (uint64_t *)d_ids, n);
}

// a dictionary of G words for the plan out of the n-word key output of dense_ids (the group-by needs room for n groups; the plan
// keeps what there is)
int shrink_dict(rhj_ctx *ctx, hipStream_t st, Temps &tmp, u64 *d_big, u64 G, u64 **out)
{
    void *p = nullptr;
    const int rc = rhj_dev_alloc(ctx, (G ? G : 1) * 8, &p);
    if (rc != RHJ_OK) return rc;
    hipError_t e = hipMemcpyAsync(p, d_big, (size_t)G * 8, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)rhj_dev_free(ctx, p); return hip_fail(ctx, "rhj_keys_pack_dev: dictionary copy", e); }
    tmp.drop(d_big);
    *out = (u64 *)p;
    return RHJ_OK;
}

}  // namespace

extern "C" {

int rhj_keys_layout(uint32_t nkeys, const uint8_t *range_bits, uint64_t n_total, rhj_keys_layout_t *out)
{
    if (!out || !range_bits || nkeys == 0 || nkeys > RHJ_KEYS_MAX_COLS) return RHJ_E_INVALID;
    rhj_keys_layout_t L = {};
    L.nkeys = nkeys;
    u32 id[RHJ_KEYS_MAX_COLS], width[RHJ_KEYS_MAX_COLS], nf = nkeys, sum = 0;
    for (u32 j = 0; j < nkeys; j++) {
        if (range_bits[j] > 64) return RHJ_E_INVALID;
        L.kind[j] = RHJ_KEYS_RANGE;
        L.range_bits[j] = range_bits[j];
        id[j] = j;
        width[j] = range_bits[j];
        sum += width[j];
    }
    if (sum > 64) {
        if (n_total >= (1ull << 32)) return RHJ_E_INVALID;              // dense ids are 32-bit at most (and so is the group-by's gid)
        const u32 wd = bits_of(n_total ? n_total - 1 : 0);
        L.wd = wd;
        while (sum > 64) {                                              // widest RANGE column above wd -> DICT
            int pick = -1;
            for (u32 j = 0; j < nkeys; j++)
                if (L.kind[j] == RHJ_KEYS_RANGE && width[j] > wd && (pick < 0 || width[j] > width[pick])) pick = (int)j;
            if (pick < 0) break;
            L.kind[pick] = RHJ_KEYS_DICT;
            sum -= width[pick] - wd;
            width[pick] = wd;
        }
        while (sum > 64) {                                              // every field is <= wd <= 32 bits now: fold the first two
            if (L.nfolds == RHJ_KEYS_MAX_FOLDS || nf < 3) return RHJ_E_INVALID;   // (unreachable: 4 * 32 - 2 * 32 <= 64)
            const u32 f = L.nfolds++;
            L.fold_a[f] = id[0];
            L.fold_b[f] = id[1];
            L.fold_shift[f] = width[0];
            sum -= width[0] + width[1] - wd;
            id[0] = RHJ_KEYS_FOLD0 + f;
            width[0] = wd;
            for (u32 i = 1; i + 1 < nf; i++) { id[i] = id[i + 1]; width[i] = width[i + 1]; }
            nf--;
        }
    }
    L.nfields = nf;
    u32 shift = 0;
    for (u32 i = 0; i < nf; i++) {
        L.field_id[i] = id[i];
        L.field_width[i] = width[i];
        L.field_shift[i] = shift;
        shift += width[i];
    }
    L.total_bits = shift;
    *out = L;
    return RHJ_OK;
}

int rhj_keys_pack_dev(rhj_ctx *ctx, uint32_t nkeys,
                      const uint64_t *const *d_keysR, uint64_t nR,
                      const uint64_t *const *d_keysS, uint64_t nS,
                      uint32_t flags, uint64_t *d_outR, uint64_t *d_outS, rhj_keyplan **out_plan)
{
    int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    if (!out_plan) return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_pack_dev: out_plan is null");
    *out_plan = nullptr;
    if (nkeys == 0 || nkeys > RHJ_KEYS_MAX_COLS)
        return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_pack_dev: nkeys must be 1 .. RHJ_KEYS_MAX_COLS");
    if (flags & ~RHJ_KEYS_NO_UNPACK) return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_pack_dev: unknown flags");
    if ((nR && (!d_keysR || !d_outR)) || (nS && (!d_keysS || !d_outS)))
        return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_pack_dev: null column array or output with a non-zero row count");
    for (u32 j = 0; j < nkeys; j++)
        if ((nR && !d_keysR[j]) || (nS && !d_keysS[j]))
            return rhj_internal_fail(ctx, RHJ_E_INVALID, ("rhj_keys_pack_dev: key column " + std::to_string(j) + " is null").c_str());
    if (nR + nS < nR) return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_pack_dev: nR + nS overflows");
    const u64 n = nR + nS;
    const bool no_unpack = (flags & RHJ_KEYS_NO_UNPACK) != 0;
    hipStream_t st = rhj_internal_stream(ctx);
    Temps tmp(ctx);
    hipError_t e;

    // 1. the range probe: one launch, four words per column
    u64 base[RHJ_KEYS_MAX_COLS] = {};
    uint8_t rbits[RHJ_KEYS_MAX_COLS] = {};
    if (n) {
        u64 *d_mm = nullptr;
        u64 h_mm[4 * RHJ_KEYS_MAX_COLS];
        for (u32 j = 0; j < RHJ_KEYS_MAX_COLS; j++) { h_mm[4 * j] = h_mm[4 * j + 2] = ~0ull; h_mm[4 * j + 1] = h_mm[4 * j + 3] = 0; }
        if ((rc = tmp.get(4 * RHJ_KEYS_MAX_COLS, &d_mm)) != RHJ_OK) return rc;
        e = hipMemcpyAsync(d_mm, h_mm, sizeof h_mm, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);                // (h_mm is pageable and read back below)
        if (e != hipSuccess) return hip_fail(ctx, "rhj_keys_pack_dev: range words", e);
        RangeArgs ra = {};
        for (u32 j = 0; j < nkeys; j++) {
            ra.col[2 * j] = nR ? (const u64 *)d_keysR[j] : nullptr; ra.n[2 * j] = nR;
            ra.col[2 * j + 1] = nS ? (const u64 *)d_keysS[j] : nullptr; ra.n[2 * j + 1] = nS;
        }
        unsigned gx = grid_for((nR > nS ? nR : nS) / 2);                  // KEYS_MAX_GRID blocks over all columns and sides
        if (gx > KEYS_MAX_GRID / (2 * nkeys)) gx = KEYS_MAX_GRID / (2 * nkeys);
        hipLaunchKernelGGL(k_keys_range, dim3(gx, 2 * nkeys), dim3(KEYS_THREADS), 0, st, ra, d_mm);
        if ((rc = check(ctx, "k_keys_range")) != RHJ_OK) return rc;
        e = hipMemcpyAsync(h_mm, d_mm, sizeof h_mm, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(ctx, "k_keys_range", e);
        for (u32 j = 0; j < nkeys; j++) {
            const u32 plain = bits_of(h_mm[4 * j + 1] - h_mm[4 * j]), biased = bits_of(h_mm[4 * j + 3] - h_mm[4 * j + 2]);
            rbits[j] = (uint8_t)(biased < plain ? biased : plain);
            base[j] = biased < plain ? h_mm[4 * j + 2] ^ BIAS : h_mm[4 * j];
        }
        tmp.drop(d_mm);
    }

    // 2. the layout
    rhj_keyplan *plan = new rhj_keyplan();
    plan->no_unpack = no_unpack;
    if (rhj_keys_layout(nkeys, rbits, n, &plan->lay) != RHJ_OK) {
        delete plan;
        return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_pack_dev: the key columns do not fit 64 bits as value ranges, and a layout "
                                                     "with dictionaries needs nR + nS < 2^32 (a RANGE-only layout has no such limit)");
    }
    rhj_keys_layout_t &L = plan->lay;
    for (u32 j = 0; j < nkeys; j++) L.base[j] = L.kind[j] == RHJ_KEYS_RANGE ? base[j] : 0;
    if (n == 0) { *out_plan = plan; return RHJ_OK; }

    // 3. dense ids of the DICT columns, then of the folds; src[id]: what field `id` is packed from
    FieldSrc src[RHJ_KEYS_FOLD0 + RHJ_KEYS_MAX_FOLDS];
    u32 width[RHJ_KEYS_FOLD0 + RHJ_KEYS_MAX_FOLDS] = {};
    auto ids_of = [&](const u64 *d_vals, u64 **dict, uint64_t *G, FieldSrc *out) -> int {     // d_vals: n words, R's rows first
        u64 *d_ids = nullptr, *d_big = nullptr;
        int r = tmp.get(n, &d_ids);
        if (r == RHJ_OK && !no_unpack) r = tmp.get(n, &d_big);
        if (r == RHJ_OK) r = dense_ids(ctx, d_vals, n, d_big, d_ids, G);
        if (r == RHJ_OK && !no_unpack) r = shrink_dict(ctx, st, tmp, d_big, *G, dict);
        out->R = d_ids; out->S = d_ids + nR; out->base = 0;
        return r;
    };
    for (u32 j = 0; j < nkeys && rc == RHJ_OK; j++) {
        width[j] = L.kind[j] == RHJ_KEYS_DICT ? L.wd : L.range_bits[j];
        if (L.kind[j] == RHJ_KEYS_RANGE) {
            src[j].R = nR ? (const u64 *)d_keysR[j] : nullptr; src[j].S = nS ? (const u64 *)d_keysS[j] : nullptr; src[j].base = base[j];
            continue;
        }
        const u64 *vals = nS == 0 ? (const u64 *)d_keysR[j] : nR == 0 ? (const u64 *)d_keysS[j] : nullptr;
        u64 *cat = nullptr;
        if (!vals) {                                                     // the concatenation: two device-to-device copies
            if ((rc = tmp.get(n, &cat)) != RHJ_OK) break;
            e = hipMemcpyAsync(cat, d_keysR[j], (size_t)nR * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(cat + nR, d_keysS[j], (size_t)nS * 8, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) { rc = hip_fail(ctx, "rhj_keys_pack_dev: concatenation", e); break; }
            vals = cat;
        }
        rc = ids_of(vals, &plan->dict[j], &L.dict_size[j], &src[j]);
        if (cat) tmp.drop(cat);
    }
    for (u32 f = 0; f < L.nfolds && rc == RHJ_OK; f++) {
        const u32 a = L.fold_a[f], b = L.fold_b[f];
        const FieldSrc two[2] = {src[a], src[b]};
        const u32 w2[2] = {width[a], width[b]};
        u64 *word = nullptr;
        if ((rc = tmp.get(n, &word)) != RHJ_OK) break;
        if ((rc = pack_fields(ctx, st, two, w2, 2, nR, nS, word, word + nR)) != RHJ_OK) break;
        rc = ids_of(word, &plan->fold_dict[f], &L.fold_size[f], &src[RHJ_KEYS_FOLD0 + f]);
        width[RHJ_KEYS_FOLD0 + f] = L.wd;
        tmp.drop(word);
        for (u32 x : {a, b})                                             // id arrays the fold has consumed
            if (x >= RHJ_KEYS_FOLD0 || L.kind[x] == RHJ_KEYS_DICT) tmp.drop((void *)src[x].R);
    }

    // 4. the final word
    if (rc == RHJ_OK) {
        FieldSrc fs[RHJ_KEYS_MAX_COLS];
        for (u32 i = 0; i < L.nfields; i++) fs[i] = src[L.field_id[i]];
        rc = pack_fields(ctx, st, fs, L.field_width, L.nfields, nR, nS, (u64 *)d_outR, (u64 *)d_outS);
    }
    if (rc == RHJ_OK && (e = hipStreamSynchronize(st)) != hipSuccess) rc = hip_fail(ctx, "k_keys_pack", e);
    if (rc != RHJ_OK) {
        (void)hipStreamSynchronize(st);                                   // nothing in flight reads what is freed next
        free_plan(ctx, plan);
        return rc;
    }
    *out_plan = plan;
    return RHJ_OK;
}

int rhj_keys_unpack_dev(rhj_ctx *ctx, const rhj_keyplan *plan, const uint64_t *d_packed, uint64_t n, uint64_t *const *d_out_cols)
{
    int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    if (!plan) return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_unpack_dev: plan is null");
    if (plan->no_unpack)
        return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_unpack_dev: the plan was packed with RHJ_KEYS_NO_UNPACK and keeps no dictionaries");
    if (n == 0) return RHJ_OK;
    if (!d_packed || !d_out_cols) return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_unpack_dev: null d_packed or d_out_cols");
    const rhj_keys_layout_t &L = plan->lay;
    UnpackPlan p = {};
    p.nkeys = L.nkeys;
    p.nfolds = L.nfolds;
    for (u32 i = 0; i < L.nfields; i++) {
        const u32 w = L.field_width[i];
        p.fshift[i] = w ? L.field_shift[i] : 0;
        p.fmask[i] = w == 64 ? ~0ull : (1ull << w) - 1;
    }
    for (u32 f = 0; f < L.nfolds; f++) {
        p.fold_shift[f] = L.fold_shift[f];                                // (<= 32: the low input is at most wd wide)
        p.fold_mask[f] = (1ull << L.fold_shift[f]) - 1;
        p.fold_dict[f] = plan->fold_dict[f];
        p.fold_size[f] = L.fold_size[f];
    }
    for (u32 j = 0; j < L.nkeys; j++) {
        if (!d_out_cols[j]) return rhj_internal_fail(ctx, RHJ_E_INVALID, ("rhj_keys_unpack_dev: output column " + std::to_string(j) + " is null").c_str());
        p.dict[j] = L.kind[j] == RHJ_KEYS_DICT ? plan->dict[j] : nullptr;
        p.dict_size[j] = L.dict_size[j];
        p.base[j] = L.base[j];
        p.out[j] = (u64 *)d_out_cols[j];
    }
    u32 *bad = (u32 *)rhj_internal_counters(ctx);
    if (!bad) return RHJ_E_NOMEM;
    bad += 10;                                                            // (the word the query-layer counters use: slot 5 of 8)
    hipStream_t st = rhj_internal_stream(ctx);
    hipError_t e = hipMemsetAsync(bad, 0, 4, st);
    if (e != hipSuccess) return hip_fail(ctx, "rhj_keys_unpack_dev: memset", e);
    hipLaunchKernelGGL(k_keys_unpack, dim3(grid_for(n)), dim3(KEYS_THREADS), 0, st, p, (const u64 *)d_packed, (u64)n, bad);
    if ((rc = check(ctx, "k_keys_unpack")) != RHJ_OK) return rc;
    u32 h_bad = 0;
    e = hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(ctx, "k_keys_unpack", e);
    if (h_bad)
        return rhj_internal_fail(ctx, RHJ_E_INVALID, "rhj_keys_unpack_dev: a packed word decodes to an id at or past its dictionary's size "
                                                     "(not a word this plan produced); it was not used as an index");
    return RHJ_OK;
}

int rhj_keys_plan_info(const rhj_keyplan *plan, rhj_keys_layout_t *out)
{
    if (!plan || !out) return RHJ_E_INVALID;
    *out = plan->lay;
    return RHJ_OK;
}

int rhj_keys_plan_free(rhj_ctx *ctx, rhj_keyplan *plan)
{
    if (!plan) return RHJ_OK;
    const int rc = rhj_internal_use_device(ctx);
    if (rc != RHJ_OK) return rc;
    free_plan(ctx, plan);
    return RHJ_OK;
}

}  // extern "C"
