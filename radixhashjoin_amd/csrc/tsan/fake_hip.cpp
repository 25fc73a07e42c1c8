// fake_hip.cpp -- the host-only stand-in behind tsan/hip/hip_runtime.h, and stand-ins for the kernel launchers of
// rhj_internal.h.  See the header: test infrastructure for `make -C radixhashjoin_amd/csrc tsan`, nothing of the product.
#include "../rhj_internal.h"

#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>

// ---- optional trace (off by default: tsan/entries.cpp switches it on) ------------------------------------------------
// One line per stream operation and per launcher call, appended on the calling thread in call order: the name and the scalar
// arguments; a pointer shows as "set" or "null", never as an address.
static std::string *g_trace = nullptr;
void fake_trace_into(std::string *sink) { g_trace = sink; }
static void tr(const char *fmt, ...)
{
    if (!g_trace) return;
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    *g_trace += line;
    *g_trace += '\n';
}
static const char *np(const void *p) { return p ? "set" : "null"; }
typedef unsigned long long llu;

// ---- streams: one thread each, executing its queue in order --------------------------------------------------------
struct FakeStream {
    std::mutex mu;
    std::condition_variable cv, idle;
    std::deque<std::function<void()>> q;
    bool quit = false, busy = false;
    std::thread th;
    FakeStream() : th([this] { run(); }) {}
    ~FakeStream()
    {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv.notify_all();
        th.join();
    }
    void run()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return quit || !q.empty(); });
                if (q.empty()) return;
                f = std::move(q.front());
                q.pop_front();
                busy = true;
            }
            f();
            {
                std::lock_guard<std::mutex> lk(mu);
                busy = false;
            }
            idle.notify_all();
        }
    }
    void push(std::function<void()> f)
    {
        { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(f)); }
        cv.notify_all();
    }
    void drain()
    {
        std::unique_lock<std::mutex> lk(mu);
        idle.wait(lk, [&] { return q.empty() && !busy; });
    }
};

static FakeStream *null_stream()
{
    static FakeStream *s = new FakeStream();          // (leaked on purpose: alive for every static destructor)
    return s;
}
static FakeStream *S(hipStream_t st) { return st ? st : null_stream(); }
void fake_enqueue(hipStream_t st, std::function<void()> f) { S(st)->push(std::move(f)); }

// ---- events: "everything enqueued on the stream before the record has run" ------------------------------------------
struct FakeEvent {
    std::mutex mu;
    std::condition_variable cv;
    unsigned long long recorded = 0, done = 0;
};

hipError_t hipIpcGetMemHandle(hipIpcMemHandle_t *h, void *p) { memcpy(h->reserved, &p, sizeof p); return hipSuccess; }
hipError_t hipIpcOpenMemHandle(void **p, hipIpcMemHandle_t h, unsigned) { memcpy(p, h.reserved, sizeof *p); return hipSuccess; }
hipError_t hipIpcCloseMemHandle(void *) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : "fake hip error"; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *value, hipDeviceAttribute_t, int) { *value = 256; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t bytes) { *p = malloc(bytes ? bytes : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { *p = malloc(bytes ? bytes : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned) { *dev = host; return hipSuccess; }
hipError_t hipMemGetInfo(size_t *f, size_t *t) { *f = *t = (size_t)64 << 30; return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    tr("hipMemcpy bytes=%llu kind=%d", (llu)bytes, (int)kind);
    null_stream()->drain();
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
    tr("hipMemcpyAsync bytes=%llu kind=%d", (llu)bytes, (int)kind);
    S(st)->push([=] { memcpy(dst, src, bytes); });    // the "DMA engine": reads the source when the stream gets there
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t st)
{
    tr("hipMemsetAsync value=%d bytes=%llu", value, (llu)bytes);
    S(st)->push([=] { memset(dst, value, bytes); });
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *st, unsigned) { *st = new FakeStream(); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t st) { delete st; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t st) { tr("hipStreamSynchronize"); S(st)->drain(); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *ev) { *ev = new FakeEvent(); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned) { return hipEventCreate(ev); }
hipError_t hipEventDestroy(hipEvent_t ev) { delete ev; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st)
{
    unsigned long long seq;
    { std::lock_guard<std::mutex> lk(ev->mu); seq = ++ev->recorded; }
    S(st)->push([=] {
        std::lock_guard<std::mutex> lk(ev->mu);           // (notify under the lock: a waiter may destroy the event as soon as it returns)
        if (ev->done < seq) ev->done = seq;
        ev->cv.notify_all();
    });
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev)
{
    std::unique_lock<std::mutex> lk(ev->mu);
    const unsigned long long want = ev->recorded;
    ev->cv.wait(lk, [&] { return ev->done >= want; });
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t ev)
{
    std::lock_guard<std::mutex> lk(ev->mu);
    return ev->done >= ev->recorded ? hipSuccess : hipErrorNotReady;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned)
{
    tr("hipStreamWaitEvent");
    unsigned long long want;
    { std::lock_guard<std::mutex> lk(ev->mu); want = ev->recorded; }
    S(st)->push([=] {
        std::unique_lock<std::mutex> lk(ev->mu);
        ev->cv.wait(lk, [&] { return ev->done >= want; });
    });
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.001f; return hipSuccess; }

// ---- the launchers of rhj_internal.h ---------------------------------------------------------------------------------
// Host-logic helpers keep plausible values; kernels are nothing, except that a "bucket join" leaves a result behind: it
// appends FAKE_PAIRS pairs {i, ~i} (i = position in the pair buffer) and moves the result counter on, in stream order --
// what the host paths read back, hand to the downloader and copy into the result page.
static const u64 FAKE_PAIRS = (u64)1 << 20;
struct FPair { u64 r, s; };

const char *launch_attr_error() { return nullptr; }
size_t scan_tmp_bytes(int bits) { return (size_t)64 * ((size_t)8 << bits); }
size_t part_lds_bytes(int) { return 0; }

static void tr_geom(const char *name, const void *in, const PassGeom &g)
{
    tr("%s in=%s n=%llu nseg=%u shift=%d bits=%d mix=%d", name, np(in), (llu)g.n, g.nseg, g.shift, g.bits, g.mix);
}
void launch_init_single_segment(hipStream_t, u64 n, u64 L, u64 *d_seg_start, u32 *d_unit_start)
{
    tr("init_single_segment n=%llu L=%llu seg=%s unit=%s", (llu)n, (llu)L, np(d_seg_start), np(d_unit_start));
}
void launch_make_units(hipStream_t, const u64 *, u32 nseg, u64 L, u32 *) { tr("make_units nseg=%u L=%llu", nseg, (llu)L); }
void launch_hist_units(hipStream_t, const void *in, const PassGeom &g, const u64 *, const u32 *, u32 *, u64 *mm, const DupSniff &sn)
{
    tr_geom("hist_units", in, g);
    tr("  minmax=%s sniff=%s", np(mm), np(sn.tab));
}
void launch_scan_units(hipStream_t, const PassGeom &g, const u64 *, const u32 *, const u32 *, u64 *, u64 *, u64 *) { tr_geom("scan_units", &g, g); }
void launch_scatter_units(hipStream_t, const void *in, void *, const PassGeom &g, const u64 *, const u32 *, const u64 *) { tr_geom("scatter_units", in, g); }
void launch_diff_hist(hipStream_t, const u64 *, u64 n, u64 *) { tr("diff_hist n=%llu", (llu)n); }
void launch_check_radix(hipStream_t, const void *, const u64 *, const void *, const u64 *, u64 nparts, int radix_bits, u64 *, const PartEnds &)
{
    tr("check_radix nparts=%llu radix_bits=%d", (llu)nparts, radix_bits);
}
void launch_prefix(hipStream_t, const u64 *, u64 nbins, u64 *) { tr("prefix nbins=%llu", (llu)nbins); }
void launch_make_tasks(hipStream_t st, const u64 *psR, const u64 *psS, u64 nparts, u32 probe_split, JoinTask *, u32 *d_ntasks, u32 max_tasks, u64 *,
                       int kind, const SniffVerdict &sv, const PartEnds &pe)
{
    tr("make_tasks psR=%s psS=%s nparts=%llu probe_split=%u max_tasks=%u kind=%d sniff=%s endR=%s endS=%s", np(psR), np(psS), (llu)nparts,
       probe_split, max_tasks, kind, np(sv.tab), np(pe.endR), np(pe.endS));
    fake_enqueue(st, [=] { *d_ntasks = 1; });
}
static void fake_join(void *d_out, u64 cap, u64 *d_out_count, u64 *host_count, void *host_out, u64 host_cap)
{
    const u64 at = *d_out_count;
    for (u64 i = at; i < at + FAKE_PAIRS; i++) {
        const FPair p{i, ~i};
        if (d_out && i < cap) ((FPair *)d_out)[i] = p;
        if (host_out && i < host_cap) ((FPair *)host_out)[i] = p;
    }
    if (host_count) { *host_count = at + FAKE_PAIRS; *d_out_count = 0; }     // (the direct kernel publishes and re-zeroes)
    else *d_out_count = at + FAKE_PAIRS;
}
void launch_join(hipStream_t st, const void *d_R, const u64 *, const void *d_S, const u64 *, const JoinTask *, const u32 *, u32 grid, int radix_bits,
                 void *d_out, u64 out_capacity, u64 *d_out_count, int kind, const u32 *kR, const u32 *kS, const u64 *tag_base, const u32 *flag,
                 u64 *host_pub, u32 *ticket)
{
    tr("join R=%s S=%s grid=%u radix_bits=%d out=%s cap=%llu kind=%d kR=%s kS=%s tag_base=%s flag=%s host_pub=%s ticket=%s", np(d_R), np(d_S), grid,
       radix_bits, np(d_out), (llu)out_capacity, kind, np(kR), np(kS), np(tag_base), np(flag), np(host_pub), np(ticket));
    fake_enqueue(st, [=] {
        fake_join(d_out, out_capacity, d_out_count, nullptr, nullptr, 0);
        if (host_pub) for (int i = 0; i < 7; i++) host_pub[i] = d_out_count[i];      // (the last workgroup publishes the counters)
    });
}
void launch_make_semi_tasks(hipStream_t st, const u64 *psR, const u64 *psS, u64 nparts, u32 split, int anti, JoinTask *, u32 *d_ntasks,
                            u32 max_tasks, u64 *)
{
    tr("make_semi_tasks psR=%s psS=%s nparts=%llu split=%u anti=%d max_tasks=%u", np(psR), np(psS), (llu)nparts, split, anti, max_tasks);
    fake_enqueue(st, [=] { *d_ntasks = 1; });
}
void launch_semi_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *, const u32 *, u32 grid, int radix_bits, int anti, u64 *d_out,
                      u64 out_capacity, u64 *d_out_count, u64 *, const u32 *kR, const u32 *kS, const u32 *flag)
{
    tr("semi_join R=%s S=%s grid=%u radix_bits=%d anti=%d out=%s cap=%llu kR=%s kS=%s flag=%s", np(d_R), np(d_S), grid, radix_bits, anti, np(d_out),
       (llu)out_capacity, np(kR), np(kS), np(flag));
    fake_enqueue(st, [=] {
        const u64 at = *d_out_count;
        for (u64 i = at; i < at + FAKE_PAIRS; i++)
            if (d_out && i < out_capacity) d_out[i] = i;
        *d_out_count = at + FAKE_PAIRS;
    });
}
void launch_outer_sweep(hipStream_t st, const void *d_P, const void *d_T, const JoinTask *, const u32 *, u32 grid, int radix_bits, int preserved_is_S,
                        void *d_out, u64 out_capacity, u64 *d_out_count, u64 *, const u32 *kP, const u32 *kT, const u32 *flag)
{
    tr("outer_sweep P=%s T=%s grid=%u radix_bits=%d side=%d out=%s cap=%llu kP=%s kT=%s flag=%s", np(d_P), np(d_T), grid, radix_bits, preserved_is_S,
       np(d_out), (llu)out_capacity, np(kP), np(kT), np(flag));
    fake_enqueue(st, [=] {                                          // (rows {i, all ones} / {all ones, i} behind what the counter holds)
        const u64 at = *d_out_count;
        u64 *pairs = (u64 *)d_out;
        for (u64 i = at; i < at + FAKE_PAIRS; i++)
            if (pairs && i < out_capacity) { pairs[2 * i + (preserved_is_S ? 1 : 0)] = i; pairs[2 * i + (preserved_is_S ? 0 : 1)] = ~0ull; }
        *d_out_count = at + FAKE_PAIRS;
    });
}
static const char *np4(const void *const *a)          // the null / non-null pattern of an array of AGG_MAX_COLS pointers
{
    static char buf[4][8];
    static int turn = 0;
    char *b = buf[turn++ & 3];
    if (!a) return "null";
    for (int j = 0; j < 4; j++) b[j] = a[j] ? 'x' : '-';
    b[4] = 0;
    return b;
}
void launch_agg_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *, const u32 *, u32 grid, int radix_bits, const u64 *const *d_cols,
                     u32 ncols, u64 col_rows, u64 *d_sums, u32 *, u64 *, const u32 *kR, const u32 *kS, const u32 *flag)
{
    tr("agg_join R=%s S=%s grid=%u radix_bits=%d cols=%s ncols=%u col_rows=%llu kR=%s kS=%s flag=%s", np(d_R), np(d_S), grid, radix_bits,
       np4((const void *const *)d_cols), ncols, (llu)col_rows, np(kR), np(kS), np(flag));
    fake_enqueue(st, [=] { for (u32 j = 0; j <= ncols; j++) d_sums[j] += FAKE_PAIRS; });
}
void launch_mult_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *, const u32 *, u32 grid, int radix_bits, const u64 *d_w,
                      u64 w_rows, u64 *d_out, u64 out_rows, u64 *d_total, u32 *, u64 *, const u32 *kR, const u32 *kS, const u32 *flag)
{
    tr("mult_join R=%s S=%s grid=%u radix_bits=%d w=%s w_rows=%llu out=%s out_rows=%llu kR=%s kS=%s flag=%s", np(d_R), np(d_S), grid, radix_bits,
       np(d_w), (llu)w_rows, np(d_out), (llu)out_rows, np(kR), np(kS), np(flag));
    fake_enqueue(st, [=] { if (out_rows) d_out[0] += FAKE_PAIRS; *d_total += FAKE_PAIRS; });
}
void launch_lookup_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *, const u32 *, u32 grid, int radix_bits, int which, u64 *d_out,
                        u64 out_rows, u64 *d_matched, u32 *, u64 *, const u32 *kR, const u32 *kS, const u32 *flag)
{
    tr("lookup_join R=%s S=%s grid=%u radix_bits=%d which=%d out=%s out_rows=%llu kR=%s kS=%s flag=%s", np(d_R), np(d_S), grid, radix_bits, which,
       np(d_out), (llu)out_rows, np(kR), np(kS), np(flag));
    fake_enqueue(st, [=] { if (out_rows) d_out[0] = 0; *d_matched += out_rows ? 1 : 0; });
}
void launch_group(hipStream_t st, const void *d_R, const JoinTask *, const u32 *, u32 grid, int radix_bits, bool mixed, const u64 *const *d_cols,
                  u32 ncols, u64 col_rows, u64 *d_keys, u64 *d_counts, u64 *const *d_sums, u64 capacity, u64 *d_ngroups, u32 *, u64 *, const u32 *kR,
                  const u32 *flag, u32 ops, bool ids, u64 *const *d_rows)
{
    tr("group R=%s grid=%u radix_bits=%d mixed=%d cols=%s ncols=%u col_rows=%llu keys=%s counts=%s sums=%s cap=%llu kR=%s flag=%s ops=0x%x ids=%d "
       "rows=%s", np(d_R), grid, radix_bits, (int)mixed, np4((const void *const *)d_cols), ncols, (llu)col_rows, np(d_keys), np(d_counts),
       np4((const void *const *)d_sums), (llu)capacity, np(kR), np(flag), ops, (int)ids, np4((const void *const *)d_rows));
    fake_enqueue(st, [=] { *d_ngroups += FAKE_PAIRS; });
}
void launch_group_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *, const u32 *, u32 grid, int radix_bits, bool mixed, bool left,
                       const u64 *const *d_colsR, u32 ncolsR, u64 colR_rows, const u64 *const *d_colsS, u32 ncolsS, u64 colS_rows, u64 *d_keys,
                       u64 *d_cntR, u64 *d_cntS, u64 *const *d_sumsR, u64 *const *d_sumsS, u64 capacity, u64 *d_ngroups, u32 *, u64 *,
                       const u32 *kR, const u32 *kS, const u32 *flag, u32 ops, bool ids)
{
    tr("group_join R=%s S=%s grid=%u radix_bits=%d mixed=%d left=%d colsR=%s ncolsR=%u colR_rows=%llu colsS=%s ncolsS=%u colS_rows=%llu keys=%s "
       "cntR=%s cntS=%s sumsR=%s sumsS=%s cap=%llu kR=%s kS=%s flag=%s ops=0x%x ids=%d", np(d_R), np(d_S), grid, radix_bits, (int)mixed, (int)left,
       np4((const void *const *)d_colsR), ncolsR, (llu)colR_rows, np4((const void *const *)d_colsS), ncolsS, (llu)colS_rows, np(d_keys), np(d_cntR),
       np(d_cntS), np4((const void *const *)d_sumsR), np4((const void *const *)d_sumsS), (llu)capacity, np(kR), np(kS), np(flag), ops, (int)ids);
    fake_enqueue(st, [=] { *d_ngroups += FAKE_PAIRS; });
}
void launch_group_id_words(hipStream_t st, u64 *d_ngroups, u64 *d_gidR, u64 gidR_rows, u64 *d_gidS, u64 gidS_rows)
{
    tr("group_id_words gidR=%s gidR_rows=%llu gidS=%s gidS_rows=%llu", np(d_gidR), (llu)gidR_rows, np(d_gidS), (llu)gidS_rows);
    fake_enqueue(st, [=] { d_ngroups[1] = (u64)d_gidR; d_ngroups[2] = gidR_rows; d_ngroups[3] = (u64)d_gidS; d_ngroups[4] = gidS_rows; });
}
int build_tie_shift() { return 4; }
size_t fuse_ctl_bytes() { return 12352; }
u32 *fuse_join_ticket(void *d_ctl) { return (u32 *)((unsigned char *)d_ctl + 12288) + 1; }
void launch_fused_pass(hipStream_t st, const PassPairHost &h, int bits, int phase, int parity, void *, u32 probe_split, u32 max_tasks, u32 table_tuples,
                       JoinTask *, u64 *d_counters, u64 *, bool sniff)
{
    tr("fused_pass nR=%llu nS=%llu bits=%d phase=%d parity=%d probe_split=%u max_tasks=%u table_tuples=%u sniff=%d", (llu)h.side[0].g.n,
       (llu)h.side[1].g.n, bits, phase, parity, probe_split, max_tasks, table_tuples, (int)sniff);
    if (phase == 0) fake_enqueue(st, [=] { memset(d_counters, 0, 64); });           // (the histogram launch clears the join counters)
}
void launch_join_direct(hipStream_t st, const void *d_R, u64 nR, const void *d_S, u64 nS, void *d_out, u64 out_capacity, u64 *d_out_count,
                        u64 *host_count, u32 *, void *host_out, u64 host_cap)
{
    tr("join_direct R=%s nR=%llu S=%s nS=%llu out=%s cap=%llu host_count=%s", np(d_R), (llu)nR, np(d_S), (llu)nS, np(d_out), (llu)out_capacity,
       np(host_count));
    fake_enqueue(st, [=] { fake_join(d_out, out_capacity, d_out_count, host_count, host_out, host_cap); });
}
void launch_join_batch(hipStream_t st, const BatchJoinDesc *d_batch, u32 njoins, u32)
{
    fake_enqueue(st, [=] {                                          // (the descriptors arrive with the staged upload)
        for (u32 i = 0; i < njoins; i++) {
            const BatchJoinDesc &b = d_batch[i];
            fake_join(b.out, b.cap, b.count, b.host_count, b.host_out, b.host_cap);
        }
    });
}
void launch_checksum(hipStream_t, const void *, u64, u64 *) { tr("checksum"); }
void launch_generate(hipStream_t, int, void *, u64, u64, u64, u64, double) { tr("generate"); }
void launch_expected_pkfk(hipStream_t, const void *, u64, u64 *) { tr("expected_pkfk"); }
void launch_remap_keys(hipStream_t, void *, u64, int, u64) { tr("remap_keys"); }
void launch_pass_pair(hipStream_t st, const PassPairHost &h, int shift, int bits, int phase)
{
    tr("pass_pair nR=%llu nS=%llu shift=%d bits=%d phase=%d zero8=%s mix=%d", (llu)h.side[0].g.n, (llu)h.side[1].g.n, shift, bits, phase,
       np(h.zero8), h.mix);
    u64 *z = h.zero8;
    if (phase == 0 && z) fake_enqueue(st, [=] { memset(z, 0, 64); });      // (the first launch clears the join counters)
}
void launch_cf_pass1(hipStream_t, const void *, void *, const CfGeom &, const PassGeom &, const u64 *, const u32 *, u32 *, u32 *, u32, const DupSniff &) { tr("cf_pass1"); }
void launch_cf_tables(hipStream_t, const CfGeom &, u32, const u32 *, u32 *, u32 *, u64 *, u32 *, const u32 *) { tr("cf_tables"); }
void launch_cf_hist2(hipStream_t, const void *, const CfGeom &, u32, int, int, const u32 *, u32 *, const u32 *) { tr("cf_hist2"); }
void launch_cf_pass2(hipStream_t, const void *, void *, u64, const CfGeom &, u32, int, int, const u64 *, const u32 *, u32 *) { tr("cf_pass2"); }
void launch_cf2_pass2(hipStream_t, const void *, void *, const CfGeom &, const Cf2Geom &, u32, int, int, const u32 *, u64 *, u64 *, u32 *, u32) { tr("cf2_pass2"); }
void launch_hist2d_units(hipStream_t, const void *in, bool in_narrow, u64 n, u64, u32, int b1, int b2, u32, u32, u32 *, u32 *, u64, u32 *wide, const u64 *,
                         int mix, const DupSniff &sn)
{
    tr("hist2d_units in=%s narrow=%d n=%llu b1=%d b2=%d wide=%s mix=%d sniff=%s", np(in), (int)in_narrow, (llu)n, b1, b2, np(wide), mix, np(sn.tab));
}
void launch_hist2d_units_cols(hipStream_t, const ColsIn &c, u64 n, u64, u32, int b1, int b2, u32, u32, u32 *, u32 *, u32 *wide, int mix, const DupSniff &sn)
{
    tr("hist2d_units_cols val=%s id=%s n=%llu b1=%d b2=%d wide=%s mix=%d sniff=%s", np(c.val), np(c.id), (llu)n, b1, b2, np(wide), mix, np(sn.tab));
}
void launch_scatter_units_cols(hipStream_t, const ColsIn &c, void *, const PassGeom &g, const u64 *, const u32 *, const u64 *)
{
    tr_geom("scatter_units_cols", c.val, g);
}
void launch_scatter_units_narrow_cols(hipStream_t, const ColsIn &c, void *, u64, const PassGeom &g, const u64 *, const u32 *, const u64 *, u32 *)
{
    tr_geom("scatter_units_narrow_cols", c.val, g);
}
void launch_cols_to_tuples(hipStream_t, const ColsIn &c, u64 n, void *) { tr("cols_to_tuples val=%s id=%s n=%llu", np(c.val), np(c.id), (llu)n); }
void launch_cf_pass1_cols(hipStream_t, const ColsIn &, void *, const CfGeom &, const PassGeom &, const u64 *, const u32 *, u32 *, u32 *, u32,
                          const DupSniff &) { tr("cf_pass1_cols"); }
void launch_seg_units(hipStream_t, u32, const u64 *, const u64 *, u32, u64 *, u64 *, u32 *) { tr("seg_units"); }
void launch_make_group_ranges(hipStream_t, const u64 *, u32, u32, u32, u64, u64 *, u32 *) { tr("make_group_ranges"); }
void launch_scatter_ranges(hipStream_t, const void *, void *, u32, int, int, const u64 *, const u64 *) { tr("scatter_ranges"); }
void launch_hist_units_narrow(hipStream_t, const void *, const PassGeom &, const u64 *, const u32 *, u32 *) { tr("hist_units_narrow"); }
void launch_scatter_units_narrow_any(hipStream_t, const void *, const u32 *, void *, u32 *, const PassGeom &, const u64 *, const u32 *,
                                     const u64 *, u32 *) { tr("scatter_units_narrow_any"); }
void launch_scatter_units_narrow(hipStream_t, const void *, void *, u64, const PassGeom &, const u64 *, const u32 *, const u64 *, u32 *,
                                 u64) { tr("scatter_units_narrow"); }
void launch_scatter_ranges_narrow(hipStream_t, const void *, bool, void *, u64, u32, int, int, const u64 *, const u64 *, u32 *, u32, u32,
                                  const u32 *) { tr("scatter_ranges_narrow"); }
void launch_scatter_units_narrow_peer(hipStream_t, const void *, const PassGeom &, const u64 *, const u32 *, const u64 *, u32 *, u64,
                                      const u64 *, const unsigned char *, void *const *, void *const *, int) { tr("scatter_units_narrow_peer"); }
void launch_scatter_ranges_n2a(hipStream_t, const void *, void *, u64, u32, int, int, const u64 *, const u64 *, const u64 *, u32, u32,
                               const u32 *) { tr("scatter_ranges_n2a"); }
