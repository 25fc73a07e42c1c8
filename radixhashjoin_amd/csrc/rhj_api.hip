// rhj_api.hip -- the C-ABI of include/rhj.h: context, HBM workspace, radix plan, orchestration.
// Host orchestration replaces the JobScheduler dispatch of the join path: what the reference does
// with 5 barriers and <= 288 heap Job objects per join is a fixed sequence of
// asynchronous kernel launches on one HIP stream with a single host sync for the result count.
#include "../../include/rhj.h"
#include "rhj_internal.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <sys/mman.h>
#include <thread>
#include <vector>

namespace {

thread_local std::string g_last_error;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct Prof {
    bool on = false;
    bool keep = false;                     // rhj_set_profiling(ctx, 2): the spans of successive calls accumulate
    std::vector<hipEvent_t> pool;          // event pairs, reused
    std::vector<int> kinds;                // kind per recorded pair
    size_t used = 0;
};

}  // namespace

// Host -> HBM copies of PAGEABLE caller memory (the reference allocates relations with new[]).  [measured, one MI355X host]
// hipMemcpy from pageable memory 15-18 GB/s, from pinned memory 57.5 GB/s; hipHostRegister of the caller's array 60 ms per GiB
// (more than the copy itself); memcpy pageable -> pinned 24-30 GB/s per thread.  So: STAGE_BUFS pinned 16 MiB buffers filled
// by STAGE_WORKERS persistent threads (whole chunks each, > 100 GB/s together), DMA'd out in order by the calling thread on the
// copy stream: the wire runs at the pinned rate.
constexpr size_t STAGE_BYTES = (size_t)16 << 20;
constexpr int STAGE_BUFS = 8, STAGE_WORKERS = 6;

struct Stager {
    void *buf[STAGE_BUFS] = {nullptr};
    hipEvent_t ev[STAGE_BUFS] = {nullptr};
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv;
    bool quit = false;
    u64 job_id = 0;                        // bumped for every copy; workers pick the job up once
    int device = 0;
    // the current job
    const char *src = nullptr;
    size_t bytes = 0, nchunks = 0;
    std::atomic<size_t> next{0}, issued{0}, chunk0{0};
    std::atomic<int> active{0};
    std::vector<std::atomic<unsigned char>> filled;
    size_t total_chunks = 0;               // chunks DMA'd since the buffers were created (buffer = chunk number % STAGE_BUFS)

    void work()
    {
        (void)hipSetDevice(device);
        u64 seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return quit || job_id != seen; });
                if (quit) return;
                seen = job_id;
            }
            for (;;) {
                const size_t c = next.fetch_add(1);
                if (c >= nchunks) break;
                const size_t g = chunk0.load() + c;                      // global chunk number: buffer g % STAGE_BUFS
                if (g >= (size_t)STAGE_BUFS) {                            // the buffer's previous chunk must be on the device
                    while (issued.load(std::memory_order_acquire) + STAGE_BUFS <= g) std::this_thread::yield();
                    (void)hipEventSynchronize(ev[g % STAGE_BUFS]);
                }
                const size_t off = c * STAGE_BYTES, len = bytes - off < STAGE_BYTES ? bytes - off : STAGE_BYTES;
                memcpy(buf[g % STAGE_BUFS], src + off, len);
                filled[c].store(1, std::memory_order_release);
            }
            active.fetch_sub(1);
        }
    }
};

// A few helper threads that copy a list of memory segments side by side (rhj_join_batch: staging the inputs of sixteen small
// joins into pinned memory, filling sixteen result pages).  One job at a time; the caller copies too.
struct CopySeg { void *dst; const void *src; size_t bytes; };
struct CopyPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv, idle;
    const CopySeg *segs = nullptr;
    size_t nseg = 0;
    std::atomic<size_t> next{0};
    u64 gen = 0;
    int active = 0;
    bool quit = false;
    explicit CopyPool(int n)
    {
        try {
            for (int i = 0; i < n; i++) th.emplace_back([this] { work(); });
        } catch (...) {}                                   // fewer helpers (or none): the caller copies everything itself
    }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv.notify_all();
        for (std::thread &t : th) t.join();
    }
    void drain()
    {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= nseg) return;
            if (segs[i].src) memcpy(segs[i].dst, segs[i].src, segs[i].bytes);
            else memset(segs[i].dst, 0, segs[i].bytes);              // (no source: first touch of fresh pages)
        }
    }
    void work()
    {
        u64 seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return quit || gen != seen; });
                if (quit) return;
                seen = gen;
            }
            drain();
            {
                std::lock_guard<std::mutex> lk(mu);
                active--;
            }
            idle.notify_all();
        }
    }
    void run(const std::vector<CopySeg> &list)
    {
        if (list.empty()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            segs = list.data();
            nseg = list.size();
            next.store(0);
            active = (int)th.size();
            gen++;
        }
        cv.notify_all();
        drain();
        std::unique_lock<std::mutex> lk(mu);
        idle.wait(lk, [&] { return active == 0; });
    }
};

// The operator arguments of one entry call, as its phase reads them from the context.  The *_common function of the entry opens a
// CallScope, fills in what its operator takes, and the scope puts CallArgs() back on every way out: nothing here outlives the call,
// and a field added here needs no line elsewhere to be cleared.
struct CallArgs {
    int outer_how = 0;                 // an outer join's RHJ_OUTER_* bits
    // an aggregating join's weight columns (device), and where agg_phase leaves the ncols sums (host); device words: agg_out's
    const u64 *agg_cols[AGG_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    u32 agg_ncols = 0;
    u64 agg_col_rows = 0;
    u64 *agg_sums_out = nullptr;
    // a multiplicity join's arguments (its device words are agg_out's: [0] total, [5] u32 MULT_BAD_ROW_*)
    const u64 *mult_w = nullptr;       // weights by S's rowID (device), or null
    u64 mult_w_rows = 0;
    u64 *mult_out = nullptr;           // out_rows words (device)
    u64 mult_out_rows = 0;
    int lookup_which = 0;              // a lookup join's RHJ_LOOKUP_* (its output words are mult_out / mult_out_rows, its device words agg_out's: [0] matched, [5] u32 LOOKUP_BAD_ROW_*)
    // a group-by's arguments (input columns: agg_cols / agg_ncols / agg_col_rows; device words: agg_out's [0] groups, [5] u32 a rowID
    // >= col_rows was met)
    bool one_sided = false;            // partition_phase partitions R alone: no kernel touches a buffer of S, part_S does not grow
    u64 *group_keys = nullptr, *group_counts = nullptr;   // capacity words each (device; counts may be null)
    u64 *group_sums[AGG_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    u64 group_cap = 0;
    u32 group_ops = 0;                 // the columns' packed op words (AGG_OP_*; a group-by join's: both sides'); 0: every column a sum
    u64 *group_rows[AGG_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};   // rhj_group_arg_*: the rows arrays (group_sums: the values) ...
    bool group_arg = false;            // ... and that group_ops holds ARG_OP_* words: group_phase launches k_group_bkt<., GB_ARG>
    // a group-by join's arguments beyond the group-by's (R's side: agg_cols / agg_ncols / agg_col_rows, group_keys, group_counts = cntR,
    // group_sums, group_cap; device words: agg_out's [0] groups, [5] u32 GJOIN_BAD_ROW_R / _S)
    const u64 *gjoin_colsS[AGG_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    u32 gjoin_ncolsS = 0;
    u64 gjoin_colS_rows = 0;
    u64 *gjoin_cntS = nullptr;         // capacity words (device; may be null)
    u64 *gjoin_sumsS[AGG_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    bool gjoin_left = false;           // RHJ_GJ_LEFT
    // the id arrays of a group-by ([0]) or group-by join ([0] R's, [1] S's) with ids: device arrays of gid_rows[.] words
    // indexed by the side's rowID, null: none; device words: agg_out's [1 .. 4], flag bits GROUP_BAD_GID / GJOIN_BAD_GID_*
    u64 *gid[2] = {nullptr, nullptr};
    u64 gid_rows[2] = {0, 0};
};

struct rhj_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    Prof prof;
    rhj_timings last{};
    // workspace (grow-only)
    DevBuf in_R, in_S;                 // H2D staging of host inputs (rhj_join)
    DevBuf part_R, part_S, part_tmp;   // partitioned relations, pass-1 intermediate
    DevBuf ps_R, ps_S, ps_1;           // partition boundaries (final R, final S, pass-1 scratch)
    DevBuf seg0, unit_start, unit_hist, unit_base;
    DevBuf seg0_b, unit_start_b, unit_hist_b, unit_base_b, scan_tmp_b;   // second relation of a paired pass
    DevBuf hist2_b, grp_rng_b, unit_start2_b, ps_1_b, part_tmp_b;        // ... and of a two-pass join partitioned on two streams
    hipStream_t aux_stream = nullptr;  // S of a mid-size two-pass join is partitioned here while R runs on `stream`
    hipEvent_t aux_ev[2] = {nullptr, nullptr};
    DevBuf tasks, counters;            // counters: [0] u64 out_count, [1] u32 ntasks (+pad), [2] u64 checksum
    DevBuf out_pairs;                  // rhj_join's device result buffer
    DevBuf small_out;                  // small-join path: 64-byte header {count} + pairs, fetched in one D2H
    bool small_hdr_clean = false;      // the header has been zeroed behind the previous small join
    DevBuf hist_tmp, scan_tmp, hist2, grp_rng, unit_start2, seg_rng, tag_base;
    DevBuf shard_ps[2], shard_mm;      // multi-GPU sender: class boundaries per side, rowID {min, max} per side
    // rhj_join_batch: several small joins per launch
    struct CopyPool *pool = nullptr;   // helper threads for host memcpy (staging in, pages out)
    // (two slots: the host work of one group of joins overlaps the GPU work of the next)
    unsigned char *b_stage[2] = {nullptr, nullptr};  // pinned: descriptors + the inputs of one group of joins
    size_t b_stage_cap[2] = {0, 0};
    unsigned char *b_land[2] = {nullptr, nullptr}, *b_land_dev[2] = {nullptr, nullptr};   // pinned: 16 counts (128 B) + the group's first pairs, written by the kernel itself
    size_t b_land_cap[2] = {0, 0};
    DevBuf b_in[2], b_out[2], b_cnt[2];   // device: staged blob, pair buffers, per-join {count, ticket}
    hipEvent_t b_ev[2] = {nullptr, nullptr};
    DevBuf fuse_ctl;                   // one-pass joins in three launches: two copies of {global histograms, digit cursors, sample counters} + the join's ticket
    bool fuse_clean = false;           // ... whose copy for the next call the kernels leave zeroed (false: the next call clears both first)
    int fuse_parity = 0;               // the copy the next call uses
    // which side of a join has duplicate join values (DupSniff, rhj_internal.h): the sample counters of R and S for a two-pass join
    // (a one-pass join keeps them in its control block)
    DevBuf sniff_tab;
    int sniff_side = -1;               // partition_relation_fused: the side it is counting for (-1: no sampling)
    u64 sniff_n[2] = {0, 0};
    bool sniff_ready = false;          // both sides of the current join were sampled: k_make_tasks may ask
    bool shard_sniffed[2] = {false, false};   // rhj_shard_partition sampled this side's received join values
    u64 *h_pub = nullptr, *h_pub_dev = nullptr;   // pinned: the join counters as the bucket join's last workgroup publishes them
    int opt_fused = -1;                // -1: automatic (RHJ_FUSE env, default 1), 0 / 1
    int opt_sniff = -1;                // -1: automatic (RHJ_SNIFF env, default 1), 0 / 1: sample the join values for duplicates (DupSniff)
    std::vector<u64> shard_ps_host[2]; // the class boundaries of the last rhj_shard_stats of each side (host copy)
    DevBuf shard_peer_tab;             // rhj_shard_split_peer: delta[2^bits] u64 + owner[2^bits] u8 per side
    DevBuf shard_wide;                 // u32 per side: rhj_shard_split met a rowID - key_base >= 2^32 (checked by rhj_shard_join)
    // rhj_dev_alloc / rhj_dev_free keep released blocks for re-use (all work of a context is ordered on its one
    // stream, so a block may be handed out again while kernels that used it are still queued): a device-resident
    // query allocates and frees a dozen arrays per join, and hipMalloc/hipFree would synchronise every time
    std::vector<std::pair<void *, size_t>> free_blocks;
    size_t free_bytes = 0;
    // pinned staging for host -> HBM copies of pageable caller memory (rhj_join)
    Stager *stager = nullptr;
    unsigned char *h_counts = nullptr;     // pinned: the join counters of every S chunk of a pipelined rhj_join (64 B each)
    std::vector<hipEvent_t> chunk_ev;
    hipStream_t down_stream = nullptr;     // result chunks travel home while later S chunks are still on their way in
    hipStream_t copy_stream = nullptr;     // uploads of rhj_join: S travels while R is being partitioned
    hipEvent_t up_ev[2] = {nullptr, nullptr};
    // state of the last partition phase (consumed by join_phase)
    const void *cur_R = nullptr, *cur_S = nullptr;
    const u64 *cur_psR = nullptr, *cur_psS = nullptr;
    u64 cur_nparts = 0, cur_nR = 0, cur_nS = 0;
    int cur_radix_bits = 0;
    u32 cur_probe_split = 0;
    int last_join_kind = -1;
    int last_pipelined = 0;            // S chunks of the last rhj_join (0: not pipelined)
    u64 last_max_part[2] = {0, 0};     // largest partition of R / S the last task list saw (0: direct join)
    int last_semi_tables = 0;          // "last.semi_tables": LDS tables the busiest task of the last semi / anti join built (0: another call)
    int last_outer_sweeps = 0;         // "last.outer_sweeps": anti sweeps the last outer join ran behind its pair join (0: another call)
    int last_sort_bits = 0, last_sort_passes = 0;   // "last.sort_bits" / "last.sort_passes": the width the last sort's probe found, the scatter passes it ran (0: another call)
    int last_sort_units = 0;           // "last.sort_units": the units -- workgroups per launch -- of those passes (0: no pass ran)
    DevBuf sort_ws;                    // the sort's tables and ping-pong buffers (rhj_sort.hip)
    int opt_sort_units = -1;           // "sort.max_units": -1 automatic, else the most units a sort cuts its input into
    int last_topk_bits = 0, last_topk_passes = 0;   // "last.topk_bits" / "last.topk_passes": the width the last top-k's probe found, the select histograms it ran (0: another call)
    u64 last_topk_cand = 0, last_topk_sorted = 0;   // "last.topk_candidates" / "last.topk_sorted_rows": the rows tied with the threshold's digits when selection stopped, the rows its inner sort took
    DevBuf topk_ws;                    // top-k's select state, tables and kept rows (rhj_sort.hip): not sort_ws, which the inner sort regrows
    int64_t opt_topk_cand = -1;        // "topk.max_candidates": -1 automatic, else selection goes on while more rows than this are tied
    int last_window_units = 0, last_window_sorts = 0;   // "last.window_units" / "last.window_sorts": the units the last window call's scans were cut into, its inner sorts (0: another call)
    u64 last_window_parts = 0;         // "last.window_partitions": the partitions it found
    int last_asof_units = 0, last_asof_sorts = 0;       // "last.asof_units" / "last.asof_sorts": the units the last as-of call's scan was cut into, its inner sorts (0: another call)
    u64 last_asof_matched = 0;         // "last.asof_matched": the rows of R that found a partner
    int last_frame_units = 0, last_frame_sorts = 0, last_frame_scans = 0;   // "last.frame_units" / "last.frame_sorts" / "last.frame_scans": the units the last frame call's scans were cut into, its inner sorts, its value scans (0: another call)
    u64 last_frame_parts = 0;          // "last.frame_partitions": the partitions it found
    int last_frange_units = 0, last_frange_sorts = 0, last_frange_scans = 0, last_frange_levels = 0;   // "last.frame_range_units" / "_sorts" / "_scans" / "_levels": the same of the last RANGE frame call, and the sparse-table levels it built (0: another call)
    u64 last_frange_parts = 0;         // "last.frame_range_partitions": the partitions it found
    DevBuf frame_ws;                   // the frame entry's permutation, sorted words, flags, bounds, by-position scans and unit tables (rhj_frame.hip): not sort_ws, which the inner sorts regrow
    int last_range_units = 0, last_range_sorts = 0;     // "last.range_join_units" / "last.range_join_sorts": the units the last range join's rank scan was cut into, its inner sorts (0: another call)
    u64 last_range_pairs = 0, last_range_tiles = 0;     // "last.range_join_pairs" / "last.range_join_expand_tiles": the pairs of the last range join or expansion, the workgroups that wrote them
    DevBuf range_ws;                   // the range join's concatenation, permutation, order words, ranks, counts and unit tables (rhj_range.hip): not sort_ws, which the inner sorts regrow
    DevBuf asof_ws;                    // the as-of entry's concatenation, permutation, flags and unit tables (rhj_asof.hip): not sort_ws, which the inner sorts regrow
    DevBuf window_ws;                  // the window entry's permutation, sorted words, flags, starts and unit tables (rhj_window.hip): not sort_ws, which the inner sorts regrow
    CallArgs call;                     // the operator arguments of the entry in progress (CallScope)
    u64 outer_sections[3] = {0, 0, 0}; // an outer join's {matched, R-only, S-only} rows, as outer_phase leaves them
    bool counters_clean = false;       // the 64-byte join counters are zero (cleared by the partition phase's first launch)
    int cur_narrow = 0;                // partitions are in the narrow {payload, rowID} format (k_scatter_wcn); 2: so was the intermediate
    DevBuf agg_out;                    // an aggregating join's words: [0] count, [1 .. 4] sums, [5] u32 a rowID >= col_rows was met
    int last_group_rounds = 0;         // "last.group_rounds": table builds of the busiest task of the last group-by or group-by join (0: another call)
    DevBuf narrow_flag;               // u32: a rowID >= 2^32 met a narrow scatter -> the join re-runs in the 16-byte format
    // ... the next join tries the narrow format again; consecutive fall-backs make the context skip the attempt for the next
    // 2, 4, ... 32 eligible joins (a caller whose rowIDs are always wide pays one extra histogram per relation now and then)
    u32 narrow_fail_streak = 0, narrow_skip = 0;
    bool narrow_off_once = false;      // the repeat of a join that fell back
    // count-free pass 1 (rhj.h "partition.countfree"), per side of a join (0 = first relation): a side whose pass 1
    // met a run longer than its region is repeated with exact cursors inside the same call (the skip word's bit 2 << side), and
    // the context leaves that side on the exact path for the next 2, 4, ... 32 eligible joins
    int opt_countfree = -1;            // -1: automatic (RHJ_COUNTFREE env; from CF_AUTO_MIN_TUPLES on), 0: never, 1: whenever the case applies
    u32 cf_fail_streak[2] = {0, 0}, cf_skip[2] = {0, 0};
    bool cf_off_once[2] = {false, false};   // the repeat of a side that fell back
    bool cf_keep_R = false;            // ... during which R's partition of the first attempt stands (only S overflowed)
    u32 cf_over = 0;                   // the skip word as join_phase read it (bits 1, 2)
    int last_cf[2] = {0, 0};           // "last.countfree_R/_S": 0 exact, 1 count-free, 2 tried and fell back
    DevBuf cf_cnt1, cf_pre, cf_tot;
    // count-free pass 2 with one writer per final partition (rhj.h "partition.countfree2"), per side of a PAIR join: the
    // partitions lie in regions of cap2 slots with gaps between them, start[k] = k * cap2 in ps_R / ps_S and end[k] in cf2_end; a
    // side one of whose partitions did not fit (the skip word's bit 8 << side) is repeated with the pass-2 histogram inside the
    // same call, and backs off like the count-free pass 1, with a state of its own
    int opt_countfree2 = -1;           // -1: automatic (RHJ_COUNTFREE2 env; see CF2_AUTO), 0: never, 1: whenever the case applies
    u32 cf2_fail_streak[2] = {0, 0}, cf2_skip[2] = {0, 0};
    bool cf2_off_once[2] = {false, false};  // the repeat of a side that fell back
    int last_cf2[2] = {0, 0};          // "last.countfree2_R/_S": 0 histogram path, 1 count-free, 2 tried and fell back
    DevBuf cf2_end[2];
    const u64 *cur_end[2] = {nullptr, nullptr};   // state of the last partition phase: the side's end array, or null: contiguous partitions
    u64 cur_slots[2] = {0, 0};         // ... and the slots of its final arrays (the rowID array starts at 8 * slots), or 0
    int num_cus = 0;                   // compute units of the device
    // rhj_join_cols_dev: the relations of the join in progress as columns (val == nullptr: a 16-byte call); the 16-byte copy of
    // a side that a plan without a columnar first kernel asks for (converted on first use, once per call); "last.cols_R/_S"
    ColsIn cols_in[2];
    DevBuf cols_aos[2];
    bool cols_aos_done[2] = {false, false};
    int last_cols[2] = {0, 0};         // 0: not a columnar call, 1: the partition kernels read the columns, 2: converted first
    // multi-GPU receiver (rhj_shard_partition / rhj_shard_join): the partitions carry sender tags
    int shard_nseg = 0, shard_mode[2] = {0, 0};
    bool shard_side_done[2] = {false, false};
    u64 shard_n[2] = {0, 0}, shard_kmin[2] = {0, 0}, shard_kmax[2] = {0, 0};
    rhj_opts shard_plan{};
    // pinned host landing zone of the small-join path: 64-byte header {count}, then up to 128 KiB of result pairs
    unsigned char *h_land = nullptr;
    unsigned char *h_land_dev = nullptr;   // the same memory as the device addresses it
    // tuning / test knobs (rhj_set_option)
    int opt_big_tables = -1;           // -1: by average build partition size, 0: never, 1: always use an oversized-partition kernel
    int opt_big_kernel = -1;           // -1: automatic, JK_BKT_BIG: never the compact-table kernel
    int opt_narrow = -1;               // -1: automatic (RHJ_NARROW env: 0, 1 = last pass only, 2), 0: never, 1 / 2: that level
    int opt_mix = -1;                  // -1: automatic (RHJ_MIX env, default 1), 0: radix digits from the raw low payload bits (rounds 1-3),
                                       // 1: from mix64(payload) (MIX_STORE, rhj_internal.h)
};

namespace {

int fail(rhj_ctx *ctx, int code, const std::string &msg)
{
    g_last_error = msg;
    if (ctx) ctx->err = msg;
    return code;
}

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RHJ_E_NOMEM : RHJ_E_HIP,                  \
                        std::string(#call) + ": " + hipGetErrorString(e_));                        \
    } while (0)

#define RHJCHK(call)                                                                               \
    do {                                                                                           \
        int r_ = (call);                                                                           \
        if (r_ != RHJ_OK) return r_;                                                               \
    } while (0)

int ensure(rhj_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return RHJ_OK;
    if (b.p) { HIPCHK(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    // round up to 2 MiB so that repeated slightly-larger requests do not re-allocate every time
    size_t want = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();
        return fail(ctx, RHJ_E_NOMEM, "hipMalloc(" + std::to_string(want) + " B): " + hipGetErrorString(e));
    }
    b.cap = want;
    return RHJ_OK;
}

void release(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

void stager_free(Stager *st)
{
    {
        std::lock_guard<std::mutex> lk(st->mu);
        st->quit = true;
    }
    st->cv.notify_all();
    for (std::thread &t : st->workers) t.join();
    for (int i = 0; i < STAGE_BUFS; i++) {
        if (st->buf[i]) (void)hipHostFree(st->buf[i]);
        if (st->ev[i]) (void)hipEventDestroy(st->ev[i]);
    }
    delete st;
}

void stager_destroy(rhj_ctx *ctx)
{
    if (ctx->stager) stager_free(ctx->stager);
    ctx->stager = nullptr;
}

// Built completely before the context sees it: a stager with fewer than STAGE_WORKERS workers would leave h2d_staged
// waiting for chunks nobody fills.  Null when a pinned buffer, an event or a thread cannot be had (the caller then copies
// straight from the pageable source).
Stager *stager_create(int device)
{
    Stager *st = new (std::nothrow) Stager();
    if (!st) return nullptr;
    st->device = device;
    bool ok = true;
    for (int i = 0; i < STAGE_BUFS && ok; i++)
        ok = hipHostMalloc(&st->buf[i], STAGE_BYTES, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&st->ev[i], hipEventDisableTiming) == hipSuccess;
    try {
        for (int i = 0; i < STAGE_WORKERS && ok; i++) st->workers.emplace_back([st] { st->work(); });
    } catch (...) {                                        // std::system_error: no more threads -- never through the C ABI
        ok = false;
    }
    if (!ok) {
        (void)hipGetLastError();
        stager_free(st);
        return nullptr;
    }
    return st;
}

// asynchronous with respect to the device: returns when the last chunk's DMA has been ENQUEUED on `stream` (the source has
// been read completely by then)
int h2d_staged(rhj_ctx *ctx, void *d_dst, const void *src, size_t bytes, hipStream_t stream)
{
    if (bytes < 4 * STAGE_BYTES) {
        HIPCHK(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, stream));
        return RHJ_OK;
    }
    if (!ctx->stager) ctx->stager = stager_create(ctx->device);
    if (!ctx->stager) {                                                   // no pinned ring to be had: the plain (slower) copy
        HIPCHK(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, stream));
        return RHJ_OK;
    }
    Stager *st = ctx->stager;
    const size_t nchunks = (bytes + STAGE_BYTES - 1) / STAGE_BYTES;
    {
        std::lock_guard<std::mutex> lk(st->mu);
        st->src = (const char *)src;
        st->bytes = bytes;
        st->nchunks = nchunks;
        st->filled = std::vector<std::atomic<unsigned char>>(nchunks);
        for (auto &f : st->filled) f.store(0);
        st->next.store(0);
        st->chunk0.store(st->total_chunks);
        st->issued.store(st->total_chunks);
        st->active.store(STAGE_WORKERS);
        st->job_id++;
    }
    st->cv.notify_all();
    int rc = RHJ_OK;
    for (size_t c = 0; c < nchunks; c++) {
        while (!st->filled[c].load(std::memory_order_acquire)) std::this_thread::yield();
        const size_t g = st->total_chunks + c, off = c * STAGE_BYTES, len = bytes - off < STAGE_BYTES ? bytes - off : STAGE_BYTES;
        hipError_t e = hipMemcpyAsync((char *)d_dst + off, st->buf[g % STAGE_BUFS], len, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(st->ev[g % STAGE_BUFS], stream);
        if (e != hipSuccess && rc == RHJ_OK) rc = fail(ctx, RHJ_E_HIP, std::string("staged upload: ") + hipGetErrorString(e));
        st->issued.store(g + 1, std::memory_order_release);              // (on an error too: the workers must not wait for ever)
    }
    while (st->active.load() != 0) std::this_thread::yield();             // every worker has left the job
    st->total_chunks += nchunks;
    return rc;
}

int use_device(rhj_ctx *ctx)
{
    if (!ctx) return fail(nullptr, RHJ_E_INVALID, "null context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return RHJ_OK;
}

// ---- profiling: one event pair per launch, resolved lazily -------------------------------------
struct Span {
    rhj_ctx *c;
    Span(rhj_ctx *ctx, int kind) : c(ctx)
    {
        if (!c->prof.on) return;
        Prof &p = c->prof;
        if (p.used * 2 + 2 > p.pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { p.on = false; return; }
            p.pool.push_back(a);
            p.pool.push_back(b);
        }
        p.kinds.push_back(kind);
        (void)hipEventRecord(p.pool[p.used * 2], c->stream);
    }
    ~Span()
    {
        if (!c->prof.on) return;
        Prof &p = c->prof;
        (void)hipEventRecord(p.pool[p.used * 2 + 1], c->stream);
        p.used++;
    }
};

void prof_reset(rhj_ctx *ctx)
{
    if (!ctx->prof.keep) {
        ctx->prof.used = 0;
        ctx->prof.kinds.clear();
    }
    memset(&ctx->last, 0, sizeof(ctx->last));
    ctx->last_cols[0] = ctx->last_cols[1] = 0;      // "last.cols_*": every join or stage call starts here; rhj_join_cols_dev sets them as it goes
    ctx->last_semi_tables = 0;                      // "last.semi_tables": ... and semi_phase this one
    ctx->last_group_rounds = 0;                     // "last.group_rounds": ... and group_phase this one
    ctx->last_outer_sweeps = 0;                     // "last.outer_sweeps": ... and outer_phase this one
    ctx->last_sort_bits = ctx->last_sort_passes = ctx->last_sort_units = 0;   // "last.sort_*": ... and the sort entries these
    ctx->last_topk_bits = ctx->last_topk_passes = 0;                          // "last.topk_*": ... and the top-k entries these
    ctx->last_topk_cand = ctx->last_topk_sorted = 0;
    ctx->last_window_units = ctx->last_window_sorts = 0;                      // "last.window_*": ... and the window entry these
    ctx->last_window_parts = 0;
    ctx->last_asof_units = ctx->last_asof_sorts = 0;                          // "last.asof_*": ... and the as-of entry these
    ctx->last_asof_matched = 0;
    ctx->last_frame_units = ctx->last_frame_sorts = ctx->last_frame_scans = 0;   // "last.frame_*": ... and the frame entry these
    ctx->last_frame_parts = 0;
    ctx->last_frange_units = ctx->last_frange_sorts = ctx->last_frange_scans = ctx->last_frange_levels = 0;   // "last.frame_range_*": ... and the RANGE frame entry these
    ctx->last_frange_parts = 0;
    ctx->last_range_units = ctx->last_range_sorts = 0;                        // "last.range_join_*": ... and the range join entries these
    ctx->last_range_pairs = ctx->last_range_tiles = 0;
}

int check_launch(rhj_ctx *ctx, const char *what)
{
    hipError_t e = hipGetLastError();
    if (const char *attr = launch_attr_error())          // a kernel was refused its LDS size: say so instead of "invalid argument"
        return fail(ctx, RHJ_E_HIP, std::string(what) + ": " + attr);
    if (e != hipSuccess) return fail(ctx, RHJ_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return RHJ_OK;
}

// the rowID array of narrow partitions: the u32 words behind the payloads of n tuples (or slots, where a side lies in regions with gaps)
const u32 *narrow_ids(const void *base, u64 n_or_slots)
{
    return (const u32 *)((const unsigned char *)base + narrow_k_offset(n_or_slots));
}

// tuning environment variables: unset, empty or non-numeric -> the default; numeric values are clamped to [lo, hi]
u64 env_u64(const char *name, u64 dflt, u64 lo, u64 hi)
{
    const char *v = getenv(name);
    if (!v || !*v) return dflt;
    char *end = nullptr;
    const u64 x = strtoull(v, &end, 10);
    if (end == v) return dflt;
    return x < lo ? lo : x > hi ? hi : x;
}

// whether joins sample their join values for duplicates (DupSniff; RHJ_SNIFF=0: no, the first relation wins every near tie)
bool sniff_on(const rhj_ctx *ctx)
{
    static const bool on = env_u64("RHJ_SNIFF", 1, 0, 1) != 0;
    return ctx->opt_sniff >= 0 ? ctx->opt_sniff != 0 : on;
}

int ilog2_ceil(u64 x)
{
    int b = 0;
    while (((u64)1 << b) < x) b++;
    return b;
}

// ---- radix plan (host logic) --------------------------------------------------------------------
// Reference: one fixed 8-bit pass (Result.cpp:5,91).  Here: the fewest radix bits such that the
// average build-side partition fills at most 15/16 of one LDS hash table (BJ_CHUNK), in <= 2 passes.
// device_resident: the inputs are in HBM already (rhj_join_dev); else the host-pointer call, whose small path is one launch
// largest average partition (tuples, either side) JK_CT_G13 is chosen for
u64 g13_upto()
{
    // 15/16 of its table: the row guards stop paying beyond CT_GUARDED_UPTO, but half as many partitions still do ([measured, wall
    // ms, 5120 -> 5760] 43M 1.852 -> 1.760 . 46M 1.894 -> 1.710 . 86M 3.364 -> 3.164 . 93M 3.459 -> 3.363 . 170M 6.732 -> 6.097 . 185M 7.082 -> 6.297)
    static const u64 v = env_u64("RHJ_G13_UPTO", (u64)join_table_tuples(JK_CT_G13) * 15 / 16, 2048, 5760);      // tuning aid
    return v;
}

bool default_join_kernels(const rhj_ctx *ctx) { return ctx->opt_big_kernel < 0 && ctx->opt_big_tables < 0; }

// ct13_ok: the join may pick the JK_CT_G13 compact-table kernel for plans of 13-15 bits (default kernel choice, not the
// multi-GPU receiver): the plan then leaves partitions of up to CT_GUARDED_UPTO tuples
int resolve_plan(u64 nR, u64 nS, const rhj_opts *in, rhj_opts *out, bool device_resident = false, bool ct13_ok = true)
{
    rhj_opts o;
    if (in) o = *in; else rhj_default_opts(&o);
    const u64 nb = nR < nS ? nR : nS;
    const u64 fit = (u64)BJ_FIT;
    if (o.passes < -1 || o.passes > 2 || o.bits1 < 0 || o.bits2 < 0 || o.bits1 > PART_MAX_BITS ||
        o.bits2 > PART_MAX_BITS || o.probe_split < 0)
        return RHJ_E_INVALID;
    if (o.passes == -1) {
        if (o.bits1 > 0) o.passes = o.bits2 > 0 ? 2 : 1;
        else {
            int bits = 0;
            const u64 np_ = nR < nS ? nS : nR;
            // small joins stay unpartitioned (one launch, every probe tile re-builds the few table chunks): a partition
            // pass costs ~6 launches per relation, more than such a join itself
            const bool direct = nb <= (device_resident ? DIRECT_MAX_BUILD_DEV : DIRECT_MAX_BUILD) && np_ <= DIRECT_MAX_PROBE;
            if (nb > (u64)BJ_CHUNK && !direct) bits = ilog2_ceil((nb + fit - 1) / fit);
            if (bits == 0) o.passes = 0;
            else if (bits <= 9) { o.passes = 1; o.bits1 = bits; }
            // Up to two and a half JK_BKT_BIG chunks per partition after ONE 9-bit pass (three launches; the chunked
            // 16-byte-entry kernel joins): a two-pass plan costs ~27 launches, 0.2 ms of fixed latency that such a join does
            // not have to spare.  [measured, round 4, wall ms one pass / two] 8.5M 0.43 / 0.50 . 10M 0.51 / 0.54 . 12M 0.61 / 0.59
            else if (nb <= (u64)512 * 5 * join_table_tuples(JK_BKT_BIG) * 15 / 32) { o.passes = 1; o.bits1 = 9; }
            else {
                // Two passes.  Up to 16 bits both histograms come from ONE read of the input (k_hist2d_units); a 17- or
                // 18-bit plan re-reads each relation once more just to count (10.7 instead of 5.4 ms per 10^9-tuple join).
                // Partitions that 16 bits leave larger than one 16-byte-entry table go to the compact-table bucket join
                // (one JK_CT_13 table, both sides read once), which costs less than that extra read: measured at
                // 10^9 x 10^9, 8+8 bits 43 ms against 49 ms for 9+9.  Beyond 1.1 * 10^9 tuples per side a 16-bit partition
                // no longer fits ONE compact table (chunks: probe payloads streamed again per chunk) and 9+9 bits (the
                // widest line-aligned write-combining scatter) takes over: 2.2 * 10^9 x 2.2 * 10^9, 121.6 against 125.3 ms.
                // 17 bits (9+8) while the average partition stays inside one compact table (its probe side inside one task of 16 or
                // 20 slots per thread), 18 (9+9) beyond; both run in the narrow format with 16-tuple carry lines in their 9-bit passes (k_scatter_wcn
                // <GR = 16>) and a second, 8 B/tuple histogram read of the narrow intermediate.
                if (bits > 16) bits = nb <= (u64)65536 * 16800 ? 16 : nb <= (u64)131072 * 16800 ? 17 : 18;
                // One bit fewer where that leaves partitions for the JK_CT_G13 compact-table kernel (k_join_ct<.., KB = 13>, plans
                // of 13-15 bits, average partitions of up to 15/16 of its table on both sides): half as many partitions,
                // tasks and histogram rows.  [measured, one box, wall ms, bits as above -> one fewer] 34M 1.538 -> 1.431 . 40M 1.722 ->
                // 1.579 . 66M 2.814 -> 2.538 . 83M 3.397 -> 2.971 . 135M 5.692 -> 5.091 . 165M 6.729 -> 6.084
                static const bool ct13_env = env_u64("RHJ_CT13", 1, 0, 1) != 0;
                if (ct13_ok && ct13_env && bits - 1 >= join_ct_min_radix_bits(JK_CT_G13) && bits - 1 < join_ct_min_radix_bits(JK_CT) &&
                    (nb >> (bits - 1)) <= g13_upto() && (np_ >> (bits - 1)) <= g13_upto())
                    bits -= 1;
                o.passes = 2; o.bits1 = (bits + 1) / 2; o.bits2 = bits / 2;
                // 17 bits: the 9-bit pass second -- from the narrow intermediate it costs 5.3 ms per 10^9 tuples, from 16-byte
                // tuples 7.9 ([measured] 9+8 against 8+9 at 1.5 * 10^9: 68.4 against 65.2 ms)
                if (bits == 17) { o.bits1 = 8; o.bits2 = 9; }
            }
        }
    }
    if (o.passes == 0) { o.bits1 = 0; o.bits2 = 0; }
    if (o.passes == 1) { if (o.bits1 == 0) o.bits1 = 8; o.bits2 = 0; }
    if (o.passes == 2) { if (o.bits1 == 0) o.bits1 = 8; if (o.bits2 == 0) o.bits2 = 8; }
    if (o.probe_split == 0) {
        // enough tasks to fill 256 CUs even when nothing is partitioned, at most 32 Ki probe tuples each
        const u64 np = nR > nS ? nR : nS;
        u64 ps = (np + 1023) / 1024;
        ps = (ps + BJ_TILE - 1) / BJ_TILE * BJ_TILE;
        if (ps < (u64)BJ_TILE) ps = BJ_TILE;
        if (ps > 32768) ps = 32768;
        o.probe_split = (int32_t)ps;
    }
    *out = o;
    return RHJ_OK;
}

// whether the joins of this context take their radix digits from mix64(payload) (MIX_STORE) or from the raw payload
int join_mix(const rhj_ctx *ctx)
{
    static const int env = (int)env_u64("RHJ_MIX", 1, 0, 1);
    return (ctx->opt_mix >= 0 ? ctx->opt_mix : env) ? MIX_STORE : MIX_NONE;
}

PassGeom make_geom(u64 n, u32 nseg, int shift, int bits, u64 target_units = PART_TARGET_UNITS)
{
    PassGeom g;
    g.n = n;
    static const u64 forced_units = env_u64("RHJ_UNITS", 0, 1, 65536);                                   // tuning aid
    if (forced_units) target_units = forced_units;
    u64 L = (n + target_units - 1) / target_units;
    L = (L + PART_TILE - 1) / PART_TILE * PART_TILE;
    if (L < (u64)PART_TILE) L = PART_TILE;
    g.L = L;
    g.nseg = nseg;
    g.max_units = (u32)(n / L) + nseg;
    g.shift = shift;
    g.bits = bits;
    return g;
}

// One partition pass over all segments: histogram -> scan -> scatter.
// `whole_relation`: the pass has ONE segment [0,n) and d_seg_start is this context's seg0 buffer, which the pass then
// fills together with the unit table in one launch.
int run_pass(rhj_ctx *ctx, const void *d_in, void *d_out, u64 n, const u64 *d_seg_start, u32 nseg, int shift,
             int bits, u64 *d_part_start, bool whole_relation = false, int mix = MIX_NONE)
{
    PassGeom g = make_geom(n, nseg, shift, bits);
    g.mix = mix;
    const size_t nbins = (size_t)1 << bits;
    RHJCHK(ensure(ctx, ctx->unit_start, ((size_t)nseg + 1) * 4));
    RHJCHK(ensure(ctx, ctx->unit_hist, (size_t)g.max_units * nbins * 4));
    RHJCHK(ensure(ctx, ctx->unit_base, (size_t)g.max_units * nbins * 8));
    RHJCHK(ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(bits)));
    u32 *unit_start = (u32 *)ctx->unit_start.p;
    {
        Span s(ctx, RHJ_K_AUX);
        if (whole_relation) launch_init_single_segment(ctx->stream, n, g.L, (u64 *)ctx->seg0.p, unit_start);
        else launch_make_units(ctx->stream, d_seg_start, nseg, g.L, unit_start);
    }
    {
        Span s(ctx, RHJ_K_HIST);
        launch_hist_units(ctx->stream, d_in, g, d_seg_start, unit_start, (u32 *)ctx->unit_hist.p);
    }
    {
        Span s(ctx, RHJ_K_SCAN);
        launch_scan_units(ctx->stream, g, d_seg_start, unit_start, (const u32 *)ctx->unit_hist.p,
                          (u64 *)ctx->unit_base.p, d_part_start, (u64 *)ctx->scan_tmp.p);
    }
    {
        Span s(ctx, RHJ_K_SCATTER);
        launch_scatter_units(ctx->stream, d_in, d_out, g, d_seg_start, unit_start, (const u64 *)ctx->unit_base.p);
    }
    return check_launch(ctx, "partition pass");
}

// One pass over BOTH relations with shared launches (grid.y = relation): 6 launches instead of 12.  Mid-size joins
// (BASELINE config 2: 1M x 1M, one 8-bit pass) are bound by launch count and by 244-workgroup kernels that fill the
// chip only halfway.
int run_pass_pair(rhj_ctx *ctx, const void *d_R, u64 nR, void *outR, u64 *psR, const void *d_S, u64 nS, void *outS, u64 *psS,
                  int bits)
{
    const size_t nbins = (size_t)1 << bits;
    PassPairHost h;
    DevBuf *seg[2] = {&ctx->seg0, &ctx->seg0_b}, *ust[2] = {&ctx->unit_start, &ctx->unit_start_b},
           *uh[2] = {&ctx->unit_hist, &ctx->unit_hist_b}, *ub[2] = {&ctx->unit_base, &ctx->unit_base_b},
           *sc[2] = {&ctx->scan_tmp, &ctx->scan_tmp_b};
    const void *in[2] = {d_R, d_S};
    void *out[2] = {outR, outS};
    u64 *ps[2] = {psR, psS};
    const u64 n[2] = {nR, nS};
    for (int i = 0; i < 2; i++) {
        const PassGeom g = make_geom(n[i], 1, 0, bits);
        RHJCHK(ensure(ctx, *seg[i], 64));
        RHJCHK(ensure(ctx, *ust[i], 16));
        RHJCHK(ensure(ctx, *uh[i], (size_t)g.max_units * nbins * 4));
        RHJCHK(ensure(ctx, *ub[i], (size_t)g.max_units * nbins * 8));
        RHJCHK(ensure(ctx, *sc[i], scan_tmp_bytes(bits)));
        h.side[i] = PassSide{in[i], out[i], (u64 *)seg[i]->p, (u32 *)ust[i]->p, (u32 *)uh[i]->p, (u64 *)ub[i]->p, ps[i],
                             (u64 *)sc[i]->p, g};
    }
    // the first launch also clears the join counters (one memset less in front of a join that is ~10 launches in all)
    RHJCHK(ensure(ctx, ctx->counters, 64));
    h.zero8 = (u64 *)ctx->counters.p;
    h.mix = join_mix(ctx);                               // (only joins come through here)
    ctx->counters_clean = true;
    static const int kinds[4] = {RHJ_K_AUX, RHJ_K_HIST, RHJ_K_SCAN, RHJ_K_SCATTER};
    for (int phase = 0; phase < 4; phase++) {
        Span s(ctx, kinds[phase]);
        launch_pass_pair(ctx->stream, h, 0, bits, phase);
    }
    return check_launch(ctx, "paired partition pass");
}

// Two passes with ONE histogram read (k_hist2d_units): used when both passes fit the write-combining scatter
// and b1 + b2 <= 16.  Pass-2 units = pieces of each pass-1 bucket written by groups of pass-1 units.
// narrow: 0 = 16-byte tuples throughout; 1 = pass 2 writes the narrow format (what the join kernel then reads); 2 = pass 1 too
// Input: 16-byte tuples (in.aos), the same relation as columns (in.cols: the histogram and pass 1 read them directly, narrow
// level 1 or 2, exact cursors or count-free; everything behind pass 1 is unchanged), or -- the multi-GPU receiver -- narrow arrays that arrived in nseg sender segments
// (in.P / in.K / in.seg_off; narrow is then 2): pass-1 units are cut at the segment boundaries and pass 2 writes the sender
// number into the low payload bits (k_scatter_wcn's WnTag), which the join kernels resolve into global rowIDs.
// the scratch tables one relation's fused two-pass partition works in, and the stream it runs on
struct PartScratch {
    DevBuf *seg0, *unit_start, *unit_hist, *unit_base, *scan_tmp, *hist2, *grp_rng, *unit_start2, *ps_1, *part_tmp, *seg_rng;
    hipStream_t st;
};
PartScratch first_scratch(rhj_ctx *ctx)
{
    return PartScratch{&ctx->seg0, &ctx->unit_start, &ctx->unit_hist, &ctx->unit_base, &ctx->scan_tmp, &ctx->hist2, &ctx->grp_rng,
                       &ctx->unit_start2, &ctx->ps_1, &ctx->part_tmp, &ctx->seg_rng, ctx->stream};
}
PartScratch second_scratch(rhj_ctx *ctx)
{
    return PartScratch{&ctx->seg0_b, &ctx->unit_start_b, &ctx->unit_hist_b, &ctx->unit_base_b, &ctx->scan_tmp_b, &ctx->hist2_b, &ctx->grp_rng_b,
                       &ctx->unit_start2_b, &ctx->ps_1_b, &ctx->part_tmp_b, &ctx->seg_rng, ctx->aux_stream};
}

struct FusedIn {
    const void *aos = nullptr;
    ColsIn cols;                       // ... or (cols.val != nullptr) the caller's relation as columns: rhj_join_cols_dev
    const u64 *P = nullptr;
    const u32 *K = nullptr;
    int nseg = 0;
    const u64 *seg_off = nullptr;      // host, nseg + 1
    // what pass 2 writes (segmented input): 0 narrow, rowIDs as they came; 1 narrow, sender tag in the low payload bits;
    // 2 16-byte tuples with global rowIDs key_bases[sender] + rowID32 (key_bases: device, 16 u64)
    int final_form = 0;
    const u64 *key_bases = nullptr;
};

// the pass-1 units and groups of a fused two-pass partition of one unsegmented relation
void fused_units(u64 n, int b1, PassGeom &g1, u32 &units1, u32 &per, u32 &ngroups)
{
    static const u32 want_groups = (u32)env_u64("RHJ_GROUPS", 16, 1, 64);                          // tuning aid
    // 1024 pass-1 units instead of 2048: every unit flushes a 2^(b1+b2)-bin table, and the scatter does not care
    // ([measured] at 10^9 tuples: histogram 2.54 against 2.74 ms, scatter within noise)
    g1 = make_geom(n, 1, 0, b1, PART_TARGET_UNITS / 2);
    units1 = (u32)((n + g1.L - 1) / g1.L);
    per = units1 ? (units1 + want_groups - 1) / want_groups : 1;
    ngroups = units1 ? (units1 + per - 1) / per : 1;
}

// Count-free pass 1: the regions.  cap = the mean run of a unit, m = L / 2^b1, plus ten standard deviations of a hashed digit's
// count (sqrt(m)), rounded up to whole 32-tuple lines: at the headline's L = 978,944 that is 4448 for a mean of 3824 (+16 %; the
// largest of its 2 x 261,376 runs is 4116).  Small relations (L bottoms out at one tile) get regions far above 16 n bytes:
// the intermediate buffer is sized from the regions, the margin is never cut.
CfGeom cf_geometry(u64 n, int b1)
{
    PassGeom g1;
    CfGeom c;
    fused_units(n, b1, g1, c.U, c.per, c.ngroups);
    const double m = (double)g1.L / (double)((u64)1 << b1);
    c.cap = (u32)(((u64)(m + 10.0 * std::sqrt(m)) + 1 + 31) / 32 * 32);
    c.slots = ((u64)c.U << b1) * c.cap;
    return c;
}
size_t cf_tmp_bytes(const CfGeom &c) { return (size_t)c.slots * 12; }
// Count-free pass 2, one writer per final partition: the regions.  cap2 = the mean final partition, m2 = n / 2^(b1 + b2), plus ten
// standard deviations of a hashed digit's count, rounded up to whole 32-tuple lines (headline: 16,512 for a mean of 15,259, +8 %:
// 12.98 GB per relation); every region starts on a 128-byte line of both final arrays and no line has two writers.
Cf2Geom cf2_geometry(u64 n, int b1, int b2)
{
    Cf2Geom c;
    const u64 np = (u64)1 << (b1 + b2);
    const double m = (double)n / (double)np;
    c.cap2 = (u32)(((u64)(m + 10.0 * std::sqrt(m)) + 1 + 31) / 32 * 32);
    c.slots = np * c.cap2;
    return c;
}
// the case it applies to: 16-byte input, narrow level 2, digits of mix64(payload), both passes of at most 8 bits
bool cf_applies(u64 n, int b1, int b2, int narrow, int mix, bool segs)
{
    if (segs || narrow != 2 || mix != MIX_STORE || b1 > 8 || b2 > 8 || n == 0) return false;
    const CfGeom c = cf_geometry(n, b1);
    return c.per <= cf_per_max() && (double)c.slots * 12.0 < 1.0e12;
}

// mix (16-byte input only): MIX_STORE inside a join -- the histogram and pass 1 take their digits from mix64(payload) and pass 1
// writes the mixed value, so that pass 2 and the bucket join work on it unchanged
// cf_side >= 0: pass 1 runs without counts where cf_applies() (that side's bit of the skip word reports a run that did not fit)
// d_end2 (with a count-free pass 1 only; cf2_end_for): pass 2 has one writer per final partition -- d_out is sized for the regions
// of cf2_geometry(), d_ps receives the region starts and d_end2 the partitions' ends
int partition_relation_fused(rhj_ctx *ctx, const FusedIn &in, u64 n, int b1, int b2, void *d_out, u64 *d_ps, int narrow = 0,
                             int mix = MIX_NONE, const PartScratch *scratch = nullptr, int cf_side = -1, u64 *d_end2 = nullptr)
{
    // the scratch tables and the stream of this relation: the context's first set on its stream, or -- R and S of a mid-size
    // join partitioned side by side -- the second set on the auxiliary stream (partition_phase)
    const PartScratch sc = scratch ? *scratch : first_scratch(ctx);
    DevBuf &x_seg0 = *sc.seg0, &x_unit_start = *sc.unit_start, &x_unit_hist = *sc.unit_hist, &x_unit_base = *sc.unit_base,
           &x_scan_tmp = *sc.scan_tmp, &x_hist2 = *sc.hist2, &x_grp_rng = *sc.grp_rng, &x_unit_start2 = *sc.unit_start2,
           &x_ps_1 = *sc.ps_1, &x_part_tmp = *sc.part_tmp, &x_seg_rng = *sc.seg_rng;
    const hipStream_t st = sc.st;
    const bool segs = in.P != nullptr, cols = in.cols.val != nullptr;
    PassGeom g1 = make_geom(n, 1, 0, b1, PART_TARGET_UNITS / 2);           // (see fused_units)
    g1.mix = segs ? MIX_NONE : mix;
    static const u32 want_groups = (u32)env_u64("RHJ_GROUPS", 16, 1, 64);                          // tuning aid
    u32 units1, per, ngroups, groups_per_seg = 0;
    u64 segL[16] = {0};
    if (segs) {
        if (in.nseg < 1 || in.nseg > seg_max() || narrow != 2 || b1 < tag_bits() || in.final_form < 0 || in.final_form > 2 ||
            (in.final_form == 2 && !in.key_bases))
            return fail(ctx, RHJ_E_INVALID, "segmented input: 1..16 segments, narrow format, pass 1 of at least 4 bits");
        groups_per_seg = want_groups / (u32)in.nseg ? want_groups / (u32)in.nseg : 1u;
        ngroups = groups_per_seg * (u32)in.nseg;
        per = (u32)(PART_TARGET_UNITS / 2) / ngroups ? (u32)(PART_TARGET_UNITS / 2) / ngroups : 1u;
        const u32 units_per_seg = groups_per_seg * per;
        units1 = units_per_seg * (u32)in.nseg;
        for (int s_ = 0; s_ < in.nseg; s_++) {
            const u64 len = in.seg_off[s_ + 1] - in.seg_off[s_];
            u64 L = (len + units_per_seg - 1) / units_per_seg;
            L = (L + PART_TILE - 1) / PART_TILE * PART_TILE;
            segL[s_] = L ? L : (u64)PART_TILE;
        }
    } else {
        PassGeom same;
        fused_units(n, b1, same, units1, per, ngroups);
    }
    const size_t nb1 = (size_t)1 << b1, nb2 = (size_t)1 << b2;
    const u32 units2 = (u32)(nb1 * ngroups);
    const bool cf = cf_side >= 0 && cf_applies(n, b1, b2, narrow, mix, segs);
    const CfGeom cg = cf ? cf_geometry(n, b1) : CfGeom();
    RHJCHK(ensure(ctx, x_seg0, 64));
    RHJCHK(ensure(ctx, x_unit_start, 16));
    RHJCHK(ensure(ctx, x_unit_hist, (size_t)(units1 + 1) * nb1 * 4));
    RHJCHK(ensure(ctx, x_unit_base, (size_t)((units1 + 1) * nb1 > units2 * nb2 ? (units1 + 1) * nb1 : units2 * nb2) * 8));
    RHJCHK(ensure(ctx, x_scan_tmp, scan_tmp_bytes(b1)));
    RHJCHK(ensure(ctx, x_hist2, (size_t)units2 * nb2 * 4));
    RHJCHK(ensure(ctx, x_grp_rng, ((size_t)units2 + 1) * 8));
    RHJCHK(ensure(ctx, x_unit_start2, (nb1 + 1) * 4));
    RHJCHK(ensure(ctx, x_part_tmp, cf && cf_tmp_bytes(cg) > (size_t)n * 16 ? cf_tmp_bytes(cg) : (size_t)(n ? n : 1) * 16));
    RHJCHK(ensure(ctx, x_ps_1, (nb1 + 1) * 8));
    if (segs) RHJCHK(ensure(ctx, x_seg_rng, ((size_t)units1 + 1) * 8));
    if (cf) {
        RHJCHK(ensure(ctx, ctx->cf_cnt1, (size_t)units1 * nb1 * 4));
        RHJCHK(ensure(ctx, ctx->cf_pre, cf_pre_words(units2) * 4));
        RHJCHK(ensure(ctx, ctx->cf_tot, (size_t)units2 * 4));
    }
    u64 *seg0 = (u64 *)x_seg0.p;
    u32 *unit_start1 = (u32 *)x_unit_start.p;
    const u64 *rng1 = segs ? (const u64 *)x_seg_rng.p : nullptr;
    u32 *wide = narrow ? (u32 *)ctx->narrow_flag.p : nullptr;
    PassGeom gs = g1;                                   // (segmented: the scan only needs the unit count)
    gs.max_units = units1;
    {
        Span s(ctx, RHJ_K_AUX);
        if (segs) launch_seg_units(st, (u32)in.nseg, in.seg_off, segL, groups_per_seg * per, (u64 *)x_seg_rng.p, seg0, unit_start1);
        else launch_init_single_segment(st, n, g1.L, seg0, unit_start1);          // seg0 = {0,n}, unit_start1 = {0, units1}
        if (!cf) HIPCHK(ctx, hipMemsetAsync(x_hist2.p, 0, (size_t)units2 * nb2 * 4, st));
    }
    DupSniff sn;
    if (ctx->sniff_side >= 0) {                         // a join's relation: sample its join values for duplicates
        const int side = ctx->sniff_side;
        sn.tab = (u32 *)ctx->sniff_tab.p + (size_t)side * SNIFF_SLOTS;
        sn.sel_bits = sniff_sel_bits(n);
        ctx->sniff_n[side] = n;
        Span s(ctx, RHJ_K_AUX);
        HIPCHK(ctx, hipMemsetAsync(sn.tab, 0, (size_t)SNIFF_SLOTS * 4, st));
    }
    if (cf) {
        // No histogram of the 16-byte input: pass 1 into fixed regions, the piece tables, pass 2's histogram over the narrow
        // payloads, today's pass-2 scan and scatter.  d_ps and the contents of every final partition are the exact path's.
        ctx->last_cf[cf_side] = 1;
        const u32 *pre = (const u32 *)ctx->cf_pre.p;
        {
            Span s(ctx, RHJ_K_SCATTER);
            if (cols) launch_cf_pass1_cols(st, in.cols, x_part_tmp.p, cg, g1, seg0, unit_start1, (u32 *)ctx->cf_cnt1.p, wide, 2u << cf_side, sn);
            else launch_cf_pass1(st, in.aos, x_part_tmp.p, cg, g1, seg0, unit_start1, (u32 *)ctx->cf_cnt1.p, wide, 2u << cf_side, sn);
        }
        if (d_end2) {                                   // no piece tables, no histogram, no scan: pass 2 builds its prefix itself
            Span s(ctx, RHJ_K_SCATTER);
            launch_cf2_pass2(st, x_part_tmp.p, d_out, cg, cf2_geometry(n, b1, b2), (u32)nb1, b1, b2, (const u32 *)ctx->cf_cnt1.p, d_ps,
                             d_end2, wide, 8u << cf_side);
            return check_launch(ctx, "count-free two-pass partition");
        }
        {
            Span s(ctx, RHJ_K_AUX);
            launch_cf_tables(st, cg, (u32)nb1, (const u32 *)ctx->cf_cnt1.p, (u32 *)ctx->cf_pre.p, (u32 *)ctx->cf_tot.p,
                             (u64 *)x_ps_1.p, (u32 *)x_unit_start2.p, wide);
        }
        {
            Span s(ctx, RHJ_K_HIST);
            launch_cf_hist2(st, x_part_tmp.p, cg, (u32)nb1, b1, b2, pre, (u32 *)x_hist2.p, wide);
        }
        PassGeom g2;
        g2.n = n; g2.L = 0; g2.nseg = (u32)nb1; g2.max_units = units2; g2.shift = b1; g2.bits = b2;
        {
            Span s(ctx, RHJ_K_SCAN);
            launch_scan_units(st, g2, (const u64 *)x_ps_1.p, (const u32 *)x_unit_start2.p, (const u32 *)x_hist2.p,
                              (u64 *)x_unit_base.p, d_ps, nullptr);
        }
        {
            Span s(ctx, RHJ_K_SCATTER);
            launch_cf_pass2(st, x_part_tmp.p, d_out, n, cg, (u32)nb1, b1, b2, (const u64 *)x_unit_base.p, pre, wide);
        }
        return check_launch(ctx, "count-free two-pass partition");
    }
    {
        Span s(ctx, RHJ_K_HIST);                        // (16-byte input: also reports a rowID that does not fit the narrow format)
        if (cols)
            launch_hist2d_units_cols(st, in.cols, n, g1.L, units1, b1, b2, per, ngroups, (u32 *)x_unit_hist.p, (u32 *)x_hist2.p, wide,
                                     g1.mix, sn);
        else
            launch_hist2d_units(st, segs ? (const void *)in.P : in.aos, segs, n, g1.L, units1, b1, b2, per, ngroups,
                                (u32 *)x_unit_hist.p, (u32 *)x_hist2.p, 0, wide, rng1, g1.mix, sn);
    }
    {
        Span s(ctx, RHJ_K_SCAN);
        launch_scan_units(st, gs, seg0, unit_start1, (const u32 *)x_unit_hist.p, (u64 *)x_unit_base.p,
                          (u64 *)x_ps_1.p, (u64 *)x_scan_tmp.p);
    }
    {
        Span s(ctx, RHJ_K_SCATTER);
        if (segs)
            launch_scatter_ranges_narrow(st, in.P, true, x_part_tmp.p, n, units1, 0, b1, (const u64 *)x_unit_base.p,
                                         rng1, wide, 0, 0, in.K);
        else if (cols && narrow == 2)
            launch_scatter_units_narrow_cols(st, in.cols, x_part_tmp.p, n, g1, seg0, unit_start1, (const u64 *)x_unit_base.p, wide);
        else if (cols)
            launch_scatter_units_cols(st, in.cols, x_part_tmp.p, g1, seg0, unit_start1, (const u64 *)x_unit_base.p);
        else if (narrow == 2)
            launch_scatter_units_narrow(st, in.aos, x_part_tmp.p, n, g1, seg0, unit_start1, (const u64 *)x_unit_base.p,
                                        wide);
        else
            launch_scatter_units(st, in.aos, x_part_tmp.p, g1, seg0, unit_start1, (const u64 *)x_unit_base.p);
    }
    {
        Span s(ctx, RHJ_K_AUX);
        launch_make_group_ranges(st, (const u64 *)x_unit_base.p, (u32)nb1, per, ngroups, n, (u64 *)x_grp_rng.p,
                                 (u32 *)x_unit_start2.p);
    }
    PassGeom g2;
    g2.n = n; g2.L = 0; g2.nseg = (u32)nb1; g2.max_units = units2; g2.shift = b1; g2.bits = b2;
    {
        Span s(ctx, RHJ_K_SCAN);
        launch_scan_units(st, g2, (const u64 *)x_ps_1.p, (const u32 *)x_unit_start2.p, (const u32 *)x_hist2.p,
                          (u64 *)x_unit_base.p, d_ps, nullptr);
    }
    {
        Span s(ctx, RHJ_K_SCATTER);
        if (segs && in.final_form == 2)
            launch_scatter_ranges_n2a(st, x_part_tmp.p, d_out, n, units2, b1, b2, (const u64 *)x_unit_base.p,
                                      (const u64 *)x_grp_rng.p, in.key_bases, ngroups, groups_per_seg, wide);
        else if (narrow)
            launch_scatter_ranges_narrow(st, x_part_tmp.p, narrow == 2, d_out, n, units2, b1, b2,
                                         (const u64 *)x_unit_base.p, (const u64 *)x_grp_rng.p, wide,
                                         segs && in.final_form == 1 ? ngroups : 0u, segs && in.final_form == 1 ? groups_per_seg : 0u);
        else
            launch_scatter_ranges(st, x_part_tmp.p, d_out, units2, b1, b2, (const u64 *)x_unit_base.p,
                                  (const u64 *)x_grp_rng.p);
    }
    return check_launch(ctx, "fused two-pass partition");
}

int partition_relation_fused(rhj_ctx *ctx, const void *d_in, u64 n, int b1, int b2, void *d_out, u64 *d_ps, int narrow = 0,
                             int mix = MIX_NONE, const PartScratch *scratch = nullptr, int cf_side = -1)
{
    FusedIn in;
    in.aos = d_in;
    return partition_relation_fused(ctx, in, n, b1, b2, d_out, d_ps, narrow, mix, scratch, cf_side);
}

// Two narrow passes with SEPARATE histograms (plans of 17-18 bits: 2^(b1+b2) packed counters do not fit the LDS, so the
// histogram of pass 2 is a second read -- of the narrow intermediate, 8 B/tuple): 16-byte tuples -> narrow part_tmp -> narrow
// d_out.  A rowID >= 2^32 raises ctx->narrow_flag in pass 1 (every later kernel of the join returns at once).
// d_inK != nullptr: the input is narrow already (d_in = payloads, d_inK = rowIDs: a received shard whose rowIDs are global).
int partition_relation_narrow2(rhj_ctx *ctx, const void *d_in, u64 n, int b1, int b2, void *d_out, u64 *d_ps,
                               const u32 *d_inK = nullptr, int mix = MIX_NONE)
{
    RHJCHK(ensure(ctx, ctx->seg0, 64));
    RHJCHK(ensure(ctx, ctx->part_tmp, (size_t)(n ? n : 1) * 16));
    RHJCHK(ensure(ctx, ctx->ps_1, (((size_t)1 << b1) + 1) * 8));
    u32 *wide = (u32 *)ctx->narrow_flag.p;
    for (int pass = 0; pass < 2; pass++) {
        const int bits = pass ? b2 : b1, shift = pass ? b1 : 0;
        const u32 nseg = pass ? 1u << b1 : 1u;
        const u64 *seg_start = pass ? (const u64 *)ctx->ps_1.p : (const u64 *)ctx->seg0.p;
        u64 *part_start = pass ? d_ps : (u64 *)ctx->ps_1.p;
        PassGeom g = make_geom(n, nseg, shift, bits);
        g.mix = (!pass && !d_inK) ? mix : MIX_NONE;       // (the 16-byte input of pass 1; from there on the mixed value is the payload)
        const size_t nbins = (size_t)1 << bits;
        RHJCHK(ensure(ctx, ctx->unit_start, ((size_t)nseg + 1) * 4));
        RHJCHK(ensure(ctx, ctx->unit_hist, (size_t)g.max_units * nbins * 4));
        RHJCHK(ensure(ctx, ctx->unit_base, (size_t)g.max_units * nbins * 8));
        RHJCHK(ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(bits)));
        u32 *unit_start = (u32 *)ctx->unit_start.p;
        {
            Span s(ctx, RHJ_K_AUX);
            if (!pass) launch_init_single_segment(ctx->stream, n, g.L, (u64 *)ctx->seg0.p, unit_start);
            else launch_make_units(ctx->stream, seg_start, nseg, g.L, unit_start);
        }
        DupSniff sn;
        if (!pass && !d_inK && ctx->sniff_side >= 0) {  // a join's relation: sample its join values for duplicates
            sn.tab = (u32 *)ctx->sniff_tab.p + (size_t)ctx->sniff_side * SNIFF_SLOTS;
            sn.sel_bits = sniff_sel_bits(n);
            ctx->sniff_n[ctx->sniff_side] = n;
            Span s(ctx, RHJ_K_AUX);
            HIPCHK(ctx, hipMemsetAsync(sn.tab, 0, (size_t)SNIFF_SLOTS * 4, ctx->stream));
        }
        {
            Span s(ctx, RHJ_K_HIST);
            if (!pass && !d_inK) launch_hist_units(ctx->stream, d_in, g, seg_start, unit_start, (u32 *)ctx->unit_hist.p, nullptr, sn);
            else launch_hist_units_narrow(ctx->stream, pass ? ctx->part_tmp.p : d_in, g, seg_start, unit_start, (u32 *)ctx->unit_hist.p);
        }
        {
            Span s(ctx, RHJ_K_SCAN);
            launch_scan_units(ctx->stream, g, seg_start, unit_start, (const u32 *)ctx->unit_hist.p, (u64 *)ctx->unit_base.p,
                              part_start, (u64 *)ctx->scan_tmp.p);
        }
        {
            Span s(ctx, RHJ_K_SCATTER);
            void *out = pass ? d_out : ctx->part_tmp.p;
            launch_scatter_units_narrow_any(ctx->stream, pass ? ctx->part_tmp.p : d_in,
                                            pass ? narrow_ids(ctx->part_tmp.p, n) : d_inK,
                                            out, (u32 *)((unsigned char *)out + narrow_k_offset(n)), g, seg_start, unit_start,
                                            (const u64 *)ctx->unit_base.p, wide);
        }
    }
    return check_launch(ctx, "two-pass narrow partition");
}

// Partition one relation with `passes` passes into d_out; boundaries into d_ps[2^(b1+b2) + 1].
int partition_relation(rhj_ctx *ctx, const void *d_in, u64 n, int passes, int b1, int b2, void *d_out, u64 *d_ps, int mix = MIX_NONE)
{
    if (passes == 2 && fused_two_pass_ok(b1, b2) && n > 0 && n < ((u64)1 << 32))
        return partition_relation_fused(ctx, d_in, n, b1, b2, d_out, d_ps, 0, mix);
    RHJCHK(ensure(ctx, ctx->seg0, 64));
    u64 *seg0 = (u64 *)ctx->seg0.p;                 // {0, n}: written by the first pass itself
    if (passes == 1) return run_pass(ctx, d_in, d_out, n, seg0, 1, 0, b1, d_ps, true, mix);
    RHJCHK(ensure(ctx, ctx->part_tmp, (size_t)(n ? n : 1) * 16));
    RHJCHK(ensure(ctx, ctx->ps_1, (((size_t)1 << b1) + 1) * 8));
    RHJCHK(run_pass(ctx, d_in, ctx->part_tmp.p, n, seg0, 1, 0, b1, (u64 *)ctx->ps_1.p, true, mix));
    return run_pass(ctx, ctx->part_tmp.p, d_out, n, (const u64 *)ctx->ps_1.p, 1u << b1, b1, b2, d_ps);
}

// Which bucket-join kernel a partitioned join runs (JoinKernel).
// Average build partition larger than one JK_BKT table (an explicit plan with too few bits, or more than 2^30
// tuples): the compact-table kernel when the plan removed enough payload bits for 48-bit keys, else JK_BKT_BIG
// chunks.  The compact-table kernel keeps a task's probe rowIDs in registers, so a task is at most that many tuples.
// allow13: plans of 13-15 bits may take the compact-table kernel with 13-bit arrival indices (keys of up to 51 bits) for
// average partitions of 2-5 K tuples (not the multi-GPU receiver, whose sender tags the one-table kernel resolves).
int choose_join_kind(const rhj_ctx *ctx, u64 nR, u64 nS, u64 nparts, int radix_bits, bool narrow = false, bool allow13 = true)
{
    const u64 nbuild = nR < nS ? nR : nS, nprobe = nR < nS ? nS : nR, ab = nbuild / nparts, ap = nprobe / nparts;   // (nparts >= 1: every caller)
    // the average partition fits kind k's table AND its probe tasks (a partition cut into two tasks builds its table twice)
    auto fits = [&](int k) { return ab <= (u64)join_table_tuples(k) * 15 / 16 && ap <= (u64)join_probe_split(k) * 15 / 16; };
    if (radix_bits < join_ct_min_radix_bits(JK_CT) && radix_bits >= join_ct_min_radix_bits(JK_CT_Q12) && allow13 &&
        (ctx->opt_big_kernel < 0 || ctx->opt_big_kernel == JK_CT_Q12) && (radix_bits == join_ct_min_radix_bits(JK_CT_Q12) || ctx->opt_big_kernel == JK_CT_Q12)) {
        // plans of exactly 12 bits (and a forced kernel 11 from 12 bits on): JK_CT_Q12's table with 12-bit arrival indices
        static const bool on12 = env_u64("RHJ_CT13", 1, 0, 1) != 0;
        if ((ctx->opt_big_kernel == JK_CT_Q12 && ctx->opt_big_tables == 1) ||
            (on12 && ctx->opt_big_tables < 0 && ab > (u64)CT_GUARDED_FROM && fits(JK_CT_Q12)))
            return JK_CT_Q12;
    }
    if (radix_bits < join_ct_min_radix_bits(JK_CT) && radix_bits >= join_ct_min_radix_bits(JK_CT_G13) && allow13 &&
        (ctx->opt_big_kernel < 0 || ctx->opt_big_kernel == JK_CT_G13)) {
        static const bool on = env_u64("RHJ_CT13", 1, 0, 1) != 0;              // tuning aid: 0 = the one-table kernel as before
        if ((ctx->opt_big_kernel == JK_CT_G13 && ctx->opt_big_tables == 1) ||
            (on && ctx->opt_big_tables < 0 && ab > (u64)CT_GUARDED_FROM && fits(JK_CT_G13) && ab <= g13_upto() && ap <= g13_upto()))
            return JK_CT_G13;
    }
    // ... and from half a table on when the plan allows the compact-table kernel: its JK_CT_HALF_MID_G geometry (row guards)
    // handles a tuple in two thirds of the one-table kernel's time ([measured] 1.5 - 2.7 * 10^8 tuples under 16 bits)
    const bool ct_ok = radix_bits >= join_ct_min_radix_bits(JK_CT) && ctx->opt_big_kernel != JK_BKT_BIG;
    const u64 big_from = ct_ok ? (u64)CT_GUARDED_FROM : (u64)BJ_CHUNK;
    if (!(ctx->opt_big_tables == 1 || (ctx->opt_big_tables < 0 && ab > big_from))) return JK_BKT;
    if (radix_bits < join_ct_min_radix_bits(JK_CT) || ctx->opt_big_kernel == JK_BKT_BIG) return JK_BKT_BIG;
    if (jk_is_ct(ctx->opt_big_kernel) && !jk_ct_narrow_only(ctx->opt_big_kernel)) return ctx->opt_big_kernel;
    if (ctx->opt_big_kernel == JK_CT_WIDE) return narrow ? JK_CT_WIDE : JK_CT_13;
    if (ctx->opt_big_kernel == JK_CT_HALF_WIDE) return narrow ? JK_CT_HALF_WIDE : JK_CT_HALF;
    // the compact-table kernel at half size (two workgroups per CU) while the average partition fits
    // JK_CT_HALF_MID: partitions of up to 5.76 K tuples; with row guards while two or more rows stay empty
    if (fits(JK_CT_HALF_MID)) return ab <= (u64)CT_GUARDED_UPTO && ap <= (u64)CT_GUARDED_UPTO ? JK_CT_HALF_MID_G : JK_CT_HALF_MID;
    if (fits(JK_CT_HALF)) return JK_CT_HALF;
    // 20 probe slots per thread (narrow partitions only) before a partition's probe side is cut into two tasks that build the
    // table twice: [measured] 2.2 * 10^9 x 2.2 * 10^9, join kernel 32.5 ms with two 16-slot tasks per partition
    if (narrow && fits(JK_CT_HALF_WIDE)) return JK_CT_HALF_WIDE;
    if (fits(JK_CT_MID)) return JK_CT_MID;           // 12 + 12 slot rows instead of 18 + 16 for partitions of up to 11.5 K tuples
    if (fits(JK_CT)) return JK_CT;                   // (up to 1.005 * 10^9 tuples under 16 bits)
    if (fits(JK_CT_13)) return JK_CT_13;             // the larger table in half the buckets
    if (narrow && fits(JK_CT_WIDE)) return JK_CT_WIDE;
    return JK_CT_13;
}

bool narrow_fused_plan(const rhj_opts &plan)
{
    return fused_two_pass_ok(plan.bits1, plan.bits2) && narrow_pass_ok(plan.bits1) && narrow_pass_ok(plan.bits2);
}

// The narrow intermediate format applies to fused two-pass plans (both passes <= 8 bits) whose bucket join is the one-table
// kernel or the compact-table kernel, for relations of < 2^32 tuples (rowIDs that CAN be 32 bits; whether they are is
// found out on the device).  Returns the level (0 = not at all).
int narrow_level(const rhj_ctx *ctx, u64 nR, u64 nS, const rhj_opts &plan)
{
    static const int env = (int)env_u64("RHJ_NARROW", 2, 0, 2);
    const int want = ctx->opt_narrow >= 0 ? ctx->opt_narrow : env;
    if (want <= 0 || ctx->narrow_off_once || plan.passes != 2) return 0;
    if (ctx->opt_narrow < 0 && ctx->narrow_skip > 0) return 0;              // backing off after repeated wide rowIDs (automatic mode only)
    const bool fused = narrow_fused_plan(plan);
    // plans beyond 16 bits: two narrow passes with separate histograms (level 2 only), 9-bit passes in the 16-tuple-line geometry
    if (!fused && !(want >= 2 && plan.bits1 + plan.bits2 > 16 && narrow_pass9_ok(plan.bits1) && narrow_pass9_ok(plan.bits2))) return 0;
    const u64 lo = nR < nS ? nR : nS, hi = nR < nS ? nS : nR;
    if (lo < NARROW_MIN_TUPLES || hi >= ((u64)1 << 32)) return 0;
    const int tb = plan.bits1 + plan.bits2;
    const int kind = choose_join_kind(ctx, nR, nS, (u64)1 << tb, tb, true);
    if (kind == JK_BKT_BIG) return 0;
    // the narrow scatter has one 1024-thread workgroup per CU and 32-tuple lines to start and finish per digit and unit:
    // below a few million tuples its fixed costs outweigh the bytes it saves (forced levels, used by the tests, skip this)
    static const u64 min_auto = env_u64("RHJ_NARROW_MIN", NARROW_AUTO_MIN_TUPLES, 0, ~0ull);
    if (ctx->opt_narrow < 0 && hi < min_auto) return 0;
    return want >= 2 ? 2 : 1;
}

// Small unpartitioned joins run as ONE launch without a task list (k_join_bkt DIRECT).
bool is_direct(const rhj_ctx *ctx, u64 nparts, u64 nR, u64 nS)
{
    return nparts == 1 && ctx->opt_big_tables != 1 && (nR < nS ? nR : nS) <= DIRECT_MAX_BUILD &&
           (nR < nS ? nS : nR) <= DIRECT_MAX_PROBE;
}

// "partition.countfree" as it stands: the option, else RHJ_COUNTFREE=0 / 1 in the environment (A/B aid), else -1 (automatic)
// no side of the current partitions lies in regions with gaps, and none took the one-writer pass 2
void clear_gaps(rhj_ctx *ctx)
{
    for (int side = 0; side < 2; side++) { ctx->last_cf2[side] = 0; ctx->cur_end[side] = nullptr; ctx->cur_slots[side] = 0; }
}
int cf_want(const rhj_ctx *ctx)
{
    static const int env = getenv("RHJ_COUNTFREE") ? (int)env_u64("RHJ_COUNTFREE", 0, 0, 1) : -1;
    return ctx->opt_countfree >= 0 ? ctx->opt_countfree : env;
}

// R and S of a fused two-pass plan side by side on two streams: device-resident joins (nothing to upload in between) of at
// most 2^28 tuples per side (the second pass-1 intermediate costs 16 B per tuple of S), not while profiling (spans are timed
// on one stream).  RHJ_TWO_STREAMS=0 switches it off.
bool two_streams_ok(const rhj_ctx *ctx, u64 nR, u64 nS, const rhj_opts &plan, std::function<int()> *before_S)
{
    static const bool on = env_u64("RHJ_TWO_STREAMS", 1, 0, 1) != 0;
    if (!on || ctx->prof.on || (before_S && *before_S)) return false;
    // forced count-free pass 1, or the repeat of a side that overflowed: the one-stream path carries both
    if (cf_want(ctx) == 1 || ctx->cf_keep_R || ctx->cf_off_once[0] || ctx->cf_off_once[1] || ctx->cf2_off_once[0] || ctx->cf2_off_once[1])
        return false;
    if (plan.passes != 2 || !fused_two_pass_ok(plan.bits1, plan.bits2)) return false;
    if (ctx->cur_narrow && !narrow_fused_plan(plan)) return false;
    const u64 hi = nR > nS ? nR : nS, lo = nR > nS ? nS : nR;
    return lo > 0 && hi <= ((u64)1 << 28);
}

// Count-free pass 1 for this side of this join?  (Only the one-stream path of partition_phase asks: the two-stream mid-size
// path, the pipelined host path and the multi-GPU receiver keep exact cursors.)  Returns the side, or -1.
constexpr u64 CF_AUTO_MIN_TUPLES = (u64)1 << 28;       // automatic mode: the larger relation has more tuples than this
int cf_side_for(rhj_ctx *ctx, int side, u64 nR, u64 nS, const rhj_opts &plan, int mix)
{
    const int want = cf_want(ctx);
    if (want == 0 || ctx->cf_off_once[side] || ctx->cur_narrow != 2 || !narrow_fused_plan(plan)) return -1;
    if (!cf_applies(side ? nS : nR, plan.bits1, plan.bits2, ctx->cur_narrow, mix, false)) return -1;
    if (want < 0 && (nR > nS ? nR : nS) <= CF_AUTO_MIN_TUPLES) return -1;
    if (ctx->cf_skip[side] > 0) { ctx->cf_skip[side]--; return -1; }          // backing off after a fall-back of this side
    return side;
}

// "partition.countfree2" as it stands: the option, else RHJ_COUNTFREE2=0 / 1 in the environment (A/B aid), else -1 (automatic)
int cf2_want(const rhj_ctx *ctx)
{
    static const int env = getenv("RHJ_COUNTFREE2") ? (int)env_u64("RHJ_COUNTFREE2", 0, 0, 1) : -1;
    return ctx->opt_countfree2 >= 0 ? ctx->opt_countfree2 : env;
}
// Automatic mode of the one-writer pass 2: where the automatic count-free pass 1 is on (DESIGN 4.20 says what was measured).
constexpr bool CF2_AUTO = true;
// the case a one-writer pass 2 applies to, given that the count-free pass 1 applies: one workgroup per pass-1 bucket fills the
// device (fewer leave compute units idle), and the bucket's U piece lengths fit the kernel's prefix table
bool cf2_applies(const rhj_ctx *ctx, u64 n, int b1, int b2)
{
    if (ctx->num_cus <= 0 || ((u64)1 << b1) < (u64)ctx->num_cus) return false;
    const CfGeom c = cf_geometry(n, b1);                  // (the kernel addresses a slot inside its bucket with 32 bits)
    return c.U <= CF2_PRE - 1 && (u64)c.U * c.cap < ((u64)1 << 31) && (double)cf2_geometry(n, b1, b2).slots * 12.0 < 1.0e12;
}
// Count-free pass 2 for this side of this pair join?  cf_side: what cf_side_for() answered for it.  d_end: the side's end array
// (buffers grown, ctx->cur_end / cur_slots / last_cf2 set), or null: exact boundaries.
int cf2_end_for(rhj_ctx *ctx, int side, int cf_side, u64 nR, u64 nS, const rhj_opts &plan, u64 *&d_end)
{
    d_end = nullptr;
    const int want = cf2_want(ctx);
    const u64 n = side ? nS : nR;
    if (cf_side < 0 || want == 0 || ctx->cf2_off_once[side] || !cf2_applies(ctx, n, plan.bits1, plan.bits2)) return RHJ_OK;
    if (want < 0 && (!CF2_AUTO || (nR > nS ? nR : nS) <= CF_AUTO_MIN_TUPLES)) return RHJ_OK;
    if (ctx->cf2_skip[side] > 0) { ctx->cf2_skip[side]--; return RHJ_OK; }    // backing off after a fall-back of this side
    const Cf2Geom c2 = cf2_geometry(n, plan.bits1, plan.bits2);
    RHJCHK(ensure(ctx, side ? ctx->part_S : ctx->part_R, cf2_part_bytes(c2)));
    RHJCHK(ensure(ctx, ctx->cf2_end[side], (size_t)8 << (plan.bits1 + plan.bits2)));
    d_end = (u64 *)ctx->cf2_end[side].p;
    ctx->cur_end[side] = d_end;
    ctx->cur_slots[side] = c2.slots;
    ctx->last_cf2[side] = 1;
    return RHJ_OK;
}

// A relation of a columnar join (rhj_join_cols_dev; a 16-byte call passes through both unchanged).  fused_input: for
// partition_relation_fused, whose first kernels read the columns themselves ("last.cols" 1).  cols_to_aos: for every other path --
// d becomes the side's 16-byte copy in the workspace, converted by one linear kernel the first time the call asks ("last.cols" 2).
FusedIn fused_input(rhj_ctx *ctx, int side, const void *d)
{
    FusedIn in;
    in.aos = d;
    if (!d && ctx->cols_in[side].val) { in.cols = ctx->cols_in[side]; ctx->last_cols[side] = 1; }   // (d != nullptr: converted already)
    return in;
}
int cols_to_aos(rhj_ctx *ctx, int side, u64 n, const void *&d)
{
    if (!ctx->cols_in[side].val) return RHJ_OK;
    ctx->last_cols[side] = 2;
    if (!ctx->cols_aos_done[side]) {
        RHJCHK(ensure(ctx, ctx->cols_aos[side], (size_t)(n ? n : 1) * 16));
        Span s(ctx, RHJ_K_AUX);
        launch_cols_to_tuples(ctx->stream, ctx->cols_in[side], n, ctx->cols_aos[side].p);
        ctx->cols_aos_done[side] = true;
    }
    d = ctx->cols_aos[side].p;
    return RHJ_OK;
}
int cols_to_aos(rhj_ctx *ctx, u64 nR, const void *&d_R, u64 nS, const void *&d_S)
{
    RHJCHK(cols_to_aos(ctx, 0, nR, d_R));
    return cols_to_aos(ctx, 1, nS, d_S);
}

// Partition phase of a join: leaves ctx->cur_* describing partitioned R and S.
// before_S (optional, consumed by the first call that gets it): invoked once, after the kernels that partition R have been
// enqueued and before anything reads S -- rhj_join uploads S there, so that S crosses PCIe while R is being partitioned
// (plans that push both relations through the same launches call it first).
// ctx->call.one_sided (a group-by): R alone is partitioned, under the plan, the format and the count-free choice of a join of (nR, nS = nR)
// -- S is skipped explicitly: no kernel reads or writes a buffer of S, part_S is not grown, nothing is sampled (one side has no tie
// to break), R takes the one-stream path and, under a one-pass plan, run_pass instead of the paired launches.  cur_S is null.
// gaps_ok: the consumer is the pair join's join_phase, which takes partitions in regions with gaps (cf2_end_for); every other
// consumer reads contiguous partitions under exact boundaries.
int partition_phase(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, const rhj_opts &plan,
                    std::function<int()> *before_S = nullptr, bool gaps_ok = false)
{
    const bool one = ctx->call.one_sided;
    ctx->sniff_ready = false;
    auto s_ready = [&]() -> int {
        if (!before_S || !*before_S) return RHJ_OK;
        std::function<int()> f;
        f.swap(*before_S);
        return f();
    };
    ctx->cur_nR = nR;
    ctx->cur_nS = nS;
    ctx->cur_probe_split = (u32)plan.probe_split;
    ctx->last.passes = plan.passes;
    ctx->last.bits1 = plan.bits1;
    ctx->last.bits2 = plan.bits2;
    ctx->counters_clean = false;
    ctx->cur_narrow = narrow_level(ctx, nR, nS, plan);
    const bool keep_R = ctx->cf_keep_R;
    if (!keep_R && !ctx->cf_off_once[0]) ctx->last_cf[0] = 0;
    if (!ctx->cf_off_once[1]) ctx->last_cf[1] = 0;
    for (int side = keep_R ? 1 : 0; side < 2; side++) {
        if (!ctx->cf2_off_once[side]) ctx->last_cf2[side] = 0;
        ctx->cur_end[side] = nullptr;
        ctx->cur_slots[side] = 0;
    }
    if (ctx->cur_narrow) {
        RHJCHK(ensure(ctx, ctx->narrow_flag, 64));
        Span s(ctx, RHJ_K_AUX);
        HIPCHK(ctx, hipMemsetAsync(ctx->narrow_flag.p, 0, 64, ctx->stream));
    }
    // a columnar join: the fused two-pass path in a narrow format reads the columns; every other path takes 16-byte copies
    if (!(plan.passes == 2 && ctx->cur_narrow && narrow_fused_plan(plan))) {
        if (one) RHJCHK(cols_to_aos(ctx, 0, nR, d_R));
        else RHJCHK(cols_to_aos(ctx, nR, d_R, nS, d_S));
    }
    if (plan.passes == 0) {
        RHJCHK(s_ready());
        RHJCHK(ensure(ctx, ctx->ps_R, 64));
        RHJCHK(ensure(ctx, ctx->ps_S, 64));
        if (!is_direct(ctx, 1, nR, nS)) {                               // boundaries {0, n} for the task list (the direct launch needs none)
            Span s(ctx, RHJ_K_AUX);
            launch_init_single_segment(ctx->stream, nR, PART_TILE, (u64 *)ctx->ps_R.p, (u32 *)((u64 *)ctx->ps_R.p + 4));
            if (!one) launch_init_single_segment(ctx->stream, nS, PART_TILE, (u64 *)ctx->ps_S.p, (u32 *)((u64 *)ctx->ps_S.p + 4));
        }
        ctx->cur_R = d_R;
        ctx->cur_S = one ? nullptr : d_S;
        ctx->cur_nparts = 1;
        ctx->cur_radix_bits = 0;
    } else {
        const int tb = plan.bits1 + (plan.passes == 2 ? plan.bits2 : 0);
        const size_t np = (size_t)1 << tb;
        const int mix = join_mix(ctx);
        RHJCHK(ensure(ctx, ctx->ps_R, (np + 1) * 8));
        RHJCHK(ensure(ctx, ctx->ps_S, (np + 1) * 8));
        RHJCHK(ensure(ctx, ctx->part_R, (size_t)(nR ? nR : 1) * 16));
        if (!one) RHJCHK(ensure(ctx, ctx->part_S, (size_t)(nS ? nS : 1) * 16));
        if (ctx->cur_narrow && !narrow_fused_plan(plan)) {
            const bool sniff = sniff_on(ctx) && !one;
            if (sniff) RHJCHK(ensure(ctx, ctx->sniff_tab, (size_t)2 * SNIFF_SLOTS * 4));
            ctx->sniff_side = sniff ? 0 : -1;
            int prc = partition_relation_narrow2(ctx, d_R, nR, plan.bits1, plan.bits2, ctx->part_R.p, (u64 *)ctx->ps_R.p, nullptr, mix);
            if (prc == RHJ_OK) prc = s_ready();
            ctx->sniff_side = sniff ? 1 : -1;
            if (prc == RHJ_OK && !one)
                prc = partition_relation_narrow2(ctx, d_S, nS, plan.bits1, plan.bits2, ctx->part_S.p, (u64 *)ctx->ps_S.p, nullptr, mix);
            ctx->sniff_side = -1;
            RHJCHK(prc);
            ctx->sniff_ready = sniff;
        } else if (!one && two_streams_ok(ctx, nR, nS, plan, before_S)) {
            // Mid-size joins are launch-bound (a fused two-pass partition is ~11 short dependent launches per relation): R and S
            // are independent until the join, so S is partitioned on a second stream, in a second set of scratch tables, while R
            // runs on the first -- the gaps between one relation's launches are filled by the other's kernels.
            if (!ctx->aux_stream) {
                HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
                for (int i = 0; i < 2; i++) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->aux_ev[i], hipEventDisableTiming));
            }
            const bool sniff = sniff_on(ctx);
            if (sniff) RHJCHK(ensure(ctx, ctx->sniff_tab, (size_t)2 * SNIFF_SLOTS * 4));
            HIPCHK(ctx, hipEventRecord(ctx->aux_ev[0], ctx->stream));             // (the inputs, the cleared flag: everything so far)
            HIPCHK(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->aux_ev[0], 0));
            const PartScratch s2 = second_scratch(ctx);
            ctx->sniff_side = sniff ? 0 : -1;
            int prc = partition_relation_fused(ctx, fused_input(ctx, 0, d_R), nR, plan.bits1, plan.bits2, ctx->part_R.p, (u64 *)ctx->ps_R.p,
                                               ctx->cur_narrow, mix);
            ctx->sniff_side = sniff ? 1 : -1;
            if (prc == RHJ_OK)
                prc = partition_relation_fused(ctx, fused_input(ctx, 1, d_S), nS, plan.bits1, plan.bits2, ctx->part_S.p, (u64 *)ctx->ps_S.p,
                                               ctx->cur_narrow, mix, &s2);
            ctx->sniff_side = -1;
            RHJCHK(prc);
            ctx->sniff_ready = sniff;
            HIPCHK(ctx, hipEventRecord(ctx->aux_ev[1], ctx->aux_stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->aux_ev[1], 0));
        } else if (ctx->cur_narrow) {
            const bool sniff = sniff_on(ctx) && !one;
            if (sniff) RHJCHK(ensure(ctx, ctx->sniff_tab, (size_t)2 * SNIFF_SLOTS * 4));
            ctx->sniff_side = sniff ? 0 : -1;
            int prc = RHJ_OK;
            u64 *end2 = nullptr;
            if (!keep_R) {                                      // (the repeat after an overflow of S alone: R stands, samples included)
                const int cfs = cf_side_for(ctx, 0, nR, nS, plan, mix);
                if (gaps_ok && !one) prc = cf2_end_for(ctx, 0, cfs, nR, nS, plan, end2);
                if (prc == RHJ_OK)
                    prc = partition_relation_fused(ctx, fused_input(ctx, 0, d_R), nR, plan.bits1, plan.bits2, ctx->part_R.p,
                                                   (u64 *)ctx->ps_R.p, ctx->cur_narrow, mix, nullptr, cfs, end2);
            }
            if (prc == RHJ_OK) prc = s_ready();
            ctx->sniff_side = sniff ? 1 : -1;
            if (prc == RHJ_OK && !one) {
                const int cfs = cf_side_for(ctx, 1, nR, nS, plan, mix);
                end2 = nullptr;
                if (gaps_ok) prc = cf2_end_for(ctx, 1, cfs, nR, nS, plan, end2);
                if (prc == RHJ_OK)
                    prc = partition_relation_fused(ctx, fused_input(ctx, 1, d_S), nS, plan.bits1, plan.bits2, ctx->part_S.p,
                                                   (u64 *)ctx->ps_S.p, ctx->cur_narrow, mix, nullptr, cfs, end2);
            }
            ctx->sniff_side = -1;
            RHJCHK(prc);
            ctx->sniff_ready = sniff;
        } else if (!one && plan.passes == 1 && plan.bits1 <= PASS_PAIR_MAX_BITS) {
            RHJCHK(s_ready());
            RHJCHK(run_pass_pair(ctx, d_R, nR, ctx->part_R.p, (u64 *)ctx->ps_R.p, d_S, nS, ctx->part_S.p, (u64 *)ctx->ps_S.p,
                                 plan.bits1));
        } else {
            RHJCHK(partition_relation(ctx, d_R, nR, plan.passes, plan.bits1, plan.bits2, ctx->part_R.p, (u64 *)ctx->ps_R.p, mix));
            RHJCHK(s_ready());
            if (!one) RHJCHK(partition_relation(ctx, d_S, nS, plan.passes, plan.bits1, plan.bits2, ctx->part_S.p, (u64 *)ctx->ps_S.p, mix));
        }
        ctx->cur_R = ctx->part_R.p;
        ctx->cur_S = one ? nullptr : ctx->part_S.p;
        ctx->cur_nparts = np;
        ctx->cur_radix_bits = tb;
    }
    ctx->cur_psR = (const u64 *)ctx->ps_R.p;
    ctx->cur_psS = (const u64 *)ctx->ps_S.p;
    return check_launch(ctx, "partition phase");
}

// Join phase on explicit partitioned inputs.  Synchronises to read the exact result count.
// narrow: the partitions are narrow arrays; tag_base (device, 2 x 16 u64; narrow only): the low payload bits name the sender
// of a tuple and rowIDs are local to it (multi-GPU receiver).  allow_direct: the boundaries are known to be {0, n}.
int join_phase_on(rhj_ctx *ctx, const void *d_Rp, const u64 *d_psR, u64 nR, const void *d_Sp, const u64 *d_psS,
                  u64 nS, u64 nparts, int radix_bits, u32 probe_split, void *d_out, u64 cap, u64 *out_count, bool narrow = false,
                  const u64 *d_tag_base = nullptr, bool allow_direct = true, bool check_radix = false, bool keep_count = false,
                  bool enqueue_only = false, bool allow13 = true, const PartEnds &pe = PartEnds(), u64 slotsR = 0, u64 slotsS = 0)
{
    // pe / slotsR / slotsS (narrow only): a side's partitions lie in regions with gaps -- its end array, and the slots
    // of its final arrays, which place the rowID array (0: the side's tuple count, as always)
    // keep_count: the result counter goes on from where the previous join on this context left it (the pairs of several joins
    // land behind one another in d_out); enqueue_only: no read-back, the caller collects the counters itself
    if (probe_split == 0) probe_split = 32768;
    // a task addresses its build range with 32 bits; k_make_tasks reports any partition whose build side is larger
    // (counters[5], checked below) whatever the plan
    const int kind = choose_join_kind(ctx, nR, nS, nparts, radix_bits, narrow, allow13);
    if (narrow && kind != JK_BKT && !jk_is_ct(kind))
        return fail(ctx, RHJ_E_INVALID, "no bucket-join kernel for narrow partitions under this plan");
    if (join_probe_split(kind) && probe_split > join_probe_split(kind)) probe_split = join_probe_split(kind);
    // the kernels address a task's probe side through a buffer descriptor of 32-bit byte size (16 B per tuple)
    if (probe_split > BJ_MAX_PROBE_SPLIT) probe_split = BJ_MAX_PROBE_SPLIT;
    const u64 max_tasks64 = nparts + (nR + nS) / probe_split + 1;
    if (max_tasks64 > 0x7fffffffull) return fail(ctx, RHJ_E_INVALID, "too many join tasks");
    const u32 max_tasks = (u32)max_tasks64;
    RHJCHK(ensure(ctx, ctx->tasks, (size_t)max_tasks * sizeof(JoinTask)));
    RHJCHK(ensure(ctx, ctx->counters, 64));
    u64 *d_count = (u64 *)ctx->counters.p;
    u32 *d_ntasks = (u32 *)(d_count + 1);
    if (keep_count) {
        Span s(ctx, RHJ_K_AUX);
        HIPCHK(ctx, hipMemsetAsync((unsigned char *)ctx->counters.p + 8, 0, 56, ctx->stream));
    } else if (!ctx->counters_clean) {               // (a paired partition pass has cleared them already)
        Span s(ctx, RHJ_K_AUX);
        HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
    }
    ctx->counters_clean = false;
    const bool direct = allow_direct && !narrow && is_direct(ctx, nparts, nR, nS);
    ctx->last_join_kind = direct ? -1 : kind;
    if (check_radix && !direct && jk_is_ct(kind)) {       // counters[6]: the partitions break the radix_bits contract
        Span s(ctx, RHJ_K_AUX);
        launch_check_radix(ctx->stream, d_Rp, d_psR, d_Sp, d_psS, nparts, radix_bits, d_count + 6, pe);
    }
    if (direct) {
        Span s(ctx, RHJ_K_JOIN);                                     // small unpartitioned join: one launch, no task list
        launch_join_direct(ctx->stream, d_Rp, nR, d_Sp, nS, d_out, d_out ? cap : 0, d_count);
    } else {
        {
            Span s(ctx, RHJ_K_TASKS);
            SniffVerdict sv;                                        // (the partition phase of THIS join sampled both sides: ask them)
            if (ctx->sniff_ready && ctx->sniff_n[0] == nR && ctx->sniff_n[1] == nS) {
                sv.tab = (const u32 *)ctx->sniff_tab.p;
                sv.expect_R = (u32)(nR >> sniff_sel_bits(nR));
                sv.expect_S = (u32)(nS >> sniff_sel_bits(nS));
            }
            ctx->sniff_ready = false;
            launch_make_tasks(ctx->stream, d_psR, d_psS, nparts, probe_split, (JoinTask *)ctx->tasks.p, d_ntasks, max_tasks,
                              d_count + 2, kind, sv, pe);           // counters[2..3]: largest partition of R, S
        }
        {
            Span s(ctx, RHJ_K_JOIN);
            launch_join(ctx->stream, d_Rp, d_psR, d_Sp, d_psS, (const JoinTask *)ctx->tasks.p, d_ntasks, max_tasks,
                        radix_bits, d_out, d_out ? cap : 0, d_count, kind,
                        narrow ? narrow_ids(d_Rp, slotsR ? slotsR : nR) : nullptr,
                        narrow ? narrow_ids(d_Sp, slotsS ? slotsS : nS) : nullptr,
                        d_tag_base, narrow ? (const u32 *)ctx->narrow_flag.p : nullptr);
        }
    }
    RHJCHK(check_launch(ctx, "join phase"));
    if (enqueue_only) return RHJ_OK;
    u64 host[7] = {0, 0, 0, 0, 0, 0, 0};       // count, ntasks, max |R_k|, max |S_k|, (checksum scratch), oversized build side, contract
    u32 wide_rowid = 0;
    HIPCHK(ctx, hipMemcpyAsync(host, ctx->counters.p, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    if (narrow) HIPCHK(ctx, hipMemcpyAsync(&wide_rowid, ctx->narrow_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (wide_rowid & 1u) return RHJ_RETRY_WIDE;                  // a rowID did not fit 32 bits: nothing of this run is valid
    if (wide_rowid) { ctx->cf_over = wide_rowid; return RHJ_RETRY_CF; }   // a count-free pass 1 met a run longer than its region
    *out_count = host[0];
    ctx->last.ntasks = (u32)(host[1] & 0xffffffffu);
    ctx->last_max_part[0] = direct ? 0 : host[2];
    ctx->last_max_part[1] = direct ? 0 : host[3];
    if (host[5])
        return fail(ctx, RHJ_E_INVALID, "a partition's build side has " + std::to_string(host[5]) +
                                        " tuples (>= 2^32): use more radix bits");
    if (host[6])
        return fail(ctx, RHJ_E_INVALID, "rhj_bucket_join: the payloads of a partition do not share their low radix_bits bits "
                                        "(radix_bits must be the number of low payload bits that are constant inside every partition)");
    return RHJ_OK;
}

int join_phase(rhj_ctx *ctx, void *d_out, u64 cap, u64 *out_count)
{
    PartEnds pe;
    pe.endR = ctx->cur_end[0]; pe.endS = ctx->cur_end[1]; pe.nR = ctx->cur_nR; pe.nS = ctx->cur_nS;
    return join_phase_on(ctx, ctx->cur_R, ctx->cur_psR, ctx->cur_nR, ctx->cur_S, ctx->cur_psS, ctx->cur_nS,
                         ctx->cur_nparts, ctx->cur_radix_bits, ctx->cur_probe_split, d_out, cap, out_count, ctx->cur_narrow != 0,
                         nullptr, true, false, false, false, true, pe, ctx->cur_slots[0], ctx->cur_slots[1]);
}

// What a join reports once both sides are partitioned: the pairs (join_phase), the rowIDs of the tuples of R with (RHJ_SEMI) or
// without (RHJ_ANTI) a partner in S (semi_phase), the pair count and sums over the pairs (agg_phase), or every row of R's
// multiplicity in S (mult_phase).
// OUT_GROUP: one row per distinct join value of R alone (group_phase; partition_phase in its one-sided mode).
// OUT_GJOIN: one row per join value of R join S, with the counts and sums of both sides (gjoin_phase).
// OUT_OUTER: the pairs, then {row, RHJ_NO_ROW} for the tuples of the preserved side(s) without a partner (outer_phase).
// OUT_LOOKUP: one partner rowID of S per row of R, the smallest or the largest (lookup_phase).
enum JoinOutput { OUT_PAIRS = -1, OUT_SEMI = RHJ_SEMI, OUT_ANTI = RHJ_ANTI, OUT_SUMS = 2, OUT_MULT = 3, OUT_GROUP = 4, OUT_GJOIN = 5, OUT_OUTER = 6, OUT_LOOKUP = 7 };

// ---- the scaffold of the keyed-table phases: semi_phase, outer_sweep, agg_phase, mult_phase, lookup_phase, group_phase, gjoin_phase ----
// Each builds a task list with k_make_semi_tasks over the partitions ctx->cur_* describe, launches its own kernel over it and reads
// the join counters back.  keyed_begin is everything in front of the kernel, keyed_finish everything behind it up to the words the
// phase interprets itself.  Stream order: counters, agg_out, the empty boundaries of a missing table side, the operator's fill, the
// single segments, the task list, the kernel.
constexpr u32 NEVER_CUT = 0xffffffffu;                 // a split cap: a partition is never cut -- its keys would be emitted twice
enum KeyedClear {
    CLEAR_COUNTERS,                                    // the 64 counter bytes, unless a paired partition pass has cleared them already
    CLEAR_COUNTERS_AGG,                                // ... and agg_out's 64, on EVERY attempt: a repeat (count-free overflow, wide rowID) starts from nothing
    CLEAR_TAIL                                         // counter words 1..7: word 0, the result counter, goes on (outer_sweep; cf. join_phase_on's keep_count)
};
struct Keyed {                                         // what keyed_begin leaves for the launch and for keyed_finish
    KeyedClear clear;
    bool narrow;
    u32 max_tasks;
    const JoinTask *tasks;
    const u32 *ntasks;                                 // counters[1]
    u64 *count, *max_tables;                           // counters[0], counters[7]
    u64 *agg;                                          // agg_out's words (CLEAR_COUNTERS_AGG, else null) ...
    u32 *bad;                                          // ... and the guard flags among them
    const u32 *skip;                                   // the narrow flag word, or null
};

// split_cap: the most probe tuples per task the kernel takes (the context's probe split counts below it), or NEVER_CUT; rows: the probe
// side's tuples, which bound the task list; psP / psT: the boundaries of the probe side and of the table side -- psT null: there is no
// table side, its boundary array is ctx->ps_S, zeroed here (every partition empty, at 0); fill: the operator's own work between the
// clears and the task builder, inside the clears' span.
int keyed_begin(rhj_ctx *ctx, Keyed &k, KeyedClear clear, int kind, u32 split_cap, u64 rows, int anti, const u64 *psP, const u64 *psT,
                const std::function<int()> &fill = nullptr)
{
    const u64 nparts = ctx->cur_nparts;
    u32 split = split_cap;
    if (split_cap != NEVER_CUT) {
        split = ctx->cur_probe_split ? ctx->cur_probe_split : 32768;
        if (split > split_cap) split = split_cap;
    }
    const u64 max_tasks64 = nparts + rows / split + 1;
    if (max_tasks64 > 0x7fffffffull) return fail(ctx, RHJ_E_INVALID, "too many join tasks");
    const bool no_T = psT == nullptr;
    const size_t empty_bytes = (size_t)(nparts + 1) * 8;
    k.clear = clear;
    k.narrow = ctx->cur_narrow != 0;
    k.max_tasks = (u32)max_tasks64;
    RHJCHK(ensure(ctx, ctx->tasks, (size_t)k.max_tasks * sizeof(JoinTask)));
    if (clear != CLEAR_TAIL) RHJCHK(ensure(ctx, ctx->counters, 64));
    if (clear == CLEAR_COUNTERS_AGG) RHJCHK(ensure(ctx, ctx->agg_out, 64));
    if (no_T) { RHJCHK(ensure(ctx, ctx->ps_S, empty_bytes)); psT = (const u64 *)ctx->ps_S.p; }
    k.tasks = (const JoinTask *)ctx->tasks.p;
    k.count = (u64 *)ctx->counters.p;
    k.ntasks = (const u32 *)(k.count + 1);
    k.max_tables = k.count + 7;
    k.agg = clear == CLEAR_COUNTERS_AGG ? (u64 *)ctx->agg_out.p : nullptr;
    k.bad = k.agg ? (u32 *)(k.agg + AGG_MAX_COLS + 1) : nullptr;
    k.skip = k.narrow ? (const u32 *)ctx->narrow_flag.p : nullptr;
    if (clear != CLEAR_COUNTERS || !ctx->counters_clean) {
        Span s(ctx, RHJ_K_AUX);
        if (clear == CLEAR_TAIL) HIPCHK(ctx, hipMemsetAsync((unsigned char *)ctx->counters.p + 8, 0, 56, ctx->stream));
        else if (!ctx->counters_clean) HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
        if (k.agg) HIPCHK(ctx, hipMemsetAsync(ctx->agg_out.p, 0, 64, ctx->stream));
        if (no_T) HIPCHK(ctx, hipMemsetAsync(ctx->ps_S.p, 0, empty_bytes, ctx->stream));
        if (fill) RHJCHK(fill());
    }
    if (clear != CLEAR_TAIL) {                         // (a sweep runs behind a phase that has done all this)
        ctx->counters_clean = false;
        if (ctx->cur_radix_bits == 0) {                // unpartitioned: partition_phase writes the boundaries {0, n} for some sizes only
            Span s(ctx, RHJ_K_AUX);
            launch_init_single_segment(ctx->stream, ctx->cur_nR, PART_TILE, (u64 *)ctx->ps_R.p, (u32 *)((u64 *)ctx->ps_R.p + 4));
            if (!no_T) launch_init_single_segment(ctx->stream, ctx->cur_nS, PART_TILE, (u64 *)ctx->ps_S.p, (u32 *)((u64 *)ctx->ps_S.p + 4));
        }
        ctx->last_join_kind = kind;
        ctx->sniff_ready = false;                      // (the samples of the partition phase are not asked)
    }
    Span s(ctx, RHJ_K_TASKS);
    launch_make_semi_tasks(ctx->stream, psP, psT, nparts, split, anti, (JoinTask *)ctx->tasks.p, (u32 *)(k.count + 1), k.max_tasks, k.count + 2);
    return RHJ_OK;
}

// Behind the phase's kernel: the launch check, the counters (host[8]: count, ntasks, max |R_k|, max |S_k|, -, oversized table side, -,
// most tables or rounds of a task if > 1), agg_out's words (agg[8], where the phase has them) and the narrow flag in one synchronisation;
// the retry codes of join_phase_on; "last.ntasks" and "last.max_part_*".  A sweep (CLEAR_TAIL) gets its counters and adds them up itself.
int keyed_finish(rhj_ctx *ctx, const Keyed &k, const char *what, u64 *host, u64 *agg = nullptr)
{
    RHJCHK(check_launch(ctx, what));
    u32 wide_rowid = 0;
    memset(host, 0, 64);
    HIPCHK(ctx, hipMemcpyAsync(host, ctx->counters.p, 64, hipMemcpyDeviceToHost, ctx->stream));
    if (k.agg) {
        memset(agg, 0, 64);
        HIPCHK(ctx, hipMemcpyAsync(agg, ctx->agg_out.p, 64, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (k.narrow && k.clear != CLEAR_TAIL) HIPCHK(ctx, hipMemcpyAsync(&wide_rowid, ctx->narrow_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (k.clear == CLEAR_TAIL) return RHJ_OK;
    if (wide_rowid & 1u) return RHJ_RETRY_WIDE;                  // a rowID did not fit 32 bits: nothing of this run is valid
    if (wide_rowid) { ctx->cf_over = wide_rowid; return RHJ_RETRY_CF; }   // a count-free pass 1 met a run longer than its region
    ctx->last.ntasks = (u32)(host[1] & 0xffffffffu);
    ctx->last_max_part[0] = ctx->cur_nparts > 1 ? host[2] : 0;
    ctx->last_max_part[1] = ctx->cur_nparts > 1 ? host[3] : 0;
    return RHJ_OK;
}

// "last.semi_tables" / "last.group_rounds" of a task list: the kernels report only a task that built more than one
int keyed_rounds(const u64 *host, u32 ntasks) { return host[7] ? (int)host[7] : (ntasks ? 1 : 0); }

int part_too_large(rhj_ctx *ctx, const char *side, u64 n)
{
    return fail(ctx, RHJ_E_INVALID, std::string("a partition of ") + side + " has " + std::to_string(n) + " tuples (>= 2^32): use more radix bits");
}

// Semi / anti join phase on the partitions partition_phase left: k_make_semi_tasks + k_semi_bkt.  d_out: u64 rowIDs.
// A task's match bits are 4 KiB of LDS: SEMI_MAX_SPLIT tuples of R at most.
int semi_phase(rhj_ctx *ctx, JoinOutput what, void *d_out, u64 cap, u64 *out_count)
{
    Keyed k;
    RHJCHK(keyed_begin(ctx, k, CLEAR_COUNTERS, JK_SEMI, SEMI_MAX_SPLIT, ctx->cur_nR, what == OUT_ANTI, ctx->cur_psR, ctx->cur_psS));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_semi_join(ctx->stream, ctx->cur_R, ctx->cur_S, k.tasks, k.ntasks, k.max_tasks, ctx->cur_radix_bits, what == OUT_ANTI, (u64 *)d_out,
                         d_out ? cap : 0, k.count, k.max_tables, k.narrow ? narrow_ids(ctx->cur_R, ctx->cur_nR) : nullptr,
                         k.narrow ? narrow_ids(ctx->cur_S, ctx->cur_nS) : nullptr, k.skip);
    }
    u64 host[8];
    RHJCHK(keyed_finish(ctx, k, "semi join phase", host));
    *out_count = host[0];
    ctx->last_semi_tables = keyed_rounds(host, (u32)ctx->last.ntasks);
    if (host[5]) return part_too_large(ctx, "S", host[5]);
    return RHJ_OK;
}

// One anti sweep of an outer join over the partitions ctx->cur_* describe: the tuples of the preserved side -- R
// (side 0: the tables on S's partitions) or S (side 1: the roles exchanged, the tables on R's partitions) -- without a partner, as
// {rowID, NO_ROW} / {NO_ROW, rowID} behind whatever the result counter already counts.  *out_total: the counter after the sweep.
int outer_sweep(rhj_ctx *ctx, int side, void *d_out, u64 cap, u64 *out_total)
{
    const u64 nP = side ? ctx->cur_nS : ctx->cur_nR, nT = side ? ctx->cur_nR : ctx->cur_nS;
    const void *d_P = side ? ctx->cur_S : ctx->cur_R, *d_T = side ? ctx->cur_R : ctx->cur_S;
    Keyed k;
    RHJCHK(keyed_begin(ctx, k, CLEAR_TAIL, JK_SEMI, SEMI_MAX_SPLIT, nP, 1, side ? ctx->cur_psS : ctx->cur_psR, side ? ctx->cur_psR : ctx->cur_psS));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_outer_sweep(ctx->stream, d_P, d_T, k.tasks, k.ntasks, k.max_tasks, ctx->cur_radix_bits, side, d_out, d_out ? cap : 0, k.count,
                           k.max_tables, k.narrow ? narrow_ids(d_P, nP) : nullptr, k.narrow ? narrow_ids(d_T, nT) : nullptr, k.skip);
    }
    u64 host[8];
    RHJCHK(keyed_finish(ctx, k, "outer join sweep", host));
    *out_total = host[0];
    const u32 ntasks = (u32)(host[1] & 0xffffffffu);
    ctx->last.ntasks += ntasks;
    const int tables = keyed_rounds(host, ntasks);
    if (tables > ctx->last_semi_tables) ctx->last_semi_tables = tables;
    ctx->last_outer_sweeps++;
    if (host[5]) return part_too_large(ctx, side ? "R" : "S", host[5]);
    return RHJ_OK;
}

// Outer join phase on the partitions partition_phase left: join_phase -- whose retry codes come back before any sweep
// runs: the narrow flag is final once the partition kernels have ended --, then one outer_sweep per preserved side on the same stream
// and the same result counter.  The sections are the differences of the counter between the phases; a repeat starts from a zeroed
// counter (join_phase_on clears it) and produces every section again.
int outer_phase(rhj_ctx *ctx, void *d_out, u64 cap, u64 *out_count)
{
    ctx->last_outer_sweeps = 0;
    ctx->last_semi_tables = 0;
    ctx->outer_sections[0] = ctx->outer_sections[1] = ctx->outer_sections[2] = 0;
    const int rc = join_phase(ctx, d_out, cap, out_count);
    if (rc != RHJ_OK) return rc;
    const int pair_kind = ctx->last_join_kind;                           // "last.join_kernel": the pair kernel
    ctx->outer_sections[0] = *out_count;
    if (ctx->cur_radix_bits == 0) {                    // unpartitioned: partition_phase writes the boundaries {0, n} for some sizes only
        Span s(ctx, RHJ_K_AUX);
        launch_init_single_segment(ctx->stream, ctx->cur_nR, PART_TILE, (u64 *)ctx->ps_R.p, (u32 *)((u64 *)ctx->ps_R.p + 4));
        launch_init_single_segment(ctx->stream, ctx->cur_nS, PART_TILE, (u64 *)ctx->ps_S.p, (u32 *)((u64 *)ctx->ps_S.p + 4));
    }
    u64 before = *out_count;
    for (int side = 0; side < 2; side++) {
        if (!(ctx->call.outer_how & (1 << side))) continue;
        u64 total = before;
        RHJCHK(outer_sweep(ctx, side, d_out, cap, &total));
        ctx->outer_sections[1 + side] = total - before;
        before = total;
    }
    *out_count = before;
    ctx->last_join_kind = pair_kind;
    return RHJ_OK;
}

// Aggregating join phase on the partitions partition_phase left: k_make_semi_tasks (anti = 0) + k_agg_bkt over the
// weight columns of the call.  Retry codes as semi_phase.
int agg_phase(rhj_ctx *ctx, u64 *out_count)
{
    const CallArgs &a = ctx->call;
    Keyed k;
    RHJCHK(keyed_begin(ctx, k, CLEAR_COUNTERS_AGG, JK_AGG, AGG_MAX_SPLIT, ctx->cur_nR, 0, ctx->cur_psR, ctx->cur_psS));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_agg_join(ctx->stream, ctx->cur_R, ctx->cur_S, k.tasks, k.ntasks, k.max_tasks, ctx->cur_radix_bits, a.agg_cols, a.agg_ncols,
                        a.agg_col_rows, k.agg, k.bad, k.max_tables, k.narrow ? narrow_ids(ctx->cur_R, ctx->cur_nR) : nullptr,
                        k.narrow ? narrow_ids(ctx->cur_S, ctx->cur_nS) : nullptr, k.skip);
    }
    u64 host[8], agg[8];                               // agg: count, sums, guard flag
    RHJCHK(keyed_finish(ctx, k, "aggregating join phase", host, agg));
    ctx->last_semi_tables = keyed_rounds(host, (u32)ctx->last.ntasks);
    if (host[5]) return part_too_large(ctx, "S", host[5]);
    if ((u32)agg[AGG_MAX_COLS + 1])
        return fail(ctx, RHJ_E_INVALID, "a rowID of R is >= col_rows: the weight columns have no such row");
    *out_count = agg[0];
    for (u32 j = 0; j < a.agg_ncols; j++) a.agg_sums_out[j] = agg[1 + j];
    return RHJ_OK;
}

// Multiplicity join phase on the partitions partition_phase left: k_make_semi_tasks (anti = 0) + k_mult_bkt over the
// weights and the output words of the call.  EVERY attempt zeroes the output words too.  Retry codes as semi_phase.
int mult_phase(rhj_ctx *ctx, u64 *out_total)
{
    const CallArgs &a = ctx->call;
    Keyed k;
    RHJCHK(keyed_begin(ctx, k, CLEAR_COUNTERS_AGG, JK_MULT, AGG_MAX_SPLIT, ctx->cur_nR, 0, ctx->cur_psR, ctx->cur_psS, [&]() -> int {
        if (a.mult_out_rows) HIPCHK(ctx, hipMemsetAsync(a.mult_out, 0, a.mult_out_rows * 8, ctx->stream));
        return RHJ_OK;
    }));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_mult_join(ctx->stream, ctx->cur_R, ctx->cur_S, k.tasks, k.ntasks, k.max_tasks, ctx->cur_radix_bits, a.mult_w, a.mult_w_rows,
                         a.mult_out, a.mult_out_rows, k.agg, k.bad, k.max_tables, k.narrow ? narrow_ids(ctx->cur_R, ctx->cur_nR) : nullptr,
                         k.narrow ? narrow_ids(ctx->cur_S, ctx->cur_nS) : nullptr, k.skip);
    }
    u64 host[8], agg[8];                               // agg: total, -, -, -, -, guard flags
    RHJCHK(keyed_finish(ctx, k, "multiplicity join phase", host, agg));
    ctx->last_semi_tables = keyed_rounds(host, (u32)ctx->last.ntasks);
    if (host[5]) return part_too_large(ctx, "S", host[5]);
    const u32 bad = (u32)agg[AGG_MAX_COLS + 1];
    if (bad & MULT_BAD_ROW_R) return fail(ctx, RHJ_E_INVALID, "a rowID of R is >= out_rows: d_out has no such word");
    if (bad & MULT_BAD_ROW_S) return fail(ctx, RHJ_E_INVALID, "a rowID of S is >= wS_rows: the weight column has no such row");
    *out_total = agg[0];
    return RHJ_OK;
}

// Lookup join phase on the partitions partition_phase left: k_make_semi_tasks (anti = 0) + k_lookup_bkt over the output
// words of the call.  EVERY attempt fills the output words with all ones (RHJ_NO_ROW).  Retry codes as semi_phase.
int lookup_phase(rhj_ctx *ctx, u64 *out_matched)
{
    const CallArgs &a = ctx->call;
    Keyed k;
    RHJCHK(keyed_begin(ctx, k, CLEAR_COUNTERS_AGG, JK_LOOKUP, AGG_MAX_SPLIT, ctx->cur_nR, 0, ctx->cur_psR, ctx->cur_psS, [&]() -> int {
        if (a.mult_out_rows) HIPCHK(ctx, hipMemsetAsync(a.mult_out, 0xFF, a.mult_out_rows * 8, ctx->stream));
        return RHJ_OK;
    }));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_lookup_join(ctx->stream, ctx->cur_R, ctx->cur_S, k.tasks, k.ntasks, k.max_tasks, ctx->cur_radix_bits, a.lookup_which, a.mult_out,
                           a.mult_out_rows, k.agg, k.bad, k.max_tables, k.narrow ? narrow_ids(ctx->cur_R, ctx->cur_nR) : nullptr,
                           k.narrow ? narrow_ids(ctx->cur_S, ctx->cur_nS) : nullptr, k.skip);
    }
    u64 host[8], agg[8];                               // agg: matched, -, -, -, -, guard flags
    RHJCHK(keyed_finish(ctx, k, "lookup join phase", host, agg));
    ctx->last_semi_tables = keyed_rounds(host, (u32)ctx->last.ntasks);
    if (host[5]) return part_too_large(ctx, "S", host[5]);
    const u32 bad = (u32)agg[AGG_MAX_COLS + 1];
    if (bad & LOOKUP_BAD_ROW_R) return fail(ctx, RHJ_E_INVALID, "a rowID of R is >= out_rows: d_out has no such word");
    if (bad & LOOKUP_BAD_ROW_S) return fail(ctx, RHJ_E_INVALID, "a rowID of S is >= 2^63: RHJ_LOOKUP_LAST orders rowIDs as signed words");
    *out_matched = agg[0];
    return RHJ_OK;
}

// Group-by phase on the partitions of R that a one-sided partition_phase left: k_make_semi_tasks with anti = 1 over a
// ZEROED boundary array of S and a split that never cuts -- one task per non-empty partition of R, the whole partition -- then
// k_group_bkt over the columns and outputs of the call.  Retry codes as semi_phase.
int group_phase(rhj_ctx *ctx, u64 *out_groups)
{
    const CallArgs &a = ctx->call;
    Keyed k;
    RHJCHK(keyed_begin(ctx, k, CLEAR_COUNTERS_AGG, JK_GROUP, NEVER_CUT, ctx->cur_nR, 1, ctx->cur_psR, nullptr, [&]() -> int {
        if (a.gid[0]) launch_group_id_words(ctx->stream, k.agg, a.gid[0], a.gid_rows[0], nullptr, 0);
        return RHJ_OK;
    }));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_group(ctx->stream, ctx->cur_R, k.tasks, k.ntasks, k.max_tasks, ctx->cur_radix_bits,
                     ctx->cur_radix_bits != 0 && join_mix(ctx) != MIX_NONE, a.agg_cols, a.agg_ncols, a.agg_col_rows, a.group_keys, a.group_counts,
                     a.group_sums, a.group_cap, k.agg, k.bad, k.max_tables, k.narrow ? narrow_ids(ctx->cur_R, ctx->cur_nR) : nullptr, k.skip,
                     a.group_ops, a.gid[0] != nullptr, a.group_arg ? a.group_rows : nullptr);
    }
    u64 host[8], agg[8];                               // agg: groups, -, -, -, -, guard flag
    RHJCHK(keyed_finish(ctx, k, "group-by phase", host, agg));
    ctx->last_max_part[1] = 0;
    ctx->last_group_rounds = keyed_rounds(host, (u32)ctx->last.ntasks);
    if (host[2] >> 32) return part_too_large(ctx, "R", host[2]);   // (such a partition was cut in two: its groups are not the result)
    if ((u32)agg[AGG_MAX_COLS + 1] & GROUP_BAD_ROW)
        return fail(ctx, RHJ_E_INVALID, "a rowID of R is >= col_rows: the weight columns have no such row");
    if ((u32)agg[AGG_MAX_COLS + 1] & GROUP_BAD_GID)
        return fail(ctx, RHJ_E_INVALID, "a rowID of R is >= gid_rows: d_out_gid has no such word");
    *out_groups = agg[0];
    return RHJ_OK;
}

// The id arrays of a group-by join, all ones -- "no group" -- in every word, on the context's stream.
static int fill_no_group(rhj_ctx *ctx)
{
    for (int side = 0; side < 2; side++)
        if (ctx->call.gid[side] && ctx->call.gid_rows[side])
            HIPCHK(ctx, hipMemsetAsync(ctx->call.gid[side], 0xff, (size_t)ctx->call.gid_rows[side] * 8, ctx->stream));
    return RHJ_OK;
}

// Group-by join phase on the partitions partition_phase left: k_make_semi_tasks over the boundary arrays of R and S with
// a split that never cuts and anti = 1 under RHJ_GJ_LEFT (a task wherever R_k is non-empty), 0 under RHJ_GJ_INNER (R_k and S_k
// non-empty), then k_gjoin_bkt over the columns and outputs of the call.  After a one-sided partition_phase (LEFT with an empty S) S's
// boundary array is a zeroed one, as in group_phase.  Retry codes as semi_phase.
int gjoin_phase(rhj_ctx *ctx, u64 *out_groups)
{
    const CallArgs &a = ctx->call;
    const bool ids = a.gid[0] != nullptr || a.gid[1] != nullptr;
    Keyed k;
    RHJCHK(keyed_begin(ctx, k, CLEAR_COUNTERS_AGG, JK_GJOIN, NEVER_CUT, ctx->cur_nR, a.gjoin_left ? 1 : 0, ctx->cur_psR,
                       a.one_sided ? nullptr : ctx->cur_psS, [&]() -> int {
        if (!ids) return RHJ_OK;                       // "no group" everywhere, on every attempt: the kernel stores group indices only
        RHJCHK(fill_no_group(ctx));
        launch_group_id_words(ctx->stream, k.agg, a.gid[0], a.gid_rows[0], a.gid[1], a.gid_rows[1]);
        return RHJ_OK;
    }));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_group_join(ctx->stream, ctx->cur_R, ctx->cur_S, k.tasks, k.ntasks, k.max_tasks, ctx->cur_radix_bits,
                          ctx->cur_radix_bits != 0 && join_mix(ctx) != MIX_NONE, a.gjoin_left, a.agg_cols, a.agg_ncols, a.agg_col_rows,
                          a.gjoin_colsS, a.gjoin_ncolsS, a.gjoin_colS_rows, a.group_keys, a.group_counts, a.gjoin_cntS, a.group_sums,
                          a.gjoin_sumsS, a.group_cap, k.agg, k.bad, k.max_tables, k.narrow ? narrow_ids(ctx->cur_R, ctx->cur_nR) : nullptr,
                          k.narrow && ctx->cur_S ? narrow_ids(ctx->cur_S, ctx->cur_nS) : nullptr, k.skip, a.group_ops, ids);
    }
    u64 host[8], agg[8];                               // agg: groups, -, -, -, -, guard flags
    RHJCHK(keyed_finish(ctx, k, "group-by join phase", host, agg));
    ctx->last_group_rounds = keyed_rounds(host, (u32)ctx->last.ntasks);
    if (host[2] >> 32) return part_too_large(ctx, "R", host[2]);   // (such a partition was cut in two: its groups are not the result)
    if (host[5]) return part_too_large(ctx, "S", host[5]);
    const u32 bad = (u32)agg[AGG_MAX_COLS + 1];
    if (bad & GJOIN_BAD_ROW_R) return fail(ctx, RHJ_E_INVALID, "a rowID of R is >= colR_rows: the weight columns of R have no such row");
    if (bad & GJOIN_BAD_ROW_S) return fail(ctx, RHJ_E_INVALID, "a rowID of S is >= colS_rows: the weight columns of S have no such row");
    if (bad & GJOIN_BAD_GID_R) return fail(ctx, RHJ_E_INVALID, "a rowID of R is >= gidR_rows: d_out_gidR has no such word");
    if (bad & GJOIN_BAD_GID_S) return fail(ctx, RHJ_E_INVALID, "a rowID of S is >= gidS_rows: d_out_gidS has no such word");
    *out_groups = agg[0];
    return RHJ_OK;
}

// bookkeeping of the narrow-format back-off (rhj.h "partition.narrow"), shared by the plain and the pipelined host path
void narrow_note_fallback(rhj_ctx *ctx)                  // a join met a rowID >= 2^32 in the narrow format
{
    ctx->narrow_fail_streak++;
    ctx->narrow_skip = ctx->narrow_fail_streak < 2 ? 0u : (ctx->narrow_fail_streak > 5 ? 32u : 1u << (ctx->narrow_fail_streak - 1));
}
void narrow_note_done(rhj_ctx *ctx, const rhj_opts &plan, bool tried_narrow)   // a join ran to its end in one format
{
    if (tried_narrow) ctx->narrow_fail_streak = 0;
    else if (ctx->narrow_skip > 0 && plan.passes == 2) ctx->narrow_skip--;
}

// One-pass joins (plans of <= 9 bits: 2 * 10^4 ... 8 * 10^6 build tuples) in THREE launches and no device-to-host copy:
// k_hist_fused2 (histograms of both relations, the join counters cleared, the next call's control block zeroed),
// k_scatter_fused2 (both relations; every workgroup derives the partition boundaries itself, a planner workgroup writes them
// and the join task list meanwhile), the bucket join, which publishes its count to pinned host memory.  Was: unit tables, histogram, three scan launches, scatter, k_make_tasks,
// join, a 56-byte D2H copy -- 8 dependent launches for 77 us of kernel time at 10^6 x 10^6 (BASELINE config 2).
bool fused_one_pass_ok(const rhj_ctx *ctx, u64 nR, u64 nS, const rhj_opts &plan)
{
    static const int env = (int)env_u64("RHJ_FUSE", 1, 0, 1);
    if (!(ctx->opt_fused >= 0 ? ctx->opt_fused : env)) return false;
    return plan.passes == 1 && plan.bits1 >= 1 && plan.bits1 <= PASS_PAIR_MAX_BITS && nR > 0 && nS > 0 && nR < ((u64)1 << 32) &&
           nS < ((u64)1 << 32);
}

int join_one_pass_fused(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, const rhj_opts &plan, void *d_out, u64 cap,
                        u64 *out_count, std::function<int()> *before_S)
{
    const int bits = plan.bits1;
    const size_t nbins = (size_t)1 << bits;
    if (before_S && *before_S) {                             // (both relations go through the same launches: S must be there)
        std::function<int()> f;
        f.swap(*before_S);
        RHJCHK(f());
    }
    RHJCHK(cols_to_aos(ctx, nR, d_R, nS, d_S));              // (a columnar join: no columnar form of the one-pass kernels)
    ctx->cur_nR = nR;
    ctx->cur_nS = nS;
    ctx->last.passes = 1;
    ctx->last.bits1 = bits;
    ctx->last.bits2 = 0;
    ctx->cur_narrow = 0;
    ctx->last_cf[0] = ctx->last_cf[1] = 0;                   // (no partition_phase here: "last.countfree_*" must not keep the last join's)
    clear_gaps(ctx);
    ctx->counters_clean = false;
    int kind = choose_join_kind(ctx, nR, nS, nbins, bits, false);
    u32 probe_split = plan.probe_split ? (u32)plan.probe_split : 32768u;
    if (join_probe_split(kind) && probe_split > join_probe_split(kind)) probe_split = join_probe_split(kind);
    if (probe_split > BJ_MAX_PROBE_SPLIT) probe_split = BJ_MAX_PROBE_SPLIT;
    ctx->cur_probe_split = probe_split;
    const u64 max_tasks64 = nbins + (nR + nS) / probe_split + 1;
    if (max_tasks64 > 0x7fffffffull) return fail(ctx, RHJ_E_INVALID, "too many join tasks");
    const u32 max_tasks = (u32)max_tasks64;
    PassPairHost h;
    DevBuf *uh[2] = {&ctx->unit_hist, &ctx->unit_hist_b};
    const void *in[2] = {d_R, d_S};
    const u64 n[2] = {nR, nS};
    RHJCHK(ensure(ctx, ctx->ps_R, (nbins + 1) * 8));
    RHJCHK(ensure(ctx, ctx->ps_S, (nbins + 1) * 8));
    RHJCHK(ensure(ctx, ctx->part_R, (size_t)nR * 16));
    RHJCHK(ensure(ctx, ctx->part_S, (size_t)nS * 16));
    void *out[2] = {ctx->part_R.p, ctx->part_S.p};
    u64 *ps[2] = {(u64 *)ctx->ps_R.p, (u64 *)ctx->ps_S.p};
    // units: the scatter's workgroups of R and S together fill the chip ONCE (9 bits: one 1024-thread workgroup per CU, below two
    // of 512 threads) -- every workgroup of k_scatter_fused2 first derives the partition starts and reserves its ranges with
    // 2^bits atomics, so a second round of workgroups pays that again ([measured] 3 * 10^6 x 3 * 10^6, 9 bits, units per
    // relation 733 / 256 / 128: scatter 85 / 54 / 44 us, the join 0.191 / 0.157 / 0.148 ms)
    const u64 target_units = bits >= 9 ? 128 : 256;
    for (int i = 0; i < 2; i++) {
        const PassGeom g = make_geom(n[i], 1, 0, bits, target_units);
        RHJCHK(ensure(ctx, *uh[i], (size_t)g.max_units * nbins * 4));
        h.side[i] = PassSide{in[i], out[i], nullptr, nullptr, (u32 *)uh[i]->p, nullptr, ps[i], nullptr, g};
    }
    h.mix = join_mix(ctx);
    RHJCHK(ensure(ctx, ctx->tasks, (size_t)max_tasks * sizeof(JoinTask)));
    RHJCHK(ensure(ctx, ctx->counters, 64));
    if (ctx->fuse_ctl.cap < fuse_ctl_bytes()) { RHJCHK(ensure(ctx, ctx->fuse_ctl, fuse_ctl_bytes())); ctx->fuse_clean = false; }
    if (!ctx->h_pub) {
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_pub, 64, hipHostMallocDefault));
        if (hipHostGetDevicePointer((void **)&ctx->h_pub_dev, ctx->h_pub, 0) != hipSuccess || !ctx->h_pub_dev) {
            (void)hipGetLastError();
            (void)hipHostFree(ctx->h_pub);
            ctx->h_pub = nullptr;
            return fail(ctx, RHJ_E_HIP, "no device address for the pinned counter block");
        }
    }
    if (!ctx->fuse_clean) {
        Span s(ctx, RHJ_K_AUX);
        HIPCHK(ctx, hipMemsetAsync(ctx->fuse_ctl.p, 0, fuse_ctl_bytes(), ctx->stream));
    }
    ctx->fuse_clean = false;                                 // until this call has run to its end
    u64 *d_count = (u64 *)ctx->counters.p;
    const int parity = ctx->fuse_parity;
    ctx->fuse_parity ^= 1;
    for (int phase = 0; phase < 2; phase++) {
        Span s(ctx, phase == 0 ? RHJ_K_HIST : RHJ_K_SCATTER);
        launch_fused_pass(ctx->stream, h, bits, phase, parity, ctx->fuse_ctl.p, probe_split, max_tasks, join_table_tuples(kind),
                          (JoinTask *)ctx->tasks.p, d_count, ctx->h_pub_dev, sniff_on(ctx));
    }
    // the packed result counter (rhj_kernels.hip bj_count_packed) while pairs and workgroups fit its two fields
    const bool packed = max_tasks < (1u << 16) && (double)nR * (double)nS < 2.8e14;
    ctx->cur_R = ctx->part_R.p;
    ctx->cur_S = ctx->part_S.p;
    ctx->cur_psR = ps[0];
    ctx->cur_psS = ps[1];
    ctx->cur_nparts = nbins;
    ctx->cur_radix_bits = bits;
    ctx->last_join_kind = kind;
    volatile u64 *pub = ctx->h_pub;
    pub[0] = ~0ull;
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_join(ctx->stream, ctx->cur_R, ps[0], ctx->cur_S, ps[1], (const JoinTask *)ctx->tasks.p, (const u32 *)(d_count + 1), max_tasks, bits,
                    d_out, d_out ? cap : 0, d_count, kind, nullptr, nullptr, nullptr, nullptr, ctx->h_pub_dev,
                    packed ? nullptr : fuse_join_ticket(ctx->fuse_ctl.p));
    }
    RHJCHK(check_launch(ctx, "one-pass join"));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (pub[0] == ~0ull) return fail(ctx, RHJ_E_HIP, "the bucket join did not publish its counters");
    ctx->fuse_clean = true;
    *out_count = pub[0];
    ctx->last.ntasks = (u32)(pub[1] & 0xffffffffu);
    ctx->last_max_part[0] = pub[2];
    ctx->last_max_part[1] = pub[3];
    return RHJ_OK;
}

// partition + join.  A run in the narrow format whose histogram kernel met a rowID >= 2^32 costs two histogram launches
// (every later kernel of the run returns at once) and is repeated in the 16-byte format; the fall-back is per join.
// what: the phase that follows every partition phase of the ladder -- the pair join, or semi_phase / agg_phase / mult_phase / group_phase / gjoin_phase / lookup_phase / outer_phase (which always take the
// unfused path: the one-pass form has the pair join built into its launches).
int partition_and_join(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, const rhj_opts &plan, void *d_out,
                       u64 cap, u64 *out_count, std::function<int()> *before_S = nullptr, JoinOutput what = OUT_PAIRS)
{
    if (what == OUT_PAIRS && fused_one_pass_ok(ctx, nR, nS, plan))
        return join_one_pass_fused(ctx, d_R, nR, d_S, nS, plan, d_out, cap, out_count, before_S);
    auto after_partition = [&]() {
        switch (what) {
        case OUT_PAIRS: return join_phase(ctx, d_out, cap, out_count);
        case OUT_SEMI:
        case OUT_ANTI: return semi_phase(ctx, what, d_out, cap, out_count);
        case OUT_SUMS: return agg_phase(ctx, out_count);
        case OUT_MULT: return mult_phase(ctx, out_count);
        case OUT_GROUP: return group_phase(ctx, out_count);
        case OUT_GJOIN: return gjoin_phase(ctx, out_count);
        case OUT_OUTER: return outer_phase(ctx, d_out, cap, out_count);
        case OUT_LOOKUP: return lookup_phase(ctx, out_count);
        }
        return fail(ctx, RHJ_E_INVALID, "no phase for this output");
    };
    const bool gaps_ok = what == OUT_PAIRS;                  // the pair join's task builder reads boundaries with gaps
    int rc = partition_phase(ctx, d_R, nR, d_S, nS, plan, before_S, gaps_ok);
    if (rc != RHJ_OK) { ctx->counters_clean = false; return rc; }
    const bool tried_narrow = ctx->cur_narrow != 0;
    rc = after_partition();
    // A side whose count-free pass 1 overflowed is partitioned again with exact cursors (k_hist2d_units), inside this call.  R's
    // partition stands when only S overflowed; after an overflow of R the kernels of S returned at once, so S runs again (count-free
    // as before: at most two repeats).
    for (int attempt = 0; rc == RHJ_RETRY_CF && attempt < 2; attempt++) {
        const u32 over = ctx->cf_over;
        for (int side = 0; side < 2; side++) {
            if (over & (2u << side)) {
                ctx->cf_off_once[side] = true;
                ctx->last_cf[side] = 2;
                ctx->cf_fail_streak[side]++;
                ctx->cf_skip[side] = ctx->cf_fail_streak[side] > 4 ? 32u : 1u << ctx->cf_fail_streak[side];
            }
            // a final partition did not fit its region: that side again with the pass-2 histogram (its count-free pass 1 may stay)
            if (over & (8u << side)) {
                ctx->cf2_off_once[side] = true;
                ctx->last_cf2[side] = 2;
                ctx->cf2_fail_streak[side]++;
                ctx->cf2_skip[side] = ctx->cf2_fail_streak[side] > 4 ? 32u : 1u << ctx->cf2_fail_streak[side];
            }
        }
        ctx->cf_keep_R = !(over & (2u | 8u));
        rc = partition_phase(ctx, d_R, nR, d_S, nS, plan, nullptr, gaps_ok);
        ctx->cf_keep_R = false;
        if (rc == RHJ_OK) rc = after_partition();
    }
    ctx->cf_off_once[0] = ctx->cf_off_once[1] = false;
    ctx->cf2_off_once[0] = ctx->cf2_off_once[1] = false;
    if (rc == RHJ_RETRY_CF) return fail(ctx, RHJ_E_HIP, "count-free partition: overflow flag after the exact repeat");
    if (rc == RHJ_OK)
        for (int side = 0; side < 2; side++) {
            if (ctx->last_cf[side] == 1) ctx->cf_fail_streak[side] = 0;
            if (ctx->last_cf2[side] == 1) ctx->cf2_fail_streak[side] = 0;
        }
    if (rc != RHJ_OK && rc != RHJ_RETRY_WIDE) { ctx->counters_clean = false; return rc; }
    if (rc != RHJ_RETRY_WIDE) {
        if (rc == RHJ_OK && !ctx->narrow_off_once) narrow_note_done(ctx, plan, tried_narrow);   // (off_once: the repeat of a join that fell back)
        return rc;
    }
    narrow_note_fallback(ctx);
    ctx->narrow_off_once = true;
    rc = partition_phase(ctx, d_R, nR, d_S, nS, plan);
    ctx->narrow_off_once = false;
    if (rc != RHJ_OK) { ctx->counters_clean = false; return rc; }
    return after_partition();
}

// one relation under a resolved two-pass (or one-pass) plan; narrow: the level narrow_level() returned for the join
int partition_side(rhj_ctx *ctx, const void *d_in, u64 n, const rhj_opts &plan, int narrow, void *part, u64 *ps)
{
    const int mix = join_mix(ctx);
    if (narrow && !narrow_fused_plan(plan)) return partition_relation_narrow2(ctx, d_in, n, plan.bits1, plan.bits2, part, ps, nullptr, mix);
    if (narrow) return partition_relation_fused(ctx, d_in, n, plan.bits1, plan.bits2, part, ps, narrow, mix);
    return partition_relation(ctx, d_in, n, plan.passes, plan.bits1, plan.bits2, part, ps, mix);
}

}  // namespace

static std::mutex g_pool_sizes_mu;
static std::map<void *, size_t> g_pool_sizes;             // size of every live rhj_dev_alloc block (all contexts)

// hooks for rhj_query.hip (same shared library, separate translation unit)
int rhj_internal_use_device(rhj_ctx *ctx) { return use_device(ctx); }
hipStream_t rhj_internal_stream(rhj_ctx *ctx) { return ctx->stream; }
int rhj_internal_fail(rhj_ctx *ctx, int code, const char *msg) { return fail(ctx, code, msg); }
void *rhj_internal_counters(rhj_ctx *ctx)
{
    ctx->counters_clean = false;                     // the caller is about to use them as scratch
    return ensure(ctx, ctx->counters, 64) == RHJ_OK ? ctx->counters.p : nullptr;
}
// ... and for rhj_sort.hip
void rhj_internal_sort_begin(rhj_ctx *ctx)
{
    prof_reset(ctx);
    ctx->last_join_kind = -1;                        // no join kernel runs
}
void rhj_internal_sort_report(rhj_ctx *ctx, int bits, int passes, int units)
{
    ctx->last_sort_bits = bits;
    ctx->last_sort_passes = passes;
    ctx->last_sort_units = units;
}
int rhj_internal_sort_max_units(rhj_ctx *ctx) { return ctx->opt_sort_units; }
void rhj_internal_topk_report(rhj_ctx *ctx, int bits, int passes, u64 candidates, u64 sorted_rows)
{
    ctx->last_topk_bits = bits;
    ctx->last_topk_passes = passes;
    ctx->last_topk_cand = candidates;
    ctx->last_topk_sorted = sorted_rows;
}
int64_t rhj_internal_topk_max_candidates(rhj_ctx *ctx) { return ctx->opt_topk_cand; }
// ... and for rhj_window.hip
void rhj_internal_window_report(rhj_ctx *ctx, int units, int sorts, u64 partitions)
{
    ctx->last_window_units = units;
    ctx->last_window_sorts = sorts;
    ctx->last_window_parts = partitions;
}
// ... and for rhj_asof.hip
void rhj_internal_asof_report(rhj_ctx *ctx, int units, int sorts, u64 matched)
{
    ctx->last_asof_units = units;
    ctx->last_asof_sorts = sorts;
    ctx->last_asof_matched = matched;
}
// ... and for rhj_range.hip
void rhj_internal_range_report(rhj_ctx *ctx, int units, int sorts, u64 pairs, u64 tiles)
{
    ctx->last_range_units = units;
    ctx->last_range_sorts = sorts;
    ctx->last_range_pairs = pairs;
    ctx->last_range_tiles = tiles;
}
void rhj_internal_range_last(rhj_ctx *ctx, int *units, int *sorts)
{
    *units = ctx->last_range_units;
    *sorts = ctx->last_range_sorts;
}
// ... and for rhj_frame.hip
void rhj_internal_frame_report(rhj_ctx *ctx, int units, int sorts, int scans, u64 partitions)
{
    ctx->last_frame_units = units;
    ctx->last_frame_sorts = sorts;
    ctx->last_frame_scans = scans;
    ctx->last_frame_parts = partitions;
}
void rhj_internal_frame_range_report(rhj_ctx *ctx, int units, int sorts, int scans, int levels, u64 partitions)
{
    ctx->last_frange_units = units;
    ctx->last_frange_sorts = sorts;
    ctx->last_frange_scans = scans;
    ctx->last_frange_levels = levels;
    ctx->last_frange_parts = partitions;
}
// one accessor for the six entries' buffers (RHJ_WS_*): separate buffers, so that an outer entry's survives the inner sorts regrowing theirs
int rhj_internal_workspace(rhj_ctx *ctx, int which, size_t bytes, void **out)
{
    DevBuf *const ws[RHJ_WS_COUNT] = {&ctx->sort_ws, &ctx->topk_ws, &ctx->window_ws, &ctx->asof_ws, &ctx->frame_ws, &ctx->range_ws};
    RHJCHK(ensure(ctx, *ws[which], bytes));
    *out = ws[which]->p;
    return RHJ_OK;
}
void *rhj_internal_span_open(rhj_ctx *ctx, int kind) { return new Span(ctx, kind); }
void rhj_internal_span_close(void *span) { delete (Span *)span; }

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

int rhj_abi_version(void) { return RHJ_ABI_VERSION; }

// the bijection joins partition by (rhj_kernels.hip mix64 / unmix64: splitmix64's finaliser and its inverse)
uint64_t rhj_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

uint64_t rhj_unmix64(uint64_t x)
{
    x ^= (x >> 31) ^ (x >> 62);
    x *= 0x319642B2D24D8EC3ULL;
    x ^= (x >> 27) ^ (x >> 54);
    x *= 0x96DE1B173F119089ULL;
    x ^= (x >> 30) ^ (x >> 60);
    return x - 0x9E3779B97F4A7C15ULL;
}

int rhj_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

void rhj_default_opts(rhj_opts *o)
{
    if (!o) return;
    o->passes = -1;
    o->bits1 = 0;
    o->bits2 = 0;
    o->probe_split = 0;
}

int rhj_plan(uint64_t nR, uint64_t nS, const rhj_opts *in, rhj_opts *resolved)
{
    if (!resolved) return RHJ_E_INVALID;
    return resolve_plan(nR, nS, in, resolved);
}

const char *rhj_last_error(const rhj_ctx *ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int rhj_init(int device, rhj_ctx **out_ctx)
{
    if (!out_ctx) return fail(nullptr, RHJ_E_INVALID, "out_ctx is null");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, RHJ_E_NODEVICE, "no HIP device available");
    }
    if (device < 0 || device >= n) return fail(nullptr, RHJ_E_INVALID, "device index out of range");
    rhj_ctx *ctx = new rhj_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        delete ctx;
        return fail(nullptr, RHJ_E_HIP, "cannot create a stream on the device");
    }
    ctx->stream = ctx->own_stream;
    if (hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        (void)hipGetLastError();
        ctx->num_cus = 0;                                   // (unknown: the one-writer pass 2 never applies)
    }
    *out_ctx = ctx;
    return RHJ_OK;
}

int rhj_release_workspace(rhj_ctx *ctx)
{
    RHJCHK(use_device(ctx));
    (void)hipStreamSynchronize(ctx->stream);
    DevBuf *all[] = {&ctx->in_R, &ctx->in_S, &ctx->part_R, &ctx->part_S, &ctx->part_tmp, &ctx->ps_R, &ctx->ps_S,
                     &ctx->ps_1, &ctx->seg0, &ctx->unit_start, &ctx->unit_hist, &ctx->unit_base, &ctx->seg0_b,
                     &ctx->unit_start_b, &ctx->unit_hist_b, &ctx->unit_base_b, &ctx->scan_tmp_b, &ctx->tasks,
                     &ctx->counters, &ctx->out_pairs, &ctx->small_out, &ctx->hist_tmp, &ctx->scan_tmp, &ctx->hist2,
                     &ctx->grp_rng, &ctx->unit_start2, &ctx->narrow_flag, &ctx->agg_out, &ctx->seg_rng, &ctx->tag_base,
                     &ctx->shard_ps[0], &ctx->shard_ps[1], &ctx->shard_mm, &ctx->shard_wide, &ctx->shard_peer_tab, &ctx->fuse_ctl, &ctx->sniff_tab, &ctx->hist2_b, &ctx->grp_rng_b,
                     &ctx->unit_start2_b, &ctx->ps_1_b, &ctx->part_tmp_b, &ctx->cf_cnt1, &ctx->cf_pre, &ctx->cf_tot, &ctx->cf2_end[0], &ctx->cf2_end[1], &ctx->cols_aos[0], &ctx->cols_aos[1], &ctx->b_in[0], &ctx->b_out[0], &ctx->b_cnt[0],
                     &ctx->b_in[1], &ctx->b_out[1], &ctx->b_cnt[1], &ctx->sort_ws, &ctx->topk_ws, &ctx->window_ws, &ctx->asof_ws, &ctx->frame_ws, &ctx->range_ws};
    ctx->fuse_clean = false;
    for (DevBuf *b : all) release(*b);
    ctx->small_hdr_clean = false;
    for (auto &b : ctx->free_blocks) {
        { std::lock_guard<std::mutex> lk(g_pool_sizes_mu); g_pool_sizes.erase(b.first); }
        (void)hipFree(b.first);
    }
    ctx->free_blocks.clear();
    ctx->free_bytes = 0;
    if (ctx->h_land) { (void)hipHostFree(ctx->h_land); ctx->h_land = nullptr; }
    stager_destroy(ctx);
    if (ctx->h_counts) { (void)hipHostFree(ctx->h_counts); ctx->h_counts = nullptr; }
    if (ctx->h_pub) { (void)hipHostFree(ctx->h_pub); ctx->h_pub = nullptr; ctx->h_pub_dev = nullptr; }
    for (hipEvent_t e : ctx->chunk_ev) (void)hipEventDestroy(e);
    ctx->chunk_ev.clear();
    return RHJ_OK;
}

void rhj_destroy(rhj_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)rhj_release_workspace(ctx);
    for (hipEvent_t ev : ctx->prof.pool) (void)hipEventDestroy(ev);
    for (int i = 0; i < 2; i++) if (ctx->up_ev[i]) (void)hipEventDestroy(ctx->up_ev[i]);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    for (int i = 0; i < 2; i++) if (ctx->aux_ev[i]) (void)hipEventDestroy(ctx->aux_ev[i]);
    if (ctx->down_stream) (void)hipStreamDestroy(ctx->down_stream);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx->pool;
    for (int i = 0; i < 2; i++) {
        if (ctx->b_stage[i]) (void)hipHostFree(ctx->b_stage[i]);
        if (ctx->b_land[i]) (void)hipHostFree(ctx->b_land[i]);
        if (ctx->b_ev[i]) (void)hipEventDestroy(ctx->b_ev[i]);
    }
    delete ctx;
}

int rhj_set_stream(rhj_ctx *ctx, void *hip_stream)
{
    RHJCHK(use_device(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return RHJ_OK;
}

int rhj_set_option(rhj_ctx *ctx, const char *name, int64_t value)
{
    if (!ctx || !name) return fail(ctx, RHJ_E_INVALID, "rhj_set_option: null argument");
    const std::string n(name);
    if (n == "join.big_tables" && value >= -1 && value <= 1) { ctx->opt_big_tables = (int)value; return RHJ_OK; }
    if (n == "join.big_kernel" && (value == -1 || (value >= JK_BKT_BIG && value <= JK_LAST))) {
        ctx->opt_big_kernel = (int)value;
        return RHJ_OK;
    }
    if (n == "partition.narrow" && value >= -1 && value <= 2) {
        ctx->opt_narrow = (int)value;
        ctx->narrow_fail_streak = ctx->narrow_skip = 0;
        return RHJ_OK;
    }
    if (n == "partition.mix" && value >= -1 && value <= 1) { ctx->opt_mix = (int)value; return RHJ_OK; }
    if (n == "partition.countfree" && value >= -1 && value <= 1) {
        ctx->opt_countfree = (int)value;
        for (int side = 0; side < 2; side++) ctx->cf_fail_streak[side] = ctx->cf_skip[side] = 0;
        return RHJ_OK;
    }
    if (n == "partition.countfree2" && value >= -1 && value <= 1) {
        ctx->opt_countfree2 = (int)value;
        for (int side = 0; side < 2; side++) ctx->cf2_fail_streak[side] = ctx->cf2_skip[side] = 0;
        return RHJ_OK;
    }
    if (n == "join.fused" && value >= -1 && value <= 1) { ctx->opt_fused = (int)value; return RHJ_OK; }
    if (n == "join.sniff" && value >= -1 && value <= 1) { ctx->opt_sniff = (int)value; return RHJ_OK; }
    if (n == "sort.max_units" && (value == -1 || (value >= 1 && value <= 2048))) { ctx->opt_sort_units = (int)value; return RHJ_OK; }
    if (n == "topk.max_candidates" && (value == -1 || (value >= 1 && value <= 0x7FFFFFFF))) { ctx->opt_topk_cand = value; return RHJ_OK; }
    return fail(ctx, RHJ_E_INVALID, "rhj_set_option: unknown option or value: " + n);
}

int rhj_get_info(rhj_ctx *ctx, const char *name, int64_t *value)
{
    if (!ctx || !name || !value) return fail(ctx, RHJ_E_INVALID, "rhj_get_info: null argument");
    const std::string n(name);
    if (n == "last.narrow") { *value = ctx->cur_narrow; return RHJ_OK; }
    if (n == "last.countfree_R") { *value = ctx->last_cf[0]; return RHJ_OK; }
    if (n == "last.countfree_S") { *value = ctx->last_cf[1]; return RHJ_OK; }
    if (n == "last.countfree2_R") { *value = ctx->last_cf2[0]; return RHJ_OK; }
    if (n == "last.countfree2_S") { *value = ctx->last_cf2[1]; return RHJ_OK; }
    if (n == "last.cols_R") { *value = ctx->last_cols[0]; return RHJ_OK; }
    if (n == "last.cols_S") { *value = ctx->last_cols[1]; return RHJ_OK; }
    if (n == "last.join_kernel") { *value = ctx->last_join_kind; return RHJ_OK; }
    if (n == "last.pipelined") { *value = ctx->last_pipelined; return RHJ_OK; }
    if (n == "last.max_part_R") { *value = (int64_t)ctx->last_max_part[0]; return RHJ_OK; }
    if (n == "last.max_part_S") { *value = (int64_t)ctx->last_max_part[1]; return RHJ_OK; }
    if (n == "last.semi_tables") { *value = ctx->last_semi_tables; return RHJ_OK; }
    if (n == "last.group_rounds") { *value = ctx->last_group_rounds; return RHJ_OK; }
    if (n == "last.outer_sweeps") { *value = ctx->last_outer_sweeps; return RHJ_OK; }
    if (n == "last.sort_bits") { *value = ctx->last_sort_bits; return RHJ_OK; }
    if (n == "last.sort_passes") { *value = ctx->last_sort_passes; return RHJ_OK; }
    if (n == "last.sort_units") { *value = ctx->last_sort_units; return RHJ_OK; }
    if (n == "sort.tile_rows") { *value = SORT_TILE; return RHJ_OK; }
    if (n == "last.topk_bits") { *value = ctx->last_topk_bits; return RHJ_OK; }
    if (n == "last.topk_passes") { *value = ctx->last_topk_passes; return RHJ_OK; }
    if (n == "last.topk_candidates") { *value = (int64_t)ctx->last_topk_cand; return RHJ_OK; }
    if (n == "last.topk_sorted_rows") { *value = (int64_t)ctx->last_topk_sorted; return RHJ_OK; }
    if (n == "topk.auto_candidates") { *value = TOPK_AUTO_CANDIDATES; return RHJ_OK; }
    if (n == "last.window_units") { *value = ctx->last_window_units; return RHJ_OK; }
    if (n == "last.window_sorts") { *value = ctx->last_window_sorts; return RHJ_OK; }
    if (n == "last.window_partitions") { *value = (int64_t)ctx->last_window_parts; return RHJ_OK; }
    if (n == "window.tile_rows") { *value = WINDOW_TILE; return RHJ_OK; }
    if (n == "last.asof_units") { *value = ctx->last_asof_units; return RHJ_OK; }
    if (n == "last.asof_sorts") { *value = ctx->last_asof_sorts; return RHJ_OK; }
    if (n == "last.asof_matched") { *value = (int64_t)ctx->last_asof_matched; return RHJ_OK; }
    if (n == "asof.tile_rows") { *value = ASOF_TILE; return RHJ_OK; }
    if (n == "last.frame_units") { *value = ctx->last_frame_units; return RHJ_OK; }
    if (n == "last.frame_sorts") { *value = ctx->last_frame_sorts; return RHJ_OK; }
    if (n == "last.frame_scans") { *value = ctx->last_frame_scans; return RHJ_OK; }
    if (n == "last.frame_partitions") { *value = (int64_t)ctx->last_frame_parts; return RHJ_OK; }
    if (n == "last.frame_range_units") { *value = ctx->last_frange_units; return RHJ_OK; }
    if (n == "last.frame_range_sorts") { *value = ctx->last_frange_sorts; return RHJ_OK; }
    if (n == "last.frame_range_scans") { *value = ctx->last_frange_scans; return RHJ_OK; }
    if (n == "last.frame_range_levels") { *value = ctx->last_frange_levels; return RHJ_OK; }
    if (n == "last.frame_range_partitions") { *value = (int64_t)ctx->last_frange_parts; return RHJ_OK; }
    if (n == "last.range_join_units") { *value = ctx->last_range_units; return RHJ_OK; }
    if (n == "last.range_join_sorts") { *value = ctx->last_range_sorts; return RHJ_OK; }
    if (n == "last.range_join_pairs") { *value = (int64_t)ctx->last_range_pairs; return RHJ_OK; }
    if (n == "last.range_join_expand_tiles") { *value = (int64_t)ctx->last_range_tiles; return RHJ_OK; }
    if (n == "range_join.tile_rows") { *value = RANGE_TILE; return RHJ_OK; }
    if (n == "range_join.expand_tile") { *value = RANGE_EXPAND_TILE; return RHJ_OK; }
    if (n == "partition.mix") { *value = join_mix(ctx) != MIX_NONE; return RHJ_OK; }
    return fail(ctx, RHJ_E_INVALID, "rhj_get_info: unknown name: " + n);
}

int rhj_set_profiling(rhj_ctx *ctx, int enabled)
{
    if (!ctx) return RHJ_E_INVALID;
    ctx->prof.on = enabled != 0;
    ctx->prof.keep = false;
    prof_reset(ctx);                       // (also the start of an accumulating series)
    ctx->prof.keep = enabled == 2;
    return RHJ_OK;
}

int rhj_get_timings(rhj_ctx *ctx, rhj_timings *out)
{
    if (!ctx || !out) return RHJ_E_INVALID;
    RHJCHK(use_device(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    rhj_timings t = ctx->last;
    for (int k = 0; k < RHJ_K_COUNT; k++) { t.ms[k] = 0; t.launches[k] = 0; }
    Prof &p = ctx->prof;
    for (size_t i = 0; i < p.used; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.pool[2 * i], p.pool[2 * i + 1]) != hipSuccess) { (void)hipGetLastError(); continue; }
        t.ms[p.kinds[i]] += ms;
        t.launches[p.kinds[i]]++;
    }
    if (p.used) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.pool[0], p.pool[2 * (p.used - 1) + 1]) == hipSuccess) t.total_ms = ms;
    }
    *out = t;
    return RHJ_OK;
}

int rhj_get_launch_timings(rhj_ctx *ctx, int32_t *kinds, double *ms, uint32_t capacity, uint32_t *n)
{
    if (!ctx || !n || (capacity && (!kinds || !ms))) return RHJ_E_INVALID;
    RHJCHK(use_device(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    Prof &p = ctx->prof;
    *n = (uint32_t)p.used;
    for (size_t i = 0; i < p.used && i < capacity; i++) {
        float t = 0;
        if (hipEventElapsedTime(&t, p.pool[2 * i], p.pool[2 * i + 1]) != hipSuccess) { (void)hipGetLastError(); t = 0; }
        kinds[i] = p.kinds[i];
        ms[i] = t;
    }
    return RHJ_OK;
}

int rhj_sync(rhj_ctx *ctx)
{
    RHJCHK(use_device(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RHJ_OK;
}

int rhj_reserve(rhj_ctx *ctx, uint64_t nR, uint64_t nS, const rhj_opts *opts)
{
    RHJCHK(use_device(ctx));
    rhj_opts plan;
    if (resolve_plan(nR, nS, opts, &plan, false, default_join_kernels(ctx)) != RHJ_OK) return fail(ctx, RHJ_E_INVALID, "bad rhj_opts");
    if (plan.passes >= 1) {
        RHJCHK(ensure(ctx, ctx->part_R, (size_t)(nR ? nR : 1) * 16));
        RHJCHK(ensure(ctx, ctx->part_S, (size_t)(nS ? nS : 1) * 16));
    }
    if (plan.passes == 2) RHJCHK(ensure(ctx, ctx->part_tmp, (size_t)((nR > nS ? nR : nS) + 1) * 16));
    if (plan.passes == 2 && narrow_fused_plan(plan) && ctx->opt_countfree != 0) {       // count-free pass 1: regions and small tables
        for (int side = 0; side < 2; side++) {
            const u64 n = side ? nS : nR;
            if (!cf_applies(n, plan.bits1, plan.bits2, 2, MIX_STORE, false)) continue;
            if (ctx->opt_countfree < 0 && (nR > nS ? nR : nS) <= CF_AUTO_MIN_TUPLES) continue;
            const CfGeom c = cf_geometry(n, plan.bits1);
            const size_t nb1 = (size_t)1 << plan.bits1, units2 = nb1 * c.ngroups;
            RHJCHK(ensure(ctx, ctx->part_tmp, cf_tmp_bytes(c)));
            RHJCHK(ensure(ctx, ctx->cf_cnt1, (size_t)c.U * nb1 * 4));
            RHJCHK(ensure(ctx, ctx->cf_pre, cf_pre_words((u32)units2) * 4));
            RHJCHK(ensure(ctx, ctx->cf_tot, units2 * 4));
            // ... and a one-writer pass 2: final arrays with the regions' slack, the end array
            if (cf2_want(ctx) == 0 || !cf2_applies(ctx, n, plan.bits1, plan.bits2)) continue;
            if (cf2_want(ctx) < 0 && (!CF2_AUTO || (nR > nS ? nR : nS) <= CF_AUTO_MIN_TUPLES)) continue;
            RHJCHK(ensure(ctx, side ? ctx->part_S : ctx->part_R, cf2_part_bytes(cf2_geometry(n, plan.bits1, plan.bits2))));
            RHJCHK(ensure(ctx, ctx->cf2_end[side], (size_t)8 << (plan.bits1 + plan.bits2)));
        }
    }
    return RHJ_OK;
}

// ---- the scaffold of the device entries, rhj_join_dev through rhj_group_join_agg_ids_cols_dev ---------------------------------------
// Every entry starts here: the device, the out word -- named as the entry names it -- checked and zeroed, the profile and the
// "last.*" state reset.
static int entry_begin(rhj_ctx *ctx, uint64_t *out_word, const char *name)
{
    RHJCHK(use_device(ctx));
    if (!out_word) return fail(ctx, RHJ_E_INVALID, std::string(name) + " is null");
    *out_word = 0;
    prof_reset(ctx);
    return RHJ_OK;
}

// The relations of a columnar entry, in the context for the length of the call: partition_phase and the one-pass join hand them to the
// kernels that read columns (fused_input) or convert the side they need (cols_to_aos), also when a join repeats itself (count-free
// overflow: columns again; wide rowID: the 16-byte copy).  No valS: no S, or an empty one; no idS: rowID = index.
struct ColsScope {
    rhj_ctx *c;
    ColsScope(rhj_ctx *ctx, const uint64_t *valR, const uint64_t *idR, const uint64_t *valS = nullptr, const uint64_t *idS = nullptr) : c(ctx)
    {
        c->cols_in[0].val = (const u64 *)valR; c->cols_in[0].id = (const u64 *)idR;
        c->cols_in[1].val = (const u64 *)valS; c->cols_in[1].id = (const u64 *)idS;
        c->cols_aos_done[0] = c->cols_aos_done[1] = false;
    }
    ~ColsScope() { c->cols_in[0] = c->cols_in[1] = ColsIn(); }
};

// The operator arguments of an entry (ctx->call) go back to CallArgs() on every way out of its *_common function.
struct CallScope {
    rhj_ctx *c;
    explicit CallScope(rhj_ctx *ctx) : c(ctx) {}
    ~CallScope() { c->call = CallArgs(); }
};

// the caller's options as the plan of a device-resident join
static int entry_plan(rhj_ctx *ctx, u64 nR, u64 nS, const rhj_opts *opts, rhj_opts *plan)
{
    if (resolve_plan(nR, nS, opts, plan, true, default_join_kernels(ctx)) != RHJ_OK) return fail(ctx, RHJ_E_INVALID, "bad rhj_opts");
    return RHJ_OK;
}

// the end of an entry that writes rows: more of them than the caller's arrays hold (a count-only call has no array)
static int check_capacity(rhj_ctx *ctx, const void *d_out, u64 rows, u64 capacity, const char *what = "result buffer")
{
    if (d_out && rows > capacity) return fail(ctx, RHJ_E_OVERFLOW, std::string(what) + " too small");
    return RHJ_OK;
}

// a join with an empty input runs no kernel: "last.join_kernel" / "last.narrow" say so instead of describing the join before it
static int join_nothing(rhj_ctx *ctx)
{
    ctx->last_join_kind = -1;
    ctx->cur_narrow = 0;
    return RHJ_OK;
}

// What a partition phase would leave for a join whose one side is empty: the other side (`side`, d_P) unpartitioned, its one partition
// standing for both sides -- no tuple of the empty side is read.
static int one_partition(rhj_ctx *ctx, u64 nR, u64 nS, int side, const void *d_P)
{
    ctx->cur_nR = nR;
    ctx->cur_nS = nS;
    ctx->cur_probe_split = 0;
    ctx->cur_narrow = 0;
    ctx->last_cf[0] = ctx->last_cf[1] = 0;
    clear_gaps(ctx);
    RHJCHK(cols_to_aos(ctx, side, side ? nS : nR, d_P));
    RHJCHK(ensure(ctx, ctx->ps_R, 64));
    RHJCHK(ensure(ctx, ctx->ps_S, 64));
    ctx->cur_R = ctx->cur_S = d_P;
    ctx->cur_psR = (const u64 *)ctx->ps_R.p;
    ctx->cur_psS = (const u64 *)ctx->ps_S.p;
    ctx->cur_nparts = 1;
    ctx->cur_radix_bits = 0;
    return RHJ_OK;
}

int rhj_join_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                 const rhj_opts *opts, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count)
{
    RHJCHK(entry_begin(ctx, out_count, "out_count"));
    if (nR == 0 || nS == 0) return join_nothing(ctx);  // nothing to schedule (Result.cpp:101 never fires)
    if (!d_R || !d_S) return fail(ctx, RHJ_E_INVALID, "null input relation");
    rhj_opts plan;
    RHJCHK(entry_plan(ctx, nR, nS, opts, &plan));
    RHJCHK(partition_and_join(ctx, d_R, nR, d_S, nS, plan, d_out, d_out ? out_capacity : 0, (u64 *)out_count));
    return check_capacity(ctx, d_out, *out_count, out_capacity);
}

// rhj_join_dev on relations given as columns
int rhj_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR, const uint64_t *d_valS,
                      const uint64_t *d_idS, uint64_t nS, const rhj_opts *opts, rhj_pair *d_out, uint64_t out_capacity,
                      uint64_t *out_count)
{
    RHJCHK(entry_begin(ctx, out_count, "out_count"));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    if (nR == 0 || nS == 0) return join_nothing(ctx);
    rhj_opts plan;
    RHJCHK(entry_plan(ctx, nR, nS, opts, &plan));
    ColsScope cols(ctx, d_valR, d_idR, d_valS, d_idS);
    RHJCHK(partition_and_join(ctx, nullptr, nR, nullptr, nS, plan, d_out, d_out ? out_capacity : 0, (u64 *)out_count));
    return check_capacity(ctx, d_out, *out_count, out_capacity);
}

// Semi / anti join: the partition phase and the repeat ladder of rhj_join_dev / rhj_join_cols_dev, then semi_phase.
// d_R / d_S null: the relations are ctx->cols_in.  An empty S under RHJ_ANTI: every tuple of R, by the bucket kernel over empty
// tables -- R unpartitioned, its one partition cut into tasks.
static int semi_join_common(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, int kind, const rhj_opts *opts,
                            uint64_t *d_out_ids, u64 out_capacity, uint64_t *out_count)
{
    if (nR == 0 || (nS == 0 && kind == RHJ_SEMI)) return join_nothing(ctx);
    const u64 cap = d_out_ids ? out_capacity : 0;
    if (nS == 0) {
        ctx->counters_clean = false;
        RHJCHK(one_partition(ctx, nR, 0, 0, d_R));
        const int rc = semi_phase(ctx, OUT_ANTI, d_out_ids, cap, (u64 *)out_count);
        if (rc != RHJ_OK) return rc > 0 ? fail(ctx, RHJ_E_HIP, "semi join: a repeat was asked for without a partition phase") : rc;
    } else {
        rhj_opts plan;
        RHJCHK(entry_plan(ctx, nR, nS, opts, &plan));
        RHJCHK(partition_and_join(ctx, d_R, nR, d_S, nS, plan, d_out_ids, cap, (u64 *)out_count, nullptr,
                                  kind == RHJ_ANTI ? OUT_ANTI : OUT_SEMI));
    }
    return check_capacity(ctx, d_out_ids, *out_count, out_capacity);
}

int rhj_semi_join_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, int kind,
                      const rhj_opts *opts, uint64_t *d_out_ids, uint64_t out_capacity, uint64_t *out_count)
{
    RHJCHK(entry_begin(ctx, out_count, "out_count"));
    if (kind != RHJ_SEMI && kind != RHJ_ANTI) return fail(ctx, RHJ_E_INVALID, "kind is neither RHJ_SEMI nor RHJ_ANTI");
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return semi_join_common(ctx, d_R, nR, d_S, nS, kind, opts, d_out_ids, out_capacity, out_count);
}

int rhj_semi_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR, const uint64_t *d_valS,
                           uint64_t nS, int kind, const rhj_opts *opts, uint64_t *d_out_ids, uint64_t out_capacity,
                           uint64_t *out_count)
{
    RHJCHK(entry_begin(ctx, out_count, "out_count"));
    if (kind != RHJ_SEMI && kind != RHJ_ANTI) return fail(ctx, RHJ_E_INVALID, "kind is neither RHJ_SEMI nor RHJ_ANTI");
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, d_valS);        // S has no id column: rowID = index, never reported
    return semi_join_common(ctx, nullptr, nR, nullptr, nS, kind, opts, d_out_ids, out_capacity, out_count);
}

// Outer join: the partition phase and the repeat ladder of rhj_join_dev / rhj_join_cols_dev, then outer_phase.
// d_R / d_S null: the relations are ctx->cols_in.  One side empty: no pair, and every tuple of the other side if its bit is set -- by
// one sweep over empty tables, that side unpartitioned and its one partition cut into tasks (semi_join_common's path for an empty S).
static int outer_join_common(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, int how, const rhj_opts *opts,
                             rhj_pair *d_out, u64 out_capacity, uint64_t *out_count, uint64_t *out_sections)
{
    const u64 cap = d_out ? out_capacity : 0;
    CallScope call(ctx);
    ctx->call.outer_how = how;
    ctx->outer_sections[0] = ctx->outer_sections[1] = ctx->outer_sections[2] = 0;
    if (nR == 0 || nS == 0) {
        const int side = nR == 0 ? 1 : 0;              // the side that may have tuples
        if ((nR == 0 && nS == 0) || !(how & (1 << side))) return join_nothing(ctx);
        RHJCHK(one_partition(ctx, nR, nS, side, side ? d_S : d_R));
        RHJCHK(ensure(ctx, ctx->counters, 64));
        {
            Span s(ctx, RHJ_K_AUX);
            HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
            launch_init_single_segment(ctx->stream, nR, PART_TILE, (u64 *)ctx->ps_R.p, (u32 *)((u64 *)ctx->ps_R.p + 4));
            launch_init_single_segment(ctx->stream, nS, PART_TILE, (u64 *)ctx->ps_S.p, (u32 *)((u64 *)ctx->ps_S.p + 4));
        }
        ctx->counters_clean = false;
        ctx->sniff_ready = false;
        ctx->last_join_kind = JK_SEMI;
        ctx->last_max_part[0] = ctx->last_max_part[1] = 0;
        RHJCHK(outer_sweep(ctx, side, d_out, cap, (u64 *)out_count));
        ctx->outer_sections[1 + side] = *out_count;
    } else {
        rhj_opts plan;
        RHJCHK(entry_plan(ctx, nR, nS, opts, &plan));
        RHJCHK(partition_and_join(ctx, d_R, nR, d_S, nS, plan, d_out, cap, (u64 *)out_count, nullptr, OUT_OUTER));
    }
    if (out_sections) for (int i = 0; i < 3; i++) out_sections[i] = ctx->outer_sections[i];
    return check_capacity(ctx, d_out, *out_count, out_capacity);
}

// the prologue of the two outer-join entries: entry_begin, the sections zeroed beside the out word, `how`
static int outer_begin(rhj_ctx *ctx, int how, uint64_t *out_count, uint64_t *out_sections)
{
    RHJCHK(entry_begin(ctx, out_count, "out_count"));
    if (out_sections) out_sections[0] = out_sections[1] = out_sections[2] = 0;
    if (how < RHJ_OUTER_LEFT || how > RHJ_OUTER_FULL) return fail(ctx, RHJ_E_INVALID, "how is none of RHJ_OUTER_LEFT, RHJ_OUTER_RIGHT, RHJ_OUTER_FULL");
    return RHJ_OK;
}

int rhj_outer_join_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, int how,
                       const rhj_opts *opts, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count, uint64_t *out_sections)
{
    RHJCHK(outer_begin(ctx, how, out_count, out_sections));
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return outer_join_common(ctx, d_R, nR, d_S, nS, how, opts, d_out, out_capacity, out_count, out_sections);
}

int rhj_outer_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR, const uint64_t *d_valS,
                            const uint64_t *d_idS, uint64_t nS, int how, const rhj_opts *opts, rhj_pair *d_out,
                            uint64_t out_capacity, uint64_t *out_count, uint64_t *out_sections)
{
    RHJCHK(outer_begin(ctx, how, out_count, out_sections));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, d_valS, d_idS);
    return outer_join_common(ctx, nullptr, nR, nullptr, nS, how, opts, d_out, out_capacity, out_count, out_sections);
}

// Aggregating join: the partition phase and the repeat ladder of rhj_join_dev / rhj_join_cols_dev, then agg_phase.
// d_R / d_S null: the relations are ctx->cols_in.
static int join_sum_common(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, const uint64_t *const *d_cols, uint32_t ncols,
                           uint64_t col_rows, const rhj_opts *opts, uint64_t *out_count, uint64_t *out_sums)
{
    if (ncols > RHJ_SUM_MAX_COLS) return fail(ctx, RHJ_E_INVALID, "ncols is above RHJ_SUM_MAX_COLS");
    if (ncols && (!d_cols || !out_sums)) return fail(ctx, RHJ_E_INVALID, "null weight column array or out_sums");
    for (u32 j = 0; j < ncols; j++) {
        if (!d_cols[j]) return fail(ctx, RHJ_E_INVALID, "null weight column");
        out_sums[j] = 0;
    }
    if (nR == 0 || nS == 0) return join_nothing(ctx);
    rhj_opts plan;
    RHJCHK(entry_plan(ctx, nR, nS, opts, &plan));
    CallScope call(ctx);
    CallArgs &a = ctx->call;
    for (u32 j = 0; j < ncols; j++) a.agg_cols[j] = (const u64 *)d_cols[j];
    a.agg_ncols = ncols;
    a.agg_col_rows = ncols ? col_rows : ~0ull;
    a.agg_sums_out = (u64 *)out_sums;
    return partition_and_join(ctx, d_R, nR, d_S, nS, plan, nullptr, 0, (u64 *)out_count, nullptr, OUT_SUMS);
}

int rhj_join_sum_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                     const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows,
                     const rhj_opts *opts, uint64_t *out_count, uint64_t *out_sums)
{
    RHJCHK(entry_begin(ctx, out_count, "out_count"));
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return join_sum_common(ctx, d_R, nR, d_S, nS, d_cols, ncols, col_rows, opts, out_count, out_sums);
}

int rhj_join_sum_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR, const uint64_t *d_valS, uint64_t nS,
                          const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                          uint64_t *out_count, uint64_t *out_sums)
{
    RHJCHK(entry_begin(ctx, out_count, "out_count"));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, d_valS);        // S has no id column: rowID = index, never looked at
    return join_sum_common(ctx, nullptr, nR, nullptr, nS, d_cols, ncols, col_rows, opts, out_count, out_sums);
}

// The words of a multiplicity or lookup join with an empty input -- all `byte` -- complete when the call returns.
static int fill_out_words(rhj_ctx *ctx, uint64_t *d_out, uint64_t out_rows, int byte)
{
    if (out_rows) {
        HIPCHK(ctx, hipMemsetAsync(d_out, byte, out_rows * 8, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return join_nothing(ctx);
}

// Multiplicity join: the partition phase and the repeat ladder of rhj_join_dev / rhj_join_cols_dev, then mult_phase.
// d_R / d_S null: the relations are ctx->cols_in.
static int join_mult_common(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, const uint64_t *d_wS, uint64_t wS_rows,
                            const rhj_opts *opts, uint64_t *d_out, uint64_t out_rows, uint64_t *out_total)
{
    if (out_rows && !d_out) return fail(ctx, RHJ_E_INVALID, "d_out is null");
    if (nR == 0 || nS == 0) return fill_out_words(ctx, d_out, out_rows, 0);
    rhj_opts plan;
    RHJCHK(entry_plan(ctx, nR, nS, opts, &plan));
    CallScope call(ctx);
    ctx->call.mult_w = (const u64 *)d_wS;
    ctx->call.mult_w_rows = d_wS ? wS_rows : 0;
    ctx->call.mult_out = (u64 *)d_out;
    ctx->call.mult_out_rows = out_rows;
    return partition_and_join(ctx, d_R, nR, d_S, nS, plan, nullptr, 0, (u64 *)out_total, nullptr, OUT_MULT);
}

int rhj_join_mult_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                      const uint64_t *d_wS, uint64_t wS_rows, const rhj_opts *opts,
                      uint64_t *d_out, uint64_t out_rows, uint64_t *out_total)
{
    RHJCHK(entry_begin(ctx, out_total, "out_total"));
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return join_mult_common(ctx, d_R, nR, d_S, nS, d_wS, wS_rows, opts, d_out, out_rows, out_total);
}

int rhj_join_mult_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
                           const uint64_t *d_wS, uint64_t wS_rows, const rhj_opts *opts,
                           uint64_t *d_out, uint64_t out_rows, uint64_t *out_total)
{
    RHJCHK(entry_begin(ctx, out_total, "out_total"));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, d_valS, d_idS);  // S's rowIDs name its weights
    return join_mult_common(ctx, nullptr, nR, nullptr, nS, d_wS, wS_rows, opts, d_out, out_rows, out_total);
}

// Lookup join: the partition phase and the repeat ladder of rhj_join_mult_dev / rhj_join_mult_cols_dev, then
// lookup_phase.  d_R / d_S null: the relations are ctx->cols_in.
static_assert(RHJ_LOOKUP_FIRST == 0 && RHJ_LOOKUP_LAST == 1, "launch_lookup_join's which");
static int lookup_common(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS, int which, const rhj_opts *opts,
                         uint64_t *d_out, uint64_t out_rows, uint64_t *out_matched)
{
    if (which != RHJ_LOOKUP_FIRST && which != RHJ_LOOKUP_LAST) return fail(ctx, RHJ_E_INVALID, "which is neither RHJ_LOOKUP_FIRST nor RHJ_LOOKUP_LAST");
    if (out_rows && !d_out) return fail(ctx, RHJ_E_INVALID, "d_out is null");
    if (nR == 0 || nS == 0) return fill_out_words(ctx, d_out, out_rows, 0xFF);
    rhj_opts plan;
    RHJCHK(entry_plan(ctx, nR, nS, opts, &plan));
    CallScope call(ctx);
    ctx->call.mult_out = (u64 *)d_out;
    ctx->call.mult_out_rows = out_rows;
    ctx->call.lookup_which = which;
    return partition_and_join(ctx, d_R, nR, d_S, nS, plan, nullptr, 0, (u64 *)out_matched, nullptr, OUT_LOOKUP);
}

int rhj_lookup_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, int which,
                   const rhj_opts *opts, uint64_t *d_out, uint64_t out_rows, uint64_t *out_matched)
{
    RHJCHK(entry_begin(ctx, out_matched, "out_matched"));
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return lookup_common(ctx, d_R, nR, d_S, nS, which, opts, d_out, out_rows, out_matched);
}

int rhj_lookup_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                        const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS, int which, const rhj_opts *opts,
                        uint64_t *d_out, uint64_t out_rows, uint64_t *out_matched)
{
    RHJCHK(entry_begin(ctx, out_matched, "out_matched"));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, d_valS, d_idS);  // S's rowIDs are the answer
    return lookup_common(ctx, nullptr, nR, nullptr, nS, which, opts, d_out, out_rows, out_matched);
}

// Group-by: R alone through the partition phase and the repeat ladder of the joins (one-sided, planned as an aggregating
// join of R with itself), then group_phase.  d_R null: the relation is ctx->cols_in[0].
static_assert(RHJ_GROUP_MAX_COLS == AGG_MAX_COLS, "rhj.h and rhj_internal.h disagree");
// The RHJ_AGG_* of a call's columns (null: every one RHJ_AGG_SUM) as the kernels' op words (AGG_OP_*), column j at bit AGG_OP_BITS *
// (first + j) of *packed.  Returns the first column whose op is none of them, or ncols.
static u32 pack_ops(const uint32_t *ops, u32 ncols, u32 first, u32 *packed)
{
    static const u32 word[RHJ_AGG_MAX_I64 + 1] = {AGG_OP_ADD, AGG_OP_MIN, AGG_OP_MAX, AGG_OP_MIN | AGG_OP_SIGNED, AGG_OP_MAX | AGG_OP_SIGNED};
    static_assert(RHJ_AGG_SUM == 0 && RHJ_AGG_MIN_U64 == 1 && RHJ_AGG_MAX_U64 == 2 && RHJ_AGG_MIN_I64 == 3 && RHJ_AGG_MAX_I64 == 4, "word[]");
    for (u32 j = 0; ops && j < ncols; j++) {
        if (ops[j] > RHJ_AGG_MAX_I64) return j;
        *packed |= word[ops[j]] << (AGG_OP_BITS * (first + j));
    }
    return ncols;
}

static int group_run(rhj_ctx *ctx, const void *d_R, u64 nR, const uint64_t *const *d_cols, u32 packed, u32 nsum, uint64_t col_rows,
                     const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_sums,
                     uint64_t *const *d_out_rows, uint64_t out_capacity, uint64_t *out_groups, uint64_t *d_out_gid, uint64_t gid_rows);
static int group_common(rhj_ctx *ctx, const void *d_R, u64 nR, const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols,
                        uint64_t col_rows, const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                        uint64_t *const *d_out_sums, uint64_t out_capacity, uint64_t *out_groups, uint64_t *d_out_gid = nullptr,
                        uint64_t gid_rows = 0)
{
    if (ncols > RHJ_GROUP_MAX_COLS) return fail(ctx, RHJ_E_INVALID, "ncols is above RHJ_GROUP_MAX_COLS");
    u32 packed = 0;
    if (const u32 j = pack_ops(ops, ncols, 0, &packed); j != ncols)
        return fail(ctx, RHJ_E_INVALID, "ops[" + std::to_string(j) + "] = " + std::to_string(ops[j]) + " of column " + std::to_string(j) +
                                            " is above RHJ_AGG_MAX_I64");
    if (!d_out_keys && out_capacity) return fail(ctx, RHJ_E_INVALID, "d_out_keys is null with out_capacity > 0");
    const u32 nsum = d_out_keys ? ncols : 0;           // count only: no sum sweep, d_cols is never read
    if (nsum && (!d_cols || !d_out_sums)) return fail(ctx, RHJ_E_INVALID, "null weight column array or d_out_sums");
    for (u32 j = 0; j < nsum; j++)
        if (!d_cols[j] || !d_out_sums[j]) return fail(ctx, RHJ_E_INVALID, "null weight column or sum column");
    return group_run(ctx, d_R, nR, d_cols, packed, nsum, col_rows, opts, d_out_keys, d_out_counts, d_out_sums, nullptr, out_capacity,
                     out_groups, d_out_gid, gid_rows);
}

// The checked arguments of a group-by entry into the context, the one-sided partition phase and group_phase.
// nsum: the columns the kernel sweeps (0 in a count-only call); packed: their op words -- AGG_OP_*, or with d_out_rows (DESIGN 4.23:
// nsum rows arrays beside the nsum value arrays) ARG_OP_*.
static int group_run(rhj_ctx *ctx, const void *d_R, u64 nR, const uint64_t *const *d_cols, u32 packed, u32 nsum, uint64_t col_rows,
                     const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_sums,
                     uint64_t *const *d_out_rows, uint64_t out_capacity, uint64_t *out_groups, uint64_t *d_out_gid, uint64_t gid_rows)
{
    if (nR == 0) return join_nothing(ctx);
    rhj_opts plan;
    RHJCHK(entry_plan(ctx, nR, nR, opts, &plan));
    CallScope call(ctx);
    CallArgs &a = ctx->call;
    for (u32 j = 0; j < nsum; j++) {
        a.agg_cols[j] = (const u64 *)d_cols[j];
        a.group_sums[j] = (u64 *)d_out_sums[j];
        a.group_rows[j] = d_out_rows ? (u64 *)d_out_rows[j] : nullptr;
    }
    a.group_arg = d_out_rows != nullptr && nsum != 0;
    a.agg_ncols = nsum;
    a.agg_col_rows = nsum ? col_rows : ~0ull;
    a.group_keys = (u64 *)d_out_keys;
    a.group_counts = d_out_keys ? (u64 *)d_out_counts : nullptr;
    a.group_cap = d_out_keys ? out_capacity : 0;
    a.group_ops = packed;
    a.gid[0] = (u64 *)d_out_gid;
    a.gid_rows[0] = d_out_gid ? gid_rows : 0;
    a.one_sided = true;
    RHJCHK(partition_and_join(ctx, d_R, nR, nullptr, nR, plan, nullptr, 0, (u64 *)out_groups, nullptr, OUT_GROUP));
    return check_capacity(ctx, d_out_keys, *out_groups, out_capacity, "result buffers");
}

int rhj_group_sum_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                      const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                      uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_sums,
                      uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_R) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return group_common(ctx, d_R, nR, d_cols, nullptr, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_sums, out_capacity, out_groups);
}

// (in the columnar twins the ids travel with the values, also with ncols == 0)
int rhj_group_sum_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                           uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_sums,
                           uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_valR) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR);
    return group_common(ctx, nullptr, nR, d_cols, nullptr, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_sums, out_capacity,
                        out_groups);
}

// ... with an aggregate per column: the same host path, the columns' ops beside them
int rhj_group_agg_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                      const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                      uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_aggs,
                      uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_R) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return group_common(ctx, d_R, nR, d_cols, ops, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_aggs, out_capacity, out_groups);
}

int rhj_group_agg_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                           uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_aggs,
                           uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_valR) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR);
    return group_common(ctx, nullptr, nR, d_cols, ops, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_aggs, out_capacity,
                        out_groups);
}

// ... with the group of every row: the same host path, the id array beside the outputs; a null array: the entry above
int rhj_group_agg_ids_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                          const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                          uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_aggs,
                          uint64_t out_capacity, uint64_t *out_groups, uint64_t *d_out_gid, uint64_t gid_rows)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_R) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return group_common(ctx, d_R, nR, d_cols, ops, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_aggs, out_capacity, out_groups,
                        d_out_gid, gid_rows);
}

int rhj_group_agg_ids_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                               const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                               uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_aggs,
                               uint64_t out_capacity, uint64_t *out_groups, uint64_t *d_out_gid, uint64_t gid_rows)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_valR) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR);
    return group_common(ctx, nullptr, nR, d_cols, ops, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_aggs, out_capacity,
                        out_groups, d_out_gid, gid_rows);
}

// ... with the row of every extreme: the same host path; the checks are this entry's own -- a row column has neither a
// column nor a value array --, the op and tie words travel as ARG_OP_* words, the rows arrays beside the value arrays.  Nothing is
// filled here: the kernel seeds the rows word of every group it emits below the capacity.
static_assert(RHJ_GROUP_ARG_MAX_COLS == AGG_MAX_COLS, "rhj.h and rhj_internal.h disagree");
static int group_arg_common(rhj_ctx *ctx, const void *d_R, u64 nR, const uint64_t *const *d_cols, const uint32_t *ops,
                            const uint32_t *ties, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts, uint64_t *d_out_keys,
                            uint64_t *d_out_counts, uint64_t *const *d_out_vals, uint64_t *const *d_out_rows, uint64_t out_capacity,
                            uint64_t *out_groups)
{
    static const u32 word[RHJ_ARG_ROW + 1] = {AGG_OP_MIN, AGG_OP_MAX, AGG_OP_MIN | AGG_OP_SIGNED, AGG_OP_MAX | AGG_OP_SIGNED, ARG_OP_ROW};
    static_assert(RHJ_ARG_MIN_U64 == 0 && RHJ_ARG_MAX_U64 == 1 && RHJ_ARG_MIN_I64 == 2 && RHJ_ARG_MAX_I64 == 3 && RHJ_ARG_ROW == 4, "word[]");
    if (ncols > RHJ_GROUP_ARG_MAX_COLS) return fail(ctx, RHJ_E_INVALID, "ncols is above RHJ_GROUP_ARG_MAX_COLS");
    if (ncols && !ops) return fail(ctx, RHJ_E_INVALID, "ops is null with ncols > 0");
    u32 packed = 0;
    bool value_op = false;
    for (u32 j = 0; j < ncols; j++) {
        if (ops[j] > RHJ_ARG_ROW)
            return fail(ctx, RHJ_E_INVALID, "ops[" + std::to_string(j) + "] = " + std::to_string(ops[j]) + " of column " + std::to_string(j) +
                                                " is above RHJ_ARG_ROW");
        if (ties && ties[j] > RHJ_ARG_TIE_LAST)
            return fail(ctx, RHJ_E_INVALID, "ties[" + std::to_string(j) + "] = " + std::to_string(ties[j]) + " of column " + std::to_string(j) +
                                                " is above RHJ_ARG_TIE_LAST");
        packed |= (word[ops[j]] | (ties && ties[j] == RHJ_ARG_TIE_LAST ? ARG_OP_LAST : 0u)) << (ARG_OP_BITS * j);
        value_op = value_op || ops[j] != RHJ_ARG_ROW;
    }
    if (!d_out_keys && out_capacity) return fail(ctx, RHJ_E_INVALID, "d_out_keys is null with out_capacity > 0");
    const u32 nsum = d_out_keys && out_capacity ? ncols : 0;      // count only: no sweep, no array is read
    if (nsum && !d_out_rows) return fail(ctx, RHJ_E_INVALID, "d_out_rows is null with out_capacity > 0");
    for (u32 j = 0; j < nsum; j++) {
        if (!d_out_rows[j]) return fail(ctx, RHJ_E_INVALID, "d_out_rows[" + std::to_string(j) + "] of column " + std::to_string(j) + " is null");
        if (ops[j] != RHJ_ARG_ROW && (!d_cols || !d_cols[j] || !d_out_vals || !d_out_vals[j]))
            return fail(ctx, RHJ_E_INVALID, "d_cols[" + std::to_string(j) + "] or d_out_vals[" + std::to_string(j) + "] of column " +
                                                std::to_string(j) + " is null under a value op");
    }
    const uint64_t *cols[AGG_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};   // (a row column's two pointers are never read: null)
    uint64_t *vals[AGG_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    for (u32 j = 0; j < nsum; j++)
        if (ops[j] != RHJ_ARG_ROW) { cols[j] = d_cols[j]; vals[j] = d_out_vals[j]; }
    return group_run(ctx, d_R, nR, cols, packed, nsum, value_op ? col_rows : ~0ull, opts, d_out_keys, d_out_counts, vals, d_out_rows,
                     out_capacity, out_groups, nullptr, 0);
}

int rhj_group_arg_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                      const uint64_t *const *d_cols, const uint32_t *ops, const uint32_t *ties, uint32_t ncols, uint64_t col_rows,
                      const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                      uint64_t *const *d_out_vals, uint64_t *const *d_out_rows, uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_R) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return group_arg_common(ctx, d_R, nR, d_cols, ops, ties, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_vals, d_out_rows,
                            out_capacity, out_groups);
}

int rhj_group_arg_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *const *d_cols, const uint32_t *ops, const uint32_t *ties, uint32_t ncols, uint64_t col_rows,
                           const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                           uint64_t *const *d_out_vals, uint64_t *const *d_out_rows, uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if (nR && !d_valR) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR);
    return group_arg_common(ctx, nullptr, nR, d_cols, ops, ties, ncols, col_rows, opts, d_out_keys, d_out_counts, d_out_vals,
                            d_out_rows, out_capacity, out_groups);
}

// Group-by join: the two-sided partition phase and the repeat ladder of rhj_join_mult_dev / rhj_join_mult_cols_dev,
// then gjoin_phase.  d_R / d_S null: the relations are ctx->cols_in.  An empty S under RHJ_GJ_LEFT: R alone, one-sided and planned
// as the group-by plans it, over a zeroed boundary array of S.
static_assert(RHJ_GROUP_JOIN_MAX_COLS == AGG_MAX_COLS, "rhj.h and rhj_internal.h disagree");
static int group_join_common(rhj_ctx *ctx, const void *d_R, u64 nR, const void *d_S, u64 nS,
                             const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
                             const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows, int mode, const rhj_opts *opts,
                             uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
                             uint64_t *const *d_out_sumsR, uint64_t *const *d_out_sumsS, uint64_t out_capacity, uint64_t *out_groups,
                             uint64_t *d_out_gidR = nullptr, uint64_t gidR_rows = 0, uint64_t *d_out_gidS = nullptr, uint64_t gidS_rows = 0)
{
    if (mode != RHJ_GJ_INNER && mode != RHJ_GJ_LEFT) return fail(ctx, RHJ_E_INVALID, "mode is neither RHJ_GJ_INNER nor RHJ_GJ_LEFT");
    if (ncolsR > RHJ_GROUP_JOIN_MAX_COLS) return fail(ctx, RHJ_E_INVALID, "ncolsR is above RHJ_GROUP_JOIN_MAX_COLS");
    if (ncolsS > RHJ_GROUP_JOIN_MAX_COLS) return fail(ctx, RHJ_E_INVALID, "ncolsS is above RHJ_GROUP_JOIN_MAX_COLS");
    u32 packed = 0;
    if (const u32 j = pack_ops(opsR, ncolsR, 0, &packed); j != ncolsR)
        return fail(ctx, RHJ_E_INVALID, "opsR[" + std::to_string(j) + "] = " + std::to_string(opsR[j]) + " of column " + std::to_string(j) +
                                            " of R is above RHJ_AGG_MAX_I64");
    if (const u32 j = pack_ops(opsS, ncolsS, AGG_MAX_COLS, &packed); j != ncolsS)
        return fail(ctx, RHJ_E_INVALID, "opsS[" + std::to_string(j) + "] = " + std::to_string(opsS[j]) + " of column " + std::to_string(j) +
                                            " of S is above RHJ_AGG_MAX_I64");
    if (!d_out_keys && out_capacity) return fail(ctx, RHJ_E_INVALID, "d_out_keys is null with out_capacity > 0");
    const u32 nsumR = d_out_keys ? ncolsR : 0, nsumS = d_out_keys ? ncolsS : 0;   // count only: no sum sweep, no column is read
    if (nsumR && (!d_colsR || !d_out_sumsR)) return fail(ctx, RHJ_E_INVALID, "null weight column array of R or d_out_sumsR");
    if (nsumS && (!d_colsS || !d_out_sumsS)) return fail(ctx, RHJ_E_INVALID, "null weight column array of S or d_out_sumsS");
    for (u32 j = 0; j < nsumR; j++)
        if (!d_colsR[j] || !d_out_sumsR[j]) return fail(ctx, RHJ_E_INVALID, "null weight column or sum column of R");
    for (u32 j = 0; j < nsumS; j++)
        if (!d_colsS[j] || !d_out_sumsS[j]) return fail(ctx, RHJ_E_INVALID, "null weight column or sum column of S");
    CallScope call(ctx);
    CallArgs &a = ctx->call;
    a.gid[0] = (u64 *)d_out_gidR; a.gid_rows[0] = d_out_gidR ? gidR_rows : 0;
    a.gid[1] = (u64 *)d_out_gidS; a.gid_rows[1] = d_out_gidS ? gidS_rows : 0;
    if (nR == 0 || (nS == 0 && mode == RHJ_GJ_INNER)) {    // no group, no kernel: every id word says so when the call returns
        RHJCHK(fill_no_group(ctx));
        if (a.gid[0] || a.gid[1]) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return join_nothing(ctx);
    }
    const bool one = nS == 0;                          // LEFT over an empty S: the group-by of R with zero S fields
    rhj_opts plan;
    RHJCHK(entry_plan(ctx, nR, one ? nR : nS, opts, &plan));
    for (u32 j = 0; j < nsumR; j++) { a.agg_cols[j] = (const u64 *)d_colsR[j]; a.group_sums[j] = (u64 *)d_out_sumsR[j]; }
    for (u32 j = 0; j < nsumS; j++) { a.gjoin_colsS[j] = (const u64 *)d_colsS[j]; a.gjoin_sumsS[j] = (u64 *)d_out_sumsS[j]; }
    a.agg_ncols = nsumR;
    a.agg_col_rows = nsumR ? colR_rows : ~0ull;
    a.gjoin_ncolsS = nsumS;
    a.gjoin_colS_rows = nsumS ? colS_rows : ~0ull;
    a.group_keys = (u64 *)d_out_keys;
    a.group_counts = d_out_keys ? (u64 *)d_out_cntR : nullptr;
    a.gjoin_cntS = d_out_keys ? (u64 *)d_out_cntS : nullptr;
    a.group_cap = d_out_keys ? out_capacity : 0;
    a.gjoin_left = mode == RHJ_GJ_LEFT;
    a.group_ops = packed;
    a.one_sided = one;
    RHJCHK(partition_and_join(ctx, d_R, nR, one ? nullptr : d_S, one ? nR : nS, plan, nullptr, 0, (u64 *)out_groups, nullptr, OUT_GJOIN));
    return check_capacity(ctx, d_out_keys, *out_groups, out_capacity, "result buffers");
}

int rhj_group_join_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                       const uint64_t *const *d_colsR, uint32_t ncolsR, uint64_t colR_rows,
                       const uint64_t *const *d_colsS, uint32_t ncolsS, uint64_t colS_rows,
                       int mode, const rhj_opts *opts,
                       uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
                       uint64_t *const *d_out_sumsR, uint64_t *const *d_out_sumsS,
                       uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return group_join_common(ctx, d_R, nR, d_S, nS, d_colsR, nullptr, ncolsR, colR_rows, d_colsS, nullptr, ncolsS, colS_rows, mode, opts,
                             d_out_keys, d_out_cntR, d_out_cntS, d_out_sumsR, d_out_sumsS, out_capacity, out_groups);
}

// (in the columnar twins the ids travel with the values, also with no column; an empty S has no columns)
int rhj_group_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                            const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
                            const uint64_t *const *d_colsR, uint32_t ncolsR, uint64_t colR_rows,
                            const uint64_t *const *d_colsS, uint32_t ncolsS, uint64_t colS_rows,
                            int mode, const rhj_opts *opts,
                            uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
                            uint64_t *const *d_out_sumsR, uint64_t *const *d_out_sumsS,
                            uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, nS ? d_valS : nullptr, nS ? d_idS : nullptr);
    return group_join_common(ctx, nullptr, nR, nullptr, nS, d_colsR, nullptr, ncolsR, colR_rows, d_colsS, nullptr, ncolsS, colS_rows,
                             mode, opts, d_out_keys, d_out_cntR, d_out_cntS, d_out_sumsR, d_out_sumsS, out_capacity, out_groups);
}

// ... with an aggregate per column: the same host path, each side's ops beside its columns
int rhj_group_join_agg_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                           const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
                           const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
                           int mode, const rhj_opts *opts,
                           uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
                           uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
                           uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return group_join_common(ctx, d_R, nR, d_S, nS, d_colsR, opsR, ncolsR, colR_rows, d_colsS, opsS, ncolsS, colS_rows, mode, opts,
                             d_out_keys, d_out_cntR, d_out_cntS, d_out_aggsR, d_out_aggsS, out_capacity, out_groups);
}

int rhj_group_join_agg_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                                const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
                                const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
                                const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
                                int mode, const rhj_opts *opts,
                                uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
                                uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
                                uint64_t out_capacity, uint64_t *out_groups)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, nS ? d_valS : nullptr, nS ? d_idS : nullptr);
    return group_join_common(ctx, nullptr, nR, nullptr, nS, d_colsR, opsR, ncolsR, colR_rows, d_colsS, opsS, ncolsS, colS_rows,
                             mode, opts, d_out_keys, d_out_cntR, d_out_cntS, d_out_aggsR, d_out_aggsS, out_capacity, out_groups);
}

// ... with the group of every row of either side: the same host path, the id arrays beside the outputs
int rhj_group_join_agg_ids_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                               const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
                               const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
                               int mode, const rhj_opts *opts,
                               uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
                               uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
                               uint64_t out_capacity, uint64_t *out_groups,
                               uint64_t *d_out_gidR, uint64_t gidR_rows, uint64_t *d_out_gidS, uint64_t gidS_rows)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if ((nR && !d_R) || (nS && !d_S)) return fail(ctx, RHJ_E_INVALID, "null input relation");
    return group_join_common(ctx, d_R, nR, d_S, nS, d_colsR, opsR, ncolsR, colR_rows, d_colsS, opsS, ncolsS, colS_rows, mode, opts,
                             d_out_keys, d_out_cntR, d_out_cntS, d_out_aggsR, d_out_aggsS, out_capacity, out_groups,
                             d_out_gidR, gidR_rows, d_out_gidS, gidS_rows);
}

int rhj_group_join_agg_ids_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                                    const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
                                    const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
                                    const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
                                    int mode, const rhj_opts *opts,
                                    uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
                                    uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
                                    uint64_t out_capacity, uint64_t *out_groups,
                                    uint64_t *d_out_gidR, uint64_t gidR_rows, uint64_t *d_out_gidS, uint64_t gidS_rows)
{
    RHJCHK(entry_begin(ctx, out_groups, "out_groups"));
    if ((nR && !d_valR) || (nS && !d_valS)) return fail(ctx, RHJ_E_INVALID, "null value column");
    ColsScope cols(ctx, d_valR, d_idR, nS ? d_valS : nullptr, nS ? d_idS : nullptr);
    return group_join_common(ctx, nullptr, nR, nullptr, nS, d_colsR, opsR, ncolsR, colR_rows, d_colsS, opsS, ncolsS, colS_rows,
                             mode, opts, d_out_keys, d_out_cntR, d_out_cntS, d_out_aggsR, d_out_aggsS, out_capacity, out_groups,
                             d_out_gidR, gidR_rows, d_out_gidS, gidS_rows);
}


namespace {

// A large result page is fresh mmap'd memory: every 4 KiB (or, with transparent huge pages, 2 MiB) page must
// be faulted in before the device-to-host copy can land, and a DMA that takes those faults itself runs at
// ~18 GB/s.  PagePrefault allocates the page for the optimistic size early and touches it from a few helper
// threads WHILE the inputs are copied in and the kernels run; the final copy then runs at the PCIe rate.
struct PagePrefault {
    unsigned char *page = nullptr;
    size_t pairs = 0;
    std::vector<std::thread> workers;
    std::atomic<bool> stop{false};         // drop(): the result turned out empty / too large -- stop touching at once
    void start(size_t npairs)
    {
        const size_t bytes = 8 + npairs * 16;
        if (npairs * 16 < ((size_t)64 << 20)) return;             // small pages: not worth threads
        page = (unsigned char *)malloc(bytes);
        if (!page) return;
        pairs = npairs;
        const uintptr_t lo = ((uintptr_t)page + ((uintptr_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1);
        const uintptr_t hi = ((uintptr_t)page + bytes) & ~(((uintptr_t)2 << 20) - 1);
        if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
        const int nt = 4;
        for (int t = 0; t < nt; t++)
            workers.emplace_back([=] {
                const size_t from = bytes / nt * t, to = t + 1 == nt ? bytes : bytes / nt * (t + 1);
                for (size_t o = from; o < to && !stop.load(std::memory_order_relaxed); o += 4096)
                    ((volatile unsigned char *)page)[o] = 0;
            });
    }
    void wait() { for (std::thread &w : workers) w.join(); workers.clear(); }
    void drop() { stop.store(true); wait(); free(page); page = nullptr; pairs = 0; }
    ~PagePrefault() { wait(); }
};

}  // namespace

namespace {

// rhj_join for small inputs (the 94 joins of small.work are <= 43 K tuples).  Every asynchronous operation
// costs 5-10 us of latency on this platform whatever its size (measured: 2 H2D + memset + kernel + 2 D2H = 48 us for a
// 3754 x 14368 join whose kernel runs ~10 us), so the sequence is cut to THREE operations and one host synchronisation:
//   H2D R, H2D S, ONE kernel (k_join_bkt DIRECT) that stores the pairs into HBM AND, the first MiB of them, straight into
//   pinned host memory, and whose last workgroup publishes the result count there and zeroes the device counters for the
//   next call.  One memcpy fills the exact-size page; what a larger result has beyond the first MiB is fetched from HBM
//   straight into the page (no second run: the pairs have the same positions in both places).
constexpr size_t LAND_BYTES = (size_t)1 << 20;

int join_small_host(rhj_ctx *ctx, const rhj_tuple *R, u64 nR, const rhj_tuple *S, u64 nS, void **out_page, u64 *out_count)
{
    static const bool trace = getenv("RHJ_TRACE_SMALL") != nullptr;       // tuning aid: host-side timeline on stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::micro>(b - a).count();
    };
    const auto t0 = now();
    const u64 guess = (nR > nS ? nR : nS) + 1024, landcap = LAND_BYTES / 16;
    RHJCHK(ensure(ctx, ctx->in_R, (size_t)nR * 16));
    RHJCHK(ensure(ctx, ctx->in_S, (size_t)nS * 16));
    if (!ctx->h_land || !ctx->h_land_dev) {
        if (ctx->h_land) { (void)hipHostFree(ctx->h_land); ctx->h_land = nullptr; }      // an earlier attempt got the memory but no device address
        ctx->h_land_dev = nullptr;
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_land, 64 + LAND_BYTES, hipHostMallocDefault));
        const hipError_t e = hipHostGetDevicePointer((void **)&ctx->h_land_dev, ctx->h_land, 0);
        if (e != hipSuccess || !ctx->h_land_dev) {
            (void)hipHostFree(ctx->h_land);
            ctx->h_land = nullptr;
            ctx->h_land_dev = nullptr;
            return fail(ctx, RHJ_E_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
        }
    }
    if (ctx->small_out.cap < 64 + (size_t)guess * 16) {
        RHJCHK(ensure(ctx, ctx->small_out, 64 + (size_t)guess * 16));
        ctx->small_hdr_clean = false;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->in_R.p, R, (size_t)nR * 16, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->in_S.p, S, (size_t)nS * 16, hipMemcpyHostToDevice, ctx->stream));
    ctx->last.passes = 0;
    ctx->last.bits1 = ctx->last.bits2 = 0;
    ctx->last.ntasks = 0;
    ctx->last_join_kind = -1;
    ctx->cur_narrow = 0;
    u64 count = 0, landed = 0;
    const u64 unpublished = ~0ull;                                            // the kernel's last workgroup overwrites it with the count
    for (int attempt = 0; attempt < 2; attempt++) {
        *(volatile u64 *)ctx->h_land = unpublished;
        // device buffer: {64-byte header: [0] count, [8] finished workgroups | pairs}; the first MiB of pairs and the count
        // land in pinned host memory as well, written by the kernel itself
        unsigned char *d_hdr = (unsigned char *)ctx->small_out.p;
        const u64 dcap = (ctx->small_out.cap - 64) / 16;
        if (!ctx->small_hdr_clean) HIPCHK(ctx, hipMemsetAsync(d_hdr, 0, 64, ctx->stream));
        ctx->small_hdr_clean = false;
        {
            Span s(ctx, RHJ_K_JOIN);
            launch_join_direct(ctx->stream, ctx->in_R.p, nR, ctx->in_S.p, nS, d_hdr + 64, dcap, (u64 *)d_hdr,
                               (u64 *)ctx->h_land_dev, (u32 *)(d_hdr + 8), ctx->h_land_dev + 64, landcap);
        }
        RHJCHK(check_launch(ctx, "direct join"));
        const auto t1 = now();
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->small_hdr_clean = true;                                      // the last workgroup zeroed the counters
        count = *(volatile const u64 *)ctx->h_land;
        if (count == unpublished) return fail(ctx, RHJ_E_HIP, "the direct join kernel did not publish its result count");
        landed = dcap < landcap ? dcap : landcap;
        if (trace) fprintf(stderr, "[small join %llu x %llu -> %llu] enqueue %.1f  sync %.1f us\n", (unsigned long long)nR,
                           (unsigned long long)nS, (unsigned long long)count, us(t0, t1), us(t1, now()));
        if (count <= dcap) break;                                         // every pair is in HBM (and the first MiB on the host)
        if (attempt == 1) return fail(ctx, RHJ_E_HIP, "result count changed between join phases");
        RHJCHK(ensure(ctx, ctx->small_out, 64 + (size_t)count * 16));     // more pairs than the buffer holds: exact size known now
        ctx->small_hdr_clean = false;
    }
    unsigned char *page = nullptr;
    if (count) {
        page = (unsigned char *)malloc(8 + (size_t)count * 16);
        if (!page) return fail(ctx, RHJ_E_NOMEM, "malloc of the result page failed");
        memset(page, 0, 8);                                               // bucket_info::next = nullptr (Result.h:14-17)
        const u64 got = count < landed ? count : landed;
        memcpy(page + 8, ctx->h_land + 64, (size_t)got * 16);
        if (count > got) {                                                // the rest straight from HBM into the page
            hipError_t e = hipMemcpyAsync(page + 8 + got * 16, (const unsigned char *)ctx->small_out.p + 64 + got * 16,
                                          (size_t)(count - got) * 16, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) { free(page); return fail(ctx, RHJ_E_HIP, std::string("result copy: ") + hipGetErrorString(e)); }
        }
    }
    *out_page = page;                                                     // nullptr when nothing matched (Result::isEmpty)
    *out_count = count;
    return RHJ_OK;
}

}  // namespace

namespace {

// rhj_join for inputs of hundreds of MiB: PCIe is full duplex, so the call should cost about max(upload, download), not their
// sum.  R is uploaded and partitioned once; S goes through in CHUNKS -- R join S = union of R join S_i --: while chunk i+1 is
// being staged and uploaded, chunk i is partitioned (same radix plan) and joined against the partitioned R, its pairs landing
// behind the earlier chunks' in the pair buffer (the result counter simply runs on), and a downloader thread brings finished
// ranges of pairs home into the result page.  Returns RHJ_NOT_PIPELINED when the call should take the plain path instead
// (small inputs, a rowID that does not fit the narrow format, more pairs than the optimistic page holds).
constexpr int RHJ_NOT_PIPELINED = 1001;
constexpr int RHJ_NOT_PIPELINED_WIDE = 1002;           // ... because a rowID did not fit the narrow format: the repeat runs 16-byte
constexpr u64 PIPE_MIN_CHUNK = (u64)8 << 20;           // tuples per S chunk at least
constexpr int PIPE_MAX_CHUNKS = 16;

int join_host_pipelined(rhj_ctx *ctx, const rhj_tuple *R, u64 nR, const rhj_tuple *S, u64 nS, const rhj_opts &plan,
                        void **out_page, u64 *out_count)
{
    static const bool off = getenv("RHJ_NO_PIPELINE") != nullptr;                 // tuning aid: A/B against the plain path
    static const bool trace = getenv("RHJ_TRACE_JOIN") != nullptr;
    static const u64 max_chunks = env_u64("RHJ_PIPE_CHUNKS", 12, 2, PIPE_MAX_CHUNKS);   // tuning aid
    // tests shrink the path with it (tests/pipeline_cases.py), but not below the 64 MiB result page under which PagePrefault
    // starts nothing (no page: RHJ_NOT_PIPELINED below): max(nR, nS) + 1024 >= 4 194 304 whatever the chunk size
    static const u64 min_chunk = env_u64("RHJ_PIPE_MIN_CHUNK", PIPE_MIN_CHUNK, 1 << 16, 1 << 26);
    int K = (int)(nS / min_chunk < max_chunks ? nS / min_chunk : max_chunks);
    if (off || plan.passes < 1 || nS < 4 * min_chunk || K < 2 || nR < min_chunk / 2) return RHJ_NOT_PIPELINED;
    const u64 chunk = ((nS + K - 1) / K + 4095) / 4096 * 4096;
    K = (int)((nS + chunk - 1) / chunk);
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t0 = now();
    const u64 cap = (nR > nS ? nR : nS) + 1024;
    PagePrefault pre;
    pre.start((size_t)cap);
    if (!pre.page) return RHJ_NOT_PIPELINED;
    const int narrow = narrow_level(ctx, nR, chunk, plan);
    const int tb = plan.bits1 + (plan.passes == 2 ? plan.bits2 : 0);
    const size_t np = (size_t)1 << tb;
    auto setup = [&]() -> int {
        RHJCHK(ensure(ctx, ctx->in_R, (size_t)nR * 16));
        RHJCHK(ensure(ctx, ctx->in_S, (size_t)nS * 16));
        RHJCHK(ensure(ctx, ctx->part_R, (size_t)nR * 16));
        RHJCHK(ensure(ctx, ctx->part_S, (size_t)chunk * 16));
        RHJCHK(ensure(ctx, ctx->ps_R, (np + 1) * 8));
        RHJCHK(ensure(ctx, ctx->ps_S, (np + 1) * 8));
        RHJCHK(ensure(ctx, ctx->out_pairs, (size_t)cap * 16));
        RHJCHK(ensure(ctx, ctx->counters, 64));
        RHJCHK(ensure(ctx, ctx->narrow_flag, 64));
        if (!ctx->copy_stream) {
            HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
            for (int i = 0; i < 2; i++) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->up_ev[i], hipEventDisableTiming));
        }
        if (!ctx->down_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
        if (!ctx->h_counts) HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_counts, (size_t)PIPE_MAX_CHUNKS * 128, hipHostMallocDefault));
        while ((int)ctx->chunk_ev.size() < K) {
            hipEvent_t e;
            HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ctx->chunk_ev.push_back(e);
        }
        return RHJ_OK;
    };
    int rc = setup();
    if (rc != RHJ_OK) { pre.drop(); return rc; }
    const u64 dcap = ctx->out_pairs.cap / 16 < pre.pairs ? ctx->out_pairs.cap / 16 : pre.pairs;
    unsigned char *page = pre.page;

    // downloader: finished ranges of pairs -> result page, on its own stream, while later chunks are still coming in
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::pair<u64, u64>> todo;                 // (first pair, pairs)
    bool closing = false, dl_failed = false;
    std::chrono::steady_clock::time_point t_faulted = t0, t_dl_first = t0;
    std::thread downloader([&] {
        (void)hipSetDevice(ctx->device);
        pre.wait();                                        // the helper threads still WRITE into the page while they fault it in
        t_faulted = now();
        for (;;) {
            std::pair<u64, u64> job;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return closing || !todo.empty(); });
                if (todo.empty()) return;
                job = todo.front();
                todo.erase(todo.begin());
            }
            hipError_t e = hipMemcpyAsync(page + 8 + job.first * 16, (const unsigned char *)ctx->out_pairs.p + job.first * 16,
                                          (size_t)job.second * 16, hipMemcpyDeviceToHost, ctx->down_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->down_stream);
            if (e != hipSuccess) dl_failed = true;
            if (t_dl_first == t0) t_dl_first = now();
        }
    });
    auto finish_downloader = [&] {
        { std::lock_guard<std::mutex> lk(mu); closing = true; }
        cv.notify_all();
        downloader.join();
    };

    bool abandon = false, saw_wide = false;                // wide rowID / more pairs than the page holds: take the plain path
    std::string errtext;
    u64 handed = 0, count = 0;
    int collected = 0;
    auto collect = [&](int j) {                            // chunk j's join has finished: hand its pairs to the downloader
        const u64 *h = (const u64 *)(ctx->h_counts + (size_t)j * 128);
        const u32 wide = *(const u32 *)(ctx->h_counts + (size_t)j * 128 + 64);
        if (wide || h[0] > dcap) { abandon = true; saw_wide = wide != 0; return; }
        if (h[5]) { errtext = "a partition's build side has " + std::to_string(h[5]) + " tuples (>= 2^32): use more radix bits"; return; }
        count = h[0];
        ctx->last.ntasks += (u32)(h[1] & 0xffffffffu);
        if (count > handed) {
            { std::lock_guard<std::mutex> lk(mu); todo.emplace_back(handed, count - handed); }
            cv.notify_all();
            handed = count;
        }
    };
    auto body = [&]() -> int {
        ctx->cur_narrow = narrow;
        ctx->last.passes = plan.passes;
        ctx->last.bits1 = plan.bits1;
        ctx->last.bits2 = plan.bits2;
        ctx->counters_clean = false;
        HIPCHK(ctx, hipMemsetAsync(ctx->narrow_flag.p, 0, 64, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ctx->up_ev[0], ctx->stream));           // (earlier work of this context may still read in_R / in_S)
        HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->up_ev[0], 0));
        RHJCHK(h2d_staged(ctx, ctx->in_R.p, R, (size_t)nR * 16, ctx->copy_stream));
        HIPCHK(ctx, hipEventRecord(ctx->up_ev[0], ctx->copy_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->up_ev[0], 0));
        RHJCHK(partition_side(ctx, ctx->in_R.p, nR, plan, narrow, ctx->part_R.p, (u64 *)ctx->ps_R.p));
        for (int i = 0; i < K && !abandon && errtext.empty(); i++) {
            const u64 off_i = (u64)i * chunk, n_i = nS - off_i < chunk ? nS - off_i : chunk;
            void *d_Si = (unsigned char *)ctx->in_S.p + off_i * 16;
            RHJCHK(h2d_staged(ctx, d_Si, S + off_i, (size_t)n_i * 16, ctx->copy_stream));
            HIPCHK(ctx, hipEventRecord(ctx->up_ev[1], ctx->copy_stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->up_ev[1], 0));
            RHJCHK(partition_side(ctx, d_Si, n_i, plan, narrow, ctx->part_S.p, (u64 *)ctx->ps_S.p));
            u64 unused = 0;
            RHJCHK(join_phase_on(ctx, ctx->part_R.p, (const u64 *)ctx->ps_R.p, nR, ctx->part_S.p, (const u64 *)ctx->ps_S.p, n_i, np, tb,
                                 (u32)plan.probe_split, ctx->out_pairs.p, dcap, &unused, narrow != 0, nullptr, false, false, i > 0, true));
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_counts + (size_t)i * 128, ctx->counters.p, 64, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_counts + (size_t)i * 128 + 64, ctx->narrow_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipEventRecord(ctx->chunk_ev[i], ctx->stream));
            while (collected < i && hipEventQuery(ctx->chunk_ev[collected]) == hipSuccess) collect(collected++);
        }
        for (; collected < K && !abandon && errtext.empty(); collected++) {
            HIPCHK(ctx, hipEventSynchronize(ctx->chunk_ev[collected]));
            collect(collected);
        }
        return RHJ_OK;
    };
    rc = body();
    const auto t1 = now();
    finish_downloader();
    (void)hipStreamSynchronize(ctx->stream);               // nothing of this call is in flight when it returns
    (void)hipGetLastError();
    if (rc == RHJ_OK && !errtext.empty()) rc = fail(ctx, RHJ_E_INVALID, errtext);
    if (rc == RHJ_OK && dl_failed) rc = fail(ctx, RHJ_E_HIP, "result copy failed");
    if (rc != RHJ_OK || abandon || count == 0) {
        pre.page = page;                                   // (drop() frees it)
        pre.drop();
        if (rc != RHJ_OK) return rc;
        if (abandon && saw_wide) { narrow_note_fallback(ctx); return RHJ_NOT_PIPELINED_WIDE; }
        if (abandon) return RHJ_NOT_PIPELINED;
        narrow_note_done(ctx, plan, narrow != 0);
        ctx->last_pipelined = K;                           // (every chunk went through: an empty result is no fall-back)
        *out_page = nullptr;                               // no match: head stays nullptr (Result::isEmpty)
        *out_count = 0;
        return RHJ_OK;
    }
    narrow_note_done(ctx, plan, narrow != 0);
    pre.page = nullptr;                                    // the caller's now
    ctx->last_pipelined = K;
    memset(page, 0, 8);                                    // bucket_info::next = nullptr (Result.h:14-17)
    if (trace)
        fprintf(stderr, "[rhj_join pipelined %llu x %llu -> %llu, %d chunks of S] enqueued %.1f  tail (last join + download) %.1f  total %.1f ms"
                        "  (result page faulted in at %.1f, first range home at %.1f)\n",
                (unsigned long long)nR, (unsigned long long)nS, (unsigned long long)count, K, ms(t0, t1), ms(t1, now()), ms(t0, now()),
                ms(t0, t_faulted), ms(t0, t_dl_first));
    *out_page = page;
    *out_count = count;
    return RHJ_OK;
}

}  // namespace

int rhj_join(rhj_ctx *ctx, const rhj_tuple *R, uint64_t nR, const rhj_tuple *S, uint64_t nS,
             const rhj_opts *opts, void **out_page, uint64_t *out_count)
{
    RHJCHK(use_device(ctx));
    if (!out_page || !out_count) return fail(ctx, RHJ_E_INVALID, "null output argument");
    *out_page = nullptr;
    *out_count = 0;
    prof_reset(ctx);
    ctx->last_pipelined = 0;
    if (nR == 0 || nS == 0) return join_nothing(ctx);
    if (!R || !S) return fail(ctx, RHJ_E_INVALID, "null input relation");
    rhj_opts plan;
    if (resolve_plan(nR, nS, opts, &plan, false, default_join_kernels(ctx)) != RHJ_OK) return fail(ctx, RHJ_E_INVALID, "bad rhj_opts");
    if (plan.passes == 0 && is_direct(ctx, 1, nR, nS)) return join_small_host(ctx, R, nR, S, nS, out_page, (u64 *)out_count);
    {
        const int prc = join_host_pipelined(ctx, R, nR, S, nS, plan, out_page, (u64 *)out_count);
        if (prc != RHJ_NOT_PIPELINED && prc != RHJ_NOT_PIPELINED_WIDE) return prc;
        prof_reset(ctx);
        if (prc == RHJ_NOT_PIPELINED_WIDE) {                // the pipelined attempt has met a wide rowID (and recorded it): the
            ctx->narrow_off_once = true;                    // plain path below goes straight to 16-byte tuples
        }
    }
    struct OffOnce { rhj_ctx *c; ~OffOnce() { c->narrow_off_once = false; } } off_once{ctx};
    // optimistic capacity: a foreign-key join yields about max(|R|,|S|) pairs; the count is exact
    // either way, and an overflow only repeats the join phase (partitions stay in the workspace)
    u64 cap = (nR > nS ? nR : nS) + 1024;
    static const bool trace = getenv("RHJ_TRACE_JOIN") != nullptr;        // tuning aid: host-side timeline on stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t0 = now();
    std::chrono::steady_clock::time_point tR = t0, tS = t0, tK = t0;
    PagePrefault pre;
    pre.start((size_t)cap);                           // host page being faulted in while the GPU side proceeds
    int rc = RHJ_OK;
    u64 count = 0;
    auto body = [&]() -> int {
        RHJCHK(ensure(ctx, ctx->in_R, (size_t)nR * 16));
        RHJCHK(ensure(ctx, ctx->in_S, (size_t)nS * 16));
        RHJCHK(ensure(ctx, ctx->out_pairs, (size_t)cap * 16));
        u64 dcap = ctx->out_pairs.cap / 16;
        // uploads on their own stream: R first; S while the kernels that partition R run (the host is busy staging S by then)
        if (!ctx->copy_stream) {
            HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
            for (int i = 0; i < 2; i++) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->up_ev[i], hipEventDisableTiming));
        }
        HIPCHK(ctx, hipEventRecord(ctx->up_ev[0], ctx->stream));          // (earlier work of this context may still read in_R)
        HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->up_ev[0], 0));
        RHJCHK(h2d_staged(ctx, ctx->in_R.p, R, (size_t)nR * 16, ctx->copy_stream));
        tR = now();
        HIPCHK(ctx, hipEventRecord(ctx->up_ev[0], ctx->copy_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->up_ev[0], 0));
        std::function<int()> upload_S = [&]() -> int {
            RHJCHK(h2d_staged(ctx, ctx->in_S.p, S, (size_t)nS * 16, ctx->copy_stream));
            HIPCHK(ctx, hipEventRecord(ctx->up_ev[1], ctx->copy_stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->up_ev[1], 0));
            tS = now();
            return RHJ_OK;
        };
        RHJCHK(partition_and_join(ctx, ctx->in_R.p, nR, ctx->in_S.p, nS, plan, ctx->out_pairs.p, dcap, &count, &upload_S));
        if (count > dcap) {
            RHJCHK(ensure(ctx, ctx->out_pairs, (size_t)count * 16));
            dcap = ctx->out_pairs.cap / 16;
            u64 again = 0;
            RHJCHK(join_phase(ctx, ctx->out_pairs.p, dcap, &again));
            if (again != count) return fail(ctx, RHJ_E_HIP, "result count changed between join phases");
        }
        return RHJ_OK;
    };
    rc = body();
    tK = now();
    if (rc != RHJ_OK || count == 0) {                 // count == 0: head stays nullptr (Result::isEmpty)
        pre.drop();
        return rc;
    }
    unsigned char *page = nullptr;
    if (pre.page && count <= pre.pairs) {             // the pre-faulted block is large enough (it may be larger than
        pre.wait();                                   // needed: the block is the caller's to free() either way)
        page = pre.page;
        pre.page = nullptr;
    } else {
        pre.drop();
        page = (unsigned char *)malloc(8 + (size_t)count * 16);
        if (!page) return fail(ctx, RHJ_E_NOMEM, "malloc of the result page failed");
        if ((size_t)count * 16 >= ((size_t)64 << 20)) {
            const uintptr_t lo = ((uintptr_t)page + ((uintptr_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1);
            const uintptr_t hi = ((uintptr_t)page + 8 + (size_t)count * 16) & ~(((uintptr_t)2 << 20) - 1);
            if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
        }
    }
    memset(page, 0, 8);                               // bucket_info::next = nullptr (Result.h:14-17)
    hipError_t e = hipMemcpyAsync(page + 8, ctx->out_pairs.p, (size_t)count * 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { free(page); return fail(ctx, RHJ_E_HIP, std::string("result copy: ") + hipGetErrorString(e)); }
    if (trace)
        fprintf(stderr, "[rhj_join %llu x %llu -> %llu] R staged %.1f  S staged %.1f  kernels + count %.1f  result copy %.1f  total %.1f ms\n",
                (unsigned long long)nR, (unsigned long long)nS, (unsigned long long)count, ms(t0, tR), ms(tR, tS), ms(tS, tK),
                ms(tK, now()), ms(t0, now()));
    *out_page = page;
    *out_count = count;
    return RHJ_OK;
}

// ---- several small joins per launch (MainScheduler.cpp:6-30 / join.cpp:42-50: the reference keeps 8 queries in
// flight; their joins are so small -- <= 43 K tuples on small.work -- that launch, copy and synchronisation latencies are
// their whole cost) ------------------------------------------------------------------------------------------------------
namespace {

constexpr u32 BATCH_MAX = 16;                           // joins per launch (grid.y)
constexpr size_t BATCH_PIECE = (size_t)256 << 10;       // host copies are cut into pieces of this size for the helper threads

int ensure_pinned(rhj_ctx *ctx, unsigned char **p, size_t *cap, size_t bytes, unsigned char **dev = nullptr)
{
    if (*cap >= bytes) return RHJ_OK;
    if (*p) { (void)hipHostFree(*p); *p = nullptr; *cap = 0; }
    size_t want = (size_t)8 << 20;
    while (want < bytes) want <<= 1;
    HIPCHK(ctx, hipHostMalloc((void **)p, want, hipHostMallocDefault));
    *cap = want;
    if (dev) {
        if (hipHostGetDevicePointer((void **)dev, *p, 0) != hipSuccess || !*dev) {
            (void)hipGetLastError();
            (void)hipHostFree(*p);
            *p = nullptr; *cap = 0;
            return fail(ctx, RHJ_E_HIP, "no device address for pinned host memory");
        }
    }
    return RHJ_OK;
}

void add_pieces(std::vector<CopySeg> &v, void *dst, const void *src, size_t bytes)
{
    for (size_t o = 0; o < bytes; o += BATCH_PIECE)
        v.push_back(CopySeg{(char *)dst + o, (const char *)src + o, bytes - o < BATCH_PIECE ? bytes - o : BATCH_PIECE});
}

// One group of <= BATCH_MAX direct joins = ONE staged upload, ONE launch, ONE wait.  A context has two slots (staging buffer,
// device buffers, landing zone, counters, event), so that the host work of a group -- staging its inputs, filling its
// result pages -- overlaps the GPU work of its neighbour:   stage(g+1) | GPU(g)   and   pages(g) | GPU(g+1).
struct BatchSlot {
    u32 k = 0;
    const u32 *idx = nullptr;
    size_t in_bytes = 0, out_off[BATCH_MAX] = {0}, land_off[BATCH_MAX] = {0};
    u64 dcap[BATCH_MAX] = {0}, lcap[BATCH_MAX] = {0};
    u32 max_blocks = 0;
};

int batch_stage(rhj_ctx *ctx, int sl, BatchSlot &b, const rhj_join_desc *J, const u32 *idx, u32 k)
{
    const size_t A = 256;
    auto up = [&](size_t x) { return (x + A - 1) & ~(A - 1); };
    size_t in_off[BATCH_MAX][2];
    size_t in_bytes = up(BATCH_MAX * sizeof(BatchJoinDesc)), out_bytes = 0, land_bytes = 128;
    b.k = k;
    b.idx = idx;
    for (u32 i = 0; i < k; i++) {
        const rhj_join_desc &j = J[idx[i]];
        in_off[i][0] = in_bytes; in_bytes += up((size_t)j.nR * 16);
        in_off[i][1] = in_bytes; in_bytes += up((size_t)j.nS * 16);
        const u64 guess = (j.nR > j.nS ? j.nR : j.nS) + 1024;
        b.lcap[i] = guess;                                  // what a foreign-key join yields lands in pinned memory ...
        b.dcap[i] = guess * 32;                             // ... a many-to-many result still fits the device buffer
        b.out_off[i] = out_bytes; out_bytes += up((size_t)b.dcap[i] * 16);
        b.land_off[i] = land_bytes; land_bytes += up((size_t)b.lcap[i] * 16);
    }
    b.in_bytes = in_bytes;
    RHJCHK(ensure_pinned(ctx, &ctx->b_stage[sl], &ctx->b_stage_cap[sl], in_bytes));
    RHJCHK(ensure_pinned(ctx, &ctx->b_land[sl], &ctx->b_land_cap[sl], land_bytes, &ctx->b_land_dev[sl]));
    RHJCHK(ensure(ctx, ctx->b_in[sl], in_bytes));
    RHJCHK(ensure(ctx, ctx->b_out[sl], out_bytes));
    if (!ctx->b_cnt[sl].p) {
        RHJCHK(ensure(ctx, ctx->b_cnt[sl], BATCH_MAX * 16));
        HIPCHK(ctx, hipMemsetAsync(ctx->b_cnt[sl].p, 0, BATCH_MAX * 16, ctx->stream));  // the kernels leave it zeroed from here on
    }
    if (!ctx->b_ev[sl]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->b_ev[sl], hipEventDisableTiming));
    BatchJoinDesc *desc = (BatchJoinDesc *)ctx->b_stage[sl];
    volatile u64 *hcount = (volatile u64 *)ctx->b_land[sl];
    std::vector<CopySeg> segs;
    const u32 tile = join_direct_tile();
    b.max_blocks = 0;
    for (u32 i = 0; i < k; i++) {
        const rhj_join_desc &j = J[idx[i]];
        BatchJoinDesc &d = desc[i];
        d.R = (const unsigned char *)ctx->b_in[sl].p + in_off[i][0];
        d.S = (const unsigned char *)ctx->b_in[sl].p + in_off[i][1];
        d.out = (unsigned char *)ctx->b_out[sl].p + b.out_off[i];
        d.cap = b.dcap[i];
        d.count = (u64 *)((unsigned char *)ctx->b_cnt[sl].p + (size_t)i * 16);
        d.done = (u32 *)((unsigned char *)ctx->b_cnt[sl].p + (size_t)i * 16 + 8);
        d.build_is_S = j.nR >= j.nS + (j.nS >> build_tie_shift()) ? 1u : 0u;      // JobScheduler.cpp:187, near ties: R (build_on_S)
        d.nb = (u32)(d.build_is_S ? j.nS : j.nR);
        d.np = (u32)(d.build_is_S ? j.nR : j.nS);
        d.split = tile;
        d.nblocks = (d.np + tile - 1) / tile;
        d.pad = 0;
        d.host_count = (u64 *)ctx->b_land_dev[sl] + i;
        d.host_out = ctx->b_land_dev[sl] + b.land_off[i];
        d.host_cap = b.lcap[i];
        b.max_blocks = d.nblocks > b.max_blocks ? d.nblocks : b.max_blocks;
        hcount[i] = ~0ull;
        add_pieces(segs, ctx->b_stage[sl] + in_off[i][0], j.R, (size_t)j.nR * 16);
        add_pieces(segs, ctx->b_stage[sl] + in_off[i][1], j.S, (size_t)j.nS * 16);
    }
    ctx->pool->run(segs);
    return RHJ_OK;
}

int batch_launch(rhj_ctx *ctx, int sl, const BatchSlot &b)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->b_in[sl].p, ctx->b_stage[sl], b.in_bytes, hipMemcpyHostToDevice, ctx->stream));
    {
        Span s(ctx, RHJ_K_JOIN);
        launch_join_batch(ctx->stream, (const BatchJoinDesc *)ctx->b_in[sl].p, b.k, b.max_blocks);
    }
    RHJCHK(check_launch(ctx, "batched direct join"));
    HIPCHK(ctx, hipEventRecord(ctx->b_ev[sl], ctx->stream));
    return RHJ_OK;
}

// the group's launch has finished (the caller waited for its event): counts, pages.  retry: joins whose result outgrew the
// device buffer (they take the single-join path afterwards)
int batch_finish(rhj_ctx *ctx, int sl, const BatchSlot &b, void **pages, uint64_t *counts, std::vector<u32> &retry)
{
    volatile u64 *hcount = (volatile u64 *)ctx->b_land[sl];
    std::vector<CopySeg> segs, touch;
    struct Tail { void *dst; const void *src; size_t bytes; };
    std::vector<Tail> tails;                                   // what lies beyond a join's landing zone: fetched from HBM
    for (u32 i = 0; i < b.k; i++) {
        const u64 count = hcount[i];
        if (count == ~0ull) {
            (void)hipMemsetAsync(ctx->b_cnt[sl].p, 0, BATCH_MAX * 16, ctx->stream);
            return fail(ctx, RHJ_E_HIP, "a batched join did not publish its result count");
        }
        pages[b.idx[i]] = nullptr;
        counts[b.idx[i]] = count;
        if (count == 0) continue;                            // head stays nullptr (Result::isEmpty)
        if (count > b.dcap[i]) { retry.push_back(b.idx[i]); continue; }
        unsigned char *page = (unsigned char *)malloc(8 + (size_t)count * 16);
        if (!page) return fail(ctx, RHJ_E_NOMEM, "malloc of a result page failed");
        memset(page, 0, 8);                                  // bucket_info::next = nullptr (Result.h:14-17)
        pages[b.idx[i]] = page;
        const u64 got = count < b.lcap[i] ? count : b.lcap[i];
        add_pieces(segs, page + 8, ctx->b_land[sl] + b.land_off[i], (size_t)got * 16);
        if (count > got) {                                   // beyond the landing zone: straight from HBM into the page
            unsigned char *dst = page + 8 + got * 16;
            const size_t bytes = (size_t)(count - got) * 16;
            tails.push_back(Tail{dst, (const unsigned char *)ctx->b_out[sl].p + b.out_off[i] + got * 16, bytes});
            if (bytes >= ((size_t)1 << 20)) {
                // a DMA into fresh pages takes the page faults itself and runs at a third of the wire rate: fault the range in
                // first, from the helper threads, in huge pages where the kernel grants them
                const uintptr_t lo = ((uintptr_t)dst + ((uintptr_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1);
                const uintptr_t hi = ((uintptr_t)dst + bytes) & ~(((uintptr_t)2 << 20) - 1);
                if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
                for (size_t o = 0; o < bytes; o += BATCH_PIECE)
                    touch.push_back(CopySeg{dst + o, nullptr, bytes - o < BATCH_PIECE ? bytes - o : BATCH_PIECE});
            }
        }
    }
    ctx->pool->run(touch);
    if (!tails.empty()) {
        // on its own stream: the next group's kernel is already running on ctx->stream (this group's has finished: its event)
        if (!ctx->down_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
        for (const Tail &t : tails) HIPCHK(ctx, hipMemcpyAsync(t.dst, t.src, t.bytes, hipMemcpyDeviceToHost, ctx->down_stream));
    }
    ctx->pool->run(segs);                                    // the landing zones -> pages, while the tails travel
    if (!tails.empty()) HIPCHK(ctx, hipStreamSynchronize(ctx->down_stream));
    return RHJ_OK;
}

}  // namespace

int rhj_join_batch(rhj_ctx *ctx, uint32_t n, const rhj_join_desc *joins, void **out_pages, uint64_t *out_counts)
{
    RHJCHK(use_device(ctx));
    if (n && (!joins || !out_pages || !out_counts)) return fail(ctx, RHJ_E_INVALID, "rhj_join_batch: null argument");
    prof_reset(ctx);
    ctx->last_pipelined = 0;
    for (u32 i = 0; i < n; i++) { out_pages[i] = nullptr; out_counts[i] = 0; }
    auto free_all = [&]() { for (u32 i = 0; i < n; i++) { free(out_pages[i]); out_pages[i] = nullptr; out_counts[i] = 0; } };
    std::vector<u32> small, single, retry;
    for (u32 i = 0; i < n; i++) {
        const rhj_join_desc &j = joins[i];
        if (j.nR == 0 || j.nS == 0) continue;
        if (!j.R || !j.S) return fail(ctx, RHJ_E_INVALID, "rhj_join_batch: null input relation");
        rhj_opts plan;
        if (resolve_plan(j.nR, j.nS, nullptr, &plan, false, default_join_kernels(ctx)) != RHJ_OK) return fail(ctx, RHJ_E_INVALID, "bad rhj_opts");
        (plan.passes == 0 && is_direct(ctx, 1, j.nR, j.nS) ? small : single).push_back(i);
    }
    if (!small.empty()) {
        if (!ctx->pool) ctx->pool = new CopyPool((int)env_u64("RHJ_BATCH_THREADS", 3, 0, 15));
        const size_t G = (small.size() + BATCH_MAX - 1) / BATCH_MAX;
        BatchSlot slot[2];
        auto group_k = [&](size_t g) { return (u32)(small.size() - g * BATCH_MAX < BATCH_MAX ? small.size() - g * BATCH_MAX : BATCH_MAX); };
        int rc = batch_stage(ctx, 0, slot[0], joins, &small[0], group_k(0));
        if (rc == RHJ_OK) rc = batch_launch(ctx, 0, slot[0]);
        for (size_t g = 0; g < G && rc == RHJ_OK; g++) {
            const int cur = (int)(g & 1), nxt = cur ^ 1;
            if (g + 1 < G) rc = batch_stage(ctx, nxt, slot[nxt], joins, &small[(g + 1) * BATCH_MAX], group_k(g + 1));   // | GPU(g)
            if (rc == RHJ_OK && hipEventSynchronize(ctx->b_ev[cur]) != hipSuccess) rc = fail(ctx, RHJ_E_HIP, "batched join: event wait failed");
            if (rc == RHJ_OK && g + 1 < G) rc = batch_launch(ctx, nxt, slot[nxt]);
            if (rc == RHJ_OK) rc = batch_finish(ctx, cur, slot[cur], out_pages, out_counts, retry);                        // | GPU(g+1)
        }
        if (rc != RHJ_OK) { (void)hipStreamSynchronize(ctx->stream); free_all(); return rc; }
    }
    ctx->last.passes = 0;
    ctx->last.bits1 = ctx->last.bits2 = 0;
    ctx->last_join_kind = -1;
    ctx->cur_narrow = 0;
    single.insert(single.end(), retry.begin(), retry.end());
    for (u32 i : single) {                                   // too large for the one-launch path (or a result beyond 32x the guess)
        const rhj_join_desc &j = joins[i];
        const int rc = rhj_join(ctx, j.R, j.nR, j.S, j.nS, nullptr, &out_pages[i], &out_counts[i]);
        if (rc != RHJ_OK) { free_all(); return rc; }
    }
    return RHJ_OK;
}

// ---- stage entry points ---------------------------------------------------------------------------
int rhj_partition(rhj_ctx *ctx, const rhj_tuple *d_in, uint64_t n, int bits1, int bits2, rhj_tuple *d_out,
                  uint64_t *d_part_start)
{
    RHJCHK(use_device(ctx));
    if (bits1 < 1 || bits1 > PART_MAX_BITS || bits2 < 0 || bits2 > PART_MAX_BITS || !d_out || !d_part_start || (n && !d_in))
        return fail(ctx, RHJ_E_INVALID, "bad rhj_partition argument");
    prof_reset(ctx);
    return partition_relation(ctx, d_in, n, bits2 ? 2 : 1, bits1, bits2, d_out, (u64 *)d_part_start);
}

static int partition_at(rhj_ctx *ctx, const rhj_tuple *d_in, uint64_t n, int shift, int bits, rhj_tuple *d_out,
                        uint64_t *d_part_start, int mix, const char *who)
{
    RHJCHK(use_device(ctx));
    if (bits < 1 || bits > PART_MAX_BITS || shift < 0 || shift + bits > 64 || !d_out || !d_part_start || (n && !d_in))
        return fail(ctx, RHJ_E_INVALID, std::string("bad argument: ") + who);
    prof_reset(ctx);
    RHJCHK(ensure(ctx, ctx->seg0, 64));
    return run_pass(ctx, d_in, d_out, n, (const u64 *)ctx->seg0.p, 1, shift, bits, (u64 *)d_part_start, true, mix);
}

int rhj_partition_at(rhj_ctx *ctx, const rhj_tuple *d_in, uint64_t n, int shift, int bits, rhj_tuple *d_out,
                     uint64_t *d_part_start)
{
    return partition_at(ctx, d_in, n, shift, bits, d_out, d_part_start, MIX_NONE, "rhj_partition_at");
}

int rhj_owner_split(rhj_ctx *ctx, const rhj_tuple *d_in, uint64_t n, int shift, int bits, rhj_tuple *d_out,
                    uint64_t *d_class_start)
{
    return partition_at(ctx, d_in, n, shift, bits, d_out, d_class_start, MIX_DIGIT, "rhj_owner_split");
}

static int histogram_of(rhj_ctx *ctx, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t *d_hist, int mix,
                        const char *who)
{
    RHJCHK(use_device(ctx));
    if (bits < 1 || bits > PART_MAX_BITS || shift < 0 || shift + bits > 64 || !d_hist || (n && !d_rel))
        return fail(ctx, RHJ_E_INVALID, std::string("bad argument: ") + who);
    prof_reset(ctx);
    const size_t nbins = (size_t)1 << bits;
    RHJCHK(ensure(ctx, ctx->seg0, 64));
    RHJCHK(ensure(ctx, ctx->hist_tmp, (nbins + 1) * 8));
    u64 *seg0 = (u64 *)ctx->seg0.p;
    PassGeom g = make_geom(n, 1, shift, bits);
    g.mix = mix;
    RHJCHK(ensure(ctx, ctx->unit_start, 8));
    RHJCHK(ensure(ctx, ctx->unit_hist, (size_t)g.max_units * nbins * 4));
    RHJCHK(ensure(ctx, ctx->unit_base, (size_t)g.max_units * nbins * 8));
    RHJCHK(ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(bits)));
    {
        Span s(ctx, RHJ_K_AUX);
        launch_init_single_segment(ctx->stream, n, g.L, seg0, (u32 *)ctx->unit_start.p);
    }
    {
        Span s(ctx, RHJ_K_HIST);
        launch_hist_units(ctx->stream, d_rel, g, seg0, (const u32 *)ctx->unit_start.p, (u32 *)ctx->unit_hist.p);
    }
    {
        Span s(ctx, RHJ_K_SCAN);
        launch_scan_units(ctx->stream, g, seg0, (const u32 *)ctx->unit_start.p, (const u32 *)ctx->unit_hist.p,
                          (u64 *)ctx->unit_base.p, (u64 *)ctx->hist_tmp.p, (u64 *)ctx->scan_tmp.p);
        launch_diff_hist(ctx->stream, (const u64 *)ctx->hist_tmp.p, nbins, (u64 *)d_hist);
    }
    return check_launch(ctx, who);
}

int rhj_histogram(rhj_ctx *ctx, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t *d_hist)
{
    return histogram_of(ctx, d_rel, n, shift, bits, d_hist, MIX_NONE, "rhj_histogram");
}

int rhj_owner_histogram(rhj_ctx *ctx, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t *d_hist)
{
    return histogram_of(ctx, d_rel, n, shift, bits, d_hist, MIX_DIGIT, "rhj_owner_histogram");
}

int rhj_prefix(rhj_ctx *ctx, const uint64_t *d_hist, uint64_t nbins, uint64_t *d_start)
{
    RHJCHK(use_device(ctx));
    if (!d_hist || !d_start || nbins == 0) return fail(ctx, RHJ_E_INVALID, "bad rhj_prefix argument");
    prof_reset(ctx);
    {
        Span s(ctx, RHJ_K_SCAN);
        launch_prefix(ctx->stream, (const u64 *)d_hist, nbins, (u64 *)d_start);
    }
    return check_launch(ctx, "rhj_prefix");
}

int rhj_bucket_join(rhj_ctx *ctx, const rhj_tuple *d_Rp, const uint64_t *d_startR, const rhj_tuple *d_Sp,
                    const uint64_t *d_startS, uint64_t nparts, int radix_bits, int probe_split, rhj_pair *d_out,
                    uint64_t out_capacity, uint64_t *out_count)
{
    RHJCHK(use_device(ctx));
    if (!d_startR || !d_startS || !out_count || nparts == 0 || radix_bits < 0 || radix_bits > 40 || probe_split < 0)
        return fail(ctx, RHJ_E_INVALID, "bad rhj_bucket_join argument");
    prof_reset(ctx);
    // sizes are the last boundary of each side
    u64 ends[2] = {0, 0}, begs[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(&ends[0], d_startR + nparts, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&ends[1], d_startS + nparts, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&begs[0], d_startR, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&begs[1], d_startS, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out_count = 0;
    if (ends[0] <= begs[0] || ends[1] <= begs[1]) return RHJ_OK;
    // the one-launch small-join path assumes boundaries {0, n}; the compact-table kernel trusts radix_bits: checked on the device
    RHJCHK(join_phase_on(ctx, d_Rp, (const u64 *)d_startR, ends[0], d_Sp, (const u64 *)d_startS, ends[1], nparts,
                         radix_bits, (u32)probe_split, d_out, out_capacity, (u64 *)out_count, false, nullptr,
                         begs[0] == 0 && begs[1] == 0, true));
    if (d_out && *out_count > out_capacity) return fail(ctx, RHJ_E_OVERFLOW, "result buffer too small");
    return RHJ_OK;
}


// ---- multi-GPU stage entry points ---------------------------------------------------------------------
// Sender: class histogram (+ rowID range) of a shard, then the class split into the narrow wire format; receiver: the fused
// two-pass partition of what arrived (sender segments -> sender tags) and the bucket join that resolves the tags.
namespace {

struct ShardTables { DevBuf *seg0, *unit_start, *unit_hist, *unit_base, *scan_tmp; };

ShardTables shard_tables(rhj_ctx *ctx, int side)
{
    if (side == 0) return {&ctx->seg0, &ctx->unit_start, &ctx->unit_hist, &ctx->unit_base, &ctx->scan_tmp};
    return {&ctx->seg0_b, &ctx->unit_start_b, &ctx->unit_hist_b, &ctx->unit_base_b, &ctx->scan_tmp_b};
}

}  // namespace

// Test aid, not part of rhj.h: the partitions of side (0 R, 1 S) as the last two-pass narrow rhj_join_dev left them -- payloads
// (n u64), rowIDs (n u32) and the 2^(bits1 + bits2) + 1 boundaries -- copied to host arrays of the caller.
extern "C" int rhj_debug_read_partitions(rhj_ctx *ctx, int side, uint64_t *payloads, uint32_t *rowids, uint64_t *bounds)
{
    RHJCHK(use_device(ctx));
    if (side < 0 || side > 1 || !payloads || !rowids || !bounds || ctx->cur_narrow == 0 || ctx->cur_nparts < 2)
        return fail(ctx, RHJ_E_INVALID, "rhj_debug_read_partitions: no narrow partitions to read");
    const u64 n = side ? ctx->cur_nS : ctx->cur_nR;
    const unsigned char *part = (const unsigned char *)(side ? ctx->cur_S : ctx->cur_R);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->cur_end[side] != nullptr) {                // regions with gaps: compacted here, exact prefix boundaries
        const u64 np = ctx->cur_nparts, slots = ctx->cur_slots[side], cap2 = slots / np;
        std::vector<u64> hp((size_t)slots), he((size_t)np);
        std::vector<u32> hk((size_t)slots);
        HIPCHK(ctx, hipMemcpy(hp.data(), part, (size_t)slots * 8, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(hk.data(), part + narrow_k_offset(slots), (size_t)slots * 4, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(he.data(), ctx->cur_end[side], (size_t)np * 8, hipMemcpyDeviceToHost));
        u64 at = 0;
        for (u64 k = 0; k < np; k++) {
            const u64 s = k * cap2, len = he[k] > s ? he[k] - s : 0;
            if (len > cap2 || at + len > n) return fail(ctx, RHJ_E_HIP, "rhj_debug_read_partitions: a partition's end lies outside its region");
            bounds[k] = at;
            for (u64 i = 0; i < len; i++) { payloads[at + i] = hp[s + i]; rowids[at + i] = hk[s + i]; }
            at += len;
        }
        bounds[np] = at;
        return RHJ_OK;
    }
    HIPCHK(ctx, hipMemcpy(payloads, part, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(rowids, part + narrow_k_offset(n), (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(bounds, side ? ctx->cur_psS : ctx->cur_psR, (size_t)(ctx->cur_nparts + 1) * 8, hipMemcpyDeviceToHost));
    return RHJ_OK;
}

uint64_t rhj_narrow_key_offset(uint64_t n) { return narrow_k_offset(n); }
uint64_t rhj_narrow_bytes(uint64_t n) { return (narrow_k_offset(n) + n * 4 + 255) & ~(uint64_t)255; }

int rhj_shard_plan(uint64_t nR, uint64_t nS, const rhj_opts *in, rhj_opts *resolved)
{
    if (!resolved) return RHJ_E_INVALID;
    rhj_opts o;
    if (resolve_plan(nR, nS, in, &o, true, false) != RHJ_OK) return RHJ_E_INVALID;     // (the receiver's join: sender tags or 16-byte partitions)
    *resolved = o;
    if (o.passes != 2 || nR < NARROW_MIN_TUPLES || nS < NARROW_MIN_TUPLES || nR >= ((u64)1 << 32) || nS >= ((u64)1 << 32)) return 0;
    if (!narrow_fused_plan(o))                          // 17-18 bits: no sender-aligned pass-2 units, so only rowIDs that need no restoring
        return o.bits1 + o.bits2 > 16 && narrow_pass9_ok(o.bits1) && narrow_pass9_ok(o.bits2) ? RHJ_SHARD_PLAIN : 0;
    if (o.bits1 < tag_bits()) return 0;
    rhj_ctx probe;                                      // default options: which kernel would join partitions of this size
    const int tb = o.bits1 + o.bits2;
    const int kind = choose_join_kind(&probe, nR, nS, (u64)1 << tb, tb, false, false);
    if (kind == JK_BKT) return RHJ_SHARD_TAGGED;
    if (jk_is_ct(kind) && !jk_ct_narrow_only(kind)) return RHJ_SHARD_GLOBAL16;
    return 0;
}

int rhj_shard_stats(rhj_ctx *ctx, int side, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t *hist,
                    uint64_t *key_min, uint64_t *key_max)
{
    RHJCHK(use_device(ctx));
    if ((side != 0 && side != 1) || bits < 1 || bits > 8 || shift < 0 || shift + bits > 64 || !hist || (n && !d_rel))
        return fail(ctx, RHJ_E_INVALID, "bad rhj_shard_stats argument");
    prof_reset(ctx);
    const size_t nbins = (size_t)1 << bits;
    const ShardTables t = shard_tables(ctx, side);
    PassGeom g = make_geom(n, 1, shift, bits);
    g.mix = MIX_STORE;                                   // classes are bits of mix64(payload): see rhj.h
    RHJCHK(ensure(ctx, *t.seg0, 64));
    RHJCHK(ensure(ctx, *t.unit_start, 16));
    RHJCHK(ensure(ctx, *t.unit_hist, (size_t)g.max_units * nbins * 4));
    RHJCHK(ensure(ctx, *t.unit_base, (size_t)g.max_units * nbins * 8));
    RHJCHK(ensure(ctx, *t.scan_tmp, scan_tmp_bytes(bits)));
    RHJCHK(ensure(ctx, ctx->shard_ps[side], (nbins + 1) * 8));
    RHJCHK(ensure(ctx, ctx->shard_mm, 64));
    RHJCHK(ensure(ctx, ctx->shard_wide, 64));
    HIPCHK(ctx, hipMemsetAsync((u32 *)ctx->shard_wide.p + side, 0, 4, ctx->stream));
    u64 *mm = (u64 *)ctx->shard_mm.p + 2 * side;
    const u64 init[2] = {~0ull, 0ull};
    {
        Span s(ctx, RHJ_K_AUX);
        HIPCHK(ctx, hipMemcpyAsync(mm, init, 16, hipMemcpyHostToDevice, ctx->stream));
        launch_init_single_segment(ctx->stream, n, g.L, (u64 *)t.seg0->p, (u32 *)t.unit_start->p);
    }
    {
        Span s(ctx, RHJ_K_HIST);
        launch_hist_units(ctx->stream, d_rel, g, (const u64 *)t.seg0->p, (const u32 *)t.unit_start->p, (u32 *)t.unit_hist->p, mm);
    }
    {
        Span s(ctx, RHJ_K_SCAN);
        launch_scan_units(ctx->stream, g, (const u64 *)t.seg0->p, (const u32 *)t.unit_start->p, (const u32 *)t.unit_hist->p,
                          (u64 *)t.unit_base->p, (u64 *)ctx->shard_ps[side].p, (u64 *)t.scan_tmp->p);
    }
    RHJCHK(check_launch(ctx, "rhj_shard_stats"));
    std::vector<u64> ps(nbins + 1);
    u64 hmm[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(ps.data(), ctx->shard_ps[side].p, (nbins + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hmm, mm, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t b = 0; b < nbins; b++) hist[b] = n ? ps[b + 1] - ps[b] : 0;
    ctx->shard_ps_host[side] = ps;
    if (key_min) *key_min = n ? hmm[0] : 0;
    if (key_max) *key_max = n ? hmm[1] : 0;
    ctx->shard_n[side] = n;
    ctx->shard_kmin[side] = n ? hmm[0] : 0;
    ctx->shard_kmax[side] = n ? hmm[1] : 0;
    return RHJ_OK;
}

int rhj_shard_split(rhj_ctx *ctx, int side, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t key_base,
                    void *d_narrow_out, uint64_t *d_class_start)
{
    RHJCHK(use_device(ctx));
    if ((side != 0 && side != 1) || bits < 1 || bits > 8 || shift < 0 || shift + bits > 64 || !d_narrow_out || (n && !d_rel))
        return fail(ctx, RHJ_E_INVALID, "bad rhj_shard_split argument");
    if (ctx->shard_n[side] != n || !ctx->shard_ps[side].p)
        return fail(ctx, RHJ_E_INVALID, "rhj_shard_split: call rhj_shard_stats for this side and relation first");
    if (n && (key_base > ctx->shard_kmin[side] || ctx->shard_kmax[side] - key_base >= ((u64)1 << 32)))
        return fail(ctx, RHJ_E_INVALID, "rhj_shard_split: rowID - key_base must lie in [0, 2^32) for every tuple of the shard "
                                        "(rhj_shard_stats reports the range)");
    prof_reset(ctx);
    const size_t nbins = (size_t)1 << bits;
    const ShardTables t = shard_tables(ctx, side);
    PassGeom g = make_geom(n, 1, shift, bits);
    g.mix = MIX_STORE;                                   // the wire carries mix64(payload); the receiver never mixes again
    {
        // the range check above holds for the relation rhj_shard_stats saw; a DIFFERENT relation handed in here may still hold a
        // rowID whose offset from key_base does not fit 32 bits: the kernel raises this side's word of shard_wide (cleared by
        // rhj_shard_stats) and rhj_shard_join of this context reports it
        Span s(ctx, RHJ_K_SCATTER);
        launch_scatter_units_narrow(ctx->stream, d_rel, d_narrow_out, n, g, (const u64 *)t.seg0->p, (const u32 *)t.unit_start->p,
                                    (const u64 *)t.unit_base->p, (u32 *)ctx->shard_wide.p + side, key_base);
    }
    if (d_class_start)
        HIPCHK(ctx, hipMemcpyAsync(d_class_start, ctx->shard_ps[side].p, (nbins + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return check_launch(ctx, "rhj_shard_split");
}

// The class split of rhj_shard_split written STRAIGHT INTO THE OWNERS' RECEIVE ARRAYS (peer-mapped HBM over xGMI; on one GPU:
// any device buffers), instead of into a local send buffer that an all-to-all then copies.
int rhj_shard_split_peer(rhj_ctx *ctx, int side, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t key_base,
                         const uint8_t *owner, const uint64_t *dst_class_start, void *const *peer_payloads, void *const *peer_rowids,
                         int nranks)
{
    RHJCHK(use_device(ctx));
    if ((side != 0 && side != 1) || bits < 1 || bits > 8 || shift < 0 || shift + bits > 64 || (n && !d_rel) || !owner || !dst_class_start ||
        !peer_payloads || !peer_rowids || nranks < 1 || nranks > seg_max())
        return fail(ctx, RHJ_E_INVALID, "bad rhj_shard_split_peer argument");
    const size_t nbins = (size_t)1 << bits;
    if (ctx->shard_n[side] != n || ctx->shard_ps_host[side].size() != nbins + 1)
        return fail(ctx, RHJ_E_INVALID, "rhj_shard_split_peer: call rhj_shard_stats for this side and relation first");
    if (n && (key_base > ctx->shard_kmin[side] || ctx->shard_kmax[side] - key_base >= ((u64)1 << 32)))
        return fail(ctx, RHJ_E_INVALID, "rhj_shard_split_peer: rowID - key_base must lie in [0, 2^32) for every tuple of the shard");
    for (size_t c = 0; c < nbins; c++)
        if (owner[c] >= nranks || !peer_payloads[owner[c]] || !peer_rowids[owner[c]])
            return fail(ctx, RHJ_E_INVALID, "rhj_shard_split_peer: a class is owned by a rank without receive arrays");
    prof_reset(ctx);
    const ShardTables t = shard_tables(ctx, side);
    PassGeom g = make_geom(n, 1, shift, bits);
    g.mix = MIX_STORE;
    // delta[c] = (index of this rank's class c in its owner's arrays) - (index it would have in a local send buffer)
    const size_t tab_bytes = nbins * 8 + nbins;
    RHJCHK(ensure(ctx, ctx->shard_peer_tab, 2 * ((tab_bytes + 255) & ~(size_t)255)));
    unsigned char *d_tab = (unsigned char *)ctx->shard_peer_tab.p + (size_t)side * ((tab_bytes + 255) & ~(size_t)255);
    std::vector<unsigned char> tab(tab_bytes);
    for (size_t c = 0; c < nbins; c++) {
        const u64 d = dst_class_start[c] - ctx->shard_ps_host[side][c];          // (mod 2^64: added to the cursors, wraps back)
        memcpy(&tab[c * 8], &d, 8);
        tab[nbins * 8 + c] = owner[c];
    }
    // (a synchronous copy: the table is a stack object of this call)
    HIPCHK(ctx, hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    {
        Span s(ctx, RHJ_K_SCATTER);
        launch_scatter_units_narrow_peer(ctx->stream, d_rel, g, (const u64 *)t.seg0->p, (const u32 *)t.unit_start->p,
                                         (const u64 *)t.unit_base->p, (u32 *)ctx->shard_wide.p + side, key_base, (const u64 *)d_tab,
                                         d_tab + nbins * 8, peer_payloads, peer_rowids, nranks);
    }
    return check_launch(ctx, "rhj_shard_split_peer");
}

// Peer mapping of HBM between the processes of one node (one process per GPU): the owner of a receive array exports a handle,
// the senders open it and pass the resulting pointer to rhj_shard_split_peer.  Thin wrappers over hipIpc*; UNVERIFIED on this
// pool (one GPU per box: there is no second process with a GPU to open a handle in).
int rhj_ipc_export(rhj_ctx *ctx, void *d_ptr, void *handle64)
{
    RHJCHK(use_device(ctx));
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "handle size");
    if (!d_ptr || !handle64) return fail(ctx, RHJ_E_INVALID, "bad rhj_ipc_export argument");
    HIPCHK(ctx, hipIpcGetMemHandle((hipIpcMemHandle_t *)handle64, d_ptr));
    return RHJ_OK;
}

int rhj_ipc_open(rhj_ctx *ctx, const void *handle64, void **d_ptr)
{
    RHJCHK(use_device(ctx));
    if (!d_ptr || !handle64) return fail(ctx, RHJ_E_INVALID, "bad rhj_ipc_open argument");
    hipIpcMemHandle_t h;
    memcpy(&h, handle64, sizeof h);
    HIPCHK(ctx, hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return RHJ_OK;
}

int rhj_ipc_close(rhj_ctx *ctx, void *d_ptr)
{
    RHJCHK(use_device(ctx));
    if (!d_ptr) return RHJ_OK;
    HIPCHK(ctx, hipIpcCloseMemHandle(d_ptr));
    return RHJ_OK;
}

int rhj_shard_partition(rhj_ctx *ctx, int side, const uint64_t *d_payloads, const uint32_t *d_rowids, uint64_t m, int nseg,
                        const uint64_t *seg_off, const uint64_t *row0, const rhj_opts *plan, int mode)
{
    RHJCHK(use_device(ctx));
    if ((side != 0 && side != 1) || !plan || plan->passes != 2 || !seg_off || !row0 || nseg < 1 || nseg > seg_max() ||
        seg_off[0] != 0 || seg_off[nseg] != m || (m && (!d_payloads || !d_rowids)) ||
        (mode != RHJ_SHARD_TAGGED && mode != RHJ_SHARD_GLOBAL16 && mode != RHJ_SHARD_PLAIN))
        return fail(ctx, RHJ_E_INVALID, "bad rhj_shard_partition argument");
    if (mode == RHJ_SHARD_PLAIN)
        for (int i = 0; i < nseg; i++)
            if (row0[i] != 0) return fail(ctx, RHJ_E_INVALID, "RHJ_SHARD_PLAIN: every rank must have split with key_base 0");
    const bool fused = narrow_fused_plan(*plan) && plan->bits1 >= tag_bits();
    const bool deep = !narrow_fused_plan(*plan) && plan->bits1 + plan->bits2 > 16 && narrow_pass9_ok(plan->bits1) && narrow_pass9_ok(plan->bits2);
    if (!(fused || (deep && mode == RHJ_SHARD_PLAIN)) || m >= ((u64)1 << 32))
        return fail(ctx, RHJ_E_INVALID, "rhj_shard_partition: not a plan of the narrow format for this mode (see rhj_shard_plan)");
    for (int i = 0; i < nseg; i++)
        if (seg_off[i] > seg_off[i + 1]) return fail(ctx, RHJ_E_INVALID, "rhj_shard_partition: segment offsets must not decrease");
    prof_reset(ctx);
    const int tb = plan->bits1 + plan->bits2;
    const size_t np = (size_t)1 << tb;
    DevBuf &part = side == 0 ? ctx->part_R : ctx->part_S;
    DevBuf &ps = side == 0 ? ctx->ps_R : ctx->ps_S;
    RHJCHK(ensure(ctx, part, (size_t)(m ? m : 1) * 16));
    RHJCHK(ensure(ctx, ps, (np + 1) * 8));
    RHJCHK(ensure(ctx, ctx->narrow_flag, 64));
    {
        Span s(ctx, RHJ_K_AUX);
        HIPCHK(ctx, hipMemsetAsync(ctx->narrow_flag.p, 0, 64, ctx->stream));
    }
    ctx->counters_clean = false;
    u64 bases[16] = {0};
    for (int i = 0; i < nseg; i++) bases[i] = row0[i];
    RHJCHK(ensure(ctx, ctx->tag_base, 2 * sizeof(bases)));
    u64 *d_bases = (u64 *)ctx->tag_base.p + 16 * side;
    HIPCHK(ctx, hipMemcpyAsync(d_bases, bases, sizeof(bases), hipMemcpyHostToDevice, ctx->stream));   // (pageable source: staged before the call returns)
    ctx->shard_sniffed[side] = false;
    if (m == 0) {                                       // nothing arrived: all boundaries 0
        HIPCHK(ctx, hipMemsetAsync(ps.p, 0, (np + 1) * 8, ctx->stream));
    } else {
        FusedIn in;
        in.P = (const u64 *)d_payloads;
        in.K = (const u32 *)d_rowids;
        in.nseg = nseg;
        in.seg_off = (const u64 *)seg_off;
        in.final_form = mode == RHJ_SHARD_TAGGED ? 1 : mode == RHJ_SHARD_GLOBAL16 ? 2 : 0;
        in.key_bases = d_bases;
        if (fused) {
            const bool sniff = sniff_on(ctx);                                   // (the received join values are sampled for duplicates too)
            if (sniff) RHJCHK(ensure(ctx, ctx->sniff_tab, (size_t)2 * SNIFF_SLOTS * 4));
            ctx->sniff_side = sniff ? side : -1;
            const int prc = partition_relation_fused(ctx, in, m, plan->bits1, plan->bits2, part.p, (u64 *)ps.p, 2);
            ctx->sniff_side = -1;
            RHJCHK(prc);
            ctx->shard_sniffed[side] = sniff;
        }
        else RHJCHK(partition_relation_narrow2(ctx, d_payloads, m, plan->bits1, plan->bits2, part.p, (u64 *)ps.p, (const u32 *)d_rowids));
    }
    ctx->shard_side_done[side] = true;
    ctx->shard_n[side] = m;
    ctx->shard_nseg = nseg;
    ctx->shard_mode[side] = mode;
    ctx->shard_plan = *plan;
    return RHJ_OK;
}

int rhj_shard_join(rhj_ctx *ctx, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count)
{
    RHJCHK(use_device(ctx));
    if (!out_count) return fail(ctx, RHJ_E_INVALID, "bad rhj_shard_join argument");
    if (!ctx->shard_side_done[0] || !ctx->shard_side_done[1] || ctx->shard_mode[0] != ctx->shard_mode[1])
        return fail(ctx, RHJ_E_INVALID, "rhj_shard_join: rhj_shard_partition both sides (0 and 1) in the same mode first");
    *out_count = 0;
    prof_reset(ctx);
    const u64 mR = ctx->shard_n[0], mS = ctx->shard_n[1];
    if (mR == 0 || mS == 0) {                              // an empty input: no kernel runs ("last.join_kernel" -1, rhj.h)
        ctx->last_join_kind = -1;
        return RHJ_OK;
    }
    const int mode = ctx->shard_mode[0];
    const int tb = ctx->shard_plan.bits1 + ctx->shard_plan.bits2;
    const bool narrow = mode != RHJ_SHARD_GLOBAL16;
    if (mode == RHJ_SHARD_TAGGED && choose_join_kind(ctx, mR, mS, (u64)1 << tb, tb, false, false) != JK_BKT)
        return fail(ctx, RHJ_E_INVALID, "rhj_shard_join: partitions this large need RHJ_SHARD_GLOBAL16 (see rhj_shard_plan)");
    ctx->cur_narrow = narrow ? 2 : 0;
    ctx->sniff_ready = ctx->shard_sniffed[0] && ctx->shard_sniffed[1];
    ctx->last.passes = 2;
    ctx->last.bits1 = ctx->shard_plan.bits1;
    ctx->last.bits2 = ctx->shard_plan.bits2;
    int rc = join_phase_on(ctx, ctx->part_R.p, (const u64 *)ctx->ps_R.p, mR, ctx->part_S.p, (const u64 *)ctx->ps_S.p, mS,
                           (u64)1 << tb, tb, (u32)ctx->shard_plan.probe_split, d_out, d_out ? out_capacity : 0, (u64 *)out_count, narrow,
                           mode == RHJ_SHARD_TAGGED ? (const u64 *)ctx->tag_base.p : nullptr, false, false, false, false, false);
    if (rc == RHJ_RETRY_WIDE) return fail(ctx, RHJ_E_HIP, "rhj_shard_join: unexpected wide-rowID flag");
    RHJCHK(rc);
    if (ctx->shard_wide.p) {                               // what this context's own rhj_shard_split calls met (the stream is idle here)
        u32 w[2] = {0, 0};
        HIPCHK(ctx, hipMemcpy(w, ctx->shard_wide.p, 8, hipMemcpyDeviceToHost));
        if (w[0] | w[1])
            return fail(ctx, RHJ_E_INVALID, "rhj_shard_split: a rowID - key_base did not fit 32 bits -- the relation differs from the "
                                            "one given to rhj_shard_stats for that side; what was sent is incomplete");
    }
    if (d_out && *out_count > out_capacity) return fail(ctx, RHJ_E_OVERFLOW, "result buffer too small");
    return RHJ_OK;
}

// ---- utilities --------------------------------------------------------------------------------------
static int reduce_to_host(rhj_ctx *ctx, uint64_t *host_out, void (*launch)(hipStream_t, const void *, u64, u64 *),
                          const void *d_in, u64 n)
{
    RHJCHK(ensure(ctx, ctx->counters, 64));
    ctx->counters_clean = false;
    u64 *d_sum = (u64 *)ctx->counters.p + 4;
    HIPCHK(ctx, hipMemsetAsync(d_sum, 0, 8, ctx->stream));
    if (n) {
        Span s(ctx, RHJ_K_AUX);
        launch(ctx->stream, d_in, n, d_sum);
    }
    RHJCHK(check_launch(ctx, "reduction"));
    HIPCHK(ctx, hipMemcpyAsync(host_out, d_sum, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return RHJ_OK;
}

int rhj_pairs_checksum_dev(rhj_ctx *ctx, const rhj_pair *d_pairs, uint64_t n, uint64_t *checksum)
{
    RHJCHK(use_device(ctx));
    if (!checksum || (n && !d_pairs)) return fail(ctx, RHJ_E_INVALID, "bad rhj_pairs_checksum_dev argument");
    return reduce_to_host(ctx, checksum, launch_checksum, d_pairs, n);
}

int rhj_expected_pkfk_dev(rhj_ctx *ctx, const rhj_tuple *d_S, uint64_t n, uint64_t *count, uint64_t *checksum)
{
    RHJCHK(use_device(ctx));
    if (!checksum || !count || (n && !d_S)) return fail(ctx, RHJ_E_INVALID, "bad rhj_expected_pkfk_dev argument");
    *count = n;
    return reduce_to_host(ctx, checksum, launch_expected_pkfk, d_S, n);
}

int rhj_generate_dev(rhj_ctx *ctx, int kind, rhj_tuple *d_out, uint64_t n, uint64_t row0, uint64_t D, uint64_t seed,
                     int theta_milli)
{
    RHJCHK(use_device(ctx));
    if (kind < 0 || kind > 4 || (n && !d_out) || (kind != 4 && D == 0) || (kind == 2 && theta_milli == 1000))
        return fail(ctx, RHJ_E_INVALID, "bad rhj_generate_dev argument");
    if (n) {
        Span s(ctx, RHJ_K_AUX);
        launch_generate(ctx->stream, kind, d_out, n, row0, D, seed, theta_milli / 1000.0);
    }
    return check_launch(ctx, "rhj_generate_dev");
}

int rhj_remap_keys_dev(rhj_ctx *ctx, rhj_tuple *d_rel, uint64_t n, int shift, uint64_t add)
{
    RHJCHK(use_device(ctx));
    if (shift < 0 || shift > 63 || (n && !d_rel)) return fail(ctx, RHJ_E_INVALID, "bad rhj_remap_keys_dev argument");
    if (n) {
        Span s(ctx, RHJ_K_AUX);
        launch_remap_keys(ctx->stream, d_rel, n, shift, add);
    }
    return check_launch(ctx, "rhj_remap_keys_dev");
}

// block sizes are rounded up (64 KiB steps, 1/8 steps above 8 MiB) so that released blocks fit later requests
static size_t pool_round(uint64_t bytes)
{
    size_t b = bytes ? (size_t)bytes : 16;
    size_t step = (size_t)64 << 10;
    while (step * 8 < b) step <<= 1;
    return (b + step - 1) / step * step;
}
constexpr size_t POOL_KEEP_BYTES = (size_t)8 << 30;       // released blocks kept per context at most

int rhj_dev_alloc(rhj_ctx *ctx, uint64_t bytes, void **d_ptr)
{
    RHJCHK(use_device(ctx));
    if (!d_ptr) return fail(ctx, RHJ_E_INVALID, "d_ptr is null");
    *d_ptr = nullptr;
    const size_t want = pool_round(bytes);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < ctx->free_blocks.size(); i++)
        if (ctx->free_blocks[i].second == want) { best = i; break; }
    if (best != (size_t)-1) {
        *d_ptr = ctx->free_blocks[best].first;
        ctx->free_bytes -= want;
        ctx->free_blocks[best] = ctx->free_blocks.back();
        ctx->free_blocks.pop_back();
        return RHJ_OK;
    }
    hipError_t e = hipMalloc(d_ptr, want);
    if (e != hipSuccess && !ctx->free_blocks.empty()) {           // make room and try once more
        (void)hipGetLastError();
        for (auto &b : ctx->free_blocks) {
            { std::lock_guard<std::mutex> lk(g_pool_sizes_mu); g_pool_sizes.erase(b.first); }
            (void)hipFree(b.first);
        }
        ctx->free_blocks.clear();
        ctx->free_bytes = 0;
        e = hipMalloc(d_ptr, want);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *d_ptr = nullptr;
        return fail(ctx, RHJ_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lk(g_pool_sizes_mu);
    g_pool_sizes[*d_ptr] = want;
    return RHJ_OK;
}

int rhj_dev_free(rhj_ctx *ctx, void *d_ptr)
{
    RHJCHK(use_device(ctx));
    if (!d_ptr) return RHJ_OK;
    size_t sz = 0;
    {
        std::lock_guard<std::mutex> lk(g_pool_sizes_mu);
        auto it = g_pool_sizes.find(d_ptr);
        if (it != g_pool_sizes.end()) sz = it->second;
    }
    if (sz && ctx->free_bytes + sz <= POOL_KEEP_BYTES && ctx->free_blocks.size() < 256) {
        ctx->free_blocks.emplace_back(d_ptr, sz);                 // kept for re-use; returned to the device by
        ctx->free_bytes += sz;                                    // rhj_release_workspace / rhj_destroy
        return RHJ_OK;
    }
    { std::lock_guard<std::mutex> lk(g_pool_sizes_mu); g_pool_sizes.erase(d_ptr); }
    HIPCHK(ctx, hipFree(d_ptr));
    return RHJ_OK;
}

int rhj_copy_h2d(rhj_ctx *ctx, void *d_dst, const void *src, uint64_t bytes)
{
    RHJCHK(use_device(ctx));
    if (bytes) {
        HIPCHK(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RHJ_OK;
}

int rhj_copy_d2h(rhj_ctx *ctx, void *dst, const void *d_src, uint64_t bytes)
{
    RHJCHK(use_device(ctx));
    if (bytes) {
        HIPCHK(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RHJ_OK;
}

int rhj_dev_mem_info(rhj_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes)
{
    RHJCHK(use_device(ctx));
    size_t f = 0, t = 0;
    HIPCHK(ctx, hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return RHJ_OK;
}

}  // extern "C"
