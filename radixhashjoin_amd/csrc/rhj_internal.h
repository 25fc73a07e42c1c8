// rhj_internal.h -- shared between rhj_kernels.hip (device code + launchers) and rhj_api.hip (C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- partition pass geometry ------------------------------------------------------------------
// A pass partitions every SEGMENT of the input (pass 1: the whole relation; pass 2: each pass-1
// bucket) by `bits` radix bits.  A segment is cut into UNITS of at most L tuples; one workgroup
// owns one unit in the histogram kernel and again in the scatter kernel (the reference's row
// ranges, structs.cpp:146-161, with ranges = units instead of 8 threads).
constexpr int PART_THREADS = 512;                 // 8 wavefronts
constexpr int PART_TPT = 8;                       // tuples per thread per tile
constexpr int PART_TILE = PART_THREADS * PART_TPT;  // 4096 tuples = 64 KiB LDS staging
constexpr int PART_MAX_BITS = 10;                 // k_scan_units: nbins <= 1024 threads
constexpr u32 PART_TARGET_UNITS = 2048;           // ~8 units per CU

// ---- bucket join geometry: bucketized LDS table, 512 threads, two workgroups per CU ------------
constexpr int BJ_THREADS = 512;
constexpr int BJ_CHUNK = 4224;                    // build tuples per LDS table: 66 KiB keys+rowids
constexpr int BJ_BUCKET_BITS = 11;                // 2048 hash buckets (offsets: 8 KiB)
constexpr int BJ_EPT = 8;                         // probe tuples per thread per tile
constexpr int BJ_TILE = BJ_THREADS * BJ_EPT;      // 4096
constexpr int BJ_FIT = BJ_CHUNK * 15 / 16;        // plan: average build partition <= 3960 tuples
constexpr u32 BJ_MAX_PROBE_SPLIT = 1u << 24;      // probe tuples per join task at most (a caller's larger probe_split is clamped: same pairs, more tasks)
// under a plan of >= 16 bits, average build partitions of CT_GUARDED_FROM ... CT_GUARDED_UPTO tuples go to the compact-table
// kernel's JK_CT_HALF_MID_G geometry (row guards, k_join_ct<.., GUARD>): 4 ... 10 of its 12 slot rows in use
constexpr int CT_GUARDED_FROM = 2048, CT_GUARDED_UPTO = 5120;
// small joins run unpartitioned in one launch (k_join_bkt DIRECT): every 4096-tuple probe tile re-builds the table chunks
constexpr u64 DIRECT_MAX_BUILD = 12ull * BJ_CHUNK; // build side of at most 12 table chunks ...
constexpr u64 DIRECT_MAX_PROBE = 131072;          // ... probed by at most 32 workgroups
// ... with inputs already in HBM (rhj_join_dev) at most 5: a workgroup walks the chunks one after the other (20 us + 15 us
// per chunk), and one 4-6-bit pass + join is ~105 us whatever the size ([measured] 50K x 50K: 0.21 ms direct, 0.11 partitioned)
constexpr u64 DIRECT_MAX_BUILD_DEV = 5ull * BJ_CHUNK;

struct JoinTask {           // one workgroup's work: probe range [pbeg, pbeg+plen) against build range [bbeg, bbeg+blen)
    u64 pbeg;               // absolute index into the probe-side array
    u32 plen;
    u32 part;               // partition id
    u64 bbeg;               // absolute index into the build-side array
    u32 blen;
    u32 build_is_S;         // 1: build on S, probe with R (|R_k| >= |S_k|, JobScheduler.cpp:187)
};

struct PassGeom {
    u64 n;          // tuples in the relation
    u64 L;          // max tuples per unit
    u32 nseg;       // segments in this pass
    u32 max_units;  // grid size upper bound: floor(n / L) + nseg
    int shift;      // digit = (payload >> shift) & (nbins-1)
    int bits;
    int mix = 0;    // MIX_*: where the digit comes from when the input is the caller's 16-byte relation
};
// Inside a join the radix digits (and, multi-GPU, the owner classes) come from mix64(payload), a BIJECTIVE 64-bit mix
// (splitmix64's finaliser), not from the raw low payload bits: join values that are multiples of 2^16, or that differ in
// their high bits only, would otherwise all land in one partition (the reference does not degrade there: its bucket table
// hashes the whole value modulo a prime, Result.cpp:43-58).  The FIRST kernels that touch the caller's tuples apply it
// (MIX_STORE: histogram digit of the mixed value; the scatter writes the mixed value), every later kernel -- pass 2, the
// bucket joins -- works on the mixed value as if it were the payload: a bijection keeps equality, so the pair set does
// not change, and only rowIDs are reported.  The public stage calls (rhj_histogram / rhj_partition / rhj_partition_at /
// rhj_bucket_join) keep raw bits: their bucket order is documented.  MIX_DIGIT: digit of the mixed value, tuple written
// as it came (rhj_shard_split16: the multi-GPU owner split of 16-byte tuples, joined by rhj_join_dev on the receiver).
constexpr int MIX_NONE = 0, MIX_STORE = 1, MIX_DIGIT = 2;
// multi-GPU: a receiver tells SEG_MAX segments (= senders = ranks) apart; the sender number travels in the low TAG_BITS payload bits
constexpr int SEG_MAX = 16;
constexpr u32 TAG_BITS = 4, TAG_MAX = 1u << TAG_BITS;   // sender tags in the low payload bits: <= 16 ranks (== SEG_MAX)
constexpr int seg_max() { return SEG_MAX; }
constexpr int tag_bits() { return (int)TAG_BITS; }

// a relation given as COLUMNS (rhj_join_cols_dev): val[i] = join value of tuple i, id[i] = its rowID, id == nullptr: rowID = i
struct ColsIn { const u64 *val = nullptr, *id = nullptr; };

// launchers (all asynchronous on `st`)
void launch_init_single_segment(hipStream_t st, u64 n, u64 L, u64 *d_seg_start, u32 *d_unit_start);
// DupSniff: which side of a join has duplicate join values -- asked of the data, by the histogram kernels that read every tuple
// anyway.  A tuple whose mix64(payload) has sel_bits leading zero bits is SAMPLED (a fixed subset of the VALUES, so every
// duplicate of a sampled value is sampled too; sel_bits such that 256-512 tuples of the relation are) and counted in one of
// SNIFF_SLOTS counters of its side by a hash of the value: fire-and-forget atomics, nothing waits for them.  The task planners
// (k_make_tasks, the planner workgroup of k_scatter_fused2) sum max(0, counter - 1) per side -- duplicates, plus the few
// chance meetings of two values in a slot, the same for both sides -- compare the two RATES, and let the side with fewer
// duplicates be the hash table when the sizes are near (build_on_S in rhj_kernels.hip).  The counters are zero when a join
// starts (the caller clears them, or the previous join's histogram launch did).  tab == nullptr: no sampling / the first relation.
constexpr u32 SNIFF_SLOTS = 16384, SNIFF_TARGET = 512;
struct DupSniff { u32 *tab = nullptr; int sel_bits = 0; };
struct SniffVerdict { const u32 *tab = nullptr; u32 expect_R = 0, expect_S = 0; };   // tab: [2 sides][SNIFF_SLOTS]; expected samples
inline int sniff_sel_bits(u64 n) { int s = 0; while ((n >> s) > SNIFF_TARGET) s++; return s; }
int build_tie_shift();                             // sizes within 1/2^this of each other are a tie (RHJ_BUILD_TIE, default 4: 1/16)
void launch_make_units(hipStream_t st, const u64 *d_seg_start, u32 nseg, u64 L, u32 *d_unit_start);
// d_minmax (may be null): two u64, atomicMin / atomicMax of the rowIDs seen
void launch_hist_units(hipStream_t st, const void *d_in, const PassGeom &g, const u64 *d_seg_start,
                       const u32 *d_unit_start, u32 *d_unit_hist, u64 *d_minmax = nullptr, const DupSniff &sniff = DupSniff());
void launch_scan_units(hipStream_t st, const PassGeom &g, const u64 *d_seg_start, const u32 *d_unit_start,
                       const u32 *d_unit_hist, u64 *d_unit_base, u64 *d_part_start, u64 *d_scan_tmp);
void launch_scatter_units(hipStream_t st, const void *d_in, void *d_out, const PassGeom &g,
                          const u64 *d_seg_start, const u32 *d_unit_start, const u64 *d_unit_base);
void launch_diff_hist(hipStream_t st, const u64 *d_start, u64 nbins, u64 *d_hist);
// Boundaries with gaps: endR / endS null: partition k of that side is [start[k], start[k + 1]); else [start[k], end[k])
// (an end below its start: empty) and nR / nS is the side's tuple count, which start[nparts] no longer is.
struct PartEnds { const u64 *endR = nullptr, *endS = nullptr; u64 nR = 0, nS = 0; };
void launch_check_radix(hipStream_t st, const void *d_R, const u64 *d_startR, const void *d_S, const u64 *d_startS, u64 nparts,
                        int radix_bits, u64 *d_bad, const PartEnds &pe = PartEnds());
void launch_prefix(hipStream_t st, const u64 *d_hist, u64 nbins, u64 *d_start);
void launch_make_tasks(hipStream_t st, const u64 *d_startR, const u64 *d_startS, u64 nparts, u32 probe_split,
                       JoinTask *d_tasks, u32 *d_ntasks, u32 max_tasks, u64 *d_stats, int kind, const SniffVerdict &sniff = SniffVerdict(),
                       const PartEnds &pe = PartEnds());
void launch_join(hipStream_t st, const void *d_R, const u64 *d_startR, const void *d_S, const u64 *d_startS,
                 const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid, int radix_bits,
                 void *d_out, u64 out_capacity, u64 *d_out_count, int kind, const u32 *d_RK = nullptr, const u32 *d_SK = nullptr,
                 const u64 *d_tag_base = nullptr, const u32 *d_skip = nullptr, u64 *host_pub = nullptr, u32 *d_done = nullptr);
void launch_join_direct(hipStream_t st, const void *d_R, u64 nR, const void *d_S, u64 nS, void *d_out, u64 out_capacity,
                        u64 *d_out_count, u64 *host_count = nullptr, u32 *d_done = nullptr, void *host_out = nullptr,
                        u64 host_cap = 0);
// one join of a batched direct launch (k_join_bkt<.., BATCH>): what launch_join_direct passes as kernel arguments, per join
struct BatchJoinDesc {
    const void *R, *S;          // 16-byte tuples in HBM
    void *out;                  // pairs in HBM
    u64 cap;                    // ... capacity (pairs)
    u64 *count;                 // device result counter of this join (zero before, zero after)
    u32 nblocks, nb, np, build_is_S, split, pad;
    u64 *host_count;            // pinned host: the count, published by the join's last workgroup
    u32 *done;                  // device ticket of this join (zero before, zero after)
    void *host_out;             // pinned host landing zone of this join's first host_cap pairs
    u64 host_cap;
};
void launch_join_batch(hipStream_t st, const BatchJoinDesc *d_batch, u32 njoins, u32 max_blocks);
constexpr u32 join_direct_tile() { return (u32)BJ_TILE; }    // probe tuples per workgroup of a direct join
void launch_checksum(hipStream_t st, const void *d_pairs, u64 n, u64 *d_sum);
void launch_generate(hipStream_t st, int kind, void *d_out, u64 n, u64 row0, u64 D, u64 seed, double theta);
void launch_expected_pkfk(hipStream_t st, const void *d_S, u64 n, u64 *d_sum);
void launch_remap_keys(hipStream_t st, void *d_rel, u64 n, int shift, u64 add);
// one partition pass over both relations of a join with shared launches (one-pass plans)
struct PassSide {
    const void *in;
    void *out;
    u64 *seg_start;
    u32 *unit_start;
    u32 *unit_hist;
    u64 *unit_base;
    u64 *part_start;
    u64 *scan_tmp;
    PassGeom g;
};
struct PassPairHost { PassSide side[2]; u64 *zero8 = nullptr; /* eight 64-bit words cleared by the first launch, or null */ int mix = 0; };
void launch_pass_pair(hipStream_t st, const PassPairHost &h, int shift, int bits, int phase);
// one-pass joins in three launches (see k_hist_fused2): phase 0 histograms, phase 1 scatter + boundaries + task list (same
// arguments to both); parity: which of the two copies of the control block this call uses (the caller alternates)
size_t fuse_ctl_bytes();
u32 *fuse_join_ticket(void *d_ctl);
// sniff: sample the join values for duplicates (DupSniff; the counters live in the control block)
void launch_fused_pass(hipStream_t st, const PassPairHost &h, int bits, int phase, int parity, void *d_ctl, u32 probe_split, u32 max_tasks,
                       u32 table_tuples, JoinTask *d_tasks, u64 *d_counters, u64 *host_pub, bool sniff = false);
constexpr int WC_MAX_BITS = 9;                   // the write-combining scatters' range (k_scatter_wc*)
constexpr int PASS_PAIR_MAX_BITS = WC_MAX_BITS;
constexpr bool fused_two_pass_ok(int b1, int b2) { return b1 >= 1 && b2 >= 1 && b1 <= WC_MAX_BITS && b2 <= WC_MAX_BITS && b1 + b2 <= 16; }

// ---- the bucket-join kernels: one row of JOIN_GEOM per JoinKernel ------------------------------------------------------------
// k_join_bkt (JK_BKT, JK_BKT_BIG): 16-byte table entries, any radix plan.  k_join_ct (JK_CT ... JK_LAST): compact 8-byte entries
// {key | arrival index of the build tuple}, both sides read once, for plans that remove at least key_index_bits payload bits.
// The launchers, the LDS attributes and the host plan all read this table; nothing else states a geometry.
enum JoinKernel { JK_BKT = 0, JK_BKT_BIG = 1, JK_CT = 2, JK_CT_HALF = 3, JK_CT_WIDE = 4, JK_CT_HALF_WIDE = 5, JK_CT_MID = 6, JK_CT_HALF_MID = 7, JK_CT_13 = 8,
                  JK_CT_HALF_MID_G = 9, JK_CT_G13 = 10, JK_CT_Q12 = 11, JK_LAST = JK_CT_Q12 };
struct JoinGeom {
    int threads, chunk, bucket_bits, ept;   // workgroup size; build tuples per LDS table; log2 of its hash buckets; probe slots per thread
    bool guard;                             // k_join_ct GUARD: skip the slot rows a partition leaves empty
    int key_index_bits;                     // k_join_ct KB: bits of the arrival index in a table entry; 0: a k_join_bkt geometry
    bool narrow_only;                       // instantiated for {payload, rowID} partitions only
};
constexpr int CT_PT = 4;                    // k_join_ct: probe slots per tile of the register ring
constexpr JoinGeom JOIN_GEOM[JK_LAST + 1] = {
    // JK_BKT: partitions that fit one table; two workgroups per CU
    {BJ_THREADS, BJ_CHUNK, BJ_BUCKET_BITS, BJ_EPT, false, 0, false},
    // JK_BKT_BIG: one workgroup per CU (152 KiB LDS); the build side in chunks, the probe side re-read per chunk
    {1024, 8448, 12, 4, false, 0, false},
    // JK_CT: the full-size compact table (see k_join_ct)
    {1024, 16352, 14, 16, false, 16, false},
    // JK_CT_HALF: the same kernel at half size, for partitions of up to 8960 build tuples (3 ... 5.5 * 10^8 tuples under a 16-bit plan):
    // 512 threads, 80 KiB LDS -> TWO workgroups per CU, which overlap each other's memory and LDS phases; the per-thread
    // register picture (18 build slots, 16 probe slots, 128 VGPRs) is unchanged.  The kernel's cost per task does not shrink
    // with the partition (every slot row is walked), so the full-size geometry is 2-3x too expensive there (measured at
    // 3 * 10^8: 8.9 ms against 5.1 ms for the chunked 16-byte-entry kernel).
    // (8960 entries in 4096 buckets until round 3: the probe tasks of 8192 tuples bound the partition size anyway, and twice
    // the buckets are worth more than the last 800 entries)
    {512, 8160, 13, 16, false, 16, false},
    // JK_CT_WIDE, JK_CT_HALF_WIDE: ... and with 20 probe slots per thread instead of 16 (narrow format only; 12 spilled VGPRs):
    // partitions whose probe side is just beyond one 16-slot task (2.2 * 10^9 tuples under 17 or 18 bits: 16.8 K / 8.4 K per
    // partition) would otherwise be cut into two tasks that both build the whole table.  Full size: the table of JK_CT_13.
    {1024, 17920, 13, 20, false, 16, true},
    {512, 8960, 12, 20, false, 16, true},                     // the 20-slot form keeps the larger table
    // JK_CT_MID: ... and a middle geometry: 12288 entries, 12 build and 12 probe slots per thread (1024 threads, one workgroup per CU).  The
    // kernel's cost per task follows its slot rows, not the partition: partitions of 8.4 - 11.5 K tuples (5.5 - 7.5 * 10^8 tuples under
    // 16 bits, 1.1 - 1.5 * 10^9 under 17) paid for 18 + 16 rows in the full-size geometry ([measured] join kernel 8.5 -> 6.6 ms at
    // 6 * 10^8, 17.6 -> 14.1 at 1.5 * 10^9; 16 + 16 rows for the 15.3 K-tuple partitions of 10^9 tuples: 10.09 -> 10.02, not kept).
    {1024, 12288, 14, 12, false, 16, false},
    // JK_CT_HALF_MID: ... and at half size (512 threads, two workgroups per CU): 4.2 - 5.8 K-tuple partitions
    {512, 6144, 13, 12, false, 16, false},
    // JK_CT_13 (the full-size geometry of rounds 2 and 3 until the bucket count was doubled): 17920 entries, 8192 buckets.  For
    // partitions of 15.3 - 16.8 K build tuples (1.005 - 1.1 * 10^9 tuples under 16 bits), which the 16352-entry table would
    // build in two chunks; the 20-slot kernel (probe side beyond 16 K) keeps this table too.
    {1024, 17920, 13, 16, false, 16, false},
    // JK_CT_HALF_MID_G: the 6144-entry geometry with row guards, for average build partitions of CT_GUARDED_FROM ... CT_GUARDED_UPTO
    {512, 6144, 13, 12, true, 16, false},
    // JK_CT_G13: the 6144-entry geometry with row guards and 13-bit arrival indices: keys of up to 51 bits, i.e. plans of 13-15
    // radix bits (1.6 * 10^7 ... 1.3 * 10^8 tuples per side), whose 2-4 K-tuple partitions the one-table kernel served until round 4
    {512, 6144, 13, 12, true, 13, false},
    // JK_CT_Q12: a 4096-entry table with 12-bit arrival indices (keys of up to 52 bits) in 4096 buckets, 8 + 8 slot rows per thread, row
    // guards, 41 KiB of LDS: plans of exactly 12 bits (8.4 * 10^6 ... 1.6 * 10^7 tuples per side, partitions of 2-3.8 K tuples)
    {512, 4096, 12, 8, true, 12, false},
};
constexpr bool jk_is_ct(int k) { return k >= JK_CT && k <= JK_LAST; }                         // a compact-table geometry
constexpr const JoinGeom &join_geom(int kind) { return JOIN_GEOM[kind >= 0 && kind <= JK_LAST ? kind : JK_BKT]; }
constexpr bool jk_ct_narrow_only(int k) { return join_geom(k).narrow_only; }
// probe tuples per task the kernel holds at most: a compact-table task keeps its probe rowIDs in registers (0: no limit of its own)
constexpr u32 join_probe_split(int kind) { return jk_is_ct(kind) ? (u32)(join_geom(kind).threads * join_geom(kind).ept) : 0u; }
constexpr u32 join_table_tuples(int kind) { return (u32)join_geom(kind).chunk; }             // build tuples per LDS table
// radix bits a plan must remove for the key to fit beside the arrival index: 16 (48-bit keys); JK_CT_G13: 13; JK_CT_Q12: 12
constexpr int join_ct_min_radix_bits(int kind = JK_CT) { return join_geom(jk_is_ct(kind) ? kind : JK_CT).key_index_bits; }
// dynamic LDS of a launch.  k_join_bkt: keys + rowIDs, bucket offsets, scan scratch, sender bases.  k_join_ct: entries, packed
// 16-bit bucket counts, scan scratch (>= 128 B behind the table: a compare round may read 15 entries past a bucket's end)
constexpr size_t join_lds_bytes(const JoinGeom &g)
{
    return g.key_index_bits == 0
               ? (size_t)g.chunk * 16 + ((size_t)(1 << g.bucket_bits) + 4) * 4 + 64 * 4 + (size_t)(g.threads / 64) * 4 + 16 + 2 * TAG_MAX * 8
               : (size_t)g.chunk * 8 + ((size_t)(1 << g.bucket_bits) / 2 + 2 + 2 * (g.threads / 64)) * 4 + 24 + (g.threads < 1024 ? 64 : 0);
}
constexpr bool join_geom_ok(int k)
{
    const JoinGeom &g = JOIN_GEOM[k];
    return join_lds_bytes(g) <= 160 * 1024 &&                                             // what one workgroup can have
           (!jk_is_ct(k) ? g.key_index_bits == 0 && !g.guard && !g.narrow_only
                         : g.chunk <= 1 << g.key_index_bits && g.ept % CT_PT == 0 && (1 << g.bucket_bits) % (2 * g.threads) == 0) &&
           (k == 0 || join_geom_ok(k - 1));
}
static_assert(join_geom_ok(JK_LAST), "a JOIN_GEOM row breaks what its kernel needs");
// ---- the semi / anti join kernel (k_semi_bkt): one geometry -------------------------------------------------------
// An open-addressed LDS table of 8-byte KEYS of S (no rowIDs), insert-if-absent, filled while S's partition streams through it in
// tiles of SEMI_BUILD_TILE tuples and closed before a tile that could take it past SEMI_FILL distinct keys (9/16 of its slots: a
// linear probe always meets an empty slot, and soon); a 4 KiB bitmap of match bits for the task's at most SEMI_MAX_SPLIT tuples of R.
constexpr int JK_SEMI = JK_LAST + 1;              // "last.join_kernel" of a semi / anti join (12)
constexpr int SEMI_THREADS = 512;                 // 8 wavefronts; 68.3 KiB of LDS: two workgroups per CU
constexpr int SEMI_SLOT_BITS = 13;                // 8192 slots = 64 KiB
constexpr u32 SEMI_FILL = 4608;                   // distinct keys a table takes at most
constexpr int SEMI_BPT = 2;                       // tuples of S per thread per build tile
constexpr u32 SEMI_BUILD_TILE = SEMI_THREADS * SEMI_BPT;
constexpr int SEMI_EPT = 8;                       // tuples of R per thread per probe tile (4096)
constexpr u32 SEMI_MAX_SPLIT = 32768;             // tuples of R per task at most: the match bits of a task
constexpr size_t semi_lds_bytes() { return ((size_t)8 << SEMI_SLOT_BITS) + SEMI_MAX_SPLIT / 8 + 64 * 4 + 32; }
static_assert(2 * semi_lds_bytes() <= 160 * 1024 && SEMI_FILL + SEMI_BUILD_TILE <= (1u << SEMI_SLOT_BITS) &&
              SEMI_MAX_SPLIT % (SEMI_THREADS * SEMI_EPT) == 0 && SEMI_EPT * (SEMI_THREADS / 64) == 64, "k_semi_bkt's geometry");
// task list of a semi / anti join: partition k gets ceil(|R_k| / split) tasks if |R_k| != 0 && (|S_k| != 0 || anti); the table side
// is always S.  d_stats as launch_make_tasks (zeroed by the caller): largest partitions, [3] = an |S_k| >= 2^32.
void launch_make_semi_tasks(hipStream_t st, const u64 *d_startR, const u64 *d_startS, u64 nparts, u32 split, int anti,
                            JoinTask *d_tasks, u32 *d_ntasks, u32 max_tasks, u64 *d_stats);
// d_out: u64 rowIDs of R (may be null: count only); d_max_tables: atomicMax of the tables a task built, by tasks that built
// several; d_RK / d_SK: the rowID arrays of narrow partitions (both or neither); d_skip: as launch_join
void launch_semi_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid,
                      int radix_bits, int anti, u64 *d_out, u64 out_capacity, u64 *d_out_count, u64 *d_max_tables,
                      const u32 *d_RK, const u32 *d_SK, const u32 *d_skip);
// One anti sweep of an outer join: k_semi_bkt in a 16-byte pair form, anti = 1, over the task list of
// launch_make_semi_tasks(probe side's boundaries, table side's boundaries, .., anti = 1).  d_P / d_T: the partitions of the preserved
// side (probed, reported) and of the side the tables are built on; preserved_is_S 0: R against S, rows {rowID, all ones};
// 1: S against R, rows {all ones, rowID}.  d_out: rhj_pair (may be null: count only), written from the value d_out_count[0]
// already holds on and never at or past out_capacity; d_PK / d_TK: the rowID arrays of narrow partitions, probed side first.
void launch_outer_sweep(hipStream_t st, const void *d_P, const void *d_T, const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid,
                        int radix_bits, int preserved_is_S, void *d_out, u64 out_capacity, u64 *d_out_count, u64 *d_max_tables,
                        const u32 *d_PK, const u32 *d_TK, const u32 *d_skip);
// ---- the aggregating join kernel (k_agg_bkt): one geometry --------------------------------------------------------
// k_semi_bkt's table of 8-byte keys of S with a 32-bit occurrence count beside every slot, in a parallel array: 8192 + 8192 = 96 KiB,
// one workgroup of 1024 threads per CU -- four wavefronts per SIMD, and a 15 K-tuple partition of S in four tables where the
// 4096-slot shape (48 KiB, workgroups of 512) would sweep R seven times.  No match bits: a task's R range is not bound by LDS.
constexpr int JK_AGG = JK_SEMI + 1;               // "last.join_kernel" of an aggregating join (13)
constexpr int AGG_MAX_COLS = 4;                   // sums per call (rhj.h RHJ_SUM_MAX_COLS)
constexpr int AGG_THREADS = 1024;                 // 16 wavefronts
constexpr int AGG_SLOT_BITS = 13;                 // 8192 slots: 64 KiB of keys + 32 KiB of counts
constexpr u32 AGG_FILL = 4608;                    // distinct keys a table takes at most (9/16 of its slots, as SEMI_FILL)
constexpr int AGG_BPT = 1;                        // tuples of S per thread per build tile
constexpr u32 AGG_BUILD_TILE = AGG_THREADS * AGG_BPT;
constexpr int AGG_EPT = 4;                        // tuples of R per thread per probe tile (4096)
constexpr u32 AGG_MAX_SPLIT = BJ_MAX_PROBE_SPLIT; // tuples of R per task at most (rhj_opts.probe_split: values above 2^24 act as 2^24)
constexpr size_t agg_lds_bytes() { return ((size_t)12 << AGG_SLOT_BITS) + 16; }
static_assert(agg_lds_bytes() <= 160 * 1024 && AGG_FILL + AGG_BUILD_TILE <= (1u << AGG_SLOT_BITS) &&
              (size_t)(AGG_THREADS / 64) * (AGG_MAX_COLS + 1) * 8 <= ((size_t)8 << AGG_SLOT_BITS) &&
              (u64)AGG_MAX_SPLIT * 16 < (1ull << 31), "k_agg_bkt's geometry");
// The task list is launch_make_semi_tasks with anti = 0.  d_cols: HOST array of ncols (<= AGG_MAX_COLS) device columns of col_rows words indexed by
// R's rowID; d_sums: ncols + 1 words (zeroed by the caller), word 0 the count; d_bad: OR-ed with 1 when a rowID >= col_rows was
// met (ncols != 0 only); the rest as launch_semi_join.
void launch_agg_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid,
                     int radix_bits, const u64 *const *d_cols, u32 ncols, u64 col_rows, u64 *d_sums, u32 *d_bad, u64 *d_max_tables,
                     const u32 *d_RK, const u32 *d_SK, const u32 *d_skip);
// ---- the multiplicity join kernel (k_mult_bkt): k_agg_bkt's geometry, a wider slot ----------------------------------
// k_agg_bkt's table, tiles, close rule and probe tile.  Beside every key slot: the 32-bit occurrence count (unweighted, 96 KiB as
// k_agg_bkt) or a 64-bit sum of the weights of S's tuples with that key (weighted: 8192 x (8 + 8) B = 128 KiB); either way one
// workgroup of 1024 threads per CU.
constexpr int JK_MULT = JK_AGG + 1;               // "last.join_kernel" of a multiplicity join (14)
constexpr size_t mult_lds_bytes(bool weighted) { return ((size_t)(weighted ? 16 : 12) << AGG_SLOT_BITS) + 16; }
static_assert(mult_lds_bytes(true) <= 160 * 1024 && mult_lds_bytes(false) == agg_lds_bytes() &&
              (size_t)(AGG_THREADS / 64) * 8 <= ((size_t)8 << AGG_SLOT_BITS), "k_mult_bkt's geometry");
constexpr u32 MULT_BAD_ROW_R = 1, MULT_BAD_ROW_S = 2;   // bits of *d_bad
// The task list is launch_make_semi_tasks with anti = 0.  d_w: device column of w_rows words indexed by S's rowID, or null (every
// tuple of S weighs 1); d_out: out_rows words (zeroed by the caller), word rowR receives the tuple's multiplicity by a global atomic
// add; d_total: one word (zeroed by the caller), the sum of all multiplicities; d_bad: OR-ed with MULT_BAD_ROW_R when a rowID of R
// >= out_rows was met (never stored to), with MULT_BAD_ROW_S when a rowID of S >= w_rows was (never loaded from; d_w != null only);
// the rest as launch_semi_join.
void launch_mult_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid,
                      int radix_bits, const u64 *d_w, u64 w_rows, u64 *d_out, u64 out_rows, u64 *d_total, u32 *d_bad,
                      u64 *d_max_tables, const u32 *d_RK, const u32 *d_SK, const u32 *d_skip);
// ---- the group-by kernel (k_group_bkt): k_mult_bkt's weighted table over ONE relation ------------------------------
// 8192 keys + 8192 64-bit accumulators + the tail words of mult_lds_bytes(true), then what the class walk needs: the class's first
// group (8 B), the THREADS / 64 words of a workgroup scan, the 2 x AGG_MAX_COLS column pointers and one word for the columns' op
// words (k_group_bkt<., GB_OPS>).  One workgroup of 1024 threads per task, one task per partition.
constexpr int JK_GROUP = JK_MULT + 1;             // "last.join_kernel" of a group-by (15)
constexpr u32 GROUP_BAD_ROW = 1, GROUP_BAD_GID = 2;      // bits of *d_bad: a rowID >= col_rows; (a launch with ids) a rowID >= gid_rows
constexpr size_t GROUP_LDS_EXTRA = 8 + (size_t)(AGG_THREADS / 64) * 4 + (size_t)(2 * AGG_MAX_COLS + 1) * 8;
// The aggregate of a column, as the group kernels take it: AGG_OP_BITS bits per column -- the LDS atomic, and whether
// the word is biased by 1 << 63 on its way in and out (a signed minimum or maximum as an unsigned one).  A call's op words are
// packed into one u32: column j at bit AGG_OP_BITS * j; in a group-by join R's columns first, S's column j at AGG_OP_BITS *
// (AGG_MAX_COLS + j).  0: every column is a sum.
constexpr u32 AGG_OP_ADD = 0, AGG_OP_MIN = 1, AGG_OP_MAX = 2, AGG_OP_KIND = 3, AGG_OP_SIGNED = 4, AGG_OP_BITS = 4;
static_assert(2 * AGG_MAX_COLS * AGG_OP_BITS <= 32, "a call's op words fit one u32");
constexpr size_t group_lds_bytes() { return mult_lds_bytes(true) + GROUP_LDS_EXTRA; }
static_assert(group_lds_bytes() <= 160 * 1024 && mult_lds_bytes(true) % 8 == 0 && AGG_FILL + AGG_BUILD_TILE <= (1u << AGG_SLOT_BITS) &&
              (1u << AGG_SLOT_BITS) % AGG_THREADS == 0, "k_group_bkt's geometry");
// The row of a group's extreme (k_group_bkt<., GB_ARG>): ARG_OP_BITS bits per column -- AGG_OP_MIN or AGG_OP_MAX and
// AGG_OP_SIGNED as above, or ARG_OP_ROW (no column: the rowIDs are what is ordered), and ARG_OP_LAST (among the tuples that hold the
// extreme the largest rowID; clear: the smallest).  Column j at bit ARG_OP_BITS * j of one u32.  The instantiation keeps four more
// pointers in LDS than its siblings -- the rows arrays, behind the word of op words -- and has its own LDS size for them.
constexpr u32 ARG_OP_ROW = 8, ARG_OP_LAST = 16, ARG_OP_BITS = 8;
static_assert(AGG_MAX_COLS * ARG_OP_BITS <= 32 && (ARG_OP_ROW & (AGG_OP_KIND | AGG_OP_SIGNED)) == 0 && ARG_OP_LAST < (1u << ARG_OP_BITS),
              "a call's arg op words fit one u32");
constexpr size_t group_arg_lds_bytes() { return group_lds_bytes() + (size_t)AGG_MAX_COLS * 8; }
static_assert(group_arg_lds_bytes() <= 160 * 1024 && group_arg_lds_bytes() % 8 == 0, "k_group_bkt<., GB_ARG>'s geometry");
// The task list is launch_make_semi_tasks with anti = 1, a zeroed boundary array of S and split = 2^32 - 1: one task per non-empty
// partition of R, the whole partition (its S range is empty and never read).  mixed: the partitions hold rhj_mix64 of the caller's
// values (keys are unmixed on the way out).  d_cols / d_out_sums: HOST arrays of ncols (<= AGG_MAX_COLS) device columns; ncols == 0:
// no sum sweep, neither is read.  d_out_keys / d_out_counts (may be null) / d_out_sums[j]: capacity words each; capacity == 0: count
// only.  d_ngroups: one word (zeroed by the caller), the number of groups; d_bad: OR-ed with 1 when a rowID >= col_rows was met
// (never dereferenced; ncols != 0 only); d_max_rounds: atomicMax of the table builds of a task, by tasks that built several; d_RK:
// the rowID array of narrow partitions, or null; d_skip: as launch_join.  ops: the columns' packed op words (AGG_OP_*); 0 -- every
// column a sum -- launches k_group_bkt<., GB_COUNT | GB_SUMS> as before, anything else with ncols != 0 k_group_bkt<., GB_OPS>.
// ids: the same kernel with an id sweep behind the last column sweep of every class (k_group_bkt<., . | GB_IDS>);
// d_ngroups is then FIVE words, the four behind the counter written by launch_group_id_words before this launch (the second pair
// unused); d_bad is OR-ed with 2 when a rowID >= gid_rows was met (never stored to).  false: the launch is the one it was.
// d_out_rows: a HOST array of ncols device columns of capacity words, and ops are then ARG_OP_* words: with ncols != 0
// k_group_bkt<., GB_ARG>, which fills d_out_sums[j] with the extremes and d_out_rows[j] with their rows (d_cols[j] / d_out_sums[j] of an
// ARG_OP_ROW column are never touched); ids must be false.  null: the launch is the one it was.
void launch_group(hipStream_t st, const void *d_R, const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid, int radix_bits, bool mixed,
                  const u64 *const *d_cols, u32 ncols, u64 col_rows, u64 *d_out_keys, u64 *d_out_counts, u64 *const *d_out_sums,
                  u64 capacity, u64 *d_ngroups, u32 *d_bad, u64 *d_max_rounds, const u32 *d_RK, const u32 *d_skip, u32 ops,
                  bool ids = false, u64 *const *d_out_rows = nullptr);
// The id arrays of a launch with ids (either may be null: no sweep of that side) and their lengths in words, into d_ngroups[1 .. 4].
void launch_group_id_words(hipStream_t st, u64 *d_ngroups, u64 *d_gidR, u64 gidR_rows, u64 *d_gidS, u64 gidS_rows);
// ---- the group-by join kernel (k_gjoin_bkt): k_group_bkt's table and class walk over R, looked up by S ---------------
// group_lds_bytes() plus room for the pointers of S's side (4 x AGG_MAX_COLS column and output pointers in all) and for nine more
// kernel arguments, which would otherwise spill SGPRs; group_lds_bytes()'s word of op words comes last (k_gjoin_bkt<., GB_OPS>).  The slot word holds
// cntR | cntS << 32 during the count sweeps (a second 32 KiB count array would end 16 bytes above 160 KiB).
constexpr int JK_GJOIN = JK_GROUP + 1;            // "last.join_kernel" of a group-by join (16)
constexpr u32 GJOIN_BAD_ROW_R = 1, GJOIN_BAD_ROW_S = 2;   // bits of *d_bad
constexpr u32 GJOIN_BAD_GID_R = 4, GJOIN_BAD_GID_S = 8;   // ... of a launch with ids: a rowID >= gidR_rows / gidS_rows was met
constexpr u32 GJOIN_PAR_WORDS = 9;                // further kernel arguments kept in LDS across the class walk (k_gjoin_bkt)
constexpr size_t gjoin_lds_bytes() { return group_lds_bytes() + (size_t)(2 * AGG_MAX_COLS + GJOIN_PAR_WORDS) * 8; }
static_assert(gjoin_lds_bytes() <= 160 * 1024 && gjoin_lds_bytes() % 8 == 0, "k_gjoin_bkt's geometry");
// The task list is launch_make_semi_tasks over the boundary arrays of R and S with split = 2^32 - 1 and anti = left_mode: one task
// per partition k with R_k non-empty (left_mode) or R_k and S_k non-empty (inner), both whole partitions; a task's range of S may be
// empty and is then never read (d_S may be null when every one is).  mixed as launch_group.  d_colsR / d_out_sumsR: HOST arrays of
// ncolsR (<= AGG_MAX_COLS) device columns, d_colsS / d_out_sumsS of ncolsS; both 0: no sum sweep.  d_out_keys / d_out_cntR (may be
// null) / d_out_cntS (may be null) / sums: capacity words each; capacity == 0: count only.  d_ngroups: one word (zeroed by the
// caller); d_bad: OR-ed with GJOIN_BAD_ROW_R / _S when a rowID >= colR_rows / colS_rows was met (never dereferenced); d_max_rounds as
// launch_group; d_RK / d_SK: the rowID arrays of narrow partitions, or d_RK null: 16-byte tuples; d_skip: as launch_join.  ops: both
// sides' packed op words (AGG_OP_*); 0 launches k_gjoin_bkt<., GB_COUNT | GB_SUMS> as before, anything else with a column k_gjoin_bkt<., GB_OPS>.
// ids as launch_group: d_ngroups[1 .. 4] = gidR, gidR_rows, gidS, gidS_rows; the kernel stores a group index for the tuples that
// have one and nothing else -- the caller fills both arrays with all ones first; d_bad is OR-ed with GJOIN_BAD_GID_R / _S.
void launch_group_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid,
                       int radix_bits, bool mixed, bool left_mode, const u64 *const *d_colsR, u32 ncolsR, u64 colR_rows,
                       const u64 *const *d_colsS, u32 ncolsS, u64 colS_rows, u64 *d_out_keys, u64 *d_out_cntR, u64 *d_out_cntS,
                       u64 *const *d_out_sumsR, u64 *const *d_out_sumsS, u64 capacity, u64 *d_ngroups, u32 *d_bad, u64 *d_max_rounds,
                       const u32 *d_RK, const u32 *d_SK, const u32 *d_skip, u32 ops, bool ids = false);
// ---- the lookup join kernel (k_lookup_bkt): k_mult_bkt's weighted table, a partner rowID in the slot word ------------
// 8192 keys + 8192 64-bit words that start from all ones and take the minimum (first) or maximum (last) rowID of S's tuples with the
// key, the all-ones key's word beside them: mult_lds_bytes(true), one workgroup of 1024 threads per CU.
constexpr int JK_LOOKUP = JK_GJOIN + 1;           // "last.join_kernel" of a lookup join (17)
constexpr size_t lookup_lds_bytes() { return mult_lds_bytes(true); }
static_assert(lookup_lds_bytes() <= 160 * 1024 && lookup_lds_bytes() == ((size_t)16 << AGG_SLOT_BITS) + 16 &&
              AGG_FILL + AGG_BUILD_TILE <= (1u << AGG_SLOT_BITS) && (size_t)(AGG_THREADS / 64) * 8 <= ((size_t)8 << AGG_SLOT_BITS),
              "k_lookup_bkt's geometry");
constexpr u32 LOOKUP_BAD_ROW_R = 1, LOOKUP_BAD_ROW_S = 2;   // bits of *d_bad
// The task list is launch_make_semi_tasks with anti = 0.  which: 0 the smallest rowID of S among a tuple's partners, 1 the largest.
// d_out: out_rows words (filled with all ones by the caller), word rowR receives the partner by a global atomic minimum (unsigned) /
// maximum (signed); d_matched: one word (zeroed by the caller), the number of words that left all ones; d_bad: OR-ed with
// LOOKUP_BAD_ROW_R when a rowID of R >= out_rows was met (never stored to), with LOOKUP_BAD_ROW_S when a rowID of S >= 2^63 was
// (which == 1 only; never inserted); the rest as launch_semi_join.
void launch_lookup_join(hipStream_t st, const void *d_R, const void *d_S, const JoinTask *d_tasks, const u32 *d_ntasks, u32 grid,
                        int radix_bits, int which, u64 *d_out, u64 out_rows, u64 *d_matched, u32 *d_bad, u64 *d_max_tables,
                        const u32 *d_RK, const u32 *d_SK, const u32 *d_skip);
// in_narrow: d_in is a payload array (u64).  key_base / d_wide (16-byte input): d_wide (may be null) is OR-ed with 1 when some
// rowID - key_base does not fit 32 bits.  d_unit_rng (may be null): explicit pass-1 units (launch_seg_units).
void launch_hist2d_units(hipStream_t st, const void *d_in, bool in_narrow, u64 n, u64 L, u32 units, int b1, int b2,
                         u32 units_per_group, u32 ngroups, u32 *d_hist1, u32 *d_hist2, u64 key_base, u32 *d_wide,
                         const u64 *d_unit_rng, int mix = 0, const DupSniff &sniff = DupSniff());
// the kernels that may be the first to touch a caller's relation on the fused two-pass path, reading COLUMNS: the exact-cursor
// histogram, pass 1 with a 16-byte (narrow level 1) or narrow (level 2) intermediate, the count-free pass 1; and the
// conversion the other plans start with.  Same geometry, tables and outputs as the 16-byte forms they stand beside.
void launch_hist2d_units_cols(hipStream_t st, const ColsIn &cols, u64 n, u64 L, u32 units, int b1, int b2, u32 units_per_group,
                              u32 ngroups, u32 *d_hist1, u32 *d_hist2, u32 *d_wide, int mix, const DupSniff &sniff);
void launch_scatter_units_cols(hipStream_t st, const ColsIn &cols, void *d_out, const PassGeom &g, const u64 *d_seg_start,
                               const u32 *d_unit_start, const u64 *d_unit_base);
void launch_scatter_units_narrow_cols(hipStream_t st, const ColsIn &cols, void *d_out, u64 n, const PassGeom &g, const u64 *d_seg_start,
                                      const u32 *d_unit_start, const u64 *d_unit_base, u32 *d_overflow);
void launch_cols_to_tuples(hipStream_t st, const ColsIn &cols, u64 n, void *d_out);
void launch_seg_units(hipStream_t st, u32 nseg, const u64 *seg_off, const u64 *seg_L, u32 units_per_seg, u64 *d_unit_rng,
                      u64 *d_seg_start, u32 *d_unit_start);
void launch_make_group_ranges(hipStream_t st, const u64 *d_unit_base1, u32 nb1, u32 units_per_group, u32 ngroups, u64 n,
                              u64 *d_rng, u32 *d_unit_start2);
void launch_scatter_ranges(hipStream_t st, const void *d_in, void *d_out, u32 nunits, int shift, int bits,
                           const u64 *d_unit_base, const u64 *d_rng);
// narrow intermediate format (k_scatter_wcn): payloads (u64) at offset 0 of a buffer of >= 16 n bytes, rowIDs (u32) here
inline size_t narrow_k_offset(u64 n) { return ((size_t)n * 8 + 255) & ~(size_t)255; }
constexpr int RHJ_RETRY_WIDE = 1000;                    // internal: join_phase saw the narrow-format overflow flag
constexpr int RHJ_RETRY_CF = 1001;                      // internal: ... or a count-free pass 1's overflow bit (2 << side)
constexpr u64 NARROW_MIN_TUPLES = 1024;                 // 12 n + 256 <= 16 n
constexpr u64 NARROW_AUTO_MIN_TUPLES = 8000000;         // automatic choice: larger side at least this ([measured] 4M: 0.45 ms
                                                        // either way; 16M ... 256M: 5-8 % faster narrow; 10^9: 19 %)
constexpr int WN_MAX_BITS = 8, WN9_MAX_BITS = 9;
constexpr bool narrow_pass_ok(int bits) { return bits >= 1 && bits <= WN_MAX_BITS; }     // the 32-tuple-line geometry
constexpr bool narrow_pass9_ok(int bits) { return bits >= 1 && bits <= WN9_MAX_BITS; }   // ... or the 16-tuple-line geometry
void launch_hist_units_narrow(hipStream_t st, const void *d_inP, const PassGeom &g, const u64 *d_seg_start,
                              const u32 *d_unit_start, u32 *d_unit_hist);
void launch_scatter_units_narrow_any(hipStream_t st, const void *d_in, const u32 *d_inK, void *d_outP, u32 *d_outK, const PassGeom &g,
                                     const u64 *d_seg_start, const u32 *d_unit_start, const u64 *d_unit_base, u32 *d_overflow);
void launch_scatter_units_narrow(hipStream_t st, const void *d_in, void *d_out, u64 n, const PassGeom &g,
                                 const u64 *d_seg_start, const u32 *d_unit_start, const u64 *d_unit_base, u32 *d_overflow,
                                 u64 key_base = 0);
void launch_scatter_units_narrow_peer(hipStream_t st, const void *d_in, const PassGeom &g, const u64 *d_seg_start,
                                      const u32 *d_unit_start, const u64 *d_unit_base, u32 *d_overflow, u64 key_base,
                                      const u64 *d_delta, const unsigned char *d_owner, void *const *peersP, void *const *peersK,
                                      int nranks);
void launch_scatter_ranges_narrow(hipStream_t st, const void *d_in, bool in_narrow, void *d_out, u64 n, u32 nunits, int shift,
                                  int bits, const u64 *d_unit_base, const u64 *d_rng, u32 *d_overflow, u32 tag_groups = 0,
                                  u32 tag_div = 0, const u32 *d_inK = nullptr);   // d_inK: narrow input whose rowID array is not at narrow_k_offset(n)
// Count-free pass 1 of a fused 8+8 narrow partition (k_scatter_wcn_cf): U pass-1 units of g.L tuples, `per` of them
// per group; region (d, u) of the intermediate arrays = slots [(d * U + u) * cap, + cap); slots = nb1 * U * cap; payloads (u64) at
// offset 0 of the intermediate buffer, rowIDs (u32) at slots * 8.  d_flag: the join's skip word (bit 0: a wide rowID); `bit` is
// OR-ed into it when a run does not fit its region.  Tables: cnt1 [U][nb1] u32, pre cf_pre_words(units2) u32, unit_tot [units2] u32.
struct CfGeom { u32 U = 0, per = 0, ngroups = 0, cap = 0; u64 slots = 0; };
constexpr u32 CF_PER_MAX = 64, CF_PRE = CF_PER_MAX + 1;  // pieces per pass-2 unit the kernels handle; words of a unit's prefix table
constexpr u32 cf_per_max() { return CF_PER_MAX; }
constexpr size_t cf_pre_words(u32 units2) { return (size_t)units2 * CF_PRE; }
// Count-free pass 2 with one writer per final partition (k_scatter_wcn_cf2): final partition p of np = nb1 << b2 owns
// slots [p * cap2, + cap2) of the final arrays; payloads (u64) at offset 0 of the partition buffer, rowIDs (u32) at
// narrow_k_offset(slots) = 8 * slots.  The prefix of a bucket's U piece lengths lives in the kernel's LDS: U <= CF2_PRE - 1.
struct Cf2Geom { u32 cap2 = 0; u64 slots = 0; };
constexpr u32 CF2_PRE = 1025;
constexpr size_t cf2_part_bytes(const Cf2Geom &c) { return (size_t)c.slots * 12 + 256; }
void launch_cf2_pass2(hipStream_t st, const void *d_tmp, void *d_out, const CfGeom &c, const Cf2Geom &c2, u32 nb1, int b1, int b2,
                      const u32 *d_cnt1, u64 *d_start, u64 *d_end, u32 *d_flag, u32 bit);
void launch_cf_pass1(hipStream_t st, const void *d_in, void *d_tmp, const CfGeom &c, const PassGeom &g, const u64 *d_seg_start,
                     const u32 *d_unit_start, u32 *d_cnt1, u32 *d_flag, u32 bit, const DupSniff &sniff);
void launch_cf_pass1_cols(hipStream_t st, const ColsIn &cols, void *d_tmp, const CfGeom &c, const PassGeom &g, const u64 *d_seg_start,
                          const u32 *d_unit_start, u32 *d_cnt1, u32 *d_flag, u32 bit, const DupSniff &sniff);
void launch_cf_tables(hipStream_t st, const CfGeom &c, u32 nb1, const u32 *d_cnt1, u32 *d_pre, u32 *d_unit_tot, u64 *d_ps_1,
                      u32 *d_unit_start2, const u32 *d_flag);
void launch_cf_hist2(hipStream_t st, const void *d_tmp, const CfGeom &c, u32 nb1, int b1, int b2, const u32 *d_pre, u32 *d_hist2,
                     const u32 *d_flag);
void launch_cf_pass2(hipStream_t st, const void *d_tmp, void *d_out, u64 n, const CfGeom &c, u32 nb1, int b1, int b2,
                     const u64 *d_unit_base, const u32 *d_pre, u32 *d_flag);
const char *launch_attr_error();                       // text of the first refused hipFuncSetAttribute, or null
void launch_scatter_ranges_n2a(hipStream_t st, const void *d_in, void *d_out, u64 n, u32 nunits, int shift, int bits,
                               const u64 *d_unit_base, const u64 *d_rng, const u64 *d_key_bases, u32 tag_groups, u32 tag_div,
                               const u32 *d_skip);
size_t scan_tmp_bytes(int bits);
size_t part_lds_bytes(int bits);
// ---- the sort kernels (rhj_sort.hip): one geometry -----------------------------------------------------------------
// A stable LSD radix sort by 8-bit digits.  One workgroup of 512 threads ranks a tile of 4096 rows at once ("sort.tile_rows"): eight
// rows per lane, the ranked tile staged in LDS (8-byte keys, 0 / 4 / 8-byte rows) beside the per-wave digit counts.
constexpr int SORT_THREADS = 512;
constexpr int SORT_TPT = 8;                       // rows per thread per tile
constexpr int SORT_TILE = SORT_THREADS * SORT_TPT;
constexpr int SORT_DIGIT_BITS = 8;
// top-k: the automatic "topk.max_candidates" is max(k, this) -- selection stops once so few rows are tied with the
// threshold's digits that sorting them costs less than another read of the column ("topk.auto_candidates")
constexpr int TOPK_AUTO_CANDIDATES = 1 << 16;
// the window scans (rhj_window.hip) run on the sort's units and tiles: one workgroup of SORT_THREADS scans a tile of
// this many sorted positions at once ("window.tile_rows")
constexpr int WINDOW_TILE = SORT_TILE;
// ... and so does the as-of scan (rhj_asof.hip; "asof.tile_rows")
constexpr int ASOF_TILE = SORT_TILE;
// ... and the range join's two scans (rhj_range.hip; "range_join.tile_rows"); its expansion writes this many pairs per
// workgroup ("range_join.expand_tile")
constexpr int RANGE_TILE = SORT_TILE;
constexpr int RANGE_EXPAND_TILE = 2048;

// ---- rhj_api.hip's hooks for the other translation units of the library (rhj_query.hip, rhj_keys.hip and the sort-based files) -----
typedef struct rhj_ctx rhj_ctx;                 // (include/rhj.h's)
int rhj_internal_use_device(rhj_ctx *ctx);
hipStream_t rhj_internal_stream(rhj_ctx *ctx);
int rhj_internal_fail(rhj_ctx *ctx, int code, const char *msg);
void *rhj_internal_counters(rhj_ctx *ctx);      // >= 64 bytes of zeroable device scratch, or nullptr on failure
void *rhj_internal_span_open(rhj_ctx *ctx, int kind);                           // a profiling span (RHJ_K_*) around the launches that follow
void rhj_internal_span_close(void *span);
// one buffer per entry, grown to >= bytes: an outer entry's own buffer survives the inner sorts, which regrow the sort's
enum { RHJ_WS_SORT = 0, RHJ_WS_TOPK, RHJ_WS_WINDOW, RHJ_WS_ASOF, RHJ_WS_FRAME, RHJ_WS_RANGE, RHJ_WS_COUNT };
int rhj_internal_workspace(rhj_ctx *ctx, int which, size_t bytes, void **out);
void rhj_internal_sort_begin(rhj_ctx *ctx);     // the start of a call: timings and "last.*" as prof_reset leaves them, "last.join_kernel" -1
void rhj_internal_sort_report(rhj_ctx *ctx, int bits, int passes, int units);   // "last.sort_bits" / "last.sort_passes" / "last.sort_units"
int rhj_internal_sort_max_units(rhj_ctx *ctx);                                  // "sort.max_units": -1 automatic, else 1 .. SORT_MAX_UNITS
void rhj_internal_topk_report(rhj_ctx *ctx, int bits, int passes, u64 candidates, u64 sorted_rows);   // "last.topk_*"
int64_t rhj_internal_topk_max_candidates(rhj_ctx *ctx);                         // "topk.max_candidates": -1 automatic, else 1 .. 2^31 - 1
void rhj_internal_window_report(rhj_ctx *ctx, int units, int sorts, u64 partitions);   // "last.window_units" / "last.window_sorts" / "last.window_partitions"
void rhj_internal_asof_report(rhj_ctx *ctx, int units, int sorts, u64 matched);   // "last.asof_units" / "last.asof_sorts" / "last.asof_matched"
void rhj_internal_frame_report(rhj_ctx *ctx, int units, int sorts, int scans, u64 partitions);   // "last.frame_units" / "last.frame_sorts" / "last.frame_scans" / "last.frame_partitions"
void rhj_internal_frame_range_report(rhj_ctx *ctx, int units, int sorts, int scans, int levels, u64 partitions);   // "last.frame_range_*", as above and "last.frame_range_levels"
void rhj_internal_range_report(rhj_ctx *ctx, int units, int sorts, u64 pairs, u64 tiles);   // "last.range_join_units" / "_sorts" / "_pairs" / "_expand_tiles"
void rhj_internal_range_last(rhj_ctx *ctx, int *units, int *sorts);             // ... the first two as they stand
// ... and rhj_sort.hip's, for the entries that order their rows with it
int rhj_internal_sort_run(rhj_ctx *ctx, const char *who, const u64 *keys, const u64 *rows, u64 n, u32 flags, u64 *okeys, u64 *orows);
void rhj_internal_sort_units(rhj_ctx *ctx, u64 n, u64 *L, u32 *U);              // units of L rows, a whole number of tiles, under "sort.max_units"
