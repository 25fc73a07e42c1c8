/*
 * rhj.h -- C-ABI of librhj_hip.so: the MI355X (gfx950) radix hash join engine.
 *
 * This is the drop-in boundary for the hot path of pelekoudasq/radixHashJoin,
 *     void Result::multiRadixHashJoin(JobScheduler&, relation&, relation&)   (Result.h:30, Result.cpp:90-124)
 * and for the job bodies it fans out (HistogramJob / PartitionJob / JoinJob, JobScheduler.cpp:149-192).
 * Plain pointers and sizes only; no HIP, torch or C++ types.  Every entry point cites the reference
 * interface it replaces.  The reference-side binding is shown in INTEGRATION.md; the C++ host mirror
 * of the reference surface that calls this ABI lives in radixhashjoin_amd/host/.
 *
 * Conventions
 *   - all functions return RHJ_OK (0) or a negative rhj_status; rhj_last_error(ctx) has the text.
 *   - "d_" arguments are DEVICE pointers (HBM), everything else is host memory.
 *   - a context owns one HIP stream and a grow-only HBM workspace.  A context is NOT thread-safe:
 *     create one per calling thread, exactly like each query thread of the reference owns a
 *     private JobScheduler (MainScheduler.cpp:6-14).  Different contexts may run concurrently.
 *   - all arithmetic is 64-bit unsigned integer; pair ORDER in outputs is unspecified (SURVEY §8a:
 *     no consumer of Result observes it); the pair MULTISET is bit-exact with the reference.
 */
#ifndef RHJ_H
#define RHJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RHJ_ABI_VERSION 3

/* layout-identical to `struct tuple` (structs.h:33-36): key = rowID, payload = join value */
typedef struct { uint64_t key; uint64_t payload; } rhj_tuple;
/* layout-identical to `struct key_tuple` (Result.h:9-12) */
typedef struct { uint64_t keyR; uint64_t keyS; } rhj_pair;

typedef struct rhj_ctx rhj_ctx;

typedef enum {
    RHJ_OK = 0,
    RHJ_E_INVALID = -1,    /* bad argument */
    RHJ_E_NODEVICE = -2,   /* no usable HIP device */
    RHJ_E_HIP = -3,        /* a HIP call failed (rhj_last_error has hipGetErrorString) */
    RHJ_E_NOMEM = -4,      /* HBM or host allocation failed */
    RHJ_E_OVERFLOW = -5    /* d_out too small: *out_count holds the exact size needed, pairs beyond capacity dropped (slots
                              [0, capacity) hold distinct pairs of the result; nothing at or past capacity is written) */
} rhj_status;

/* Radix plan.  The reference hard-codes one 8-bit pass (HASH_LSB, Result.cpp:5,91); here the
 * number of passes and bits per pass are run-time knobs.  0/0 with passes=-1 = automatic:
 * no partitioning when the smaller input fits one LDS hash table, else the fewest bits such
 * that the average build partition fits one LDS table, split over at most two passes. */
/* WHICH bits.  Inside rhj_join / rhj_join_dev (and the multi-GPU stage calls) the radix digits are bits of
 *     h = rhj_mix64(payload),   a BIJECTIVE 64-bit mix (splitmix64's finaliser),
 * not the raw low payload bits: join values that are multiples of 2^16, share their low bits, or differ only in their high
 * bits would otherwise fall into ONE partition, and a partition far beyond an LDS table is joined in
 * (probe tasks) x (build chunks) table builds -- quadratic where the reference stays linear (its per-bucket table hashes the
 * whole value modulo a prime, Result.cpp:43-58).  The first kernel that touches a caller's tuple replaces the payload by h
 * (histogram digit of h; the scatter writes h); every later kernel compares h, and h == h' <=> payload == payload', so the
 * pair multiset is unchanged and only rowIDs are ever reported.  Cost: one mix per tuple in two HBM-bound kernels.
 * What remains: a join value REPEATED n times on both sides yields n^2 pairs under any plan (so does the reference), and
 * values chosen as rhj_unmix64(k << 16) defeat this fixed mix like any fixed hash; a partition whose build side exceeds the
 * table is then joined in ceil(build / table) x ceil(probe / probe_split) table builds, correctly.
 * The public STAGE calls rhj_histogram / rhj_partition / rhj_partition_at / rhj_bucket_join keep RAW payload bits (their
 * bucket order is the reference's).  rhj_set_option("partition.mix", 0) restores raw bits inside joins (A/B runs, tests). */
uint64_t rhj_mix64(uint64_t x);
uint64_t rhj_unmix64(uint64_t h);      /* rhj_unmix64(rhj_mix64(x)) == x */

typedef struct {
    int32_t passes;        /* -1 auto, 0, 1 or 2 */
    int32_t bits1;         /* radix bits of pass 1 (bits [0,bits1) of h, see above), 1..10; 0 = auto */
    int32_t bits2;         /* radix bits of pass 2 (bits [bits1,bits1+bits2) of h), 1..10; 0 = auto */
    int32_t probe_split;   /* max probe tuples per join task (skew/load balance); 0 = auto; values above 2^24 act as 2^24 */
} rhj_opts;

/* per-kernel device time of the LAST rhj_join / rhj_join_dev / stage call, from HIP events on the
 * context's stream (only filled while profiling is enabled, see rhj_set_profiling). */
typedef enum {
    RHJ_K_HIST = 0,        /* radix histogram           (HistogramJob::run) */
    RHJ_K_SCAN = 1,        /* prefix sums               (PartitionJob::run prefix + structs.cpp:168-173) */
    RHJ_K_SCATTER = 2,     /* scatter-partition         (PartitionJob::run scatter + structs.cpp:183-194) */
    RHJ_K_TASKS = 3,       /* join task list            (the JoinJob scheduling loop, Result.cpp:98-107) */
    RHJ_K_JOIN = 4,        /* bucket build+probe+write  (JoinJob::run / Result::join_buckets / add_result) */
    RHJ_K_AUX = 5,         /* unit tables, memsets, checksum, generators */
    RHJ_K_COUNT = 6
} rhj_kernel_kind;

typedef struct {
    double   ms[RHJ_K_COUNT];        /* summed device ms per kind */
    uint32_t launches[RHJ_K_COUNT];  /* launches per kind */
    double   total_ms;               /* first launch start -> last launch end */
    int32_t  passes, bits1, bits2;   /* the plan that ran */
    uint64_t ntasks;                 /* join tasks executed */
} rhj_timings;

/* ---- lifetime: replaces JobScheduler::init / stop / destroy for the join path
 *      (JobScheduler.cpp:67-86, 140-146, 89-97) --------------------------------------------- */
int  rhj_abi_version(void);
int  rhj_device_count(void);
int  rhj_init(int device, rhj_ctx **out_ctx);
void rhj_destroy(rhj_ctx *ctx);
const char *rhj_last_error(const rhj_ctx *ctx);          /* ctx may be NULL: last global error */
/* run on a caller-owned hipStream_t (e.g. torch's current stream); NULL = context's own stream */
int  rhj_set_stream(rhj_ctx *ctx, void *hip_stream);
/* enabled: 0 off; 1 every launch of a call is timed with a HIP event pair (rhj_get_timings / rhj_get_launch_timings report the
 * LAST call); 2 the same, and the launches of successive calls ACCUMULATE until profiling is set again (a benchmark reads the
 * events once, after its timed loop, instead of after every step) */
int  rhj_set_profiling(rhj_ctx *ctx, int enabled);
/* tuning / test knobs; results never depend on them.  "join.big_tables": -1 (default) choose the bucket-join kernel by
 * the average build partition, 0 always the one-table kernel, 1 always an oversized-partition kernel;
 * "join.big_kernel": -1 automatic, else the bucket-join kernel to use where the plan allows it (the numbers of "last.join_kernel";
 * 4 / 5 over 16-byte partitions run as 8 / 3);
 * "partition.narrow": -1 automatic, 0 never, 1 / 2: inside a join with a two-pass plan, partitions (1) and the
 * intermediate of the two passes (2; the only level of 17-18-bit plans) are stored as {payload 8 B, rowID 4 B} while every
 * rowID is below 2^32 (a larger one is detected on the device -- by the first histogram kernel -- and THAT join repeats itself
 * in the 16-byte format; the next join tries the narrow format again);
 * "partition.countfree": -1 automatic, 0 never, 1 whenever it applies, whatever the size: in a device-resident join whose two
 * passes are narrow (level 2, at most 8 bits each, digits of rhj_mix64(payload)), pass 1 writes every (digit, unit) run into
 * a fixed region instead of at exact cursors, so the histogram read of the 16-byte input is not needed; a relation with a run
 * that does not fit its region (heavy skew) is partitioned again with exact cursors inside the same call, and that side of the
 * context's joins then stays on the exact path for the next 2, 4, ... 32 eligible joins (setting the option re-arms);
 * automatic: relations of more than 2^28 tuples (RHJ_COUNTFREE=0 / 1 in the environment: A/B aid);
 * "partition.countfree2": -1 automatic, 0 never, 1 whenever it applies: in a PAIR join (rhj_join_dev / rhj_join_cols_dev) a side
 * whose pass 1 runs count-free, under a plan whose pass 1 has at least as many buckets as the device has compute units, is
 * written by pass 2 with one workgroup per pass-1 bucket into a fixed region per final partition, so pass 2's histogram and scan
 * are not needed; a side with a final partition that does not fit its region is partitioned again with the pass-2 histogram inside
 * the same call and backs off like "partition.countfree", with a state of its own (setting the option re-arms); same pairs either
 * way; automatic: wherever the automatic count-free pass 1 is on (RHJ_COUNTFREE2=0 / 1 in the environment: A/B aid); every other entry keeps exact boundaries;
 * "partition.mix": -1 automatic (= 1 unless RHJ_MIX=0 is in the environment), 1: joins take their radix digits from
 * rhj_mix64(payload), 0: from the raw payload (see rhj_opts);
 * "join.sniff": -1 automatic (= 1 unless RHJ_SNIFF=0), 1: a partitioned join samples the join values of both relations for
 * duplicates while it counts them, and where the two sides of a partition are within 1/16 of each other in size the side with
 * fewer duplicates becomes the hash table (the reference builds on the smaller bucket, S on a tie: JobScheduler.cpp:187; a table
 * without duplicates answers every probe tuple with one match); 0: the first relation wins such a tie.  Same pairs either way;
 * "sort.max_units": -1 automatic (2048), 1 .. 2048: the most units -- workgroups per launch -- the sort entries cut their input into;
 * a unit is a whole number of tiles of "sort.tile_rows" rows, so 1 makes one workgroup walk every tile (tests: several tiles per unit
 * at a few thousand rows).  Same order either way;
 * "topk.max_candidates": -1 automatic (max(k, "topk.auto_candidates")), 1 .. 2^31 - 1: the top-k entries go on selecting digits
 * while more rows than this are tied with the threshold (tests: 1 runs down every digit).  Same result either way. */
int  rhj_set_option(rhj_ctx *ctx, const char *name, int64_t value);
/* what the last join did: "last.narrow" (0 / 1 / 2, see above), "last.countfree_R" / "last.countfree_S" (pass 1 of that side:
 * 0 exact cursors, 1 count-free, 2 count-free tried and repeated with exact cursors), "last.countfree2_R" / "last.countfree2_S" (pass 2 of
 * that side: 0 histogram and exact cursors, 1 one writer per final partition, 2 tried and repeated with the histogram; 0 after every
 * entry but the pair join), "last.join_kernel" (-1 none: direct small join or empty
 * input; 0 the one-table kernel; 1 the chunked 16-byte-entry kernel; 2 ... 11 the compact-table kernel, one number per geometry:
 * 2 / 3 full / half size, 4 / 5 the same with 20 instead of 16 probe slots per thread (narrow partitions only), 6 / 7 the middle
 * geometry and its half-size form, 8 the full-size table with half the buckets, 9 the half-size middle geometry skipping the slot
 * rows a partition leaves empty, 10 the same with 13-bit arrival indices (keys of up to 51 bits: what plans of 13-15 radix bits take
 * by themselves for partitions of 2-5 K tuples), 11 a smaller table with 12-bit arrival indices (plans of 12 bits); the sizes are
 * the rows of JOIN_GEOM in radixhashjoin_amd/csrc/rhj_internal.h; 12 the semi / anti join kernel: rhj_semi_join_dev /
 * rhj_semi_join_cols_dev, whatever the plan; 13 the aggregating join kernel: rhj_join_sum_dev / rhj_join_sum_cols_dev, whatever
 * the plan; 14 the multiplicity join kernel: rhj_join_mult_dev / rhj_join_mult_cols_dev, whatever the plan; 15 the group-by kernel:
 * rhj_group_sum_dev / rhj_group_sum_cols_dev, whatever the plan; 16 the group-by join kernel: rhj_group_join_dev /
 * rhj_group_join_cols_dev, whatever the plan; the rhj_group_agg_* and rhj_group_join_agg_* entries are 15 and 16 too;
 * 17 the lookup join kernel: rhj_lookup_dev / rhj_lookup_cols_dev, whatever the plan),
 * "last.semi_tables" (the largest number of LDS tables any one task of the last
 * semi / anti join, aggregating join, multiplicity join or lookup join built: 1 when every partition of S fitted one table, 0 when no task ran, and 0 after every other call),
 * "last.group_rounds" (the largest number of LDS table builds any one task of the last group-by or group-by join made: 1 when every
 * partition of R fitted one table, 0 when no task ran, and 0 after every call that is neither; "last.semi_tables" is 0 after both),
 * "last.outer_sweeps" (the anti sweeps the last rhj_outer_join_dev / rhj_outer_join_cols_dev ran: 0, 1 or 2, one per preserved side
 * that had tuples to report on; 0 after every other call.  After an outer join "last.semi_tables" is the largest number of tables any
 * task of those sweeps built -- 0 when no sweep ran a task --, and "last.join_kernel" the pair kernel as rhj_join_cols_dev reports it,
 * 12 when an empty side left only a sweep to run, -1 when nothing ran),
 * "last.sort_bits" / "last.sort_passes" (the key width the last rhj_sort_cols_dev / rhj_sort_dev found and the scatter passes it ran; 0
 * after every other call; "last.join_kernel" is -1 after a sort), "last.sort_units" (the units -- workgroups per launch -- those passes
 * were cut into, each a whole number of tiles; 0 when no pass ran), "sort.tile_rows" (a constant of the build: the rows one workgroup
 * of the sort's scatter ranks at once),
 * "last.topk_bits" / "last.topk_passes" / "last.topk_candidates" / "last.topk_sorted_rows" (what the last rhj_topk_cols_dev /
 * rhj_topk_dev did, see there; 0 after every other call), "topk.auto_candidates" (a constant of the build),
 * "last.window_units" / "last.window_sorts" / "last.window_partitions" (what the last rhj_window_cols_dev did, see there; 0 after
 * every other call), "window.tile_rows" (a constant of the build),
 * "last.asof_units" / "last.asof_sorts" / "last.asof_matched" (what the last rhj_asof_cols_dev did, see there; 0 after every other
 * call), "asof.tile_rows" (a constant of the build),
 * "last.range_join_units" / "last.range_join_sorts" / "last.range_join_pairs" / "last.range_join_expand_tiles" (what the last
 * rhj_range_join_cols_dev / rhj_range_expand_dev did, see there; 0 after every other call), "range_join.tile_rows" /
 * "range_join.expand_tile" (constants of the build),
 * "last.pipelined" (the number
 * of S chunks the last rhj_join streamed through the device while finished pairs travelled home, also when no pair came of
 * them; 0: the plain path, which a join abandoned on the pipelined path -- a rowID that does not fit the narrow format, more pairs
 * than the optimistic page of max(nR, nS) + 1024 holds -- has taken too),
 * "last.max_part_R" / "last.max_part_S" (tuples in the largest partition of each side the last partitioned join saw; 0 for
 * an unpartitioned one), "last.cols_R" / "last.cols_S" (how the last join read that side: 0 it was not a columnar call -- every join
 * and stage call other than rhj_join_cols_dev leaves 0, as does a columnar call with an empty side; 1 the partition kernels read the side's column(s) directly; 2 the side was first
 * materialised as 16-byte tuples in the workspace; see rhj_join_cols_dev for which plans are direct),
 * "partition.mix" (0 / 1: what joins on this context do) */
int  rhj_get_info(rhj_ctx *ctx, const char *name, int64_t *value);
int  rhj_get_timings(rhj_ctx *ctx, rhj_timings *out);
/* the same per LAUNCH, in launch order: kinds[i] (rhj_kernel_kind) and ms[i] of the first min(*n, capacity) timed spans of the
 * last call; *n = how many there were.  (A fused two-pass join scatters R pass 1, R pass 2, S pass 1, S pass 2 in that order:
 * bench.py prices the two scatter variants separately with this.) */
int  rhj_get_launch_timings(rhj_ctx *ctx, int32_t *kinds, double *ms, uint32_t capacity, uint32_t *n);
int  rhj_sync(rhj_ctx *ctx);                             /* JobScheduler::barrier (JobScheduler.cpp:103-122) */
/* pre-size / release the HBM workspace (otherwise grown on demand) */
int  rhj_reserve(rhj_ctx *ctx, uint64_t nR, uint64_t nS, const rhj_opts *opts);
int  rhj_release_workspace(rhj_ctx *ctx);
void rhj_default_opts(rhj_opts *opts);
/* the plan rhj_join would use for these sizes (host logic only, no device needed).  rhj_join_dev plans the same
 * except for build sides of 21 K - 51 K tuples, which it partitions with one pass where rhj_join stays unpartitioned
 * (one launch matters more when the inputs still have to cross PCIe); rhj_get_timings reports the plan that ran. */
int  rhj_plan(uint64_t nR, uint64_t nS, const rhj_opts *in, rhj_opts *resolved);

/* ---- the drop-in: replaces the body of Result::multiRadixHashJoin (Result.cpp:90-124) ----
 * Host AoS in, one result page out.  *out_page is NULL when there is no match (Result::isEmpty,
 * Result.cpp:16-18) else a malloc() block laid out like one reference result page
 * (Result.cpp:21-35): 8 bytes `next` pointer (= NULL) followed by *out_count rhj_pair.
 * The caller owns it and releases it with free() (as ~Result does, Result.cpp:127-133).
 * Inputs are neither modified nor retained. */
int rhj_join(rhj_ctx *ctx, const rhj_tuple *R, uint64_t nR, const rhj_tuple *S, uint64_t nS,
             const rhj_opts *opts, void **out_page, uint64_t *out_count);

/* ---- several joins in one call (MainScheduler.cpp:6-30 / join.cpp:42-50 keep 8 queries in flight) -------------
 * out_pages[i] / out_counts[i] are what rhj_join(ctx, joins[i].R, .., NULL, &page, &count) would return, for every i.  Joins small
 * enough for the one-launch path (every join of small.work: <= 43 K tuples) run SIXTEEN PER LAUNCH: their inputs are staged
 * into one pinned buffer by a few helper threads and cross PCIe in one copy, one kernel launch joins them (grid.y = join), the
 * pairs land in pinned host memory written by the kernel itself, one synchronisation -- instead of two copies, a launch and a
 * synchronisation per join.  Larger joins of the list take the rhj_join path one by one.  On an error every page already
 * produced is freed and all counts are zero. */
typedef struct { const rhj_tuple *R; uint64_t nR; const rhj_tuple *S; uint64_t nS; } rhj_join_desc;
int rhj_join_batch(rhj_ctx *ctx, uint32_t n, const rhj_join_desc *joins, void **out_pages, uint64_t *out_counts);

/* ---- device-resident variant (inputs/outputs already in HBM).  d_out may be NULL with
 * out_capacity 0 to count only.  Returns RHJ_E_OVERFLOW (and the exact *out_count) when
 * out_capacity is too small; call again with a larger buffer. */
int rhj_join_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                 const rhj_opts *opts, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count);

/* ---- rhj_join_dev with each relation given as COLUMNS in HBM: d_val?[i] = join value of tuple i, d_id?[i] = its rowID, or
 * d_id? == NULL: rowID = i (a stored, unfiltered relation; a torch tensor of keys).  Same pair multiset, count-only mode,
 * RHJ_E_OVERFLOW contract, plan / options / timings / "last.*" reporting as rhj_join_dev on the tuples {id[i] or i, val[i]}.
 * The two sides are independent (one may carry ids, the other not).  A side with n == 0: count 0; a NULL value column with
 * n > 0: RHJ_E_INVALID.  Inputs are neither modified nor retained.
 * DIRECT plans ("last.cols_*" == 1): every two-pass plan of at most 8 + 8 bits that runs in a narrow format ("partition.narrow"
 * level 1 or 2: automatically from 8 * 10^6 tuples on the larger side, rowIDs below 2^32) -- the first kernels of the partition
 * (the two-pass histogram, pass 1 with exact cursors or count-free, on one stream or two) read the value column, 8 B per tuple,
 * and the id column as a second 8-byte stream, or nothing at all for NULL ids; a side that is partitioned again after a
 * count-free overflow is read from its columns again.  MATERIALISED ("last.cols_*" == 2): unpartitioned and direct joins,
 * one-pass plans, two-pass plans in the 16-byte format, 17-18-bit plans, and the 16-byte repeat of a join that met a rowID
 * >= 2^32: one linear kernel writes the side as 16-byte tuples into a grow-only workspace buffer (rhj_release_workspace frees
 * it), only for the side and at the moment a path asks, and the join continues exactly as rhj_join_dev. */
int rhj_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                      const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
                      const rhj_opts *opts, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count);

/* ---- semi-join and anti-join: WHICH tuples of R have a partner in S at all (RHJ_SEMI: EXISTS, isin on key columns, semi-join
 * reduction) or have none (RHJ_ANTI: NOT EXISTS; for a left, right or full outer join see rhj_outer_join_cols_dev).  R as columns
 * exactly as in rhj_join_cols_dev (d_idR == NULL: rowID = i); S is its value column alone: S has no id column, its rowIDs never
 * reach the result.
 * Output: d_out_ids receives the rowID (id[i], or i for a NULL id column; .key for tuples) of every tuple of R that qualifies, each
 * tuple exactly ONCE whatever the multiplicity of its value in S (a value repeated 10^4 times on both sides: 10^4 ids, not the 10^8
 * pairs of the inner join); two tuples of R with the same value are two tuples, and both are reported.  Order is unspecified.
 * d_out_ids == NULL with out_capacity 0 counts only.  Returns RHJ_E_OVERFLOW (and the exact *out_count) when out_capacity is too
 * small: slots [0, capacity) then hold distinct ids of the result, and nothing at or past capacity is written.
 * nR == 0: count 0.  nS == 0: count 0 for RHJ_SEMI, all nR ids for RHJ_ANTI.  A NULL value column (relation) with n > 0, or a kind
 * other than the two below: RHJ_E_INVALID.  Inputs are neither modified nor retained.
 * Plan, options, timings, "last.narrow", "last.countfree_*" and "last.cols_*" as rhj_join_cols_dev / rhj_join_dev on the same sizes
 * (same partition kernels, same repeats after a count-free overflow or a rowID >= 2^32 of R in a narrow format), except that a
 * one-pass plan always runs as separate partition and join launches; "last.join_kernel" is 12, "last.semi_tables" see rhj_get_info.
 * rhj_opts.probe_split above 32768 acts as 32768 (a task keeps one match bit per tuple of R in LDS). */
#define RHJ_SEMI 0   /* R tuples whose join value occurs in S          */
#define RHJ_ANTI 1   /* R tuples whose join value does not occur in S  */
int rhj_semi_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *d_valS, uint64_t nS, int kind, const rhj_opts *opts,
                           uint64_t *d_out_ids, uint64_t out_capacity, uint64_t *out_count);
/* ... on 16-byte tuples (the .key of S's tuples is not looked at) */
int rhj_semi_join_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                      int kind, const rhj_opts *opts,
                      uint64_t *d_out_ids, uint64_t out_capacity, uint64_t *out_count);

/* ---- outer joins: the pairs of rhj_join_cols_dev and, behind them, one row per tuple of a PRESERVED side whose join value does not
 * occur on the other side, the missing rowID being RHJ_NO_ROW (LEFT / RIGHT / FULL OUTER JOIN; merge(how="left" / "right" / "outer")).
 * Both sides are partitioned ONCE; the pair join runs, then one anti sweep (the kernel of rhj_semi_join_cols_dev, writing 16-byte
 * rows) per preserved side over the same partitions, on the same stream and the same result counter.
 * how: RHJ_OUTER_LEFT (bit 0) keeps the tuples of R without a partner in S as {rowR, RHJ_NO_ROW}; RHJ_OUTER_RIGHT (bit 1) those of S
 * without a partner in R as {RHJ_NO_ROW, rowS}; RHJ_OUTER_FULL both.  Each such tuple is reported ONCE: two tuples of R with the same
 * unmatched value are two rows.  The matched rows are the pair multiset of rhj_join_cols_dev on the same inputs.  Relations as
 * columns exactly as in rhj_join_cols_dev (a NULL id column: rowID = index; the two sides are independent); a caller's rowID that is
 * itself all ones cannot be told from RHJ_NO_ROW.
 * Sections: *out_count is the total; out_sections, a HOST array of three words that may be NULL, receives {matched, R-only, S-only},
 * a section the mode does not ask for being 0.  In d_out the matched pairs occupy [0, matched), the R-only rows
 * [matched, matched + R-only), the S-only rows come behind them: a caller slices instead of scanning for RHJ_NO_ROW.  Order inside a
 * section is unspecified.
 * d_out == NULL with out_capacity 0 counts only.  Returns RHJ_E_OVERFLOW when out_capacity is too small: *out_count and out_sections
 * are exact, slots [0, capacity) hold distinct rows of the result in the section layout above, nothing at or past capacity is written.
 * nR == 0: under bit 1 every tuple of S as {RHJ_NO_ROW, rowS}, otherwise 0 rows; nS == 0: symmetric; both 0: 0 rows, no launch.
 * how outside 1..3, a NULL out_count, a NULL value column (relation) with n > 0: RHJ_E_INVALID.  Inputs are neither modified nor
 * retained.
 * Plan, options, timings, "last.narrow", "last.countfree_*", "last.cols_*" and "last.max_part_*" as rhj_join_cols_dev / rhj_join_dev on
 * the same sizes (same partition kernels, same repeats after a count-free overflow or a rowID >= 2^32 in a narrow format: a repeat
 * starts from a zeroed counter and produces every section again), except that a one-pass plan always runs as separate partition and
 * join launches; rhj_timings.ntasks counts the tasks of the pair join and of the sweeps together, RHJ_K_TASKS / RHJ_K_JOIN include the
 * sweeps; "last.join_kernel", "last.outer_sweeps" and "last.semi_tables" see rhj_get_info.  In a sweep rhj_opts.probe_split above
 * 32768 acts as 32768.  An empty side: the other side is swept unpartitioned, without a partition phase. */
#define RHJ_NO_ROW      0xFFFFFFFFFFFFFFFFull   /* the missing side of an unmatched row: all ones, -1 as int64 (as the group ids' "no group") */
#define RHJ_OUTER_LEFT  1   /* bit 0: keep the tuples of R without a partner in S */
#define RHJ_OUTER_RIGHT 2   /* bit 1: keep the tuples of S without a partner in R */
#define RHJ_OUTER_FULL  3
int rhj_outer_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                            const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS, int how, const rhj_opts *opts,
                            rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count, uint64_t *out_sections);
/* ... on 16-byte tuples (value = .payload, rowID = .key) */
int rhj_outer_join_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, int how,
                       const rhj_opts *opts, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count, uint64_t *out_sections);

/* ---- aggregating join: COUNT(*) and SUM(column of R) over R join S without producing the pairs (SELECT COUNT(*), SUM(r.x) FROM R JOIN
 * S USING (key)).  For a join value repeated n times on both sides the pair set holds n^2 pairs; this call reads both relations once
 * and keeps, beside every key of S in the join kernel's table, how often it occurs. */
#define RHJ_SUM_MAX_COLS 4
/* count = |R join S| and, for j < ncols, sums[j] = sum over the pairs of d_cols[j][rowR]  (mod 2^64), without producing the pairs:
 * linear in nR + nS whatever the multiplicity of a join value.  R as columns exactly as rhj_join_cols_dev (d_idR == NULL: rowID = i);
 * S is its value column alone.  d_cols: HOST array of ncols DEVICE columns, each col_rows uint64 long, indexed by R's rowID;
 * a rowID >= col_rows is never dereferenced: RHJ_E_INVALID.  out_count / out_sums: HOST words; the call synchronises.
 * ncols == 0 is a pure COUNT(*): d_cols, out_sums and col_rows are ignored.  RHJ_E_INVALID: ncols > RHJ_SUM_MAX_COLS, a NULL
 * column (or NULL d_cols / out_sums) with ncols > 0, a NULL value column (relation) with n > 0, NULL out_count.  nR == 0 or nS == 0:
 * count 0 and all sums 0, no launch.  The sums over columns of S's side are the same call with the sides exchanged.
 * Plan, options, timings, "last.narrow", "last.countfree_*" and "last.cols_*" as rhj_join_cols_dev / rhj_join_dev on the same sizes
 * (same partition kernels, same repeats after a count-free overflow or a rowID >= 2^32 of R in a narrow format; a repeat starts its
 * sums from zero), except that a one-pass plan always runs as separate partition and join launches; "last.join_kernel" is 13,
 * "last.semi_tables" see rhj_get_info.  rhj_opts.probe_split: values above 2^24 act as 2^24.  Results are bit-exact from run to
 * run (integer addition does not depend on the order).  Inputs are neither modified nor retained. */
int rhj_join_sum_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                          const uint64_t *d_valS, uint64_t nS, const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows,
                          const rhj_opts *opts, uint64_t *out_count, uint64_t *out_sums);
/* ... on 16-byte tuples (rowR = .key; the .key of S's tuples is not looked at) */
int rhj_join_sum_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                     const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows,
                     const rhj_opts *opts, uint64_t *out_count, uint64_t *out_sums);

/* ---- multiplicity join: for every row of R, how many tuples of S carry its join value -- or, with weights on S, the sum of their
 * weights (SELECT r.id, SUM(s.w) FROM R JOIN S USING (key) GROUP BY r.id; the degree of every key; value_counts looked up per row).
 * It is what rhj_join_sum_cols_dev adds up, returned per row, and the message of a sum over a tree-shaped query: a chain or star
 * of joins is summed by at most 2 x (aliases - 1) such calls, linear in the inputs, with no pair set.
 *
 * for every tuple i of R:  d_out[rowR_i] += sum over the tuples j of S with valS[j] == valR[i] of w_j   (mod 2^64)
 * w_j = d_wS[rowS_j], or 1 when d_wS == NULL.  rowR_i = d_idR[i] or i; rowS_j = d_idS[j] or j (id column NULL).
 * Zeroing: the call zeroes all out_rows words of d_out itself, and does so again on every attempt.
 * Accumulation: every tuple of R then ADDS its multiplicity to d_out[rowR]: two tuples of R with the same rowID accumulate, words
 * that no tuple of R names stay 0.
 * out_total: a HOST word that receives the sum of all multiplicities mod 2^64 -- |R join S| when unweighted, the number
 * rhj_join_sum_cols_dev counts.  The call synchronises: d_out and *out_total are complete when it returns.
 * Guards: a rowR >= out_rows is never stored to and a rowS >= wS_rows is never loaded from (weighted only; wS_rows is ignored when
 * d_wS == NULL): either raises a flag word in HBM and the call returns RHJ_E_INVALID (d_out is then undefined, the context stays
 * usable).  The flag is raised for every such tuple whose partition holds tuples of the other side -- always when it has a
 * partner there.
 * nR == 0 or nS == 0: d_out all zero, total 0, no join launch.  RHJ_E_INVALID: NULL d_out with out_rows > 0, NULL out_total, a
 * NULL value column (relation) with n > 0.  Inputs are neither modified nor retained; d_out must not overlap them.
 * Plan, options, timings, "last.narrow", "last.countfree_*" and "last.cols_*" as rhj_join_cols_dev / rhj_join_dev on the same sizes
 * (same partition kernels, same repeats: a count-free overflow repeats with exact cursors, a rowID >= 2^32 of EITHER side in a
 * narrow format repeats at 16 bytes -- S's rowIDs are read here --, and a repeat starts from a zeroed d_out), except that a
 * one-pass plan always runs as separate partition and join launches; "last.join_kernel" is 14, "last.semi_tables" see
 * rhj_get_info.  rhj_opts.probe_split: values above 2^24 act as 2^24.  Results are bit-exact from run to run. */
int rhj_join_mult_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
                           const uint64_t *d_wS, uint64_t wS_rows, const rhj_opts *opts,
                           uint64_t *d_out, uint64_t out_rows, uint64_t *out_total);
/* ... on 16-byte tuples (rowR = d_R[i].key, rowS = d_S[j].key) */
int rhj_join_mult_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
                      const uint64_t *d_wS, uint64_t wS_rows, const rhj_opts *opts,
                      uint64_t *d_out, uint64_t out_rows, uint64_t *out_total);

/* ---- lookup join: for every row of R ONE partner row of S, aligned with R, and no pair set -- the foreign key of R looked up in a
 * unique or nearly unique key of S (pandas.Index.get_indexer, Series.map, merge(how="left") against a dimension table, a dictionary
 * lookup).  The multiplicity join's kernel shape with a rowID instead of a weight sum in the word beside every key.
 *
 * for every tuple i of R with at least one partner in S:
 *     d_out[rowR_i] = min (RHJ_LOOKUP_FIRST) / max (RHJ_LOOKUP_LAST) of its old value and the rowS_j of the tuples j of S with
 *     valS[j] == valR[i]
 * rowR_i = d_idR[i] or i; rowS_j = d_idS[j] or j (id column NULL).
 * Initialisation: the call sets all out_rows words of d_out to RHJ_NO_ROW itself, and does so again on every attempt.
 * Update: monotone, never a plain store: two tuples of R with the same rowID leave the min / max over both tuples' partners; a word
 * that no matched tuple of R names stays RHJ_NO_ROW (all ones, -1 as int64).
 * out_matched: a HOST word that receives the number of words of d_out that ended different from RHJ_NO_ROW -- exact, also with
 * repeated rowIDs of R and with a key of S spread over several LDS tables.  The call synchronises: d_out and *out_matched are
 * complete when it returns.  With unique rowIDs of R, *out_matched == the total of rhj_join_mult_cols_dev on the same inputs says
 * that no row of R has two partners (validate="m:1").
 * Guards: a rowR >= out_rows is never stored to; under RHJ_LOOKUP_LAST a rowS >= 2^63 -- which a signed maximum cannot order -- is
 * never inserted: either raises a flag word in HBM and the call returns RHJ_E_INVALID, each with its own message (d_out is then
 * undefined, the context stays usable).  The flag is raised for every such tuple whose partition holds tuples of the other side --
 * always when it has a partner there.  Under RHJ_LOOKUP_FIRST every rowS is ordered, but a rowS that is itself all ones cannot be
 * told from RHJ_NO_ROW (as in the outer join): such a partner counts as none.
 * nR == 0 or nS == 0: d_out all ones, matched 0, no join launch.  RHJ_E_INVALID: which outside 0..1, NULL d_out with out_rows > 0,
 * NULL out_matched, a NULL value column (relation) with n > 0.  Inputs are neither modified nor retained; d_out must not overlap them.
 * Plan, options, timings, "last.narrow", "last.countfree_*", "last.cols_*" and the repeats as rhj_join_mult_cols_dev on the same
 * sizes (S's id column goes through the partition phase: its rowIDs are read; a rowID >= 2^32 of EITHER side in a narrow format
 * repeats at 16 bytes, a count-free overflow with exact cursors, and a repeat starts from a d_out of all ones); a one-pass plan always
 * runs as separate partition and join launches; "last.join_kernel" is 17, "last.semi_tables" see rhj_get_info.  Results are
 * bit-exact from run to run. */
#define RHJ_LOOKUP_FIRST 0      /* the smallest rowS among the partners */
#define RHJ_LOOKUP_LAST  1      /* the largest */
#define RHJ_LOOKUP_MAX_COLS 4   /* columns per rhj_gather_cols_fill call */
int rhj_lookup_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                        const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS, int which, const rhj_opts *opts,
                        uint64_t *d_out, uint64_t out_rows, uint64_t *out_matched);
/* ... on 16-byte tuples (rowID = .key, value = .payload) */
int rhj_lookup_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, int which,
                   const rhj_opts *opts, uint64_t *d_out, uint64_t out_rows, uint64_t *out_matched);

/* ---- group-by on a key column: one output row per DISTINCT join value of R -- the value, how many tuples carry it, and up to four
 * sums over those tuples (SELECT key, COUNT(*), SUM(x) FROM R GROUP BY key; value_counts; torch.unique + index_add_).  One relation:
 * R goes through the partition phase of the joins, then one workgroup per partition keeps its distinct keys in an LDS table with a
 * 64-bit word beside every key. */
#define RHJ_GROUP_MAX_COLS 4
/* one output row per DISTINCT join value of R: the value, how many tuples carry it, and for j < ncols the sum over those tuples of
 * d_cols[j][rowR] (mod 2^64)
 * R as columns exactly as rhj_join_cols_dev: rowR = d_idR[i], or i when d_idR == NULL (rowID = index).  Ids are partitioned with the
 * values whenever they are given, also with ncols == 0.
 * Output: group g is the triple d_out_keys[g], d_out_counts[g], d_out_sums[j][g].  d_out_keys[g] is the caller's value, not rhj_mix64
 * of it.  The ORDER of groups is unspecified; the SET of groups is exact and the same from run to run (so is every count and sum:
 * integer addition does not depend on the order).  d_out_sums: HOST array of ncols DEVICE columns, each out_capacity words long;
 * d_cols: HOST array of ncols DEVICE columns, each col_rows words long, indexed by R's rowID, as in rhj_join_sum_cols_dev.
 * out_groups: a HOST word; the call synchronises.
 * Count only: d_out_keys == NULL with out_capacity == 0 counts the distinct values only -- no sum sweep runs and d_cols is never
 * read.  With a non-NULL d_out_keys, d_out_counts may be NULL and is then not written.
 * Overflow: RHJ_E_OVERFLOW with the exact *out_groups when out_capacity is too small: slots [0, capacity) of every output array then
 * hold complete, distinct groups of the result, and nothing at or past capacity is written.
 * Row guard: a rowR >= col_rows is never dereferenced: it raises a flag word in HBM and the call returns RHJ_E_INVALID, for every such
 * tuple the kernel sees (ncols > 0 and not count-only: otherwise no column is read and col_rows is ignored).  The outputs are then
 * undefined; the context stays usable.
 * nR == 0: 0 groups, no launch.  RHJ_E_INVALID: ncols > RHJ_GROUP_MAX_COLS; a NULL d_cols, d_out_sums or column with ncols > 0 and a
 * non-NULL d_out_keys; a NULL value column (relation) with nR > 0; NULL out_groups; NULL d_out_keys with out_capacity > 0.
 * Plan: the one rhj_plan(nR, nR, ...) resolves for a device-resident join -- R is planned as an aggregating join with itself would
 * be.  rhj_opts.probe_split is ignored: a partition is never cut (one task per non-empty partition, the whole partition; a partition
 * of >= 2^32 tuples: RHJ_E_INVALID, use more radix bits).  Options, timings, "last.narrow", "last.countfree_R" and "last.cols_R" as
 * rhj_join_cols_dev / rhj_join_dev on (nR, nR) -- same partition kernels, same repeats: a count-free overflow repeats with exact
 * cursors, a rowID >= 2^32 in a narrow format repeats at 16 bytes, and every attempt starts from a zeroed group counter --, except
 * that a one-pass plan always runs as separate partition and group launches; "last.countfree_S" and "last.cols_S" are 0 (there is no
 * S: no second relation-sized buffer is allocated or touched); "last.join_kernel" is 15; "last.group_rounds" see rhj_get_info;
 * "last.semi_tables" is 0.
 * Costs to know: a partition is one workgroup's work, so one value repeated n times is summed by one workgroup -- linear
 * in n, not balanced across the chip; a partition with D distinct keys beyond one table costs about 2 D / 4608 sweeps of itself.
 * Inputs are neither modified nor retained (an unpartitioned plan reads the 16-byte array in place); outputs must not overlap them. */
int rhj_group_sum_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                           uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_sums,
                           uint64_t out_capacity, uint64_t *out_groups);
/* ... on 16-byte tuples (value = .payload, rowR = .key) */
int rhj_group_sum_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                      const uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const rhj_opts *opts,
                      uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t *const *d_out_sums,
                      uint64_t out_capacity, uint64_t *out_groups);

/* ---- join with GROUP BY on the key: one output row per join value of R join S -- the value, how many tuples of each side carry it,
 * and up to four sums per side over those tuples (SELECT key, COUNT(*), SUM(r.a), SUM(s.b) FROM R JOIN S USING (key) GROUP BY key, and
 * the LEFT JOIN form; the per-key degree product of a join; intersect1d with counts).  No pair is formed: both relations go through
 * the partition phase of the joins, then one workgroup per partition keeps R's distinct keys in an LDS table with a 64-bit word beside
 * every key, and S looks its keys up. */
#define RHJ_GJ_INNER 0      /* one row per join value that occurs in R and in S */
#define RHJ_GJ_LEFT  1      /* one row per distinct join value of R; cntS may be 0 */
#define RHJ_GROUP_JOIN_MAX_COLS 4      /* per side */
/* R and S as columns exactly as rhj_join_mult_cols_dev: rowR = d_idR[i], or i when d_idR == NULL (rowID = index); rowS likewise.  Ids
 * are partitioned with the values whenever they are given, also with no column.
 * Raw per-side results: group g is d_out_keys[g], d_out_cntR[g], d_out_cntS[g], d_out_sumsR[j][g], d_out_sumsS[j][g].  d_out_keys[g] is
 * the caller's value, not rhj_mix64 of it.  cntR[g] is the number of tuples of R with that value, cntS[g] the number of tuples of S;
 * sumsR[j][g] is the sum over those tuples of R of d_colsR[j][rowR] (mod 2^64), sumsS[j][g] the sum over those tuples of S of
 * d_colsS[j][rowS].  The SQL aggregates over the pairs of the group are products of these (mod 2^64):
 *     COUNT(*) = cntR·cntS        SUM(r.a) = sumsR·cntS        SUM(s.b) = sumsS·cntR
 * The raw values are returned so that a caller can also form averages or per-side counts.
 * Modes: RHJ_GJ_INNER emits the values present on both sides; RHJ_GJ_LEFT emits every distinct value of R, with cntS and sumsS 0
 * where S has none (a LEFT JOIN's unmatched row counts once: the caller multiplies by max(cntS, 1)).
 * The ORDER of groups is unspecified; the SET of groups, every count and every sum are exact and bit-identical from run to run
 * (integer addition does not depend on the order).  d_out_sumsR / d_out_sumsS: HOST arrays of ncolsR / ncolsS DEVICE columns, each
 * out_capacity words long; d_colsR / d_colsS: HOST arrays of ncolsR / ncolsS DEVICE columns, each colR_rows / colS_rows words long,
 * indexed by the side's rowID, as in rhj_join_sum_cols_dev.  out_groups: a HOST word; the call synchronises.
 * Count only: d_out_keys == NULL with out_capacity == 0 counts the groups only -- no sum sweep runs and no column is read.  With a
 * non-NULL d_out_keys, d_out_cntR and d_out_cntS may each be NULL and are then not written.
 * Overflow: RHJ_E_OVERFLOW with the exact *out_groups when out_capacity is too small: slots [0, capacity) of every output array then
 * hold complete, distinct groups of the result, and nothing at or past capacity is written.
 * Row guard: a rowR >= colR_rows or a rowS >= colS_rows is never dereferenced: it raises a flag word in HBM and the call returns
 * RHJ_E_INVALID with a message that says which side, for every such tuple a sum sweep meets (the side has columns and the call is
 * not count-only: otherwise no column of that side is read and its *_rows is ignored; a partition no task is made for, and a class
 * of keys that emits no group, get no sum sweep).  The outputs are then undefined; the context stays usable.
 * Empty sides: nR == 0: 0 groups, no launch.  nS == 0: RHJ_GJ_INNER gives 0 groups, no launch; RHJ_GJ_LEFT gives the group-by of R
 * with zero S fields (R alone is partitioned, under the plan of rhj_group_sum_cols_dev).
 * RHJ_E_INVALID: a mode that is neither RHJ_GJ_INNER nor RHJ_GJ_LEFT; ncolsR or ncolsS > RHJ_GROUP_JOIN_MAX_COLS; with ncolsR > 0
 * and a non-NULL d_out_keys a NULL d_colsR, d_out_sumsR or column of either, and the same for S's side; a NULL value column
 * (relation) with a non-zero row count; NULL out_groups; NULL d_out_keys with out_capacity > 0.
 * Plan: the one rhj_plan(nR, nS, ...) resolves for a device-resident join.  rhj_opts.probe_split is ignored: a partition is never
 * cut (one task per partition, both whole partitions; a partition of >= 2^32 tuples on either side: RHJ_E_INVALID,
 * use more radix bits).  Options, timings, "last.narrow", "last.countfree_*" and "last.cols_*" as rhj_join_mult_cols_dev / rhj_join_mult_dev on the
 * same sizes -- same partition kernels, same repeats; both sides' ids are read, so a rowID >= 2^32 on either side in a narrow format
 * repeats at 16 bytes, a count-free overflow repeats with exact cursors, and every attempt starts from a zeroed group counter and
 * flag word; "last.join_kernel" is 16; "last.group_rounds" see rhj_get_info; "last.semi_tables" is 0.
 * Costs to know: a partition is one workgroup's work; partitions are read 1 + ncols times per side and class; the
 * table is always built on R, so under RHJ_GJ_INNER an R with many more distinct values than S pays class walks that the call with
 * the sides exchanged would not.
 * Inputs are neither modified nor retained (an unpartitioned plan reads 16-byte arrays in place); outputs must not overlap them. */
int rhj_group_join_cols_dev(rhj_ctx *ctx,
        const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
        const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
        const uint64_t *const *d_colsR, uint32_t ncolsR, uint64_t colR_rows,
        const uint64_t *const *d_colsS, uint32_t ncolsS, uint64_t colS_rows,
        int mode, const rhj_opts *opts,
        uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
        uint64_t *const *d_out_sumsR, uint64_t *const *d_out_sumsS,
        uint64_t out_capacity, uint64_t *out_groups);
/* ... on 16-byte tuples (value = .payload, rowID = .key) */
int rhj_group_join_dev(rhj_ctx *ctx,
        const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
        const uint64_t *const *d_colsR, uint32_t ncolsR, uint64_t colR_rows,
        const uint64_t *const *d_colsS, uint32_t ncolsS, uint64_t colS_rows,
        int mode, const rhj_opts *opts,
        uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
        uint64_t *const *d_out_sumsR, uint64_t *const *d_out_sumsS,
        uint64_t out_capacity, uint64_t *out_groups);

/* ---- MIN and MAX beside SUM: the two group-by entries and the two group-by join entries with an aggregate PER COLUMN (SELECT key,
 * MIN(x), MAX(x), SUM(y) FROM R GROUP BY key; first and last timestamp per key; scatter_reduce_(amin / amax) keyed by value).  The same
 * kernels' families, tables, class walk and host path: a minimum or maximum is the column sweep of a sum with another
 * LDS atomic and another starting word. */
#define RHJ_AGG_SUM     0   /* sum mod 2^64 (what rhj_group_sum_* / rhj_group_join_* compute) */
#define RHJ_AGG_MIN_U64 1   /* minimum / maximum of the column words as unsigned 64-bit ... */
#define RHJ_AGG_MAX_U64 2
#define RHJ_AGG_MIN_I64 3   /* ... and as two's-complement signed 64-bit */
#define RHJ_AGG_MAX_I64 4
/* rhj_group_sum_cols_dev with ops: a HOST array of ncols words, column j is aggregated with ops[j] (an RHJ_AGG_*), and
 * d_out_aggs[j][g] is that aggregate of d_cols[j][rowR] over the tuples of group g.  ops == NULL: every column is RHJ_AGG_SUM.  The
 * same column pointer may appear twice with different ops (MIN and MAX of one column in one call).  A group has at least one tuple,
 * so its minimum / maximum is always a column value.  A call whose ops are all RHJ_AGG_SUM returns what rhj_group_sum_cols_dev
 * returns, bit for bit.
 * Everything else is the contract of rhj_group_sum_cols_dev, word for word: the order of groups is unspecified, the set and every
 * value exact and bit-identical from run to run (minimum and maximum do not depend on the order either); count only with a NULL
 * d_out_keys and out_capacity 0 -- no sweep, no column read --; RHJ_E_OVERFLOW with the exact *out_groups, complete distinct groups
 * in [0, capacity) and nothing at or past capacity written; the row guard (a rowR >= col_rows is never dereferenced, under any op);
 * nR == 0; plans, repeats, probe_split ignored; "last.join_kernel" is 15, "last.group_rounds" as there.
 * RHJ_E_INVALID beyond that contract's: an ops[j] above RHJ_AGG_MAX_I64 -- checked before any launch, also in a count-only call;
 * rhj_last_error names the column.
 * Costs: those of rhj_group_sum_cols_dev, whatever the ops -- one sweep of the partition per column and class, one workgroup per
 * partition. */
int rhj_group_agg_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows,
                           const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                           uint64_t *const *d_out_aggs, uint64_t out_capacity, uint64_t *out_groups);
/* ... on 16-byte tuples (value = .payload, rowR = .key) */
int rhj_group_agg_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                      const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows,
                      const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                      uint64_t *const *d_out_aggs, uint64_t out_capacity, uint64_t *out_groups);
/* rhj_group_join_cols_dev with opsR / opsS: HOST arrays of ncolsR / ncolsS words (NULL: every column of that side is RHJ_AGG_SUM).
 * The RAW per-side value is returned, as for sums: d_out_aggsR[j][g] is opsR[j] over the tuples of R with the group's value,
 * d_out_aggsS[j][g] is opsS[j] over the tuples of S.  A minimum or maximum over the PAIRS of a group is the per-side one as it stands
 * (MIN(r.a) over the pairs is the minimum over R's tuples: no product with the other side's count, unlike a sum).
 * Identity rule: under RHJ_GJ_LEFT a group with cntS == 0 has no tuple of S to take a minimum or maximum of; its MIN / MAX columns of
 * S hold the op's identity -- RHJ_AGG_MIN_U64: 0xFFFFFFFFFFFFFFFF, RHJ_AGG_MAX_U64: 0, RHJ_AGG_MIN_I64: INT64_MAX
 * (0x7FFFFFFFFFFFFFFF), RHJ_AGG_MAX_I64: INT64_MIN (0x8000000000000000) -- and its RHJ_AGG_SUM columns of S stay 0.  cntS tells the
 * caller which rows these are (cntS == 0: SQL's NULL).  Under RHJ_GJ_INNER both counts of every group are non-zero and every
 * minimum / maximum is a column value.
 * Everything else is the contract of rhj_group_join_cols_dev, word for word (modes, count only, RHJ_E_OVERFLOW, the row guard and
 * its message that says which side, nR == 0 / nS == 0 -- RHJ_GJ_LEFT over an empty S: the group-by of R, S's columns at the identity
 * of their op --, plans, repeats, probe_split ignored, "last.join_kernel" is 16, "last.group_rounds").  A call whose ops are all
 * RHJ_AGG_SUM returns what rhj_group_join_cols_dev returns, bit for bit.
 * RHJ_E_INVALID beyond that contract's: an opsR[j] or opsS[j] above RHJ_AGG_MAX_I64 -- checked before any launch, also in a
 * count-only call; rhj_last_error names the side and the column.
 * Costs: those of rhj_group_join_cols_dev, whatever the ops. */
int rhj_group_join_agg_cols_dev(rhj_ctx *ctx,
        const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
        const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
        const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
        const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
        int mode, const rhj_opts *opts,
        uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
        uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
        uint64_t out_capacity, uint64_t *out_groups);
/* ... on 16-byte tuples (value = .payload, rowID = .key) */
int rhj_group_join_agg_dev(rhj_ctx *ctx,
        const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
        const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
        const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
        int mode, const rhj_opts *opts,
        uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
        uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
        uint64_t out_capacity, uint64_t *out_groups);

/* ---- group ids per row: the INVERSE INDEX of the group-by and of the group-by join (torch.unique's return_inverse; pandas.factorize;
 * dictionary-encoding a 64-bit key column into dense ids; a joint encoding of two key columns with "no partner" marked).  The same
 * kernels, tables, class walk and host path: after the last column sweep of a class, every slot word takes its group's index and the
 * class's tuples store the word of their key at their row. */
/* rhj_group_agg_cols_dev with d_out_gid: a DEVICE array of gid_rows words indexed by R's rowID.  For every tuple of R,
 * d_out_gid[rowR] = g, where group g is the one at d_out_keys[g] OF THIS CALL.  The order of groups is unspecified and may differ
 * from run to run, so ids are consistent with this call's outputs only; the PARTITION of the rows into groups is exact and the same
 * every run.  Ids are read as there: they are partitioned with the values whenever they are given.  Words of d_out_gid that no
 * tuple's rowID names are left untouched.  Two tuples with the same rowID and different values leave one of the two ids, unspecified.
 * d_out_gid == NULL: gid_rows is ignored and the call is rhj_group_agg_cols_dev.
 * Overflow: an id is never compared with out_capacity.  Under RHJ_E_OVERFLOW the ids are still the exact group indices in
 * [0, *out_groups); ids >= out_capacity name groups whose rows were not stored.  Count only (d_out_keys == NULL, out_capacity == 0)
 * may be given an id array: a dense labelling without the dictionary; no column is read, as there.
 * Row guard: a rowR >= gid_rows is never written: it raises the flag word and the call returns RHJ_E_INVALID -- rhj_last_error names
 * d_out_gid --, for every such tuple the kernel sees; nothing at or past gid_rows is touched; the other words of d_out_gid and the
 * outputs are then undefined; the context stays usable.
 * Everything else is the contract of rhj_group_agg_cols_dev, word for word: ops (checked before any launch), count only,
 * RHJ_E_OVERFLOW, the row guard of the columns, nR == 0 (0 groups, no launch, d_out_gid untouched), plans and repeats -- a repeat
 * starts from nothing and writes every id again --, probe_split ignored, "last.join_kernel" is 15, "last.group_rounds".
 * Costs beyond rhj_group_agg_cols_dev's: one more sweep of the partition per class, and one scattered 8-byte store per tuple. */
int rhj_group_agg_ids_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                               const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows,
                               const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                               uint64_t *const *d_out_aggs, uint64_t out_capacity, uint64_t *out_groups,
                               uint64_t *d_out_gid, uint64_t gid_rows);
/* ... on 16-byte tuples (value = .payload, rowR = .key) */
int rhj_group_agg_ids_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                          const uint64_t *const *d_cols, const uint32_t *ops, uint32_t ncols, uint64_t col_rows,
                          const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                          uint64_t *const *d_out_aggs, uint64_t out_capacity, uint64_t *out_groups,
                          uint64_t *d_out_gid, uint64_t gid_rows);
/* rhj_group_join_agg_cols_dev with d_out_gidR / d_out_gidS: DEVICE arrays of gidR_rows / gidS_rows words indexed by the side's rowID.
 * d_out_gidR[rowR] = g for every tuple of R whose value has a group -- every tuple under RHJ_GJ_LEFT, the tuples whose value occurs
 * in S under RHJ_GJ_INNER; d_out_gidS[rowS] = g for every tuple of S whose value has a group -- in both modes the tuples whose value
 * occurs in R.  Group g is the one at d_out_keys[g] of this call, as above.
 * EVERY OTHER word of [0, gidR_rows) and [0, gidS_rows) is all ones when the call returns (SQL's NULL; -1 as int64): both arrays are
 * filled before the kernel, on every attempt, so this holds for partitions that get no task, for classes that emit nothing, across
 * the in-call repeats, and where no kernel runs -- nR == 0, or nS == 0 under RHJ_GJ_INNER: 0 groups, both arrays all ones; nS == 0
 * under RHJ_GJ_LEFT: the group-by of R with ids.  Two tuples with the same rowID leave one of their words, unspecified.
 * Either pointer may be NULL on its own (its *_rows is ignored, that side gets no sweep); both NULL: the call is
 * rhj_group_join_agg_cols_dev.
 * Overflow and count only as above: ids are exact group indices in [0, *out_groups) whatever out_capacity is.
 * Row guard: a rowR >= gidR_rows or a rowS >= gidS_rows is never written: RHJ_E_INVALID, rhj_last_error names d_out_gidR or
 * d_out_gidS, for every such tuple an id sweep meets (a partition no task is made for, and a class of keys that emits no group, get
 * no sweep); nothing at or past *_rows is touched; the context stays usable.
 * Everything else is the contract of rhj_group_join_agg_cols_dev, word for word; "last.join_kernel" is 16.
 * Costs beyond it: the fill -- 8 bytes written per word of either array --, one more sweep of each side's partition per class that
 * emits, and one scattered 8-byte store per tuple that has a group. */
int rhj_group_join_agg_ids_cols_dev(rhj_ctx *ctx,
        const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
        const uint64_t *d_valS, const uint64_t *d_idS, uint64_t nS,
        const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
        const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
        int mode, const rhj_opts *opts,
        uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
        uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
        uint64_t out_capacity, uint64_t *out_groups,
        uint64_t *d_out_gidR, uint64_t gidR_rows, uint64_t *d_out_gidS, uint64_t gidS_rows);
/* ... on 16-byte tuples (value = .payload, rowID = .key) */
int rhj_group_join_agg_ids_dev(rhj_ctx *ctx,
        const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS,
        const uint64_t *const *d_colsR, const uint32_t *opsR, uint32_t ncolsR, uint64_t colR_rows,
        const uint64_t *const *d_colsS, const uint32_t *opsS, uint32_t ncolsS, uint64_t colS_rows,
        int mode, const rhj_opts *opts,
        uint64_t *d_out_keys, uint64_t *d_out_cntR, uint64_t *d_out_cntS,
        uint64_t *const *d_out_aggsR, uint64_t *const *d_out_aggsS,
        uint64_t out_capacity, uint64_t *out_groups,
        uint64_t *d_out_gidR, uint64_t gidR_rows, uint64_t *d_out_gidS, uint64_t gidS_rows);

/* ---- group-by argmin / argmax: WHICH ROW holds each group's minimum or maximum (the latest record per key: SELECT DISTINCT ON (key)
 * .. ORDER BY key, t DESC; ROW_NUMBER() OVER (PARTITION BY key ORDER BY t) = 1; pandas groupby.idxmin / idxmax; drop_duplicates(keep =
 * "first" | "last")).  The group-by's kernel family, table, class walk and host path: per value column the minimum / maximum sweep of
 * rhj_group_agg_cols_dev and one more sweep that finds the row. */
#define RHJ_ARG_MIN_U64 0   /* the row holding the minimum / maximum of the column words as unsigned 64-bit ... */
#define RHJ_ARG_MAX_U64 1
#define RHJ_ARG_MIN_I64 2   /* ... as two's-complement signed 64-bit */
#define RHJ_ARG_MAX_I64 3
#define RHJ_ARG_ROW     4   /* no column: the rowIDs themselves are ordered -- the first / last row of the group (d_cols[j], d_out_vals[j] ignored, may be NULL) */
#define RHJ_ARG_TIE_FIRST 0 /* among the tuples holding the extreme: the smallest rowID (unsigned) */
#define RHJ_ARG_TIE_LAST  1 /* the largest */
#define RHJ_GROUP_ARG_MAX_COLS 4
/* rhj_group_agg_cols_dev's shape with a row beside every value.  ops / ties: HOST arrays of ncols words (an RHJ_ARG_* / an
 * RHJ_ARG_TIE_*); ties == NULL: every column is RHJ_ARG_TIE_FIRST.  d_out_vals / d_out_rows: HOST arrays of ncols DEVICE columns of
 * out_capacity words.
 * Values: for group g and column j, d_out_vals[j][g] is the extreme of d_cols[j][rowR] over the group's tuples -- bit for bit what
 * rhj_group_agg_cols_dev returns under the matching RHJ_AGG_* op.
 * Rows, the tie rule: d_out_rows[j][g] is the rowID of a tuple of the group whose column word equals that extreme -- among those tuples
 * the smallest rowID under RHJ_ARG_TIE_FIRST, the largest under RHJ_ARG_TIE_LAST, rowIDs compared as unsigned 64-bit.
 * RHJ_ARG_ROW: d_out_rows[j][g] is the smallest (FIRST) or largest (LAST) rowID of the group; no column is read, so there is no row
 * guard for that column, and d_cols[j] / d_out_vals[j] are never touched.
 * The same column pointer may appear several times: MIN and MAX of one timestamp, plus ROW / FIRST and ROW / LAST, fit in one call.
 * Every group has a row: a group has at least one tuple, so every d_out_rows[j][g] with g < out_capacity names a real row of the
 * group, also when the extreme is the identity of its op -- a group whose every value is all ones under RHJ_ARG_MIN_U64, 0 under
 * RHJ_ARG_MAX_U64, INT64_MAX under RHJ_ARG_MIN_I64, INT64_MIN under RHJ_ARG_MAX_I64.
 * Everything else is the contract of rhj_group_agg_cols_dev, word for word: the order of groups is unspecified, the set and every
 * word exact and bit-identical from run to run; count only with a NULL d_out_keys and out_capacity 0 -- no sweep, no column read --;
 * RHJ_E_OVERFLOW with the exact *out_groups, complete distinct groups in [0, capacity) and nothing at or past capacity written in
 * any of the up to ten arrays, the rows arrays included; the row guard of the value ops (a rowR >= col_rows is never dereferenced: a
 * flag word, RHJ_E_INVALID, rhj_last_error names col_rows, the context stays usable); nR == 0; plans, repeats, probe_split ignored;
 * "last.join_kernel" is 15, "last.group_rounds" as there; ncols == 0 returns keys and counts only.
 * RHJ_E_INVALID beyond that contract's, each checked before any launch, also in a count-only call, rhj_last_error names the column:
 * an ops[j] above RHJ_ARG_ROW; a ties[j] above RHJ_ARG_TIE_LAST; ncols above RHJ_GROUP_ARG_MAX_COLS; with out_capacity > 0 a NULL
 * d_out_rows[j], or a NULL d_cols[j] or d_out_vals[j] under a value op.
 * Costs: per value column and class TWO sweeps of the partition and two gathers of the column word, and one global atomic per tuple
 * that holds its group's extreme -- typically one per group; a heavy group whose column is constant issues one per tuple on one
 * word.  An RHJ_ARG_ROW column costs one sweep, no gather and no global atomic. */
int rhj_group_arg_cols_dev(rhj_ctx *ctx, const uint64_t *d_valR, const uint64_t *d_idR, uint64_t nR,
                           const uint64_t *const *d_cols, const uint32_t *ops, const uint32_t *ties, uint32_t ncols, uint64_t col_rows,
                           const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                           uint64_t *const *d_out_vals, uint64_t *const *d_out_rows, uint64_t out_capacity, uint64_t *out_groups);
/* ... on 16-byte tuples (value = .payload, rowR = .key) */
int rhj_group_arg_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t nR,
                      const uint64_t *const *d_cols, const uint32_t *ops, const uint32_t *ties, uint32_t ncols, uint64_t col_rows,
                      const rhj_opts *opts, uint64_t *d_out_keys, uint64_t *d_out_counts,
                      uint64_t *const *d_out_vals, uint64_t *const *d_out_rows, uint64_t out_capacity, uint64_t *out_groups);

/* ---- framed window aggregates: a value per row from a ROWS frame around it in its partition (SUM / MIN / MAX / COUNT / FIRST_VALUE /
 * LAST_VALUE OVER [PARTITION BY k ORDER BY t ROWS BETWEEN a PRECEDING AND b FOLLOWING]; pandas groupby.rolling(w).sum / min / max,
 * groupby.transform("size" / "first" / "last")).  The window entry below computes over the rows BEFORE a row; this one
 * computes over a sliding or whole-partition frame, and a sliding MIN / MAX costs the same for every frame width.
 * Partitions, order and ties are the window entry's, word for word: rows are the indices 0 .. n - 1; d_part, d_order and every
 * d_cols[j] are device columns of n words; ops, preceding, following, the two pointer arrays and out_partitions are HOST memory.  A
 * PARTITION is the set of rows with the same d_part word -- the word is compared for equality only; d_part == NULL: one partition.
 * Inside a partition the rows are ordered by their d_order word under flags: RHJ_SORT_I64 and RHJ_SORT_DESC, with the sort entry's
 * meaning.  Ties keep their input order in both directions, so every result is defined, and bit-identical from run to run.
 * d_order == NULL: input order; a non-zero flags with d_order == NULL is RHJ_E_INVALID.  The outputs are aligned with the input rows,
 * not in sorted order.
 * The frame: for row i at 0-based position q of its partition P of m rows, the frame of op j is the positions
 *     [max(0, q - preceding[j]), min(m - 1, q + following[j])]  of P,
 * computed without wrap-around: q + following[j] saturates.  RHJ_FRAME_UNBOUNDED (all ones) on either side means "to the partition's
 * edge".  preceding == NULL: unbounded for every op; following == NULL: 0 for every op -- together the running frame ROWS UNBOUNDED
 * PRECEDING of the window entry.  The frame always contains the current row; frames that end before or start after the current row,
 * and value-based RANGE frames, are not part of this entry.  Each op has its own frame.
 * Ops: d_outs[j][i] receives
 *     RHJ_FRAME_COUNT       the rows in the frame; with both sides unbounded the partition's size (COUNT(*) OVER (PARTITION BY k))
 *     RHJ_FRAME_SUM         the sum mod 2^64 of d_cols[j][r] over the rows r in the frame
 *     RHJ_FRAME_MIN_U64 / RHJ_FRAME_MAX_U64 / RHJ_FRAME_MIN_I64 / RHJ_FRAME_MAX_I64
 *                           the minimum / maximum of those words, unsigned or as two's-complement int64: bit for bit a column word
 *     RHJ_FRAME_FIRST_ROW / RHJ_FRAME_LAST_ROW
 *                           the row at the frame's first / last position; the frame holds the current row, so there is never RHJ_NO_ROW
 * d_cols[j] is ignored for the ops without a column (d_cols may then be NULL).  The same column may be given several times; two equal
 * output pointers are undefined.  FIRST_VALUE / LAST_VALUE of a PAYLOAD is rhj_gather_u64 through the row:
 *     ops = {RHJ_FRAME_FIRST_ROW}; pre = {9}; rhj_frame_cols_dev(ctx, k, t, n, RHJ_SORT_I64, ops, pre, NULL, NULL, 1, &first, NULL);
 *     rhj_gather_u64(ctx, x, first, n, x_first);                              -- x_first[i] = x at the frame's first row
 * Each row's share of its partition: with ROW_NUMBER rn and RANK rk from rhj_window_cols_dev and the partition's size m from
 * RHJ_FRAME_COUNT with both sides unbounded, NTILE(b) is -- big = m % b, small = m / b -- rn <= big * (small + 1) ? (rn - 1) / (small
 * + 1) + 1 : big + (rn - 1 - big * (small + 1)) / small + 1; PERCENT_RANK is m > 1 ? (rk - 1) / (m - 1) : 0; CUME_DIST is (the
 * RHJ_FRAME_COUNT of a frame reaching to the last peer) / m -- over distinct order keys rn_of_last_peer / m.  Two calls, so two sets
 * of sorts.
 * *out_partitions receives the number of partitions; it may be NULL.  n == 0: RHJ_OK, no launch, 0 partitions.  RHJ_E_INVALID,
 * before any launch, with a message naming the argument: unknown flag bits; flags without d_order; nops 0 or above
 * RHJ_FRAME_MAX_OPS; NULL ops, d_outs or d_outs[j]; an op above RHJ_FRAME_LAST_ROW; a NULL d_cols[j] for a column op with n > 0.
 * Inputs are neither modified nor retained; outputs must not overlap inputs.  The call synchronises; it honours rhj_set_stream and
 * rhj_set_profiling (the inner sorts' spans; RHJ_K_AUX: heads, gather, emit; per scan RHJ_K_HIST, RHJ_K_SCAN, RHJ_K_SCATTER).
 * How: the order (partition, order key, input position) from the stable sort, as the window entry's -- 0, 1 or 2 inner sorts.  One
 * launch marks the partition heads.  Every position's partition start and end are a forward maximum scan of (head ? position : 0) and
 * a backward minimum scan of (tail ? position : all ones); lo and hi of every op are then arithmetic, and COUNT, FIRST_ROW and
 * LAST_ROW need nothing else.  Value scans are stored BY SORTED POSITION.  SUM: one forward scan S that restarts at partition heads;
 * the answer is S[hi] - (lo above the start ? S[lo - 1] : 0), exact mod 2^64.  MIN / MAX of width w = preceding + following + 1: the
 * positions are cut into blocks of w, aligned to multiples of w of the global position; F is the forward scan that restarts at
 * partition heads and block starts, B the backward scan that restarts at partition tails and block ends; a frame is never wider than
 * a block, so it is F[hi], B[lo] or op(B[lo], F[hi]) -- two stored words at most, whatever w.  A side that is unbounded or reaches n -
 * 1 positions needs one scan without blocks (F for preceding, B for following); otherwise two, with blocks when w < n.  A backward
 * scan is the forward fold over the mirrored position n - 1 - p.  Each scan is three launches ordered on the stream on the sort's
 * units ("sort.max_units" caps them here too; the result never depends on it): a reduce per unit, a one-workgroup carry over the at
 * most 2048 unit summaries, an apply per unit.  One emit launch per call reads the arrays at lo / hi and stores out[perm[p]].  No
 * workgroup waits on another inside a kernel, and no position, value or count comes from an atomic.
 * Costs in bytes per row: the sorts (see there) plus 24 for the gather between two of them; heads 8 + 1; each bound 1 + 1 + 8; each
 * value scan 2 x (1 + 8) read and two gathered 8-byte loads, 8 written; emit 8 .. 24 read, per op up to two gathered 8-byte loads
 * and one scattered 8-byte store.
 * rhj_get_info: "last.frame_units" the units the scans were cut into, "last.frame_sorts" the inner sorts that ran (0, 1 or 2),
 * "last.frame_partitions" the partitions, "last.frame_scans" the value scans: 1 per SUM, 1 or 2 per MIN / MAX, 0 for the other ops;
 * all four are 0 after every other call.  After a frame call "last.join_kernel" is -1 and "last.sort_*" / "last.topk_*" /
 * "last.window_*" / "last.asof_*" are 0.
 * Memory: a workspace buffer of its own (the inner sorts regrow the sort's), kept until rhj_release_workspace: 4 x 8 + 1 bytes per
 * row for the order and the bounds, and 8 per value scan -- up to 12 x 8 + 1.
 * There is no 16-byte tuple form. */
#define RHJ_FRAME_MAX_OPS    4
#define RHJ_FRAME_UNBOUNDED  0xFFFFFFFFFFFFFFFFull   /* preceding[j] / following[j]: to the partition's edge */
#define RHJ_FRAME_COUNT      0   /* no column */
#define RHJ_FRAME_SUM        1   /* column; mod 2^64 */
#define RHJ_FRAME_MIN_U64    2
#define RHJ_FRAME_MAX_U64    3
#define RHJ_FRAME_MIN_I64    4
#define RHJ_FRAME_MAX_I64    5
#define RHJ_FRAME_FIRST_ROW  6   /* no column */
#define RHJ_FRAME_LAST_ROW   7   /* no column */
int rhj_frame_cols_dev(rhj_ctx *ctx, const uint64_t *d_part, const uint64_t *d_order, uint64_t n, uint32_t flags,
                       const uint32_t *ops, const uint64_t *preceding, const uint64_t *following,
                       const uint64_t *const *d_cols, uint32_t nops, uint64_t *const *d_outs, uint64_t *out_partitions);

/* ---- RANGE frames: the same aggregates over a VALUE distance on the order key (SUM / COUNT / MIN / MAX / FIRST_VALUE / LAST_VALUE
 * OVER [PARTITION BY k ORDER BY t RANGE BETWEEN a PRECEDING AND b FOLLOWING]; "the same symbol's rows of the last 5 seconds"; pandas
 * groupby.rolling("5s")).  The argument list, the RHJ_FRAME_* ops and RHJ_FRAME_UNBOUNDED are rhj_frame_cols_dev's.
 * Partitions, the order inside them, ties and output alignment are the frame entry's, word for word: a PARTITION is the set of rows
 * with a bit-equal d_part word (d_part == NULL: one partition); the rows are ordered by their d_order word under RHJ_SORT_I64 /
 * RHJ_SORT_DESC; ties keep their input order in both directions; the outputs are aligned with the input rows; every result is
 * bit-identical from run to run.  d_order == NULL is RHJ_E_INVALID: a value distance needs a value.
 * The frame: let t be the row's order word in the chosen view (unsigned, or two's-complement int64).  Ascending, the frame of op j is
 * every row of the partition whose order value lies in [t - preceding[j], t + following[j]]; under RHJ_SORT_DESC the interval is
 * [t - following[j], t + preceding[j]] -- PRECEDING still means "earlier in the order".  Distances are exact integers; both ends
 * saturate at the view's minimum and maximum, nothing wraps: a distance of 2^64 - 2 between INT64_MIN and INT64_MAX is honoured.
 * RHJ_FRAME_UNBOUNDED (all ones) on a side is the partition's edge, which is also what a distance of 2^64 - 1 means.  preceding ==
 * NULL: unbounded for every op; following == NULL: 0 for every op -- together SQL's default frame, RANGE UNBOUNDED PRECEDING to
 * CURRENT ROW, under which peers share a value.  The frame is a contiguous run of sorted positions and always contains the current
 * row and all its peers, also at distance 0: this is the difference from ROWS.  pandas' time-based rolling stops at the current row
 * among peers, so the results agree with pandas exactly when the order keys are distinct within a partition.  Frames that exclude the
 * current row are not part of this entry, nor are empty frames: there is never RHJ_NO_ROW.  Each op has its own frame.
 * Ops: RHJ_FRAME_COUNT, RHJ_FRAME_SUM (the sum mod 2^64), RHJ_FRAME_MIN_U64 / RHJ_FRAME_MAX_U64 / RHJ_FRAME_MIN_I64 /
 * RHJ_FRAME_MAX_I64 (bit for bit a column word), RHJ_FRAME_FIRST_ROW / RHJ_FRAME_LAST_ROW (the row at the frame's first / last
 * sorted position, which the tie rule defines).  d_cols[j] is ignored for the ops without a column; the same column may be given
 * several times; two equal output pointers are undefined.
 * *out_partitions receives the number of partitions; it may be NULL.  n == 0: RHJ_OK, no launch, 0 partitions.  RHJ_E_INVALID,
 * before any launch, with a message naming the argument: unknown flag bits; d_order == NULL with n > 0 or with flags; nops 0 or above
 * RHJ_FRAME_MAX_OPS; NULL ops, d_outs or d_outs[j]; an op above RHJ_FRAME_LAST_ROW; a NULL d_cols[j] for a column op with n > 0.
 * Inputs are neither modified nor retained; outputs must not overlap inputs.  The call synchronises; it honours rhj_set_stream and
 * rhj_set_profiling (the inner sorts' spans; RHJ_K_AUX: heads, gathers; per scan RHJ_K_HIST, RHJ_K_SCAN, RHJ_K_SCATTER; RHJ_K_TASKS:
 * the table levels; RHJ_K_JOIN: the searches and the answers, one launch).
 * How: the order, the heads and every position's partition start and end as the frame entry's -- 1 or 2 inner sorts.  The order
 * words by sorted position (the sorted keys after one sort, one gather through the permutation after two) are read as v = word ^
 * (I64 ? 1 << 63 : 0), complemented under DESC: v is non-decreasing along a partition in all four views, and in both directions the
 * frame is max(0, v - preceding) <= v_r <= min(2^64 - 1, v + following).  Per row and distinct frame two searches: lo gallops from
 * the row's position towards the partition's start in doubling steps and bisects the bracket, hi the mirror -- about 2 log2(frame
 * rows) dependent 8-byte loads each; an unbounded side needs none.  Every column is gathered once BY SORTED POSITION (V).  SUM: S[hi]
 * - (lo above the start ? S[lo - 1] : 0).  MIN / MAX with an unbounded side: one scan, F[hi] or B[lo].  Otherwise the frame entry's
 * block-restarting scans at the FIXED block length 64 and a sparse table over the summaries of the n / 64 whole blocks, T_0[k] = F[64 k
 * + 63], T_l[k] = op(T_(l-1)[k], T_(l-1)[k + 2^(l-1)]), one small launch per level.  With bl = lo / 64 and bh = hi / 64: the same block
 * -- F[hi] when lo is the block's or the partition's start, B[lo] when hi is the block's or the partition's end, else a walk over
 * V[lo .. hi], at most 62 words --; different blocks -- op(B[lo], F[hi]), and with bh - bl >= 2 also op(T_l[bl + 1], T_l[bh - 2^l]), l =
 * floor(log2(bh - bl - 1)).  Interior blocks lie wholly inside the frame, therefore inside one partition: table words that span a
 * partition boundary are never read.  No workgroup waits on another inside a kernel, and no position, value or count comes from an
 * atomic.
 * rhj_get_info: "last.frame_range_units", "last.frame_range_sorts" (1 or 2), "last.frame_range_partitions", "last.frame_range_scans"
 * the value scans: 1 per SUM, 1 or 2 per MIN / MAX; "last.frame_range_levels" the sparse-table levels built, 0 when no op needed
 * them.  All five are 0 after every other call.  After this call "last.join_kernel" is -1 and every other entry's "last.*" (the
 * frame entry's included) is 0.  "sort.max_units" caps the units here too; the result never depends on it.
 * Memory: the frame entry's workspace buffer, kept until rhj_release_workspace: 4 x 8 + 1 bytes per row, 8 more after two sorts, 8
 * per distinct column and per value scan, and 8 x (n / 64) per table level.
 * There is no 16-byte tuple form. */
int rhj_frame_range_cols_dev(rhj_ctx *ctx, const uint64_t *d_part, const uint64_t *d_order, uint64_t n, uint32_t flags,
                             const uint32_t *ops, const uint64_t *preceding, const uint64_t *following,
                             const uint64_t *const *d_cols, uint32_t nops, uint64_t *const *d_outs, uint64_t *out_partitions);

/* ---- range join: for every row of R the rows of S of its partition whose `on` word lies in the row's interval -- SELECT r.row, s.row
 * FROM R JOIN S ON r.by = s.by AND s.t BETWEEN r.lo AND r.hi: "every quote of the same symbol within 5 s around each trade", "every
 * event that falls inside each session", the band join |r.t - s.t| <= d, the point-in-interval join against validity ranges (DESIGN
 * 4.31).  The as-of entry returns ONE partner per row, the RANGE frames look at one table and return aggregates; this entry returns the
 * partner rows, as a compact CSR result over S in sorted order and as ordered pairs.
 * Rows are the indices 0 .. n - 1 of their table.  d_byR / d_loR / d_hiR are device columns of nR words, d_byS / d_onS of nS words.
 * Neither table needs to be sorted.
 * Partitions: `by` is compared for bit-equality only.  d_byR == NULL && d_byS == NULL: one partition.  Exactly one of the two NULL
 * with both tables non-empty is RHJ_E_INVALID.
 * Partners: lo / hi / on are ordered in the chosen view, unsigned 64-bit by default, two's-complement int64 under RHJ_RANGE_I64 (as
 * RHJ_SORT_I64).  Row j of S is a partner of row i of R iff the `by` words are equal and lo[i] <= on[j] <= hi[i] in the view;
 * RHJ_RANGE_LO_OPEN turns the first <= into <, RHJ_RANGE_HI_OPEN the second.  An interval with lo > hi in the view has no partner
 * and is legal; so is an open bound with lo == hi.
 * Band form (RHJ_RANGE_BAND): d_loR holds R's own order word x and d_hiR must be NULL; lo = x - below and hi = x + above as exact
 * integers that saturate at the view's ends, nothing wraps -- the rule of the RANGE frames' distances, so all ones is "to the end of
 * the view".  Open flags apply to the saturated bound like to any other.  Without the bit `below` and `above` are ignored and d_hiR is
 * required.
 * Sorted S and the CSR form: rowsS is the rows of S ordered by (`by` word unsigned ascending, `on` in the view ascending, row index
 * ascending).  The partners of row i are the contiguous run rowsS[first[i] .. first[i] + cnt[i]), cnt[i] = offsets[i + 1] -
 * offsets[i].  d_out_offsets has nR + 1 words: the exclusive prefix of the counts, offsets[0] = 0 and offsets[nR] the total.
 * d_out_first has nR words; where cnt[i] == 0, first[i] is any value <= nS.  d_out_rowsS has nS words.  Each of the three may be NULL.
 * This compact result is 16 nR + 8 nS bytes however many pairs there are.
 * Pairs: d_out[k] = {rowR, rowS}, ordered by rowR ascending, within one row of R in the order of rowsS: d_out[offsets[i] + q] = {i,
 * rowsS[first[i] + q]}.  d_out == NULL with out_capacity == 0 writes no pairs; NULL with a non-zero capacity is RHJ_E_INVALID.  d_out
 * needs 16-byte alignment.  *out_count is a HOST pointer and may be NULL; it always receives the exact total.  When the total exceeds
 * out_capacity the return is RHJ_E_OVERFLOW: slots [0, capacity) hold the first `capacity` pairs of the defined order, nothing at or
 * past capacity is written, and the three CSR outputs are complete, so a caller can finish with rhj_range_expand_dev or slice R.
 * Every result is bit-identical from run to run.
 * Empty tables: nR == 0: RHJ_OK, total 0, offsets[0] = 0 if given, nothing else written.  nS == 0 with nR > 0: total 0, offsets all 0
 * and first all 0 (one fill launch).
 * RHJ_E_INVALID, before any launch, with a message naming the argument: unknown flag bits; NULL d_loR with nR > 0; NULL d_onS with nS
 * > 0; NULL d_hiR without RHJ_RANGE_BAND and nR > 0; non-NULL d_hiR under RHJ_RANGE_BAND; the one-sided `by`; NULL d_out with a
 * non-zero out_capacity.  *out_count and the outputs are then untouched.
 * Inputs are neither modified nor retained; outputs must not overlap inputs; pointers need 8-byte alignment.  The call synchronises;
 * it honours rhj_set_stream and rhj_set_profiling (the inner sorts' spans; RHJ_K_AUX: concatenation, gathers, fill, validation; per
 * scan RHJ_K_HIST, RHJ_K_SCAN, RHJ_K_SCATTER; RHJ_K_TASKS: the searches; RHJ_K_JOIN: the expansion).
 * How: one launch concatenates R's lower bounds (under BAND the saturated x - below, computed in the view) and S's `on` words into one
 * column of n = nR + nS words, [R ; S], under RHJ_RANGE_LO_OPEN [S ; R], and the `by` words alike; the side of a concatenated position
 * follows from its index.  The order (by, word, concatenated position) comes from the stable sort as in the as-of entry -- two sorts
 * with a gather between them, one sort without `by` --, so among equal words a row of S stands behind a row of R exactly when
 * equality qualifies at the lower end.  The rank scan -- a reduce per unit, a one-workgroup carry over the at most 2048 unit sums, an
 * apply per unit, on the sort's units ("sort.max_units" caps them here too; the result never depends on it) -- gives srank[p], the rows
 * of S before sorted position p, and stores rowsS[srank[p]] at the positions of S.  One flat launch then searches, from every
 * position p of R, the first position q at which "the same `by` word and word <= hi" (< hi under RHJ_RANGE_HI_OPEN) fails -- the test is
 * monotone from p on, a galloping search of about 2 log2(q - p) dependent loads -- and stores first[i] = srank[p], cnt[i] = srank[q] -
 * srank[p].  The same scan over cnt in row order gives offsets; the host reads the total.  The expansion runs one workgroup per
 * "range_join.expand_tile" output slots: it finds the rows that cover its slots by binary search in offsets, every thread its slot's row
 * among them, and writes the pair with one 16-byte store: work is balanced over pairs, not rows.  No workgroup waits on another inside
 * a kernel, and no position, count or value comes from an atomic.
 * Costs in bytes: per row of nR + nS the concatenation 16 (32 with `by`), the sorts (see there) plus 24 for the gather between two of
 * them and 24 for the order words after them, the rank scan 8 + 8 + 8, the search 8 + 8 and per row of R a gathered 8 (hi), the
 * dependent loads of its search and two scattered 8-byte stores; per row of R the offsets scan 8 + 8 + 8; per pair one 16-byte store, a
 * gathered 8-byte load and log2(rows per tile) cached loads.
 * rhj_get_info: "last.range_join_units" the units the rank scan was cut into, "last.range_join_sorts" the inner sorts that ran (1
 * without `by`, else 2; 0 with an empty table), "last.range_join_pairs" the total, "last.range_join_expand_tiles" the workgroups of
 * the expansion; all four are 0 after every other call.  After a range call "last.join_kernel" is -1 and "last.sort_*" / "last.topk_*"
 * / "last.window_*" / "last.asof_*" / "last.frame*" are 0.  "range_join.tile_rows": the positions one workgroup scans at once,
 * "range_join.expand_tile": the pairs one workgroup of the expansion writes; constants of the build.
 * Memory: a workspace buffer of its own (the inner sorts regrow the sort's), kept until rhj_release_workspace: 4 x 8 bytes per row of
 * nR + nS, 6 x 8 with `by`, 8 per row of R, and 8 per word of every CSR output that is NULL.
 * rhj_range_expand_dev is the second half on its own, so a caller sizes the pair buffer after one set of sorts: count with d_out ==
 * NULL, allocate *out_count pairs, expand.  d_offsets (nR + 1 words), d_first (nR words) and d_rowsS (nS words) are the CSR result of a
 * range call, or any arrays of that shape.  One flat validation launch over the rows checks offsets[0] == 0, offsets[i] <=
 * offsets[i + 1], and first[i] + cnt[i] <= nS wherever cnt[i] > 0, and reduces to one flag, which the host reads together with
 * offsets[nR] before the expansion is launched: a violation is RHJ_E_INVALID with nothing written -- an error code, never an address.
 * NULL d_offsets, NULL d_first with nR > 0, NULL d_rowsS with nS > 0 and NULL d_out with a non-zero capacity are RHJ_E_INVALID before
 * any launch.  Capacity, overflow, the first-`capacity` rule and *out_count are as above.  No sort runs in it: it leaves
 * "last.range_join_units" and "last.range_join_sorts" as the call before it left them -- behind a range call they still speak of the
 * call that made the arrays --, the other two names speak of it.
 * Out of scope: interval-overlap joins with intervals on both sides, inequality joins on two different columns, float order columns,
 * a sharded form, the query layer.  There is no 16-byte tuple form. */
#define RHJ_RANGE_I64      1u   /* order lo / hi / on as two's-complement int64 (default: unsigned), as RHJ_SORT_I64 */
#define RHJ_RANGE_LO_OPEN  2u   /* on >  lo instead of on >= lo */
#define RHJ_RANGE_HI_OPEN  4u   /* on <  hi instead of on <= hi */
#define RHJ_RANGE_BAND     8u   /* d_loR holds R's own order word x, d_hiR must be NULL: the interval is [x - below, x + above] */
int rhj_range_join_cols_dev(rhj_ctx *ctx, const uint64_t *d_byR, const uint64_t *d_loR, const uint64_t *d_hiR, uint64_t nR,
                            const uint64_t *d_byS, const uint64_t *d_onS, uint64_t nS, uint32_t flags, uint64_t below, uint64_t above,
                            uint64_t *d_out_offsets, uint64_t *d_out_first, uint64_t *d_out_rowsS,
                            rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count);
int rhj_range_expand_dev(rhj_ctx *ctx, const uint64_t *d_offsets, const uint64_t *d_first, uint64_t nR,
                         const uint64_t *d_rowsS, uint64_t nS, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count);

/* ---- composite keys: up to four key columns per relation packed into ONE 64-bit key column (JOIN .. ON r.a = s.a AND r.b = s.b; GROUP
 * BY a, b; torch.unique(dim=0); merge(on=[..])).  Every operator above compares 64-bit values by bit pattern, so what it needs is an
 * EXACT surrogate: a 64-bit word per row such that two rows of R u S get the same word if and only if all their key columns agree.
 * rhj_keys_pack_dev makes it, the caller hands the packed columns to any *_cols_dev entry, and rhj_keys_unpack_dev turns packed words
 * (a group-by's d_out_keys) back into the columns.  No operator changes; single-column callers are not touched. */
#define RHJ_KEYS_MAX_COLS 4
#define RHJ_KEYS_NO_UNPACK 1u            /* flags bit 0: keep no dictionaries; rhj_keys_unpack_dev then returns RHJ_E_INVALID */
#define RHJ_KEYS_RANGE 0                 /* a column stored as value - base */
#define RHJ_KEYS_DICT  1                 /* a column stored as its dense id in a dictionary the plan owns */
#define RHJ_KEYS_MAX_FOLDS 2
#define RHJ_KEYS_FOLD0 4                 /* field ids: 0 .. 3 the key columns, RHJ_KEYS_FOLD0 + f the output of fold step f */
typedef struct rhj_keyplan rhj_keyplan;  /* opaque; owns its dictionaries */
/* The layout of a packed word.  A FIELD is a key column (id j) or the output of a fold step (id RHJ_KEYS_FOLD0 + f).  Fold step f
 * packs the fields fold_a[f] (low bits) and fold_b[f] (from bit fold_shift[f], the width of fold_a[f]) into one word and replaces the
 * pair by that word's dense id.  The final word holds nfields fields, field i = field_id[i] in bits [field_shift[i], field_shift[i] +
 * field_width[i]), lowest first, without gaps (a field of width 0 occupies nothing; its shift is the running sum all the same);
 * bits at and above total_bits are 0.  The rule fixes the shape: fold 0 takes columns 0 and 1, fold 1 takes fold 0's output and
 * column 2.  wd: the width of every dense id, bits(n_total - 1); 0 in a RANGE-only layout.  range_bits[j]: what the probe found for
 * column j (a DICT column's field is wd wide instead).  base[j] (RANGE columns), dict_size[j] (DICT columns: the number of distinct
 * values) and fold_size[f] are filled by rhj_keys_plan_info; rhj_keys_layout leaves them 0. */
typedef struct {
    uint32_t nkeys;
    uint32_t kind[RHJ_KEYS_MAX_COLS];          /* RHJ_KEYS_RANGE or RHJ_KEYS_DICT, per key column */
    uint32_t range_bits[RHJ_KEYS_MAX_COLS];
    uint32_t wd;
    uint32_t nfolds;
    uint32_t fold_a[RHJ_KEYS_MAX_FOLDS], fold_b[RHJ_KEYS_MAX_FOLDS], fold_shift[RHJ_KEYS_MAX_FOLDS];
    uint32_t nfields;
    uint32_t field_id[RHJ_KEYS_MAX_COLS], field_width[RHJ_KEYS_MAX_COLS], field_shift[RHJ_KEYS_MAX_COLS];
    uint32_t total_bits;
    uint64_t base[RHJ_KEYS_MAX_COLS];
    uint64_t dict_size[RHJ_KEYS_MAX_COLS];
    uint64_t fold_size[RHJ_KEYS_MAX_FOLDS];
} rhj_keys_layout_t;
/* host only, no GPU: the layout the pack call will use, a pure function of its arguments.  range_bits: HOST array of nkeys widths
 * (0 .. 64), n_total = nR + nS.  The rule (rhj_keys_pack_dev follows the same code):
 *  1. the widths sum to <= 64: every column is RANGE, fields in column order.
 *  2. otherwise wd = bits(n_total - 1).  While the sum is above 64, the RANGE column of greatest width above wd -- lowest index on a
 *     tie -- becomes DICT, its field wd wide.
 *  3. no such column left and the sum still above 64 (every field is then <= wd <= 32 bits): fold -- the first two fields of the
 *     list become one field of width wd at the first one's place -- and check again; at most RHJ_KEYS_MAX_FOLDS folds for four columns.
 * RHJ_E_INVALID: nkeys 0 or above RHJ_KEYS_MAX_COLS; NULL range_bits or out; a width above 64; a layout that needs a dictionary with
 * n_total >= 2^32 (a RANGE-only layout has no such limit). */
int rhj_keys_layout(uint32_t nkeys, const uint8_t *range_bits, uint64_t n_total, rhj_keys_layout_t *out);
/* Packs the nkeys key columns of R (nR rows) and of S (nS rows) into d_outR (nR words) and d_outS (nS words): for every two rows x, y
 * of R u S, packed[x] == packed[y] if and only if key_j[x] == key_j[y] for every j < nkeys.  Column j of R is compared with column j
 * of S, by bit pattern.  d_keysR / d_keysS: HOST arrays of nkeys DEVICE columns (as d_cols elsewhere).  d_keysS NULL with nS 0: one
 * relation (a group-by).  Packing is per position: row i of d_outR belongs to row i of the key columns, so the caller passes the
 * same id column (or none) to the operator it calls next.  nkeys == 1 is legal: RANGE, up to 64 bits.
 * How: one probe launch finds, per column over both sides, the unsigned minimum and maximum of v and of v ^ (1 << 63) -- the second
 * view puts signed order into unsigned order, so an int64 column with small negative values is narrow --; per view the width is 0
 * when max == min, else 64 - clz(max - min); the narrower view is taken (the plain one on a tie) and base is the ORIGINAL value at its
 * minimum, so v - base (mod 2^64) < 2^width.  Then rhj_keys_layout's rule on those widths with n_total = nR + nS.  A DICT column's ids
 * and every fold's ids come from rhj_group_agg_ids_cols_dev over the concatenation of R's and S's column (two device-to-device
 * copies), under the automatic plan; the first dict_size words of its key output are the dictionary.  One pack launch per side.
 * *out_plan: the plan, to be released with rhj_keys_plan_free; it owns the dictionaries unless flags has RHJ_KEYS_NO_UNPACK (the
 * joins need none).  Dictionaries and temporaries are allocations of their own (blocks as rhj_dev_alloc hands them out), not the
 * context's workspace (which the group-by inside and the operator that runs next reuse); temporaries are released as rhj_dev_free
 * releases a block before the call returns, on every path.  The call
 * synchronises.  Inputs are neither modified nor retained; outputs must not overlap them.  Pointers need 8-byte alignment only (16
 * bytes everywhere lets every launch use 16-byte accesses).
 * nR + nS == 0: a plan (every column RANGE, 0 bits) and no launch.
 * RHJ_E_INVALID: nkeys 0 or above RHJ_KEYS_MAX_COLS; a NULL column array, column or output with a non-zero row count; NULL out_plan;
 * unknown flags; a layout that needs a dictionary with nR + nS >= 2^32 -- rhj_last_error says that the RANGE-only layout has no such
 * limit.  On failure *out_plan is NULL and the outputs are undefined.
 * Costs: a RANGE-only layout reads every column twice (probe, pack) and writes one word per row; every DICT column and
 * every fold is one group-by with ids over nR + nS rows, with that entry's weaknesses (all-distinct columns near 10^7 rows; a heavy
 * value is one workgroup's work). */
int rhj_keys_pack_dev(rhj_ctx *ctx, uint32_t nkeys,
                      const uint64_t *const *d_keysR, uint64_t nR,
                      const uint64_t *const *d_keysS, uint64_t nS,
                      uint32_t flags, uint64_t *d_outR, uint64_t *d_outS, rhj_keyplan **out_plan);
/* The inverse, for any array of n packed words the plan produced (a pack output, or the d_out_keys of a group-by over one):
 * d_out_cols: HOST array of the plan's nkeys DEVICE columns of n words; d_out_cols[j][i] is key column j of the rows packed[i]
 * stands for, bit for bit.  One launch: RANGE fields by shift, mask and + base, DICT fields looked up, fold fields looked up and
 * split again.  Index guard: a word that decodes to an id >= its dictionary's size is never used as an index: it raises a flag word
 * in HBM and the call returns RHJ_E_INVALID (the outputs are then undefined; the context stays usable).  The call synchronises.
 * RHJ_E_INVALID also: a NULL plan; a plan packed with RHJ_KEYS_NO_UNPACK; NULL d_packed, d_out_cols or column with n > 0. */
int rhj_keys_unpack_dev(rhj_ctx *ctx, const rhj_keyplan *plan, const uint64_t *d_packed, uint64_t n,
                        uint64_t *const *d_out_cols);
/* the plan's layout with base, dict_size and fold_size filled (host only) */
int rhj_keys_plan_info(const rhj_keyplan *plan, rhj_keys_layout_t *out);
/* frees the plan and its dictionaries; a NULL plan is fine */
int rhj_keys_plan_free(rhj_ctx *ctx, rhj_keyplan *plan);

/* ---- as-of join: for every row of R the nearest row of S of its partition at or before it -- "for every trade the latest quote of
 * the same symbol at or before the trade's time" (pandas.merge_asof, ASOF JOIN, the point-in-time lookup against a slowly changing
 * dimension).
 * Rows are the indices 0 .. n - 1 of their table.  d_byR / d_onR are device columns of nR words, d_byS / d_onS of nS words, d_out_rowS
 * a device column of nR words; out_matched is a HOST pointer and may be NULL.  Neither table needs to be sorted: pandas requires
 * sorted inputs, this entry does not.
 * Partitions: a row of R can only match rows of S whose `by` word is bit-equal -- the word is compared for equality only.
 * d_byR == NULL && d_byS == NULL: one partition.  Exactly one of the two NULL with both tables non-empty is RHJ_E_INVALID.
 * Candidates: the `on` words are ordered in the chosen view, unsigned 64-bit by default, two's-complement int64 under RHJ_ASOF_I64 (as
 * RHJ_SORT_I64).  For row i of R the candidates are the rows j of S in its partition with
 *     onS[j] <= onR[i]     backward (the default)              onS[j] <  onR[i]     backward under RHJ_ASOF_STRICT
 *     onS[j] >= onR[i]     forward (RHJ_ASOF_FORWARD)          onS[j] >  onR[i]     forward under RHJ_ASOF_STRICT
 * (RHJ_ASOF_STRICT is pandas' allow_exact_matches=False.)  Under RHJ_ASOF_TOLERANCE a candidate must also satisfy |onR[i] - onS[j]| <=
 * tolerance, a comparison of exact integers, not mod 2^64: in the int64 view the distance between INT64_MIN and INT64_MAX is 2^64 - 1
 * and still fits the word (it is computed as a difference of the order-transformed words).  tolerance 0 means equal words only;
 * together with RHJ_ASOF_STRICT that matches nothing, and it is legal.  Without the bit `tolerance` is ignored.
 * Result: d_out_rowS[i] is the candidate whose `on` is nearest to onR[i] -- the largest `on` for backward, the smallest for forward.
 * Among candidates that share that `on` word, backward takes the LARGEST row index and forward takes the SMALLEST (pandas: the last,
 * respectively the first, of the duplicates).  With no candidate the output is RHJ_NO_ROW.  The outputs are aligned with R, 8 bytes
 * per row, no pair set is written.  *out_matched receives the number of rows of R with a partner.  The result is bit-identical from
 * run to run.
 * Payloads of S go through rhj_gather_cols_fill, which reads RHJ_NO_ROW as "fill":
 *     rhj_asof_cols_dev(ctx, symR, timeR, nR, symS, timeS, nS, RHJ_ASOF_I64, 0, rowS, NULL);        -- rowS[i] = the latest quote of trade i
 *     rhj_gather_cols_fill(ctx, &bid, 1, nS, rowS, nR, &fill, &bid_R);                              -- bid_R[i] = bid[rowS[i]] or fill
 * Empty tables: nR == 0: RHJ_OK, no launch, *out_matched = 0.  nS == 0 with nR > 0: every output is RHJ_NO_ROW (one fill launch) and
 * matched is 0.
 * RHJ_E_INVALID, before any launch, with a message naming the argument: unknown flag bits (also when both tables are empty); NULL
 * d_onR with nR > 0; NULL d_onS with nS > 0; NULL d_out_rowS with nR > 0; the one-sided `by`.  *out_matched is then untouched.
 * Inputs are neither modified nor retained; outputs must not overlap inputs; pointers need 8-byte alignment.  The call synchronises;
 * it honours rhj_set_stream and rhj_set_profiling (the inner sorts' spans; RHJ_K_AUX: concatenation, gather, heads, fill; the scan
 * RHJ_K_HIST, RHJ_K_SCAN, RHJ_K_SCATTER).
 * How: one launch concatenates the `on` words (and the `by` words) of both tables into columns of n = nR + nS words, [S ; R], under
 * RHJ_ASOF_STRICT [R ; S]; the side of a concatenated position follows from its index.  The order (by, on, concatenated position) comes
 * from the stable sort -- `on` argsorted in the view, descending for RHJ_ASOF_FORWARD, then `by` gathered through that permutation and
 * sorted with the permutation as its rows; one sort without `by`.  Equal `on` words keep the concatenation's order, so the candidates
 * of a row of R are exactly the rows of S before it in its partition, and the nearest is the last of them.  One launch marks, per
 * sorted position, whether it heads a partition, whether it is a row of S, and whether the scan may land on it: backward every row
 * of S, forward only the head of a run of rows of S with one `on` word (the smallest index of the run).  The scan is the window
 * entry's, three launches ordered on the stream on the sort's units ("sort.max_units" caps them here too; the result never depends on
 * it): a reduce per unit, a one-workgroup carry over the at most 2048 unit summaries, an apply per unit.  It carries the maximum of
 * (landing position + 1) and restarts at partition heads; the apply maps the position to its row of S through the permutation, tests
 * the tolerance with two gathered loads under the flag only, and stores out[row of R] at every position of R, RHJ_NO_ROW included.
 * No workgroup waits on another inside a kernel, and no position, value or count comes from an atomic: the matches are counted per
 * unit and summed on the host.
 * Costs in bytes per row of nR + nS: the concatenation 16 (32 with `by`); the sorts (see there) plus 24 for the gather between two of
 * them; heads 8 + 1, 8 more with `by`, a gathered 8 more for forward; reduce 1; apply 1 + 8 and, per row of R, one gathered 8-byte
 * load and one scattered 8-byte store (two gathered loads more under the tolerance flag).
 * rhj_get_info: "last.asof_units" the units the scan was cut into, "last.asof_sorts" the inner sorts that ran (1 without `by`, else
 * 2; 0 when a table was empty), "last.asof_matched" the matched rows; all three are 0 after every other call.  After an as-of call
 * "last.join_kernel" is -1 and "last.sort_*" / "last.topk_*" / "last.window_*" are 0.  "asof.tile_rows": the positions one workgroup
 * scans at once, a constant of the build.
 * Memory: a workspace buffer of its own (the inner sorts regrow the sort's), kept until rhj_release_workspace: 2 x 8 + 1 bytes per row
 * of nR + nS, 5 x 8 + 1 with `by`.
 * Out of scope: direction "nearest" is not part of this entry -- a backward call, a forward call and a caller-side comparison of the
 * two distances give it.  There is no 16-byte tuple form: a table here has two key columns. */
#define RHJ_ASOF_I64        1u   /* order the `on` words as two's-complement int64 (default: unsigned), as RHJ_SORT_I64 */
#define RHJ_ASOF_FORWARD    2u   /* the nearest row of S at or AFTER (default: at or before) */
#define RHJ_ASOF_STRICT     4u   /* exclude equal `on` words (pandas allow_exact_matches=False) */
#define RHJ_ASOF_TOLERANCE  8u   /* only partners whose distance is <= tolerance; without the bit `tolerance` is ignored */
int rhj_asof_cols_dev(rhj_ctx *ctx, const uint64_t *d_byR, const uint64_t *d_onR, uint64_t nR,
                      const uint64_t *d_byS, const uint64_t *d_onS, uint64_t nS, uint32_t flags, uint64_t tolerance,
                      uint64_t *d_out_rowS, uint64_t *out_matched);

/* ---- sort: a stable radix sort of one 64-bit key column with rowIDs (ORDER BY, argsort; the ordered half of what the operators above
 * return "in no particular order").
 * Tuple i is (d_keys[i], d_rows[i]); with d_rows == NULL the rowID is the position i.  Output position p holds the tuple of rank p:
 * d_out_keys[p] its key word, the original word bit for bit, d_out_rows[p] its rowID.  Ascending order is by key word in the chosen
 * view: unsigned 64-bit by default, two's-complement int64 under RHJ_SORT_I64 (an all-ones word is then -1, not the maximum).
 * RHJ_SORT_DESC reverses the key order only.  Ties keep their input order in both directions: tuples with equal keys come out in the
 * order they went in, ascending or descending -- torch.sort(stable=True, descending=..), np.argsort(kind="stable").  The result is
 * bit-identical from run to run.
 * Rows: with implicit rowIDs d_out_rows is the argsort permutation.  Explicit d_rows are opaque 64-bit payloads -- duplicates and
 * values >= 2^32 are fine: rows are carried, never compared and never used as indices.  That is what makes ORDER BY a, b work, as a
 * chain of stable sorts, last key first:
 *     rhj_sort_cols_dev(ctx, b, NULL, n, fb, NULL, perm1);              -- perm1 = argsort of b
 *     rhj_gather_u64(ctx, a, perm1, n, a1);                             -- a in that order
 *     rhj_sort_cols_dev(ctx, a1, perm1, n, fa, a_sorted, perm);         -- ties of a keep the order of b; perm[p] = the row of rank p
 * Outputs: either output may be NULL -- a keys-only sort (no d_out_rows; d_rows is then not read) or an argsort (no d_out_keys).  Both
 * outputs NULL with n > 0 is RHJ_E_INVALID.  Inputs are neither modified nor retained; outputs must not overlap inputs.  Pointers need
 * 8-byte alignment only (16 bytes everywhere lets every launch use 16-byte accesses; the kernels of this build use 8- and 4-byte ones).
 * n == 0: RHJ_OK, no launch.  RHJ_E_INVALID, before any launch: unknown flag bits; NULL d_keys with n > 0; both outputs NULL with
 * n > 0.  The call synchronises.  It honours rhj_set_stream and rhj_set_profiling (spans RHJ_K_HIST / RHJ_K_SCAN / RHJ_K_SCATTER per
 * pass, RHJ_K_AUX for the probes and the copy).
 * How: one probe launch finds the minimum and maximum of the column in the view; the width w is 0 when max == min, else 64 - clz(max -
 * min), and the keys are sorted as t(v) - t(min) (descending: t(max) - t(v)), t the order transform -- an int64 column of -3 .. 3 is 3
 * bits wide, a column of dense ids bits(groups - 1).  Digits are 8 bits from bit 0 of that word; a second probe launch (only when w > 8)
 * finds the digits in which every key agrees, and their passes are skipped.  Each remaining pass is three launches ordered on the
 * stream -- histogram per unit and digit, scan, stable scatter --; no workgroup waits on another inside a kernel.  The first pass reads
 * the caller's column and applies the transform, the last pass writes the caller's outputs with the key words restored; w == 0 runs no
 * pass: the outputs are copies (one launch).
 * rhj_get_info: "last.sort_bits" is w, "last.sort_passes" the scatter passes that ran, "last.sort_units" the units they were cut into; all are 0 after every other call.  After a
 * sort "last.join_kernel" is -1.  "sort.tile_rows": the rows one workgroup ranks at once, a constant of the build.
 * Costs: passes <= ceil(w / 8), however many rows repeat a key -- the sort has no skew case.  Bytes per pass and tuple, histogram
 * read + scatter read + scatter write:  keys only (no d_out_rows) 8 + 8 + 8 = 24;  narrow (implicit rowIDs, n <= 2^32: positions are
 * carried as 4 bytes between passes, not read in the first pass, widened to 8 in the last) 8 + 12 + 12 = 32;  wide (explicit d_rows,
 * or n > 2^32) 8 + 16 + 16 = 40.  An argsort's last pass stores no key: 8 bytes less.  Plus 8 bytes per tuple for each probe.
 * Memory: the ping-pong buffers live in the context's workspace, grown on demand and kept until rhj_release_workspace: nothing for
 * one pass, one set of n x (8 + 0 / 4 / 8) bytes for two, and from three passes on a second set only for the parts that are not a
 * plain output array of the call (a NULL output, the 16-byte form) -- the output arrays serve as the other side; plus 3 KiB of tables
 * per unit (at most 2048 units). */
#define RHJ_SORT_I64   1u   /* flags bit 0: order the words as two's-complement int64 (default: unsigned 64-bit) */
#define RHJ_SORT_DESC  2u   /* flags bit 1: descending */
int rhj_sort_cols_dev(rhj_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_rows, uint64_t n, uint32_t flags,
                      uint64_t *d_out_keys, uint64_t *d_out_rows);
/* ... on 16-byte tuples in and out (value = .payload, rowID = .key; the wide form, words at a stride of two) */
int rhj_sort_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t n, uint32_t flags, rhj_tuple *d_out);

/* ---- top-k and k-th value: a radix select in front of the sort (ORDER BY .. LIMIT k, the k largest, a median, a quantile).
 * With m = min(k, n) the outputs hold the first m tuples of what rhj_sort_cols_dev / rhj_sort_dev would write for the same (keys,
 * rows, n, flags), bit for bit, in the same positions: the result is sorted and the key words are the original words.  d_rows NULL:
 * rowID = index; explicit rows are opaque payloads, never compared and never used as indices.  flags: RHJ_SORT_I64 and RHJ_SORT_DESC
 * (RHJ_SORT_DESC: the k largest).  Ties keep their input order in both directions, also at the cut: where the k-th key repeats, the
 * tuples earliest in the input are the ones taken.  The result is bit-identical from run to run.
 * Outputs: arrays of m words (m tuples); no word at or past m is written.  out_kth is a HOST pointer to two words, or NULL: it
 * receives {key word, row word} of the tuple of rank m - 1 -- the k-th value, with k = (n + 1) / 2 a median, a quantile.  Either
 * device output may be NULL.  Both device outputs NULL is allowed if and only if out_kth is given: a pure selection, nothing of size
 * k is materialised.  Both device outputs NULL with out_kth NULL and n, k > 0 is RHJ_E_INVALID.  Inputs are neither modified nor
 * retained; outputs must not overlap inputs; pointers need 8-byte alignment.
 * n == 0 or k == 0: RHJ_OK, no launch, nothing written, out_kth untouched.  k >= n: the call is the sort, with the same launches and
 * the same "last.sort_*" (when out_kth is asked for and a device output is missing, the selection below runs with k = n instead).
 * RHJ_E_INVALID, before any launch: unknown flag bits; NULL d_keys with n > 0.  The call synchronises; it honours rhj_set_stream and
 * rhj_set_profiling (RHJ_K_HIST: the select histograms and the count; RHJ_K_SCAN; RHJ_K_SCATTER: the compaction; the inner sort's
 * spans add to the same call).
 * How: the sort's probe gives the width w and the sort key < 2^w (w == 0: the first m rows of the input, one copy launch, no pass).
 * Select: from the top 8-bit digit of w downward, on the sort's digit grid, one histogram launch per digit over the rows whose higher
 * digits equal the threshold's, and a one-workgroup launch that picks the digit in which rank m - 1 falls; the rows of smaller digits
 * are SURE to be in the result (M of them, M <= m - 1), the c rows of the picked digit are the CANDIDATES.  The host reads the 32-byte
 * state after each digit and stops when c <= "topk.max_candidates" or digit 0 is done (n <= "topk.max_candidates": no select pass at
 * all).  Keep: a count per unit, a scan over the units and a compaction write the sure rows and the candidates, raw key words and
 * 64-bit rows, in INPUT ORDER into the workspace -- positions come from ballots, per-wave counts, running cursors and the scan, never
 * from atomics, which is what makes the cut stable and the result deterministic.  When the digits ran out every candidate holds the
 * k-th key itself and only the first m - M of them are kept (a 16-value column hands the sort m rows, not n / 16).  In a pure selection
 * no sure row is kept, only the candidates (of such a run: one).  Order: the sort runs over the kept rows, straight into the caller's
 * arrays when exactly m rows were kept, else into the workspace, and a copy launch emits the first m.  No workgroup waits on another.
 * Costs: passes <= ceil(w / 8).  Bytes per tuple of the INPUT: a probe of 8, one to three select passes of 8 each (full-range keys
 * under the automatic cap: two), a count of 8 and a compaction read of 8 = 32 .. 48, once, against 112 .. 272 for the sort (96 .. 256
 * in its passes plus 16 in its probes); plus the sort of the kept rows.  (A tie run at the threshold that is longer than the cap
 * only ends when the digits do: up to ceil(w / 8) select passes, after which exactly m rows are sorted.)  The bound: "last.topk_sorted_rows" <= m + "topk.max_candidates"
 * (from M <= m - 1); in a pure selection <= "topk.max_candidates", or 1 when the digits ran out.
 * rhj_get_info: "last.topk_bits" is w, "last.topk_passes" the select histograms that ran, "last.topk_candidates" the tuples still tied
 * with the threshold's digits when selection stopped, "last.topk_sorted_rows" the rows handed to the inner sort; all four are 0 after
 * every other call.  On the select path "last.sort_*" stay 0 and "last.join_kernel" is -1.  "topk.auto_candidates": a constant of the
 * build -- the automatic "topk.max_candidates" is max(k, "topk.auto_candidates").
 * rhj_set_option: "topk.max_candidates": -1 automatic, 1 .. 2^31 - 1: selection goes on while more rows than this are tied (a test
 * knob like "sort.max_units": the result never depends on it).  "sort.max_units" also caps the units of the histogram, count and
 * compact launches.
 * Memory: the select state, the tables and the kept rows live in a workspace buffer of their own (the inner sort regrows the sort's),
 * kept until rhj_release_workspace: up to 4 x 8 bytes per kept row. */
int rhj_topk_cols_dev(rhj_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_rows, uint64_t n, uint64_t k, uint32_t flags,
                      uint64_t *d_out_keys, uint64_t *d_out_rows, uint64_t *out_kth);
/* ... on 16-byte tuples in and out (value = .payload, rowID = .key); out_kth[0] is the value, out_kth[1] the rowID */
int rhj_topk_dev(rhj_ctx *ctx, const rhj_tuple *d_R, uint64_t n, uint64_t k, uint32_t flags, rhj_tuple *d_out, uint64_t *out_kth);

/* ---- window functions: a value per row from the rows before it in its partition (ROW_NUMBER / RANK / DENSE_RANK() OVER (PARTITION BY
 * k ORDER BY t), a running SUM / MIN / MAX, LAG / LEAD; pandas groupby.cumcount / rank / cumsum / cummin / cummax / shift; top-k per
 * group is ROW_NUMBER <= k).
 * Rows are the indices 0 .. n - 1.  d_part, d_order and every d_cols[j] are device columns of n words; ops, args, the two pointer
 * arrays and out_partitions are HOST memory.  A PARTITION is the set of rows with the same d_part word -- the word is compared for
 * equality only; d_part == NULL: one partition.  Inside a partition the rows are ordered by their d_order word under flags:
 * RHJ_SORT_I64 and RHJ_SORT_DESC, with the sort entry's meaning.  Ties keep their input order in both directions, so every result is
 * defined, and bit-identical from run to run.  d_order == NULL: input order, and every row is its own peer; a non-zero flags with
 * d_order == NULL is RHJ_E_INVALID.  Rows with equal order words in one partition are PEERS.
 * Ops: for row i at 0-based position q of its partition P, d_outs[j][i] receives -- the outputs are aligned with the input rows, not
 * in sorted order --
 *     RHJ_WIN_ROW_NUMBER   q + 1
 *     RHJ_WIN_RANK         1 + the rows of P whose order key is strictly before i's
 *     RHJ_WIN_DENSE_RANK   1 + the distinct order keys of P strictly before i's
 *     RHJ_WIN_LAG_ROW      the row at position q - off of P, RHJ_NO_ROW where there is none
 *     RHJ_WIN_LEAD_ROW     the row at position q + off of P, RHJ_NO_ROW where there is none
 *     RHJ_WIN_CUMSUM       the sum mod 2^64 of d_cols[j][r] over the rows r of P at positions <= q
 *     RHJ_WIN_CUMMIN_U64 / RHJ_WIN_CUMMAX_U64 / RHJ_WIN_CUMMIN_I64 / RHJ_WIN_CUMMAX_I64
 *                          the minimum / maximum of those words, unsigned or as two's-complement int64: bit for bit a column word
 * off = args[j] >= 1 for the two row ops; args == NULL: offset 1; args[j] is ignored for the other ops, d_cols[j] for the ops
 * without a column (d_cols may then be NULL).  The running aggregates use the frame ROWS UNBOUNDED PRECEDING -- every row up to and
 * including the current one, peers behind it excluded --, not SQL's default RANGE frame, under which peers share a value.  The same
 * column may be given several times; two equal output pointers are undefined.  Lag and lead of a PAYLOAD go through
 * rhj_gather_cols_fill, which reads RHJ_NO_ROW as "fill":
 *     ops = {RHJ_WIN_LAG_ROW}; rhj_window_cols_dev(ctx, k, t, n, RHJ_SORT_I64, ops, NULL, NULL, 1, &prev, NULL);   -- prev[i] = the row before i
 *     rhj_gather_cols_fill(ctx, &x, 1, n, prev, n, &fill, &x_lag);                                           -- x_lag[i] = x[prev[i]] or fill
 * A multi-column order is the sort entry's chain first (ORDER BY a, b), then this call on the columns gathered in that order with
 * d_order == NULL.
 * *out_partitions receives the number of partitions; it may be NULL.  n == 0: RHJ_OK, no launch, 0 partitions.  RHJ_E_INVALID,
 * before any launch, with a message naming the argument: unknown flag bits; flags without d_order; nops 0 or above
 * RHJ_WINDOW_MAX_OPS; NULL ops, d_outs or d_outs[j]; an op above RHJ_WIN_CUMMAX_I64; a lag or lead offset of 0; a NULL d_cols[j] for
 * a column op with n > 0.  Inputs are neither modified nor retained; outputs must not overlap inputs.  The call synchronises; it
 * honours rhj_set_stream and rhj_set_profiling (the inner sorts' spans; RHJ_K_AUX: heads, gather, the row ops; per scan RHJ_K_HIST,
 * RHJ_K_SCAN, RHJ_K_SCATTER).
 * How: the order (partition, order key, input position) from the stable sort -- d_order argsorted under flags, d_part gathered
 * through that permutation and sorted with the permutation as its rows; one sort when either column is NULL, none when both are (a
 * column of dense ids or a narrow range is few passes: the sort's probe).  One launch marks, per sorted position, whether it heads a
 * partition (its partition word differs from its predecessor's) and whether it heads a run of peers (or its order word does).  Every
 * result is then a scan over the sorted positions that restarts at heads, three launches ordered on the stream on the sort's units
 * ("sort.max_units" caps them here too): a reduce per unit -- "has a head" and the aggregate since the unit's last head --, a
 * one-workgroup carry over the at most 2048 unit summaries, an apply per unit that scans tile by tile from its carry-in and stores
 * out[perm[p]].  No workgroup waits on another inside a kernel, and no position or value comes from an atomic.  ROW_NUMBER, RANK,
 * LAG_ROW and LEAD_ROW follow from the partition start and the peer start of each position -- inclusive maximum scans of (head ?
 * position : 0), materialised once per call -- in one further launch; DENSE_RANK is the running count of peer heads; signed minimum
 * and maximum go through the 1 << 63 bias.
 * Costs in bytes per row: the sorts (see there) plus 24 for the gather between two of them; heads 9 .. 25; each start 1 + 1 + 8; the
 * row ops together 8 .. 40 read and one scattered 8-byte store each; each other op 2 x (1 + 8) read, for a column op two gathered
 * 8-byte loads more, and one scattered 8-byte store.
 * rhj_get_info: "last.window_units" the units the scans were cut into, "last.window_sorts" the inner sorts that ran (0, 1 or 2),
 * "last.window_partitions" the partitions; all three are 0 after every other call.  After a window call "last.join_kernel" is -1 and
 * "last.sort_*" / "last.topk_*" are 0.  "window.tile_rows": the positions one workgroup scans at once, a constant of the build.
 * Memory: a workspace buffer of its own (the inner sorts regrow the sort's), kept until rhj_release_workspace: up to 4 x 8 + 1 bytes
 * per row.
 * There is no 16-byte tuple form: two key columns do not fit a {key, payload} tuple. */
#define RHJ_WINDOW_MAX_OPS   4
#define RHJ_WIN_ROW_NUMBER   0   /* no column */
#define RHJ_WIN_RANK         1   /* no column */
#define RHJ_WIN_DENSE_RANK   2   /* no column */
#define RHJ_WIN_LAG_ROW      3   /* no column; args[j] = offset >= 1 */
#define RHJ_WIN_LEAD_ROW     4   /* no column; args[j] = offset >= 1 */
#define RHJ_WIN_CUMSUM       5   /* column; mod 2^64 */
#define RHJ_WIN_CUMMIN_U64   6
#define RHJ_WIN_CUMMAX_U64   7
#define RHJ_WIN_CUMMIN_I64   8
#define RHJ_WIN_CUMMAX_I64   9
int rhj_window_cols_dev(rhj_ctx *ctx, const uint64_t *d_part, const uint64_t *d_order, uint64_t n, uint32_t flags,
                        const uint32_t *ops, const uint64_t *args, const uint64_t *const *d_cols, uint32_t nops,
                        uint64_t *const *d_outs, uint64_t *out_partitions);

/* ---- stage entry points (device pointers), one per reference job body ---------------------
 * rhj_histogram: HistogramJob::run over the whole relation + the reduction of structs.cpp:168-173:
 *   d_hist[b] = #{ i : ((payload_i >> shift) & (2^bits-1)) == b },  d_hist has 2^bits uint64. */
int rhj_histogram(rhj_ctx *ctx, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t *d_hist);
/* rhj_prefix: the exclusive prefix of PartitionJob::run (JobScheduler.cpp:163-169):
 *   d_start[0]=0, d_start[b+1]=d_start[b]+d_hist[b]; d_start has nbins+1 uint64. */
int rhj_prefix(rhj_ctx *ctx, const uint64_t *d_hist, uint64_t nbins, uint64_t *d_start);
/* rhj_partition: relation_info::hash_relation (structs.cpp:144-204) generalised to one or two passes:
 *   d_out = tuples of d_in grouped by partition id  p = payload & (2^(bits1+bits2)-1)  laid out in the
 *   order  (p & (2^bits1-1)) * 2^bits2 + (p >> bits1)   [pass-1 digit major, pass-2 digit minor; with
 *   bits2 == 0 this is the reference's bucket order];  d_part_start[k], k in [0, 2^(bits1+bits2)], are
 *   the partition boundaries in that order.  Order of tuples INSIDE a partition is unspecified. */
int rhj_partition(rhj_ctx *ctx, const rhj_tuple *d_in, uint64_t n, int bits1, int bits2,
                  rhj_tuple *d_out, uint64_t *d_part_start);
/* rhj_partition_at: ONE scatter-partition pass on payload bits [shift, shift+bits): d_out grouped by that
 *   digit, d_part_start[2^bits + 1].  Used by the multi-GPU driver to split a shard by owner bits before
 *   the RCCL all-to-all; the owner bits lie above every bit the local plan uses. */
int rhj_partition_at(rhj_ctx *ctx, const rhj_tuple *d_in, uint64_t n, int shift, int bits,
                     rhj_tuple *d_out, uint64_t *d_part_start);
/* rhj_owner_histogram / rhj_owner_split: rhj_histogram / rhj_partition_at with the digit taken from bits [shift, shift+bits)
 *   of rhj_mix64(payload) instead of the payload; tuples are written UNCHANGED.  The multi-GPU owner split of 16-byte
 *   tuples (the wire format when the narrow one does not apply): the receiver runs rhj_join_dev on what arrives. */
int rhj_owner_histogram(rhj_ctx *ctx, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t *d_hist);
int rhj_owner_split(rhj_ctx *ctx, const rhj_tuple *d_in, uint64_t n, int shift, int bits,
                    rhj_tuple *d_out, uint64_t *d_class_start);
/* rhj_bucket_join: the JoinJob loop of Result.cpp:98-107 + JoinJob::run + Result::join_buckets +
 *   add_result: for every partition k with both sides non-empty, build an LDS hash table on the smaller
 *   side (S when |R_k| >= |S_k|, JobScheduler.cpp:187) and probe with the other; emit (rowR,rowS).
 *   radix_bits = number of low payload bits that are constant inside a partition (0 if unpartitioned). */
int rhj_bucket_join(rhj_ctx *ctx, const rhj_tuple *d_Rp, const uint64_t *d_startR,
                    const rhj_tuple *d_Sp, const uint64_t *d_startS, uint64_t nparts, int radix_bits,
                    int probe_split, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count);

/* ---- multi-GPU stage entry points (the reference has no distributed path) -------------------
 * One process per GPU; both relations range-sharded by row (structs.cpp:146-161 applied across GPUs instead of threads).
 * These calls are the COMPUTE of a sharded join; the two collectives between them (an all-gather of the class
 * histograms, an all-to-all of the tuples over RCCL / xGMI) belong to the host, which may be C++ with rccl.h or Python
 * with torch.distributed (radixhashjoin_amd/sharded.py runs exactly this schedule):
 *
 *   1. rhj_shard_stats  (R, side 0), (S, side 1)     class histogram of the shard at bits [shift, shift+bits) of
 *                                                    h = rhj_mix64(payload) and the range of its rowIDs   [16 B/tuple read]
 *   2. all-gather {histograms, rowID ranges}  ->  every rank derives the same contiguous class range per owner and its
 *      send / receive counts; key_base = the shard's smallest rowID (the narrow wire format needs max - min < 2^32)
 *   3. rhj_shard_split  per relation                 class split straight into the NARROW WIRE FORMAT:
 *         payloads  uint64[n]  at d_narrow_out, as h = rhj_mix64(payload): what every later stage works on   (8 B/tuple)
 *         rowIDs    uint32[n]  at d_narrow_out + rhj_narrow_key_offset(n), value = rowID - key_base   (4 B/tuple)
 *      tuples of one class contiguous, classes in order: 12 B/tuple cross xGMI instead of 16      [16 B read + 12 B written]
 *   4. all-to-all of the payload array and of the rowID array (same element counts; destination d gets classes
 *      [cut[d], cut[d+1]))
 *   5. rhj_shard_partition per relation              the local fused two-pass radix partition of what arrived (one histogram
 *      read of the payloads, two scatter passes).  The receive buffer is nseg sender segments; pass-1 units are cut at the
 *      segment boundaries, so that pass 2 knows the sender of every tuple it moves and can restore GLOBAL rowIDs
 *      (row0[sender] + local rowID), in the way `mode` names:
 *        RHJ_SHARD_PLAIN     every rowID of both relations is < 2^32 and every rank split with key_base 0: nothing to restore,
 *                            narrow partitions, the kernels of a single-GPU join
 *        RHJ_SHARD_TAGGED    narrow partitions, the sender number in the low 4 payload bits (dead by then), resolved by the
 *                            one-table bucket join (partitions that fit one LDS table)
 *        RHJ_SHARD_GLOBAL16  pass 2 writes 16-byte tuples with global rowIDs (larger partitions: the compact-table kernel has
 *                            no register left to carry tags in)
 *   6. rhj_shard_join                                bucket join of the two partitioned sides (Result.cpp:43-76 per bucket):
 *      global rowIDs, as if one GPU had joined everything.
 * Results stay sharded (every rank holds the pairs of the join values it owns).
 * rhj_shard_plan returns RHJ_SHARD_TAGGED or RHJ_SHARD_GLOBAL16 for sizes / plans that fit this path (the host may use
 * RHJ_SHARD_PLAIN instead when the gathered rowID ranges allow it), RHJ_SHARD_PLAIN for 17-18-bit local plans, or 0: fall back
 * to exchanging 16-byte tuples (rhj_owner_histogram + rhj_owner_split + all-to-all + rhj_join_dev).
 * Limits: at most 16 ranks (nseg), class bits <= 8, fewer than 2^32 tuples received per relation, a two-pass local plan;
 * 17-18-bit plans (receivers beyond 1.1 * 10^9 tuples) only as RHJ_SHARD_PLAIN, which is what rhj_shard_plan returns for them. */
#define RHJ_SHARD_TAGGED 1
#define RHJ_SHARD_GLOBAL16 2
#define RHJ_SHARD_PLAIN 3
uint64_t rhj_narrow_key_offset(uint64_t n);               /* byte offset of the rowID array inside a narrow buffer of n tuples */
uint64_t rhj_narrow_bytes(uint64_t n);                    /* bytes of a narrow buffer of n tuples (<= 16 n for n >= 1024) */
int rhj_shard_plan(uint64_t nR, uint64_t nS, const rhj_opts *in, rhj_opts *resolved);   /* mode / 0 / negative rhj_status */
/* hist: HOST array of 2^bits counts; key_min / key_max: HOST words (may be NULL).  Synchronises.  side: 0 or 1 -- two sets of
 * unit tables, so that R and S can both be between their rhj_shard_stats and their rhj_shard_split. */
int rhj_shard_stats(rhj_ctx *ctx, int side, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t *hist,
                    uint64_t *key_min, uint64_t *key_max);
/* asynchronous; d_narrow_out has rhj_narrow_bytes(n) bytes; d_class_start (device, 2^bits + 1, may be NULL) gets the class
 * boundaries inside the output.  Same d_rel / n / shift / bits as the rhj_shard_stats call of this side (key_base is checked
 * against the rowID range that call found; a different relation whose rowIDs do not fit is detected on the device and
 * reported by the rhj_shard_join of this context: RHJ_E_INVALID). */
int rhj_shard_split(rhj_ctx *ctx, int side, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t key_base,
                    void *d_narrow_out, uint64_t *d_class_start);
/* rhj_shard_split with NO send buffer and NO all-to-all: class c of this rank's shard is written straight into the receive
 * arrays of the rank that owns it -- peer_payloads[owner[c]] (uint64) / peer_rowids[owner[c]] (uint32), device pointers of
 * this process: a peer's HBM opened with rhj_ipc_open (xGMI peer stores), or local buffers -- starting at element
 * dst_class_start[c] of those arrays (from the gathered count matrix: where sender `rank`'s segment begins in the owner's
 * arrays + the sender's classes of that owner before c).  owner / dst_class_start: HOST arrays of 2^bits entries.
 * Same d_rel / n / shift / bits / key_base rules as rhj_shard_split; the receiver must not read its arrays before every
 * sender's call has completed (a barrier on the stream, e.g. a 1-word all-reduce), then runs rhj_shard_partition as usual.
 * HBM traffic per tuple: 16 B read + 12 B written, against + 12 B read + 12 B written by the all-to-all's copy. */
int rhj_shard_split_peer(rhj_ctx *ctx, int side, const rhj_tuple *d_rel, uint64_t n, int shift, int bits, uint64_t key_base,
                         const uint8_t *owner, const uint64_t *dst_class_start, void *const *peer_payloads, void *const *peer_rowids,
                         int nranks);
/* HBM of another process of the node mapped into this one (hipIpc*): export a 64-byte handle of a device allocation, open it
 * elsewhere, close it.  For the peer arrays of rhj_shard_split_peer.  Unverified on the one-GPU boxes of this pool. */
int rhj_ipc_export(rhj_ctx *ctx, void *d_ptr, void *handle64);
int rhj_ipc_open(rhj_ctx *ctx, const void *handle64, void **d_ptr);
int rhj_ipc_close(rhj_ctx *ctx, void *d_ptr);
/* asynchronous; seg_off: HOST array of nseg + 1 offsets into the received arrays (seg_off[0] = 0, seg_off[nseg] = m),
 * segment s = what rank s sent; row0: HOST array of nseg rowID bases (the key_base each rank split this relation with);
 * plan: the resolved two-pass plan rhj_shard_plan returned a mode for; plan and mode the same on both sides */
int rhj_shard_partition(rhj_ctx *ctx, int side, const uint64_t *d_payloads, const uint32_t *d_rowids, uint64_t m, int nseg,
                        const uint64_t *seg_off, const uint64_t *row0, const rhj_opts *plan, int mode);
/* count / overflow behaviour of rhj_join_dev */
int rhj_shard_join(rhj_ctx *ctx, rhj_pair *d_out, uint64_t out_capacity, uint64_t *out_count);

/* ---- utilities -------------------------------------------------------------------------- */
/* order-insensitive checksum of SURVEY.md App. A over a device pair array:
 *   sum over pairs of mix(keyR * 0x100000001B3 ^ mix(keyS))  (mod 2^64), mix = splitmix64 step */
int rhj_pairs_checksum_dev(rhj_ctx *ctx, const rhj_pair *d_pairs, uint64_t n, uint64_t *checksum);
/* synthetic inputs generated in HBM:  kind 0: R[i] = {i+row0, mix(1 + (i+row0) % D)}
 *   kind 1: uniform FK, counter based: S[j] = {j+row0, mix(1 + mix((j+row0) ^ seed) % D)}
 *   kind 2: Zipf(theta) FK: rank r in [1,D] by inverse-CDF of the continuous approximation from
 *           u = mix((j+row0) ^ seed) / 2^64; payload = mix(r)            (theta given as theta_milli/1000)
 *   kind 3: disjoint: S[j] = {j+row0, mix(D + 1 + j + row0)}
 *   kind 4: constant: T[i] = {i+row0, D} */
int rhj_generate_dev(rhj_ctx *ctx, int kind, rhj_tuple *d_out, uint64_t n, uint64_t row0, uint64_t D,
                     uint64_t seed, int theta_milli);
/* Re-labels the join values of a GENERATED relation in place: payload = (k << shift) + add for a payload rhj_mix64(k)
 *   (kinds 0-3 above).  Applied to both sides of a PK/FK pair of relations it leaves the pair set -- hence
 *   rhj_expected_pkfk_dev's answer, taken BEFORE the call -- unchanged while the join values become dense (shift 0: the
 *   value range of the reference's small/ data), multiples of 2^shift, or k * 2^shift + const. */
int rhj_remap_keys_dev(rhj_ctx *ctx, rhj_tuple *d_rel, uint64_t n, int shift, uint64_t add);
/* closed-form expectation for PK/FK inputs (R of kind 0 with D == |R| global, unique payloads):
 *   every S tuple {j, mix(k)} matches exactly R row k-1: *count = n, *checksum = sum mix((k-1)*0x100000001B3 ^ mix(j)).
 *   Computed by one streaming pass over S that inverts mix(); does not run the join. */
int rhj_expected_pkfk_dev(rhj_ctx *ctx, const rhj_tuple *d_S, uint64_t n, uint64_t *count, uint64_t *checksum);

/* ---- query-layer kernels (the steps immediately before and after the hot path) -------------
 * With the columns of the stored relations resident in HBM these make a whole query device-resident:
 * filters, join-input construction, intermediate-result maintenance and the SUM projections never
 * cross PCIe; only counts and 8-byte sums reach the host.  All arrays are uint64 in HBM.  A NULL row list
 * (d_rows / d_rowsA / d_rowsB / d_rows_in) stands for the identity 0..n-1 (an alias without filters).
 *
 * rhj_col_filter: the filter loops of Query::run_filters (Query.cpp:96-146).  d_rows_in == NULL means
 *   "all rows 0..n_in-1".  Keeps the rows r with  d_col[r] <op> value,  op in {'<','>','='}; writes them
 *   (unordered) to d_rows_out (capacity n_in) and their number to *n_out. */
int rhj_col_filter(rhj_ctx *ctx, const uint64_t *d_col, const uint64_t *d_rows_in, uint64_t n_in, int op,
                   uint64_t value, uint64_t *d_rows_out, uint64_t *n_out);
/* rhj_gather_tuples: relation::foo / create_relation (structs.cpp:217-243) without the host round trip:
 *   d_tuples[i] = { key = key_is_position ? i : d_rows[i],  payload = d_col[d_rows[i]] }.
 *   key_is_position = 1 builds a POSITION-CARRYING join input: the join's pairs then name intermediate rows
 *   directly, which replaces the de-duplication of structs.cpp:238-241 and the rescans of
 *   intermediate.cpp:52-87 by one gather. */
int rhj_gather_tuples(rhj_ctx *ctx, const uint64_t *d_col, const uint64_t *d_rows, uint64_t n, int key_is_position,
                      rhj_tuple *d_tuples);
/* rhj_pairs_split: getVector (intermediate.cpp:92-105): d_r[i] = pairs[i].keyR, d_s[i] = pairs[i].keyS */
int rhj_pairs_split(rhj_ctx *ctx, const rhj_pair *d_pairs, uint64_t n, uint64_t *d_r, uint64_t *d_s);
/* rhj_gather_u64: d_dst[i] = d_src[d_idx[i]]  (re-materialises one intermediate column after a join) */
int rhj_gather_u64(rhj_ctx *ctx, const uint64_t *d_src, const uint64_t *d_idx, uint64_t n, uint64_t *d_dst);
/* rhj_gather_cols_fill: for i < n and j < ncols: d_dsts[j][i] = d_idx[i] == RHJ_NO_ROW ? fills[j] : d_srcs[j][d_idx[i]]
 *   -- the index column of rhj_lookup_cols_dev, or one side of an outer join's pairs, turned into up to RHJ_LOOKUP_MAX_COLS payload
 *   columns; d_idx is read once for all columns.  d_srcs / fills / d_dsts: HOST arrays of ncols (1 .. RHJ_LOOKUP_MAX_COLS) device
 *   columns of src_rows words / fill values / device columns of n words.  Any other index >= src_rows is never dereferenced: it
 *   raises a flag word in HBM and the call returns RHJ_E_INVALID (the destinations are then undefined, the context stays usable),
 *   so the call synchronises, unlike rhj_gather_u64.  n == 0: no launch.  A destination may not overlap d_idx or a source. */
int rhj_gather_cols_fill(rhj_ctx *ctx, const uint64_t *const *d_srcs, uint32_t ncols, uint64_t src_rows,
                         const uint64_t *d_idx, uint64_t n, const uint64_t *fills, uint64_t *const *d_dsts);
/* rhj_rows_filter_equal: a predicate between two aliases that are BOTH in the intermediate already
 *   (intermediate.cpp:72-87,169-180) or a same-alias predicate (parse_table, intermediate.cpp:11-44):
 *   keeps the positions e with d_colA[d_rowsA[e]] == d_colB[d_rowsB[e]] in d_pos_out (capacity n). */
int rhj_rows_filter_equal(rhj_ctx *ctx, const uint64_t *d_colA, const uint64_t *d_rowsA, const uint64_t *d_colB,
                          const uint64_t *d_rowsB, uint64_t n, uint64_t *d_pos_out, uint64_t *n_out);
/* rhj_sum_gather: column_proj (Query.cpp:66-74): *sum = sum of d_col[d_rows[i]] (mod 2^64) */
int rhj_sum_gather(rhj_ctx *ctx, const uint64_t *d_col, const uint64_t *d_rows, uint64_t n, uint64_t *sum);
/* rhj_mul_u64: d_dst[i] = d_a[i] * d_b[i]  (mod 2^64); d_dst may be d_a (the product of a tree query's messages) */
int rhj_mul_u64(rhj_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t n, uint64_t *d_dst);
/* rhj_sum_gather_weighted: *sum = sum of d_col[d_rows[i]] * d_w[i]  (mod 2^64); d_rows == NULL: the row is i;
 *   d_col == NULL: *sum = sum of d_w[i].  sum is a HOST word; the call synchronises. */
int rhj_sum_gather_weighted(rhj_ctx *ctx, const uint64_t *d_col, const uint64_t *d_rows, const uint64_t *d_w, uint64_t n,
                            uint64_t *sum);

/* raw HBM helpers so a plain C/C++ host (no HIP headers) can use the device-resident API.  rhj_dev_free must be
 * given the context that allocated the block; released blocks are kept by the context for re-use (its work is
 * ordered on one stream) and go back to the device with rhj_release_workspace / rhj_destroy. */
int rhj_dev_alloc(rhj_ctx *ctx, uint64_t bytes, void **d_ptr);
int rhj_dev_free(rhj_ctx *ctx, void *d_ptr);
int rhj_copy_h2d(rhj_ctx *ctx, void *d_dst, const void *src, uint64_t bytes);
int rhj_copy_d2h(rhj_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);
int rhj_dev_mem_info(rhj_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RHJ_H */
