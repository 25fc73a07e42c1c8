// entries.cpp -- a characterization of the device entries of rhj_api.hip, rhj_join_dev through rhj_group_join_agg_ids_cols_dev, over
// the fake runtime and the fake launchers of fake_hip.cpp (make -C radixhashjoin_amd/csrc -f Makefile.sanitize entries).  Nothing
// here computes a join.  Every call prints what a caller can observe -- the return code, the error text, the out words, the "last.*"
// infos, the plan and task count of rhj_get_timings, the span kinds of rhj_get_launch_timings -- and the trace of fake_hip.cpp: every
// stream operation and launcher call the entry made, in order, with its scalar arguments.  tests/test_host_entries.py compares the
// output with tests/golden/host_entries_trace.txt line for line: host code that changes a line of it has changed behaviour.
#include "../../../include/rhj.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

void fake_trace_into(std::string *sink);                 // fake_hip.cpp

typedef uint64_t u64;
static std::string g_trace;
static const u64 NMAX = 4096;                            // tuples / words of every input buffer below; no call asks for more
static const u64 BIG = (u64)4 << 20;                     // the default capacity: above what the fake kernels report (2^20 per launch, three launches
                                                         // in a full outer join), so that a normal call ends well

// "device" memory: the fakes read no input; they write pairs, rowIDs and words below the capacity they are given, and nothing into the
// arrays of a group-by (keys, counts, sums, rows: small, whatever capacity the call names)
static std::vector<rhj_tuple> g_R(NMAX), g_S(NMAX);
static std::vector<u64> g_val[2] = {std::vector<u64>(NMAX), std::vector<u64>(NMAX)}, g_id[2] = {std::vector<u64>(NMAX), std::vector<u64>(NMAX)};
static std::vector<u64> g_col[2][4], g_sum[2][4], g_rows[4], g_keys(NMAX), g_cnt[2] = {std::vector<u64>(NMAX), std::vector<u64>(NMAX)};
static std::vector<u64> g_gid[2] = {std::vector<u64>(NMAX), std::vector<u64>(NMAX)}, g_words(BIG), g_w(NMAX);
static std::vector<rhj_pair> g_pairs(BIG);

static const uint32_t OPS_MIX[4] = {RHJ_AGG_SUM, RHJ_AGG_MIN_U64, RHJ_AGG_MAX_I64, RHJ_AGG_SUM};
static const uint32_t ARG_OPS[4] = {RHJ_ARG_MIN_U64, RHJ_ARG_ROW, RHJ_ARG_MAX_I64, RHJ_ARG_ROW}, ARG_TIES[4] = {0, 1, 0, 1};

// the arguments of one call: every entry takes the ones it has
struct A {
    bool cols = false;
    u64 nR = 1000, nS = 1000;
    const rhj_opts *opts = nullptr;
    int variant = 0;                                     // kind / how / which / mode
    u64 cap = BIG;                                       // out_capacity / out_rows
    bool count_only = false;                             // null outputs
    bool null_ctx = false, null_word = false, null_R = false, null_S = false;
    uint32_t ncols = 2, ncolsS = 1;
    const uint32_t *ops = OPS_MIX, *opsS = OPS_MIX, *ties = ARG_TIES;
    bool null_cols = false, null_colsS = false, null_sums = false, null_sumsS = false, null_rows = false, null_d_out = false;
    int null_col_slot = -1, null_colS_slot = -1, null_sum_slot = -1, null_row_slot = -1;
    bool ids = true;                                     // the ids entries: with id arrays
};

static std::string words(const char *name, const u64 *w, int n)
{
    std::string s = name;
    for (int i = 0; i < n; i++) s += (i ? "," : "=") + std::to_string(w[i]);
    return s + "\n";
}

struct Ptrs {                                            // the pointer arguments A asks for
    rhj_ctx *ctx;
    const rhj_tuple *R, *S;
    const u64 *valR, *idR, *valS, *idS;
    const u64 *colsR[4], *colsS[4];
    u64 *sumsR[4], *sumsS[4], *rows[4];
    const u64 *const *pcolsR, *const *pcolsS;
    u64 *const *psumsR, *const *psumsS, *const *prows;
    u64 word, *pword;
    Ptrs(rhj_ctx *c, const A &a) : ctx(a.null_ctx ? nullptr : c)
    {
        R = a.null_R ? nullptr : g_R.data(); S = a.null_S ? nullptr : g_S.data();
        valR = a.null_R ? nullptr : g_val[0].data(); idR = g_id[0].data();
        valS = a.null_S ? nullptr : g_val[1].data(); idS = g_id[1].data();
        for (int j = 0; j < 4; j++) {
            colsR[j] = j == a.null_col_slot ? nullptr : g_col[0][j].data(); colsS[j] = j == a.null_colS_slot ? nullptr : g_col[1][j].data();
            sumsR[j] = j == a.null_sum_slot ? nullptr : g_sum[0][j].data(); sumsS[j] = g_sum[1][j].data();
            rows[j] = j == a.null_row_slot ? nullptr : g_rows[j].data();
        }
        pcolsR = a.null_cols ? nullptr : colsR; pcolsS = a.null_colsS ? nullptr : colsS;
        psumsR = a.null_sums ? nullptr : sumsR; psumsS = a.null_sumsS ? nullptr : sumsS; prows = a.null_rows ? nullptr : rows;
        word = 0xDEADu; pword = a.null_word ? nullptr : &word;
    }
};

// ---- the entries, one function per pair of twins ------------------------------------------------------------------------
typedef int (*Entry)(rhj_ctx *, const A &, std::string &);

static int e_join(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    rhj_pair *out = a.count_only ? nullptr : g_pairs.data();
    const int rc = a.cols ? rhj_join_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, p.idS, a.nS, a.opts, out, a.cap, p.pword)
                          : rhj_join_dev(p.ctx, p.R, a.nR, p.S, a.nS, a.opts, out, a.cap, p.pword);
    o += words("out_count", &p.word, 1);
    return rc;
}
static int e_semi(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *out = a.count_only ? nullptr : g_words.data();
    const int rc = a.cols ? rhj_semi_join_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, a.nS, a.variant, a.opts, out, a.cap, p.pword)
                          : rhj_semi_join_dev(p.ctx, p.R, a.nR, p.S, a.nS, a.variant, a.opts, out, a.cap, p.pword);
    o += words("out_count", &p.word, 1);
    return rc;
}
static int e_outer(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    rhj_pair *out = a.count_only ? nullptr : g_pairs.data();
    u64 sec[3] = {7, 7, 7};
    const int rc = a.cols ? rhj_outer_join_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, p.idS, a.nS, a.variant, a.opts, out, a.cap, p.pword, sec)
                          : rhj_outer_join_dev(p.ctx, p.R, a.nR, p.S, a.nS, a.variant, a.opts, out, a.cap, p.pword, sec);
    o += words("out_count", &p.word, 1) + words("sections", sec, 3);
    return rc;
}
static int e_sum(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 sums[4] = {9, 9, 9, 9};
    u64 *ps = a.null_sums ? nullptr : sums;
    const int rc = a.cols ? rhj_join_sum_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, a.nS, p.pcolsR, a.ncols, 1000, a.opts, p.pword, ps)
                          : rhj_join_sum_dev(p.ctx, p.R, a.nR, p.S, a.nS, p.pcolsR, a.ncols, 1000, a.opts, p.pword, ps);
    o += words("out_count", &p.word, 1) + words("sums", sums, 4);
    return rc;
}
static int e_mult(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *out = a.count_only || a.null_d_out ? nullptr : g_words.data();
    const u64 rows = a.count_only ? 0 : a.cap;
    const u64 *w = a.variant ? g_w.data() : nullptr;     // variant 1: weighted
    const int rc = a.cols ? rhj_join_mult_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, p.idS, a.nS, w, 1000, a.opts, out, rows, p.pword)
                          : rhj_join_mult_dev(p.ctx, p.R, a.nR, p.S, a.nS, w, 1000, a.opts, out, rows, p.pword);
    o += words("out_total", &p.word, 1);
    return rc;
}
static int e_lookup(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *out = a.count_only || a.null_d_out ? nullptr : g_words.data();
    const u64 rows = a.count_only ? 0 : a.cap;
    const int rc = a.cols ? rhj_lookup_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, p.idS, a.nS, a.variant, a.opts, out, rows, p.pword)
                          : rhj_lookup_dev(p.ctx, p.R, a.nR, p.S, a.nS, a.variant, a.opts, out, rows, p.pword);
    o += words("out_matched", &p.word, 1);
    return rc;
}
static int e_group_sum(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *keys = a.count_only ? nullptr : g_keys.data();
    const int rc = a.cols ? rhj_group_sum_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.pcolsR, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR, a.cap, p.pword)
                          : rhj_group_sum_dev(p.ctx, p.R, a.nR, p.pcolsR, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR, a.cap, p.pword);
    o += words("out_groups", &p.word, 1);
    return rc;
}
static int e_group_agg(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *keys = a.count_only ? nullptr : g_keys.data();
    const int rc = a.cols ? rhj_group_agg_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.pcolsR, a.ops, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR, a.cap, p.pword)
                          : rhj_group_agg_dev(p.ctx, p.R, a.nR, p.pcolsR, a.ops, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR, a.cap, p.pword);
    o += words("out_groups", &p.word, 1);
    return rc;
}
static int e_group_ids(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *keys = a.count_only ? nullptr : g_keys.data(), *gid = a.ids ? g_gid[0].data() : nullptr;
    const int rc = a.cols ? rhj_group_agg_ids_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.pcolsR, a.ops, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR,
                                                       a.cap, p.pword, gid, 1000)
                          : rhj_group_agg_ids_dev(p.ctx, p.R, a.nR, p.pcolsR, a.ops, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR, a.cap, p.pword,
                                                  gid, 1000);
    o += words("out_groups", &p.word, 1);
    return rc;
}
static int e_group_arg(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *keys = a.count_only ? nullptr : g_keys.data();
    const uint32_t *ops = a.ops == OPS_MIX ? ARG_OPS : a.ops;
    const int rc = a.cols ? rhj_group_arg_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.pcolsR, ops, a.ties, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR,
                                                   p.prows, a.cap, p.pword)
                          : rhj_group_arg_dev(p.ctx, p.R, a.nR, p.pcolsR, ops, a.ties, a.ncols, 1000, a.opts, keys, g_cnt[0].data(), p.psumsR, p.prows, a.cap,
                                              p.pword);
    o += words("out_groups", &p.word, 1);
    return rc;
}
static int e_gjoin(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *keys = a.count_only ? nullptr : g_keys.data();
    const int rc = a.cols ? rhj_group_join_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, p.idS, a.nS, p.pcolsR, a.ncols, 1000, p.pcolsS, a.ncolsS, 1000,
                                                    a.variant, a.opts, keys, g_cnt[0].data(), g_cnt[1].data(), p.psumsR, p.psumsS, a.cap, p.pword)
                          : rhj_group_join_dev(p.ctx, p.R, a.nR, p.S, a.nS, p.pcolsR, a.ncols, 1000, p.pcolsS, a.ncolsS, 1000, a.variant, a.opts, keys,
                                               g_cnt[0].data(), g_cnt[1].data(), p.psumsR, p.psumsS, a.cap, p.pword);
    o += words("out_groups", &p.word, 1);
    return rc;
}
static int e_gjoin_agg(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *keys = a.count_only ? nullptr : g_keys.data();
    const int rc = a.cols ? rhj_group_join_agg_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, p.idS, a.nS, p.pcolsR, a.ops, a.ncols, 1000, p.pcolsS, a.opsS,
                                                        a.ncolsS, 1000, a.variant, a.opts, keys, g_cnt[0].data(), g_cnt[1].data(), p.psumsR, p.psumsS, a.cap,
                                                        p.pword)
                          : rhj_group_join_agg_dev(p.ctx, p.R, a.nR, p.S, a.nS, p.pcolsR, a.ops, a.ncols, 1000, p.pcolsS, a.opsS, a.ncolsS, 1000, a.variant,
                                                   a.opts, keys, g_cnt[0].data(), g_cnt[1].data(), p.psumsR, p.psumsS, a.cap, p.pword);
    o += words("out_groups", &p.word, 1);
    return rc;
}
static int e_gjoin_ids(rhj_ctx *c, const A &a, std::string &o)
{
    Ptrs p(c, a);
    u64 *keys = a.count_only ? nullptr : g_keys.data(), *gR = a.ids ? g_gid[0].data() : nullptr, *gS = a.ids ? g_gid[1].data() : nullptr;
    const int rc = a.cols ? rhj_group_join_agg_ids_cols_dev(p.ctx, p.valR, p.idR, a.nR, p.valS, p.idS, a.nS, p.pcolsR, a.ops, a.ncols, 1000, p.pcolsS, a.opsS,
                                                            a.ncolsS, 1000, a.variant, a.opts, keys, g_cnt[0].data(), g_cnt[1].data(), p.psumsR, p.psumsS,
                                                            a.cap, p.pword, gR, 1000, gS, 900)
                          : rhj_group_join_agg_ids_dev(p.ctx, p.R, a.nR, p.S, a.nS, p.pcolsR, a.ops, a.ncols, 1000, p.pcolsS, a.opsS, a.ncolsS, 1000,
                                                       a.variant, a.opts, keys, g_cnt[0].data(), g_cnt[1].data(), p.psumsR, p.psumsS, a.cap, p.pword, gR,
                                                       1000, gS, 900);
    o += words("out_groups", &p.word, 1);
    return rc;
}

struct Family { const char *name; Entry call; int variants; bool has_S; };
static const Family FAMILIES[] = {
    {"join", e_join, 1, true},           {"semi_join", e_semi, 2, true},       {"outer_join", e_outer, 3, true},
    {"join_sum", e_sum, 1, true},        {"join_mult", e_mult, 2, true},       {"lookup", e_lookup, 2, true},
    {"group_sum", e_group_sum, 1, false}, {"group_agg", e_group_agg, 1, false}, {"group_agg_ids", e_group_ids, 1, false},
    {"group_arg", e_group_arg, 1, false}, {"group_join", e_gjoin, 2, true},     {"group_join_agg", e_gjoin_agg, 2, true},
    {"group_join_agg_ids", e_gjoin_ids, 2, true},
};
static int first_variant(const Family &f) { return f.call == e_outer ? RHJ_OUTER_LEFT : 0; }

// ---- one call and everything a caller can see of it -------------------------------------------------------------------------
static const char *INFOS[] = {"last.narrow", "last.countfree_R", "last.countfree_S", "last.countfree2_R", "last.countfree2_S", "last.cols_R",
                              "last.cols_S", "last.join_kernel", "last.pipelined", "last.max_part_R", "last.max_part_S", "last.semi_tables",
                              "last.group_rounds", "last.outer_sweeps", "last.sort_bits", "last.topk_bits"};

// What one call shows: a line of what the caller sees (the infos that are not 0), and the trace.
struct Seen {
    std::string head, trace;
    bool operator==(const Seen &o) const { return head == o.head && trace == o.trace; }
};

static Seen observe(rhj_ctx *ctx, const Family &f, const A &a)
{
    g_trace.clear();
    std::string outs;
    const int rc = f.call(ctx, a, outs);
    Seen s;
    s.trace = g_trace;                                   // (the questions below synchronise: not part of the call)
    for (char &c : outs) if (c == '\n') c = ' ';
    s.head = "rc=" + std::to_string(rc) + " " + outs;
    if (rc != RHJ_OK) s.head += std::string("error=\"") + rhj_last_error(a.null_ctx ? nullptr : ctx) + "\" ";
    s.head += "| last";
    for (const char *name : INFOS) {
        int64_t v = -99;
        (void)rhj_get_info(ctx, name, &v);
        if (v != 0) s.head += std::string(" ") + (name + 5) + "=" + std::to_string(v);
    }
    rhj_timings tm;
    memset(&tm, 0, sizeof tm);
    (void)rhj_get_timings(ctx, &tm);
    s.head += " | plan " + std::to_string(tm.passes) + "/" + std::to_string(tm.bits1) + "/" + std::to_string(tm.bits2) + " ntasks=" +
              std::to_string(tm.ntasks) + " | kinds";
    int32_t kinds[256];
    double ms[256];
    uint32_t n = 0;
    (void)rhj_get_launch_timings(ctx, kinds, ms, 256, &n);
    for (uint32_t i = 0; i < n && i < 256; i++) s.head += " " + std::to_string(kinds[i]);
    return s;
}

static rhj_ctx *fresh(int profiling = 1)
{
    rhj_ctx *ctx = nullptr;
    if (rhj_init(0, &ctx) != RHJ_OK) { fprintf(stderr, "rhj_init failed\n"); exit(2); }
    (void)rhj_set_profiling(ctx, profiling);
    return ctx;
}

// A trace is printed in two parts: the partition phase -- up to its last launcher, the same for every operator under the same plan --
// and what follows it, the operator's own phase.  A part is printed in full the first time a call shows it, under a number; a later
// call with the same lines names the number at the end of its line.  Nothing is left out: every call's whole trace can be read off the file.
static bool partition_op(const std::string &line)
{
    static const char *ops[] = {"hist", "scan_", "scatter_", "make_group_ranges", "make_units", "pass_pair", "cf", "seg_units", "diff_hist",
                                "prefix", "cols_to_tuples", "fused_pass", "  minmax"};
    for (const char *op : ops) if (line.compare(0, strlen(op), op) == 0) return true;
    return false;
}
static std::string part(const char *kind, std::vector<std::string> &seen, const std::string &text, std::string &fresh_parts)
{
    if (text.empty()) return "";
    size_t i = 0;
    while (i < seen.size() && seen[i] != text) i++;
    const std::string name = std::string(kind) + " " + std::to_string(i + 1);
    if (i == seen.size()) { seen.push_back(text); fresh_parts += name + ":\n" + text; }
    return " | " + name;
}
static void print_seen(const Seen &s)
{
    static std::vector<std::string> partitions, phases;
    size_t cut = 0;                                      // behind the last line of the partition phase
    for (size_t at = 0; at < s.trace.size();) {
        const size_t end = s.trace.find('\n', at) + 1;
        if (partition_op(s.trace.substr(at, end - at))) cut = end;
        at = end;
    }
    std::string fresh_parts;
    const std::string names = part("partition", partitions, s.trace.substr(0, cut), fresh_parts) + part("phase", phases, s.trace.substr(cut), fresh_parts);
    printf("%s%s\n%s", s.head.c_str(), names.c_str(), fresh_parts.c_str());
}

static void show(rhj_ctx *ctx, const Family &f, const A &a, const std::string &label)
{
    printf("== %s%s %s: ", f.name, a.cols ? "_cols" : "", label.c_str());
    print_seen(observe(ctx, f, a));
}

// the second call of a pair must read as the same call on a fresh context
static void after(rhj_ctx *ctx, const Family &f, const A &a, const std::string &label)
{
    rhj_ctx *alone = fresh();
    const Seen want = observe(alone, f, a), got = observe(ctx, f, a);
    rhj_destroy(alone);
    printf("== %s%s %s: %s\n", f.name, a.cols ? "_cols" : "", label.c_str(), want == got ? "as on a fresh context" : "DIFFERS from a fresh context");
    if (!(want == got)) printf("-- fresh\n%s\n%s-- here\n%s\n%s", want.head.c_str(), want.trace.c_str(), got.head.c_str(), got.trace.c_str());
}


static void invalid_calls(rhj_ctx *ctx, const Family &f, bool cols)
{
    auto bad = [&](const char *label, const std::function<void(A &)> &set) {
        A a;
        a.cols = cols;
        a.variant = first_variant(f);
        set(a);
        show(ctx, f, a, std::string("invalid: ") + label);
    };
    static const rhj_opts bad_opts = {5, 0, 0, 0};
    static const uint32_t ops_bad[4] = {0, 9, 0, 0}, opsS_bad[4] = {9, 0, 0, 0}, ties_bad[4] = {0, 7, 0, 0};
    static const uint32_t ops_value[4] = {RHJ_ARG_MIN_U64, RHJ_ARG_MIN_U64, 0, 0};
    bad("null context", [](A &a) { a.null_ctx = true; });
    bad("null out word", [](A &a) { a.null_word = true; });
    bad("null R", [](A &a) { a.null_R = true; });
    if (f.has_S) bad("null S", [](A &a) { a.null_S = true; });
    bad("bad opts", [](A &a) { a.opts = &bad_opts; });
    if (f.call == e_semi) bad("kind", [](A &a) { a.variant = 2; });
    if (f.call == e_outer) { bad("how 0", [](A &a) { a.variant = 0; }); bad("how 4", [](A &a) { a.variant = 4; }); }
    if (f.call == e_lookup) bad("which", [](A &a) { a.variant = 2; });
    if (f.call == e_mult || f.call == e_lookup) bad("d_out null with out_rows", [](A &a) { a.null_d_out = true; });
    if (f.call == e_sum) {
        bad("ncols above the maximum", [](A &a) { a.ncols = 5; });
        bad("null column array", [](A &a) { a.null_cols = true; });
        bad("null out_sums", [](A &a) { a.null_sums = true; });
        bad("null column in a counted slot", [](A &a) { a.null_col_slot = 1; });
    }
    const bool group = f.call == e_group_sum || f.call == e_group_agg || f.call == e_group_ids;
    const bool gjoin = f.call == e_gjoin || f.call == e_gjoin_agg || f.call == e_gjoin_ids;
    if (group || gjoin || f.call == e_group_arg) {
        bad("ncols above the maximum", [](A &a) { a.ncols = 5; });
        bad("null keys with a capacity", [](A &a) { a.count_only = true; });
        if (f.call != e_group_sum && f.call != e_gjoin) bad("op out of range", [](A &a) { a.ops = ops_bad; });
    }
    if (group || gjoin) {
        bad("null column array", [](A &a) { a.null_cols = true; });
        bad("null sums array", [](A &a) { a.null_sums = true; });
        bad("null column in a counted slot", [](A &a) { a.null_col_slot = 1; });
        bad("null sum column in a counted slot", [](A &a) { a.null_sum_slot = 0; });
    }
    if (gjoin) {
        bad("mode", [](A &a) { a.variant = 2; });
        bad("ncolsS above the maximum", [](A &a) { a.ncolsS = 5; });
        if (f.call != e_gjoin) bad("op of S out of range", [](A &a) { a.opsS = opsS_bad; });
        bad("null column array of S", [](A &a) { a.null_colsS = true; });
        bad("null sums array of S", [](A &a) { a.null_sumsS = true; });
        bad("null column of S in a counted slot", [](A &a) { a.null_colS_slot = 0; });
    }
    if (f.call == e_group_arg) {
        bad("null ops", [](A &a) { a.ops = nullptr; });
        bad("tie out of range", [](A &a) { a.ties = ties_bad; });
        bad("null rows array", [](A &a) { a.null_rows = true; });
        bad("null rows column", [](A &a) { a.null_row_slot = 1; });
        bad("null column under a value op", [](A &a) { a.ops = ops_value; a.null_col_slot = 1; });
    }
}

int main()
{
    for (int s = 0; s < 2; s++)
        for (int j = 0; j < 4; j++) { g_col[s][j].assign(NMAX, 0); g_sum[s][j].assign(NMAX, 0); g_rows[j].assign(NMAX, 0); }
    fake_trace_into(&g_trace);
    static const rhj_opts unpartitioned = {0, 0, 0, 0}, one_pass = {1, 4, 0, 0}, two_pass = {2, 4, 4, 0}, split = {1, 4, 0, 100};
    for (const Family &f : FAMILIES)
        for (int cols = 0; cols < 2; cols++) {
            rhj_ctx *ctx = fresh();
            // every variant: a normal call, and the degenerate inputs
            for (int v = 0; v < f.variants; v++) {
                A a;
                a.cols = cols != 0;
                a.variant = first_variant(f) + v;
                const std::string tag = "variant " + std::to_string(a.variant) + ": ";
                show(ctx, f, a, tag + "1000 x 1000");
                a.nR = 0;
                show(ctx, f, a, tag + "empty R");
                if (f.has_S) {
                    a.nS = 0;
                    show(ctx, f, a, tag + "both empty");
                    a.nR = 1000;
                    show(ctx, f, a, tag + "empty S");
                }
            }
            // the plans, the formats, count only, overflow
            A a;
            a.cols = cols != 0;
            a.variant = first_variant(f);
            a.nR = 300000; a.nS = 200000;                        // (row counts only: no fake reads a tuple, the relations stay NMAX long)
            show(ctx, f, a, "300000 x 200000, the planner's choice");
            a.nR = 3000; a.nS = 2500;
            a.opts = &unpartitioned; show(ctx, f, a, "3000 x 2500 unpartitioned");
            a.opts = &one_pass; show(ctx, f, a, "3000 x 2500 one pass");
            a.opts = &split; show(ctx, f, a, "3000 x 2500 one pass, probe_split 100");
            (void)rhj_set_option(ctx, "partition.narrow", 0);
            a.opts = &two_pass; show(ctx, f, a, "3000 x 2500 two passes, 16-byte");
            (void)rhj_set_option(ctx, "partition.narrow", 2);
            show(ctx, f, a, "3000 x 2500 two passes, narrow");
            (void)rhj_set_profiling(ctx, 0);
            show(ctx, f, a, "3000 x 2500 two passes, narrow, not profiling");
            (void)rhj_set_profiling(ctx, 1);
            (void)rhj_set_option(ctx, "partition.narrow", -1);
            a = A();
            a.cols = cols != 0;
            a.variant = first_variant(f);
            a.count_only = true; a.cap = 0; show(ctx, f, a, "count only");
            a.count_only = false; a.cap = 1; show(ctx, f, a, "capacity 1");
            if (f.call == e_group_ids || f.call == e_gjoin_ids) { a.cap = BIG; a.ids = false; show(ctx, f, a, "no id arrays"); }
            invalid_calls(ctx, f, cols != 0);
            rhj_destroy(ctx);
        }
    // pairs: the first call leaves the most state behind, the calls after it must not see any of it
    const Family &join = FAMILIES[0], &gsum = FAMILIES[6], &gids = FAMILIES[8], &garg = FAMILIES[9], &gjids = FAMILIES[12];
    for (int cols = 0; cols < 2; cols++) {
        struct First { const Family *f; const char *what; int fails; };
        const First firsts[] = {{&gids, "an ids call", 0}, {&garg, "an arg call", 0}, {&gjids, "a group-join ids call", 0},
                                {&gjids, "a group-join ids call refused by the plan check, its id arrays installed", 1},
                                {&gids, "an ids call that overflows, behind its phase", 2},
                                {&gjids, "a group-join ids call that overflows, behind its phase", 2}};
        static const rhj_opts bad_opts = {5, 0, 0, 0};
        for (const First &first : firsts) {
            rhj_ctx *ctx = fresh();
            A a;
            a.cols = cols != 0;
            if (first.fails == 1) a.opts = &bad_opts;
            if (first.fails == 2) a.cap = 1;
            show(ctx, *first.f, a, std::string("first of a pair: ") + first.what);
            A b;                                                  // the columnar first calls are followed by 16-byte calls
            after(ctx, gsum, b, std::string("after ") + first.what);
            after(ctx, join, b, std::string("then, after ") + first.what);
            rhj_destroy(ctx);
        }
    }
    return 0;
}
