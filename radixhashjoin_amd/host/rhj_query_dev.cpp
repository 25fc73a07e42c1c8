// rhj_query_dev.cpp -- device-resident execution of a Query (SURVEY §8f ranks 1-3 on the GPU).
// Same semantics as Query::execute's host path (rhj_query.cpp), but nothing except counts and the final
// SUMs crosses PCIe: the stored columns live in HBM (uploaded once), filters are rhj_col_filter, join inputs
// are built by rhj_gather_tuples, joins are rhj_join_dev, and the intermediate result is maintained by
// gathers.  An alias that is already part of the intermediate enters a join POSITION-CARRYING
// ({key = intermediate row, payload = value}): the pairs then name intermediate rows directly, which replaces
// both the de-duplication of structs.cpp:238-241 and update_intermediate's matching (intermediate.cpp:52-87).
// RHJ_QUERY_MODE=cols: the same execution with the join inputs as COLUMNS for rhj_join_cols_dev -- the stored column itself
// (no kernel at all) for an alias without a row list, one 8-byte gather otherwise -- instead of 16-byte tuples.
// RHJ_QUERY_MODE=agg: as cols, except that a query whose LAST predicate is an equi-join through the hot path never produces that
// join's pairs: its SUMs come from rhj_join_sum_cols_dev (sum_last_join below) instead of join + split + regather + rhj_sum_gather.
// RHJ_QUERY_MODE=tree: as agg, except that a query whose join graph is a tree (tree_edges below) produces no pairs at all: every
// SUM is a sum over the rows of its alias weighted by the product of per-row multiplicities, rhj_join_mult_cols_dev's messages
// (TreeQuery below).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "rhj_query.h"

namespace {

[[noreturn]] void die(rhj_ctx *ctx, const char *what, int rc)
{
    fprintf(stderr, "rhj: %s failed (%d): %s\n", what, rc, rhj_last_error(ctx));
    exit(EXIT_FAILURE);
}
#define OK(ctx, call) do { int rc_ = (call); if (rc_ != RHJ_OK) die(ctx, #call, rc_); } while (0)

struct DevArr {                                  // a uint64 (or 16-byte record) array in HBM
    rhj_ctx *ctx = nullptr;
    uint64_t *p = nullptr;
    uint64_t n = 0;
    DevArr() = default;
    DevArr(rhj_ctx *c, uint64_t bytes) : ctx(c)
    {
        void *q = nullptr;
        OK(ctx, rhj_dev_alloc(ctx, bytes ? bytes : 16, &q));
        p = (uint64_t *)q;
    }
    DevArr(const DevArr &) = delete;
    DevArr &operator=(const DevArr &) = delete;
    DevArr(DevArr &&o) noexcept { *this = std::move(o); }
    DevArr &operator=(DevArr &&o) noexcept
    {
        if (this != &o) { reset(); ctx = o.ctx; p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    void reset() { if (p) rhj_dev_free(ctx, p); p = nullptr; n = 0; }
    ~DevArr() { reset(); }
    bool empty() const { return p == nullptr; }
};

// columns of the stored relations in HBM: uploaded once per process, shared by every context on the device
std::mutex g_cols_mu;
std::map<const uint64_t *, uint64_t *> g_cols;   // host column base -> device copy

const uint64_t *device_column(rhj_ctx *ctx, const relList &rel, uint64_t c)
{
    std::lock_guard<std::mutex> lk(g_cols_mu);
    auto it = g_cols.find(rel.values[c]);
    if (it != g_cols.end()) return it->second;
    void *d = nullptr;
    OK(ctx, rhj_dev_alloc(ctx, rel.num_tuples * 8, &d));
    OK(ctx, rhj_copy_h2d(ctx, d, rel.values[c], rel.num_tuples * 8));
    g_cols[rel.values[c]] = (uint64_t *)d;
    return (const uint64_t *)d;
}

// rows of an alias that survived its filters: device list, or "all rows" (p == nullptr, n = table size)
struct Rows {
    DevArr list;
    uint64_t n = 0;
    const uint64_t *ptr() const { return list.p; }
};

DevArr join_pairs(rhj_ctx *ctx, const DevArr &R, uint64_t nR, const DevArr &S, uint64_t nS, uint64_t &count)
{
    uint64_t cap = (nR > nS ? nR : nS) + 1024;
    for (;;) {
        DevArr out(ctx, cap * 16);
        int rc = rhj_join_dev(ctx, (const rhj_tuple *)R.p, nR, (const rhj_tuple *)S.p, nS, nullptr, (rhj_pair *)out.p, cap, &count);
        if (rc == RHJ_OK) { out.n = count; return out; }
        if (rc != RHJ_E_OVERFLOW) die(ctx, "rhj_join_dev", rc);
        cap = count;                                   // exact size is known now
    }
}

bool tree_mode()
{
    static const bool on = getenv("RHJ_QUERY_MODE") && std::string(getenv("RHJ_QUERY_MODE")) == "tree";
    return on;
}

bool agg_mode()                                        // (tree: a query that is not eligible runs as in agg)
{
    static const bool on = tree_mode() || (getenv("RHJ_QUERY_MODE") && std::string(getenv("RHJ_QUERY_MODE")) == "agg");
    return on;
}

bool cols_mode()                                       // (agg: columnar inputs for every join)
{
    static const bool on = agg_mode() || (getenv("RHJ_QUERY_MODE") && std::string(getenv("RHJ_QUERY_MODE")) == "cols");
    return on;
}

// one side of a columnar join: value column + id column (nullptr: the rowID is the position)
struct ColSide {
    const uint64_t *val = nullptr, *id = nullptr;
    DevArr gathered;                                   // owns val when it had to be gathered
};

//   alias not in the intermediate, no row list   the stored column itself              ids: none (rowID = row)
//   ... with a row list                          gather(col, rows)                     ids: the row list
//   alias already in the intermediate            gather(col, inter[a])                 ids: none (position-carrying)
ColSide col_side(rhj_ctx *ctx, const uint64_t *col, const DevArr &inter_a, const Rows &r, uint64_t n)
{
    ColSide s;
    const bool in = !inter_a.empty();
    if (!in && r.ptr() == nullptr) { s.val = col; return s; }
    s.gathered = DevArr(ctx, n * 8);
    OK(ctx, rhj_gather_u64(ctx, col, in ? inter_a.p : r.ptr(), n, s.gathered.p));
    s.gathered.n = n;
    s.val = s.gathered.p;
    s.id = in ? nullptr : r.ptr();
    return s;
}

DevArr join_pairs_cols(rhj_ctx *ctx, const ColSide &R, uint64_t nR, const ColSide &S, uint64_t nS, uint64_t &count)
{
    uint64_t cap = (nR > nS ? nR : nS) + 1024;
    for (;;) {
        DevArr out(ctx, cap * 16);
        int rc = rhj_join_cols_dev(ctx, R.val, R.id, nR, S.val, S.id, nS, nullptr, (rhj_pair *)out.p, cap, &count);
        log_cols_join("cols", nR, nS, count);
        if (rc == RHJ_OK) { out.n = count; return out; }
        if (rc != RHJ_E_OVERFLOW) die(ctx, "rhj_join_cols_dev", rc);
        cap = count;                                   // exact size is known now
    }
}

// every live intermediate column re-materialised through the positions `idx` (m of them)
void regather(rhj_ctx *ctx, std::vector<DevArr> &inter, const uint64_t *idx, uint64_t m)
{
    for (DevArr &col : inter) {
        if (col.empty()) continue;
        DevArr next(ctx, m * 8);
        OK(ctx, rhj_gather_u64(ctx, col.p, idx, m, next.p));
        next.n = m;
        col = std::move(next);
    }
}

// One projection of the last join in "agg" mode as a weight column indexed by the probe side's rowID: for a side that is the
// intermediate (position-carrying, NULL ids) the projected column gathered through the alias' rows, T words; for a new alias the
// stored column itself, indexed by the alias' rowIDs (its row list, or the position).
struct Weight {
    const uint64_t *col = nullptr;
    DevArr gathered;
};

// |P join B| and the sums of `w` (at most RHJ_SUM_MAX_COLS columns of col_rows words) over its pairs, P the side the columns belong to
uint64_t join_sums(rhj_ctx *ctx, const ColSide &P, uint64_t nP, const ColSide &B, uint64_t nB, const std::vector<Weight> &w,
                   uint64_t col_rows, uint64_t *sums)
{
    const uint64_t *cols[RHJ_SUM_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < w.size(); i++) cols[i] = w[i].col;
    uint64_t count = 0;
    OK(ctx, rhj_join_sum_cols_dev(ctx, P.val, P.id, nP, B.val, nB, cols, (uint32_t)w.size(), col_rows, nullptr, &count, sums));
    log_cols_join("sum", nP, nB, count);
    return count;
}

// a same-alias predicate (parse_table) on an alias that is not joined yet: a filter on its row list.  false: no row is left
bool same_alias_filter(rhj_ctx *ctx, const relList &rel, const join_info &j, Rows &r)
{
    const uint64_t *c1 = device_column(ctx, rel, j.column1), *c2 = device_column(ctx, rel, j.column2);
    DevArr pos(ctx, r.n * 8);
    uint64_t m = 0;
    OK(ctx, rhj_rows_filter_equal(ctx, c1, r.ptr(), c2, r.ptr(), r.n, pos.p, &m));
    if (m == 0) return false;
    if (r.ptr() == nullptr) { pos.n = m; r.list = std::move(pos); }       // positions ARE the rowIDs
    else {
        DevArr next(ctx, m * 8);
        OK(ctx, rhj_gather_u64(ctx, r.ptr(), pos.p, m, next.p));
        next.n = m;
        r.list = std::move(next);
    }
    r.n = m;
    return true;
}

// The equi-joins of a query the "tree" mode takes, or nothing.  Walking the predicates in order with the set of joined aliases: a
// same-alias predicate on an alias not joined yet is a filter on its row list (it stays in q.join, not here); a same-alias predicate
// on a joined alias, a predicate between two joined aliases (also one that appears twice), one between two new aliases while others
// are joined (the dropped-columns case of execute_device) or an alias that is never joined make the query not eligible.  What is
// left is a tree over all aliases: na - 1 edges.
bool tree_edges(const Query &q, std::vector<const join_info *> &edges)
{
    const size_t na = q.table.size();
    std::vector<bool> joined(na, false);
    bool any = false;
    edges.clear();
    for (const join_info &j : q.join) {
        if (j.table1 == j.table2) {
            if (joined[j.table1]) return false;
            continue;
        }
        if (joined[j.table1] && joined[j.table2]) return false;
        if (!joined[j.table1] && !joined[j.table2] && any) return false;
        joined[j.table1] = joined[j.table2] = any = true;
        edges.push_back(&j);
    }
    for (size_t a = 0; a < na; a++)
        if (!joined[a]) return false;
    return true;
}

// An eligible query after its filters.  Every alias is a positional vector over its row list; for a projected alias a,
// SUM(a.c) = sum over its rows of c[row] * W_a[row], W_a the product over a's neighbours of the message "how many combinations of
// the subtree behind this neighbour match this row".  The message u -> v over u.cu = v.cv is one rhj_join_mult_cols_dev call with
// v's values as R, u's as S and, as S's weights, the product of the messages INTO u from its other neighbours; messages are kept per
// directed edge, so a query costs at most 2 x (aliases - 1) calls.  A message total or a count of 0: no row, the NULL line.
struct TreeQuery {
    rhj_ctx *ctx;
    Query &q;
    std::vector<relList> &relations;
    std::vector<Rows> &rows;
    const std::vector<const join_info *> &edges;
    std::map<std::pair<size_t, uint64_t>, DevArr> gathered;       // (alias, column) -> the column through the alias' row list
    struct Message { DevArr w; uint64_t total = 0; bool done = false; };
    std::vector<Message> msg;                                     // [2 e + d]: over edge e, d = 0: table2 -> table1, 1: table1 -> table2
    bool none = false;                                            // a message came out all zero: the query has no row
    TreeQuery(rhj_ctx *c, Query &query, std::vector<relList> &rels, std::vector<Rows> &r, const std::vector<const join_info *> &e)
        : ctx(c), q(query), relations(rels), rows(r), edges(e) {}

    const uint64_t *values(size_t a, uint64_t c)
    {
        const uint64_t *col = device_column(ctx, relations[q.table[a]], c);
        if (rows[a].ptr() == nullptr) return col;
        auto it = gathered.find({a, c});
        if (it == gathered.end()) {
            DevArr g(ctx, rows[a].n * 8);
            OK(ctx, rhj_gather_u64(ctx, col, rows[a].ptr(), rows[a].n, g.p));
            it = gathered.emplace(std::make_pair(a, c), std::move(g)).first;
        }
        return it->second.p;
    }
    // the product of the messages into alias a over every edge but `except` (-1: all): nullptr when there is none (all ones); `own`
    // holds the product when it had to be formed
    const uint64_t *weights(size_t a, int except, DevArr &own)
    {
        const uint64_t *w = nullptr;
        for (size_t e = 0; e < edges.size() && !none; e++) {
            if ((int)e == except || (edges[e]->table1 != a && edges[e]->table2 != a)) continue;
            const Message &m = message(e, edges[e]->table1 == a ? 0 : 1);
            if (none) break;
            if (w == nullptr) { w = m.w.p; continue; }
            if (own.empty()) own = DevArr(ctx, rows[a].n * 8);
            OK(ctx, rhj_mul_u64(ctx, w, m.w.p, rows[a].n, own.p));
            w = own.p;
        }
        return w;
    }
    const Message &message(size_t e, int d)
    {
        Message &m = msg[2 * e + d];
        if (m.done) return m;
        const join_info &j = *edges[e];
        const size_t u = d ? j.table1 : j.table2, v = d ? j.table2 : j.table1;
        const uint64_t cu = d ? j.column1 : j.column2, cv = d ? j.column2 : j.column1;
        DevArr own;
        const uint64_t *wS = weights(u, (int)e, own);
        m.done = true;
        if (none) return m;
        m.w = DevArr(ctx, rows[v].n * 8);
        OK(ctx, rhj_join_mult_cols_dev(ctx, values(v, cv), nullptr, rows[v].n, values(u, cu), nullptr, rows[u].n, wS, rows[u].n, nullptr,
                                       m.w.p, rows[v].n, &m.total));
        log_cols_join("mult", rows[v].n, rows[u].n, m.total);
        if (m.total == 0) none = true;
        return m;
    }
    void run()
    {
        msg.resize(2 * edges.size());
        std::map<size_t, DevArr> product;                         // W_a of a projected alias with several neighbours
        for (proj_info &p : q.proj) {
            const size_t a = p.table;
            DevArr &own = product[a];
            const uint64_t *W = weights(a, -1, own);              // (memoised messages: a second projection of a costs its products only)
            uint64_t count = 0;
            if (!none) OK(ctx, rhj_sum_gather_weighted(ctx, nullptr, nullptr, W, rows[a].n, &count));
            if (none || count == 0) { q.filtered_out = true; return; }
            OK(ctx, rhj_sum_gather_weighted(ctx, device_column(ctx, relations[q.table[a]], p.column), rows[a].ptr(), W, rows[a].n, &p.sum));
        }
    }
};

}  // namespace

// Query::execute on the device.  Returns through this->filtered_out / proj[i].sum like the host path.
void Query::execute_device(JobScheduler &js, std::vector<relList> &relations)
{
    rhj_ctx *ctx = js.context();
    const size_t na = table.size();
    filtered_out = false;

    // ---- filters (Query.cpp:81-158) ------------------------------------------------------------
    std::vector<Rows> rows(na);
    for (size_t a = 0; a < na; a++) rows[a].n = relations[table[a]].num_tuples;
    for (const filter_info &f : filter) {
        const relList &rel = relations[table[f.table]];
        Rows &r = rows[f.table];
        DevArr out(ctx, r.n * 8);
        uint64_t m = 0;
        OK(ctx, rhj_col_filter(ctx, device_column(ctx, rel, f.column), r.ptr(), r.n, f.op, f.number, out.p, &m));
        if (m == 0) { filtered_out = true; return; }
        out.n = m;
        r.list = std::move(out);
        r.n = m;
    }

    // ---- RHJ_QUERY_MODE=tree, join graph a tree: same-alias predicates, then sums by message passing, no pairs -------------------
    std::vector<const join_info *> edges;
    if (tree_mode() && tree_edges(*this, edges)) {
        for (const join_info &j : join) {
            if (j.table1 != j.table2) continue;
            if (!same_alias_filter(ctx, relations[table[j.table1]], j, rows[j.table1])) { filtered_out = true; return; }
        }
        TreeQuery t(ctx, *this, relations, rows, edges);
        t.run();
        return;
    }

    // ---- join chain (Query.cpp:164-201) -------------------------------------------------------
    std::vector<DevArr> inter(na);                     // inter[a]: rowID of alias a per intermediate row
    uint64_t T = 0;                                    // intermediate rows
    for (const join_info &j : join) {
        const relList &rel1 = relations[table[j.table1]], &rel2 = relations[table[j.table2]];
        const uint64_t *c1 = device_column(ctx, rel1, j.column1), *c2 = device_column(ctx, rel2, j.column2);
        const bool in1 = !inter[j.table1].empty(), in2 = !inter[j.table2].empty();
        if (j.table1 == j.table2 || (in1 && in2)) {
            // a row filter: same-alias predicate (parse_table) or both aliases already joined (case 3)
            if (j.table1 == j.table2 && !in1) {
                if (!same_alias_filter(ctx, rel1, j, rows[j.table1])) { filtered_out = true; return; }
                continue;
            }
            DevArr pos(ctx, T * 8);
            uint64_t m = 0;
            OK(ctx, rhj_rows_filter_equal(ctx, c1, inter[j.table1].p, c2, inter[j.table2].p, T, pos.p, &m));
            if (m == 0) { filtered_out = true; return; }
            regather(ctx, inter, pos.p, m);
            T = m;
            continue;
        }
        // an equi-join through the hot path.  Side already in the intermediate: position-carrying input.
        const uint64_t nR = in1 ? T : rows[j.table1].n, nS = in2 ? T : rows[j.table2].n;
        uint64_t m = 0;
        DevArr pairs;
        bool live = false;
        for (const DevArr &c : inter) live = live || !c.empty();
        if (agg_mode() && &j == &join.back() && (in1 || in2 || !live)) {
            // The query ends here: the pairs would only be added up.  The final intermediate would hold the side that is already joined
            // (every live alias) and the new alias, or the two new aliases; a projection belongs to the side its alias arrives on and is
            // summed by a call with that side as R (the other side's call has the sides exchanged); any other alias sums to 0.
            const ColSide side[2] = {col_side(ctx, c1, inter[j.table1], rows[j.table1], nR), col_side(ctx, c2, inter[j.table2], rows[j.table2], nS)};
            const uint64_t n[2] = {nR, nS};
            const bool in[2] = {in1, in2};
            const size_t alias[2] = {j.table1, j.table2};
            std::vector<size_t> on[2];
            for (size_t i = 0; i < proj.size(); i++) {
                proj[i].sum = 0;
                for (int s = 0; s < 2; s++)
                    if (in[s] ? !inter[proj[i].table].empty() : (size_t)proj[i].table == alias[s]) { on[s].push_back(i); break; }
            }
            if (on[0].empty() && on[1].empty()) m = join_sums(ctx, side[0], n[0], side[1], n[1], {}, 0, nullptr);   // COUNT(*) alone
            bool none = false;                         // a call counted 0 pairs: every further call would
            for (int s = 0; s < 2 && !none; s++)
                for (size_t at = 0; at < on[s].size() && !none; at += RHJ_SUM_MAX_COLS) {
                    const size_t nc = on[s].size() - at < RHJ_SUM_MAX_COLS ? on[s].size() - at : RHJ_SUM_MAX_COLS;
                    std::vector<Weight> w(nc);
                    for (size_t i = 0; i < nc; i++) {
                        const proj_info &p = proj[on[s][at + i]];
                        const uint64_t *col = device_column(ctx, relations[table[p.table]], p.column);
                        if (!in[s]) { w[i].col = col; continue; }
                        w[i].gathered = DevArr(ctx, T * 8);
                        OK(ctx, rhj_gather_u64(ctx, col, inter[p.table].p, T, w[i].gathered.p));
                        w[i].col = w[i].gathered.p;
                    }
                    uint64_t sums[RHJ_SUM_MAX_COLS] = {0, 0, 0, 0};
                    m = join_sums(ctx, side[s], n[s], side[1 - s], n[1 - s], w, in[s] ? T : relations[table[alias[s]]].num_tuples, sums);
                    none = m == 0;
                    for (size_t i = 0; i < nc; i++) proj[on[s][at + i]].sum = sums[i];
                }
            if (m == 0) filtered_out = true;
            return;
        }
        if (cols_mode()) {
            const ColSide R = col_side(ctx, c1, inter[j.table1], rows[j.table1], nR), S = col_side(ctx, c2, inter[j.table2], rows[j.table2], nS);
            pairs = join_pairs_cols(ctx, R, nR, S, nS, m);                            // <-- rhj_join_cols_dev
        } else {
            DevArr R(ctx, nR * 16), S(ctx, nS * 16);
            OK(ctx, rhj_gather_tuples(ctx, c1, in1 ? inter[j.table1].p : rows[j.table1].ptr(), nR, in1 ? 1 : 0, (rhj_tuple *)R.p));
            OK(ctx, rhj_gather_tuples(ctx, c2, in2 ? inter[j.table2].p : rows[j.table2].ptr(), nS, in2 ? 1 : 0, (rhj_tuple *)S.p));
            pairs = join_pairs(ctx, R, nR, S, nS, m);                                 // <-- rhj_join_dev
        }
        if (m == 0) { filtered_out = true; return; }
        DevArr kr(ctx, m * 8), ks(ctx, m * 8);
        OK(ctx, rhj_pairs_split(ctx, (const rhj_pair *)pairs.p, m, kr.p, ks.p));
        kr.n = ks.n = m;
        if (!in1 && !in2) {                            // case 1: the pairs become the two columns
            // (a join between two aliases that are both new while OTHER aliases are already joined would need a
            //  cross product; the reference's update_intermediate drops the older columns in that case
            //  (intermediate.cpp:147-162: only table1/table2 of intermediate_upd are filled) -- same here)
            for (DevArr &c : inter) c.reset();
            inter[j.table1] = std::move(kr);
            inter[j.table2] = std::move(ks);
        } else if (in1) {                              // case 2: keyR = intermediate row, keyS = new alias' rowID
            regather(ctx, inter, kr.p, m);
            inter[j.table2] = std::move(ks);
        } else {
            regather(ctx, inter, ks.p, m);
            inter[j.table1] = std::move(kr);
        }
        T = m;
    }

    // ---- SUM projections (Query.cpp:66-74,198-200) -------------------------------------------
    for (proj_info &p : proj) {
        const uint64_t *col = device_column(ctx, relations[table[p.table]], p.column);
        // an alias that is not part of the intermediate (never joined, or dropped when a later join linked two new
        // aliases) sums to 0, as in the reference (Query.cpp:198-200 over an empty intermediate[p.table])
        uint64_t sum = 0;
        if (!inter[p.table].empty()) OK(ctx, rhj_sum_gather(ctx, col, inter[p.table].p, T, &sum));
        p.sum = sum;
    }
}
