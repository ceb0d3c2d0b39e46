// pc_split.h -- the host's half of a clustering update (do_clustering, clustering.f90:253-324; add_cluster, run_time_info.f90:303-505): which
// clusters are looked at, NN_clustering's recursion level by level, and what a split does to the labels, volumes, evidences and ids of the clusters.
// The heavy parts run on the device (pc_cluster.hip).
//
// Host only.  Included by pc_engine.hip alone, in front of Engine, which keeps one ClusterUpdate by value (and by tools/dev/split_record.hip,
// which stands a scripted Engine, a scripted device and recorders in for everything below and compares what an update sends, launches, fetches and
// waits for with lines 1292-1604 of the pc_engine.hip before this header existed, 9f0f34b: tests/test_split_record.py).
//
// The top half is plain functions and structs, vectors in and vectors out, each named after the reference routine it restates: no Engine, no HIP,
// no stream.  It needs PC_HUGE (pc_state.h) and nothing else.
//
// The bottom half, ClusterUpdate<Eng>, owns the clustering scratch on the device and holds the orchestration: each method a short sequence of
// "pure step, sends, launches or records, fetches, wait".  The including file provides, before an update is made: pc_state.h, pc_launch.h, the
// cohort's rec_clus1 / rec_clusg, RunBlocks (pc_blocks.h), engine_fail and the PC_RC_* codes, g_inject_fault; and
//   of Engine, these members and no others:
//     S, h_ctl, cfg.epoch_discard, co (rec), st, blocks (the run's ledger: the scratch below is allocated through it and goes back with the run)
//     nsplits, ncluster_peak, split_child, split_parent, split_logfrac
//     send_raw, send_pre, fetch, fetch_raw, fetch_wait, direct_op
//     grow_clusters          (which calls back regrow_counts)
#pragma once
#include <vector>
#include <algorithm>
#include <utility>
#include <cmath>
#include <cstddef>

// ---- the pure half --------------------------------------------------------------------------------------------------------------------

// What the host's half of a split reads: the points' (cluster, position) labels and the clusters' volumes, evidences, thresholds,
// ids, cross-volume rows -- the first nc entries / rows; what lies behind them stays what it is on the device.  Asked for with the
// verdicts of the update's first clustering pass (do_clustering: the same wait), it serves every split of the update: a split
// leaves on the host exactly what it sends up, so the splits of an update cost one wait each (the phantoms' counts), not two.
struct ClusterMirror {
    bool valid = false; int maxc = 0;
    std::vector<int> lc, lp; std::vector<double> Xp, ZXp, Zp, Zp2, ZpXp, thr, XQ; std::vector<unsigned> uid;
    void size(int Ncap, int maxc_now)
    {
        lc.resize(Ncap); lp.resize(Ncap);
        for (std::vector<double> *v : {&Xp, &ZXp, &Zp, &Zp2, &ZpXp, &thr}) v->resize(maxc_now);
        XQ.resize((size_t)maxc_now * maxc_now); uid.resize(maxc_now);
        maxc = maxc_now;
    }
};

// do_clustering's first pass (clustering.f90:253-324): one descriptor {cluster, n, off2, off1} per cluster with more than two points -- off2 its
// n x n blocks' offset, off1 its labels' -- which[k] the k-th descriptor's cluster, o1 / o2 the totals, nmax the largest cluster
struct FirstPass {
    std::vector<int> desc, which; int o1 = 0; long long o2 = 0; int nmax = 0;
    int nd() const { return (int)which.size(); }
};
inline FirstPass first_pass_descriptors(const std::vector<int> &cn)
{
    FirstPass f;
    for (int c = 0; c < (int)cn.size(); ++c)
        if (cn[c] > 2) { f.desc.push_back(c); f.desc.push_back(cn[c]); f.desc.push_back((int)f.o2); f.desc.push_back(f.o1); f.which.push_back(c); f.o1 += cn[c]; f.o2 += (long long)cn[c] * cn[c]; }
    for (int k = 0; k < f.nd(); ++k) f.nmax = std::max(f.nmax, f.desc[4 * k + 1]);
    return f;
}

// NN_clustering's recursion (clustering.f90:80-95) level by level.  The reference re-clusters every cluster it finds, alone, until one
// pass over it finds a single cluster; the labels it returns are the final parts numbered by first appearance (relabel after every
// step, utils.F90:713-749).  A part's own clustering depends on its points only, so the order in which the parts are looked at does
// not matter (tools/dev/split_record --order holds this against the reference's depth-first order): all parts of all clusters of an
// update that are still open are clustered in ONE launch per level (and, in step with other runs, together with theirs), on the
// similarity blocks the first pass left behind -- two or three waits per update instead of one per part.
struct PartRefiner {
    struct Part { int k; std::vector<int> idx; };              // k: descriptor; idx: positions in the cluster's point order
    // a level's launch: a descriptor {off2, n, ioff, m, koff} per part (k_knn_sort_sub), the parts' positions one behind the other, the
    // number of parts, the largest one, the neighbour lists' total
    struct Level { std::vector<int> gdesc, pool; int nb = 0, mmax = 0; long long koff = 0; };
    const FirstPass *fp = nullptr; std::vector<int> out;
    std::vector<std::vector<std::vector<int>>> done;           // final parts of every split cluster
    std::vector<Part> work, cur;
    Level lev;

    // desc, which: the first pass' descriptors; out: clusters it found in each; lab0: its labels (1-based, at the descriptors' off1)
    void open(const FirstPass &f, const std::vector<int> &out_, const std::vector<int> &lab0)
    {
        fp = &f; out = out_;
        done.assign((size_t)f.nd(), {}); work.clear(); cur.clear();
        for (int k = 0; k < f.nd(); ++k) {
            if (out[k] <= 1) continue;
            const int n = f.desc[4 * k + 1], o1 = f.desc[4 * k + 3];
            std::vector<int> all((size_t)n);
            for (int i = 0; i < n; ++i) all[i] = i;
            split_by(k, all, lab0.data() + o1, out[k]);
        }
    }
    bool work_left() const { return !work.empty(); }
    // every open part becomes a part of the next level's launch
    const Level &next_level()
    {
        cur.clear(); cur.swap(work);
        lev = Level(); lev.nb = (int)cur.size(); lev.gdesc.resize((size_t)5 * lev.nb);
        for (int b = 0; b < lev.nb; ++b) {
            const int k = cur[b].k, m = (int)cur[b].idx.size();
            int *g = &lev.gdesc[5 * b];
            g[0] = fp->desc[4 * k + 2]; g[1] = fp->desc[4 * k + 1]; g[2] = (int)lev.pool.size(); g[3] = m; g[4] = (int)lev.koff;
            lev.pool.insert(lev.pool.end(), cur[b].idx.begin(), cur[b].idx.end());
            lev.mmax = std::max(lev.mmax, m); lev.koff += (long long)m * m;
        }
        return lev;
    }
    // the level's answer: labs the parts' labels (at their ioff), nums the clusters found in each.  One cluster: the part is final
    void take(const std::vector<int> &labs, const std::vector<int> &nums)
    {
        for (int b = 0; b < lev.nb; ++b) {
            if (nums[b] > 1) split_by(cur[b].k, cur[b].idx, labs.data() + lev.gdesc[5 * b + 2], nums[b]);
            else done[(size_t)cur[b].k].push_back(std::move(cur[b].idx));
        }
    }
    // labels and their number for every cluster the first pass split (by cluster, not by descriptor): the final parts numbered by first appearance
    void finish(std::vector<std::vector<int>> &final_labels, std::vector<int> &final_num) const
    {
        for (int k = 0; k < fp->nd(); ++k) {
            if (out[k] <= 1) continue;
            const int n = fp->desc[4 * k + 1], j = fp->which[k];
            std::vector<int> part_of((size_t)n, -1), newlab(done[(size_t)k].size(), 0);
            for (size_t q = 0; q < done[(size_t)k].size(); ++q) for (int i : done[(size_t)k][q]) part_of[(size_t)i] = (int)q;
            int next = 0;
            final_labels[(size_t)j].assign((size_t)n, 0);
            for (int i = 0; i < n; ++i) { int &l = newlab[(size_t)part_of[(size_t)i]]; if (l == 0) l = ++next; final_labels[(size_t)j][(size_t)i] = l; }
            final_num[(size_t)j] = next;
        }
    }
private:
    void split_by(int k, const std::vector<int> &idx, const int *lab /* 1-based, one per entry of idx */, int num)
    {
        std::vector<std::vector<int>> parts((size_t)num);
        for (size_t a = 0; a < idx.size(); ++a) parts[(size_t)lab[a] - 1].push_back(idx[a]);
        for (auto &pt : parts) { if (pt.size() > 1) work.push_back(Part{k, std::move(pt)}); else if (!pt.empty()) done[(size_t)k].push_back(std::move(pt)); }
    }
};

// add_cluster (run_time_info.f90:303-505): cluster p of nc splits into nnew clusters appended at the end; the clusters behind p move up.
// What of the parent the evidence split needs once the mirror's arrays are compacted over it:
struct SplitParent {
    double logXp, logXp2, logZp, logZp2, logZXp, logZpXp;
    std::vector<double> rowpq;              // its cross volumes with the other clusters, in their new order
    std::vector<unsigned> olduid;           // the ids of all nc clusters before the split
};
// ... before the counts are known: labels = the new cluster (1-based) of every point of p, in p's point order.  The mirror's point labels are
// rewritten, its per-cluster arrays and the cross-volume matrix compacted over p (old clusters keep their order at 0..nc-2: old_save /
// old_target, :371-376), the new clusters get their ids (from next_uid on) and thresholds
inline SplitParent add_cluster_relabel(ClusterMirror &m, int nc, int p, const std::vector<int> &labels, int nnew, unsigned &next_uid)
{
    const int nold = nc - 1, maxc = m.maxc;
    std::vector<int> &lc = m.lc, &lp = m.lp; std::vector<double> &XQ = m.XQ; std::vector<unsigned> &uid = m.uid;
    // position of every split point inside its new cluster = rank among equal labels in list order
    std::vector<int> posnew(labels.size()), cnt(nnew, 0);
    for (size_t a = 0; a < labels.size(); ++a) posnew[a] = cnt[labels[a] - 1]++;
    for (size_t s = 0; s < lc.size(); ++s) {
        const int c = lc[s];
        if (c < 0) continue;
        if (c == p) { const int a = lp[s]; lc[s] = nold + labels[a] - 1; lp[s] = posnew[a]; }
        else if (c > p) lc[s] = c - 1;
    }
    SplitParent par{m.Xp[p], XQ[(size_t)p * maxc + p], m.Zp[p], m.Zp2[p], m.ZXp[p], m.ZpXp[p], {}, std::vector<unsigned>(uid.begin(), uid.begin() + nc)};
    for (int q = 0; q < nc; ++q) if (q != p) par.rowpq.push_back(XQ[(size_t)p * maxc + q]);
    auto shift = [&](std::vector<double> &v) { for (int c = p; c < nc - 1; ++c) v[c] = v[c + 1]; };
    shift(m.Xp); shift(m.ZXp); shift(m.Zp); shift(m.Zp2); shift(m.ZpXp); shift(m.thr);
    for (int c = p; c < nc - 1; ++c) uid[c] = uid[c + 1];
    {
        std::vector<double> t(XQ);
        for (int a = 0, na = 0; a < nc; ++a) { if (a == p) continue; for (int b = 0, nb = 0; b < nc; ++b) { if (b == p) continue; XQ[(size_t)na * maxc + nb] = t[(size_t)a * maxc + b]; nb++; } na++; }
    }
    for (int k = 0; k < nnew; ++k) { uid[nold + k] = next_uid++; m.thr[nold + k] = -PC_HUGE; }
    return par;
}
// ... once the new clusters' live points (nlv) and phantoms (nph) are counted: evidences and volumes split in proportion to nlive + nphantom
// (:458-503), the cross volumes' rows, columns and the nnew x nnew block, and the genealogy's three entries per new cluster.  (These doubles go
// to the device: the operations and their order are the reference's.)
inline void add_cluster_evidence(ClusterMirror &m, const SplitParent &par, int nc, int p, int nnew, const std::vector<int> &nlv, const std::vector<int> &nph,
                                 std::vector<unsigned> &split_child, std::vector<unsigned> &split_parent, std::vector<double> &split_logfrac)
{
    const int nold = nc - 1, maxc = m.maxc;
    std::vector<double> &Xp = m.Xp, &ZXp = m.ZXp, &Zp = m.Zp, &Zp2 = m.Zp2, &ZpXp = m.ZpXp, &XQ = m.XQ;
    std::vector<double> logni(nnew), logni1(nnew);
    for (int k = 0; k < nnew; ++k) { logni[k] = std::log((double)(nlv[nold + k] + nph[nold + k]) + 0.0); logni1[k] = std::log((double)(nlv[nold + k] + nph[nold + k]) + 1.0); }
    double mx = logni[0];
    for (int k = 1; k < nnew; ++k) mx = std::max(mx, logni[k]);
    double sm = 0.0;
    for (int k = 0; k < nnew; ++k) sm += std::exp(logni[k] - mx);
    const double logn = mx + std::log(sm);
    const double logn1 = logn > 0.0 ? logn + std::log(std::exp(0.0 - logn) + 1.0) : 0.0 + std::log(std::exp(logn - 0.0) + 1.0);
    for (int k = 0; k < nnew; ++k) { split_child.push_back(m.uid[nold + k]); split_parent.push_back(par.olduid[p]); split_logfrac.push_back(logni[k] - logn); }
    for (int k = 0; k < nnew; ++k) {
        const int c = nold + k;
        Xp[c] = par.logXp + logni[k] - logn; ZXp[c] = par.logZXp + logni[k] - logn; Zp[c] = par.logZp + logni[k] - logn;
        Zp2[c] = par.logZp2 + logni[k] + logni1[k] - logn - logn1; ZpXp[c] = par.logZpXp + logni[k] + logni1[k] - logn - logn1;
        for (int q = 0; q < nold; ++q) { XQ[(size_t)c * maxc + q] = par.rowpq[q] + logni[k] - logn; XQ[(size_t)q * maxc + c] = XQ[(size_t)c * maxc + q]; }
    }
    for (int a = 0; a < nnew; ++a)
        for (int b = 0; b < nnew; ++b)
            XQ[(size_t)(nold + a) * maxc + nold + b] = (a == b) ? par.logXp2 + logni[a] + logni1[a] - logn - logn1
                                                                 : par.logXp2 + logni[a] + logni[b] - logn - logn1;
}

// Where the clusters an update began with are in the list now: map[j] the place of the update's cluster j, -1 once it was split
inline std::vector<int> cluster_map_identity(int n) { std::vector<int> m((size_t)n); for (int j = 0; j < n; ++j) m[(size_t)j] = j; return m; }
inline void cluster_map_split_at(std::vector<int> &cmap, int p) { for (int &m : cmap) { if (m == p) m = -1; else if (m > p) m -= 1; } }
// two passes in one update: map1 through the first, map2 from the list after it through the second
inline void cluster_map_compose(std::vector<int> &map1, const std::vector<int> &map2) { for (int &m : map1) m = m >= 0 ? map2[(size_t)m] : -1; }

// What a caller may ask of a pass (the kernel-level door pchip_cluster_update, for its tests): host arrays for the first pass's similarity block,
// neighbour lists (cap x cap each) and first-level labels (cap) of the first cluster the pass looks at; n: its points, set by the pass
struct ClusterTap { double *Sm; int *knn, *lab; int cap, n; };

// ---- the device's scratch and the traffic ---------------------------------------------------------------------------------------------

template <class Eng> struct ClusterUpdate {
    Eng &e; RunBlocks &blocks;                 // (the run's ledger: the scratch is allocated through it and goes back with the run's other blocks)
    explicit ClusterUpdate(Eng &engine) : e(engine), blocks(engine.blocks) {}
    // similarity blocks, neighbour lists and labels of the first pass (c_cap = the live slots they are sized for); the phantoms' counts per
    // cluster and the ids before a split (sized with S.maxc)
    double *c_Sm = nullptr; int *c_knn = nullptr, *c_lab = nullptr, *c_cnt = nullptr; unsigned *c_olduid = nullptr; int c_cap = 0;
    int *c_desc = nullptr, *c_bout = nullptr; int c_desc_cap = 0;                                  // the first pass' descriptors and verdicts
    int *c_gdesc = nullptr, *c_gpool = nullptr, *c_glab = nullptr, *c_gout = nullptr; int c_g_cap = 0;      // a level of the recursion
    int *c_map = nullptr; int c_map_cap = 0;                                                       // the cluster map for the nursery's chains
    ClusterMirror cmir;
    long levels = 0;                                                                               // levels of the recursion launched so far

    void ensure_scratch()
    {
        if (c_cap >= e.S.Ncap) return;
        c_cap = e.S.Ncap;
        c_Sm = blocks.dev<double>((size_t)c_cap * c_cap); c_knn = blocks.dev<int>((size_t)c_cap * c_cap); c_lab = blocks.dev<int>(c_cap);
        c_cnt = blocks.dev<int>(e.S.maxc); c_olduid = blocks.dev<unsigned>(e.S.maxc);
    }
    // (Engine::grow_clusters: the list of clusters has room for maxc now)
    void regrow_counts(int maxc) { if (c_cnt) { blocks.release(c_cnt); blocks.release(c_olduid); c_cnt = blocks.dev<int>(maxc); c_olduid = blocks.dev<unsigned>(maxc); } }

    void ask_mirror()
    {
        const PcState &S = e.S;
        const int nc = e.h_ctl->ncluster, maxc = S.maxc, Ncap = S.Ncap;
        cmir.size(Ncap, maxc);
        e.fetch_raw(cmir.lc.data(), S.live_cluster, sizeof(int) * Ncap); e.fetch_raw(cmir.lp.data(), S.live_pos, sizeof(int) * Ncap);
        e.fetch_raw(cmir.Xp.data(), S.logXp, sizeof(double) * nc); e.fetch_raw(cmir.ZXp.data(), S.logZXp, sizeof(double) * nc);
        e.fetch_raw(cmir.Zp.data(), S.logZp, sizeof(double) * nc); e.fetch_raw(cmir.Zp2.data(), S.logZp2, sizeof(double) * nc);
        e.fetch_raw(cmir.ZpXp.data(), S.logZpXp, sizeof(double) * nc); e.fetch_raw(cmir.thr.data(), S.death_thr, sizeof(double) * nc);
        e.fetch_raw(cmir.XQ.data(), S.XpXq, sizeof(double) * (size_t)nc * maxc); e.fetch_raw(cmir.uid.data(), S.cl_uid, sizeof(unsigned) * nc);
    }

    // add_cluster (run_time_info.f90:303-505): cluster p splits into nnew clusters appended at the end
    void add_cluster(int p, const std::vector<int> &labels, int nnew)
    {
        const int nc = e.h_ctl->ncluster, ncn = nc + nnew - 1;
        if (g_inject_fault.load() == 2) { g_inject_fault = 0; engine_fail(PC_RC_LIMIT, "more than %d clusters (injected)", nc); }
        if (ncn > e.S.maxc) { e.grow_clusters(ncn); cmir.valid = false; }
        const PcState &S = e.S;
        const int maxc = S.maxc;
        e.nsplits++;
        // everything the host's half of the split reads: there since the update's first pass, or asked for now in ONE wait (a run in step
        // shares it with the others)
        if (!cmir.valid || cmir.maxc != maxc) { ask_mirror(); e.fetch_wait(); cmir.valid = true; }
        auto up = [&](auto *dst, const auto &v, size_t n) { e.send_raw(dst, v.data(), sizeof(v[0]) * n); };
        const SplitParent par = add_cluster_relabel(cmir, nc, p, labels, nnew, e.h_ctl->next_cluster_uid);
        up(S.live_cluster, cmir.lc, cmir.lc.size()); up(S.live_pos, cmir.lp, cmir.lp.size());
        up(c_olduid, par.olduid, (size_t)nc);
        // (the Cholesky factors and covariances of the clusters behind p move up a block: one launch, not two copies per cluster)
        e.direct_op();
        pc_launch_shift_mats(&S, p, nc, e.st);
        up(S.cl_uid, cmir.uid, (size_t)ncn); up(S.death_thr, cmir.thr, (size_t)ncn);
        // lists, contours, live log-sum-exp of every cluster; then the phantoms find their new homes
        e.direct_op();
        pc_launch_rebuild(&S, ncn, e.st);
        pc_launch_ph_rehome(&S, e.h_ctl->nphantom, ncn, c_olduid, nc, c_cnt, e.st);
        std::vector<int> nph, nlv;
        e.fetch(nph, (const int *)c_cnt, ncn); e.fetch(nlv, (const int *)S.cl_n, ncn);
        e.fetch_wait();
        add_cluster_evidence(cmir, par, nc, p, nnew, nlv, nph, e.split_child, e.split_parent, e.split_logfrac);
        up(S.logXp, cmir.Xp, (size_t)ncn); up(S.logZXp, cmir.ZXp, (size_t)ncn); up(S.logZp, cmir.Zp, (size_t)ncn); up(S.logZp2, cmir.Zp2, (size_t)ncn); up(S.logZpXp, cmir.ZpXp, (size_t)ncn);
        up(S.XpXq, cmir.XQ, (size_t)ncn * maxc);
        e.h_ctl->ncluster = ncn;
        e.ncluster_peak = std::max(e.ncluster_peak, ncn);
    }

    // one level of the recursion after the other until no part is open: a launch (in step with other runs: a record) and a wait each
    void refine(PartRefiner &parts)
    {
        while (parts.work_left()) {
            const PartRefiner::Level &lev = parts.next_level();
            const int nb = lev.nb, npool = (int)lev.pool.size();
            levels++;
            // (the parts of a cluster are disjoint: their neighbour lists fit where the first pass' did)
            if (lev.koff > (long long)c_cap * c_cap) engine_fail(PC_RC_DEVICE, "clustering: the parts' neighbour lists (%lld entries) exceed the scratch of %d points", lev.koff, c_cap);
            if (c_g_cap < std::max(nb, npool)) {
                blocks.release(c_gdesc); blocks.release(c_gpool); blocks.release(c_glab); blocks.release(c_gout);
                c_g_cap = std::max(2 * std::max(nb, npool), e.S.Ncap);
                c_gdesc = blocks.dev<int>((size_t)5 * c_g_cap); c_gpool = blocks.dev<int>(c_g_cap); c_glab = blocks.dev<int>(c_g_cap); c_gout = blocks.dev<int>(c_g_cap);
            }
            e.send_pre(c_gdesc, lev.gdesc.data(), sizeof(int) * lev.gdesc.size());
            e.send_pre(c_gpool, lev.pool.data(), sizeof(int) * lev.pool.size());
            // (not stage(): a run on its own fails where the launcher declines; in step the row's one-run launch is taken instead)
            if (e.co) e.co->rec(rec_clusg(e.S, c_gdesc, c_Sm, c_gpool, c_knn, c_glab, c_gout, nb, lev.mmax));
            else if (pc_launch_knn_cluster_sub(c_gdesc, nb, lev.mmax, c_Sm, c_gpool, c_knn, c_glab, c_gout, e.st)) engine_fail(PC_RC_LDS, "cluster of %d points too large for the LDS kNN sort", lev.mmax);
            std::vector<int> labs, nums;
            e.fetch(labs, (const int *)c_glab, lev.pool.size()); e.fetch(nums, (const int *)c_gout, (size_t)nb);
            e.fetch_wait();
            parts.take(labs, nums);
        }
    }

    // do_clustering (clustering.f90:253-324).  First pass: every cluster with more than two points at once (three launches, the counts down
    // and the verdicts back: two host waits per update); the clusters in which it finds more than one group are refined level by level
    // and split by add_cluster, in the reference's order.  cn: the clusters' sizes (asked for here when they are not the list's).
    // dims / nd_sub: the coordinates of the sub-dimension pass (nd_sub = 0: all).  cmap_out: the pass leaves the map of the list's clusters
    // through it there and does not move the nursery's chains itself (two passes in one update: the caller composes the two maps).
    // tap: the first pass's scratch of its first cluster goes to the caller's arrays, in a wait of its own before a level overwrites the lists
    bool do_clustering(std::vector<int> cn = std::vector<int>(), const int *dims = nullptr, int nd_sub = 0, std::vector<int> *cmap_out = nullptr, ClusterTap *tap = nullptr)
    {
        ensure_scratch();
        bool found = false;
        cmir.valid = false;                              // (the contraction has moved volumes and evidences since the last update)
        struct MirrorEnds { ClusterMirror &m; ~MirrorEnds() { m.valid = false; } } mirror_ends{cmir};
        const int nold = e.h_ctl->ncluster;
        if (c_desc_cap < nold) { blocks.release(c_desc); blocks.release(c_bout); c_desc_cap = std::max(2 * nold, 64); c_desc = blocks.dev<int>((size_t)4 * c_desc_cap); c_bout = blocks.dev<int>(c_desc_cap); }
        if ((int)cn.size() != nold) { e.fetch(cn, (const int *)e.S.cl_n, (size_t)nold); e.fetch_wait(); }
        std::vector<std::vector<int>> final_labels((size_t)nold); std::vector<int> final_num((size_t)nold, 1);
        const FirstPass fp = first_pass_descriptors(cn);
        if (fp.nd() > 0) {
            // (a cluster's points are live slots of its own: the blocks of all fit the scratch sized for every slot)
            if (fp.o2 > (long long)c_cap * c_cap) engine_fail(PC_RC_DEVICE, "clustering: the clusters' similarity blocks (%lld entries) exceed the scratch of %d points", fp.o2, c_cap);
            e.send_pre(c_desc, fp.desc.data(), sizeof(int) * fp.desc.size());
            // (in step with other runs: the first pass of all runs that update in this round in three launches)
            // (not stage(): a run on its own launches from the host's copy of the descriptors, pc_launch_knn_cluster_batch)
            if (e.co) e.co->rec(rec_clus1(e.S, c_desc, c_Sm, c_knn, c_lab, c_bout, dims, fp.nd(), fp.nmax, nd_sub));
            else if (pc_launch_knn_cluster_batch(&e.S, fp.desc.data(), c_desc, fp.nd(), c_Sm, c_knn, c_lab, c_bout, dims, nd_sub, e.st)) engine_fail(PC_RC_LDS, "a cluster too large for the LDS kNN sort");
            std::vector<int> out, lab0;
            e.fetch(out, (const int *)c_bout, (size_t)fp.nd());
            e.fetch(lab0, (const int *)c_lab, (size_t)fp.o1);        // (the first pass' labels of every cluster: a few KB, the same wait)
            ask_mirror();                                            // (and what a split will read, should the pass find one)
            e.fetch_wait();
            cmir.valid = true;
            if (tap) {
                const size_t n = (size_t)fp.desc[1];
                if ((int)n > tap->cap) engine_fail(PC_RC_LIMIT, "the first cluster's scratch was asked for with room for %d points; it has %d", tap->cap, (int)n);
                tap->n = (int)n;
                e.fetch_raw(tap->Sm, c_Sm, sizeof(double) * n * n); e.fetch_raw(tap->knn, c_knn, sizeof(int) * n * n); e.fetch_raw(tap->lab, c_lab, sizeof(int) * n);
                e.fetch_wait();
            }
            PartRefiner parts;
            parts.open(fp, out, lab0);
            refine(parts);
            parts.finish(final_labels, final_num);
        }
        int ic = 0;
        std::vector<int> cmap = cluster_map_identity(nold);
        for (int j = 0; j < nold; ++j) {                 // j: the cluster's number when the update began; ic: its number now
            if (ic >= e.h_ctl->ncluster) break;
            if (final_num[j] > 1) { found = true; add_cluster(ic, final_labels[j], final_num[j]); cluster_map_split_at(cmap, ic); }
            else ic++;
        }
        if (found) {
            if (e.cfg.epoch_discard) e.h_ctl->admin_epoch++;         // nested_sampling.F90:331-333 as written: every chain in flight is lost
            else if (!cmap_out) remap_nursery(cmap, nold);
            e.h_ctl->status = PC_ST_RUNNING;
            e.send_raw(e.S.ctl, e.h_ctl, sizeof(PcCtl));
        }
        if (cmap_out) cmap_out->swap(cmap);
        return found;
    }
    // the engine's rule (epoch_discard = 0): the chains seeded in clusters the update left alone stay in the nursery, under their new numbers
    void remap_nursery(const std::vector<int> &cmap, int nold)
    {
        if (e.h_ctl->i_nursery <= 0) return;
        if (c_map_cap < nold) { blocks.release(c_map); c_map_cap = std::max(2 * nold, 64); c_map = blocks.dev<int>(c_map_cap); }
        e.send_raw(c_map, cmap.data(), sizeof(int) * (size_t)nold);
        e.direct_op();
        pc_launch_remap_chains(&e.S, c_map, nold, e.h_ctl->i_nursery, e.st);
    }
};
