// pc_doors.h -- the kernel-level doors of the parity and accuracy tests: entry points of the C ABI that set up an engine (or a few device
// blocks), install a given state in it, launch what a run launches at that point and hand back what the kernels left.  No door is on a run's path.
//
// Host only.  Included by pc_engine.hip alone, behind Engine and pc_step.h, in front of its own extern "C" block (the device maximiser there
// goes through with_engine too).  The including file provides, before the include: polychord_hip.h (the doors' declarations,
// pchip_settings_default), pc_state.h, pc_launch.h, pc_plan.h, pc_prior_table.h, pc_cohort.h, pc_split.h; HIP and HIPCHK, EngineError, engine_fail
// and the PC_RC_* codes; RunBlocks (pc_blocks.h); and
//   of Engine, these members and no others:
//     setup, destroy, S, st, blocks, cfg.epoch_discard, h_ctl
//     grow_clusters, grow_phantoms, covmats
//     keep, blk, d_total, ph2, phL2, phC2, phU2, count, upd_part, upd_part_cap, upd_shift      (the update's scratch: pchip_update_factors)
//     clus, sub_dims, c_subdims, nsplits, split_child, split_parent, split_logfrac            (the clustering: pchip_cluster_update)
//
// The helpers come first, each once.  A new door is a check of its arguments, one of with_engine / with_blocks, and what it launches.
#pragma once
#include <vector>
#include <string>
#include <memory>
#include <new>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cmath>

namespace {

// body() and its code.  An EngineError: the message to stderr, HIP's last error cleared, the error's code; no host memory for a vector the
// caller sized: PC_RC_MEMORY, with pchip_run_hooks' message.  product (the device maximiser, whose callers read polychord_hip_last_error()
// and take anything but 0 for a failure): the message goes there too, and an error without a code is a device failure.
template <class Body> int door_guard(Body &&body, bool product = false)
{
    try {
        return body();
    } catch (const EngineError &e) {
        std::fprintf(stderr, "polychord_hip: %s\n", e.msg.c_str());
        if (product) pc_abi_set_last_error(e.msg.c_str());
        (void)hipGetLastError();
        return (product && e.code == 0) ? PC_RC_DEVICE : e.code;
    } catch (const std::bad_alloc &) {
        std::fprintf(stderr, "polychord_hip: out of host memory\n");
        return PC_RC_MEMORY;
    }
}
// an engine set up for the problem, body(E) under the guard, and the teardown however that ended (what the body took from E.blocks goes back there)
template <class Body> int with_engine(const pchip_settings &c, const pchip_like &like, const pchip_prior &prior, Body &&body, bool product = false)
{
    Engine E;
    const int rc = door_guard([&] { E.setup(c, like, prior); return body(E); }, product);
    E.destroy();
    return rc;
}
// the device of a door without an engine: 0, or 2 where there is none
int door_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); std::fprintf(stderr, "polychord_hip: no HIP device available -- this engine has no CPU path\n"); return 2; }
    return hipSetDevice(device >= 0 ? device % ndev : 0) == hipSuccess ? 0 : 2;
}
// ... and its blocks: body(blocks) under the guard on that device, with a ledger of its own that gives everything back once the device is
// idle, however the body ended.  These doors document "0, or 1 (arguments) / 2 (device)": whatever failed past the arguments -- a HIP call, a
// launch, a block the caches could not get (7 from the guard) -- is 2 to their callers.
template <class Body> int with_blocks(int device, Body &&body)
{
    if (door_device(device)) return 2;
    RunBlocks blocks;
    const int rc = door_guard([&] { return body(blocks); });
    if (hipDeviceSynchronize() != hipSuccess || rc) (void)hipGetLastError();
    blocks.release_all();
    return rc ? 2 : 0;
}

// nchains chains of one cluster: the settings of an engine that holds exactly them ...
pchip_settings door_chain_settings(const pchip_settings &s, int nchains)
{
    pchip_settings c = s;
    c.nlive = nchains; c.nprior = nchains; c.batch = nchains; c.do_clustering = 0;
    return c;
}
// ... and the chains in it: chain c seeded from row c of seeds (nTotal doubles), all under the same Cholesky factor and contour
void door_install_chains(Engine &E, int nchains, const double *seeds, const double *chol, double contour)
{
    PcState &S = E.S;
    const int nT = S.nT, D = S.D;
    std::vector<double> ll(nchains); std::vector<int> idn(nchains), zero(nchains, 0);
    for (int i = 0; i < nchains; ++i) { ll[i] = seeds[(size_t)i * nT + S.l0]; idn[i] = i; }
    HIPCHK(hipMemcpy(S.live, seeds, sizeof(double) * (size_t)nchains * nT, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.live_logL, ll.data(), sizeof(double) * nchains, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.live_cluster, zero.data(), sizeof(int) * nchains, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.live_pos, idn.data(), sizeof(int) * nchains, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.cl_list, idn.data(), sizeof(int) * nchains, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.cl_n, &nchains, sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.logLp, &contour, sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.chol, chol, sizeof(double) * D * D, hipMemcpyHostToDevice));
    S.seed_override = 1;
}
// the problem of the doors that bring their own points: the built-in Gaussian in the unit box (never evaluated: an engine needs one)
void door_builtin_problem(pchip_like &like, pchip_prior &prior)
{
    std::memset(&like, 0, sizeof(like)); like.kind = PC_LIKE_GAUSSIAN; like.mu = 0.5; like.sigma = 1.0;
    std::memset(&prior, 0, sizeof(prior)); prior.kind = 1;
}
// nph phantom rows as a run holds them: padded to nTotal (logL_in_row: the value in the row too), logL, the cluster's id (-1: none), ids of their own
void door_install_phantoms(Engine &E, int nph, const double *phantom, const double *ph_logL, const int *ph_cluster, bool logL_in_row)
{
    if (nph <= 0) return;
    PcState &S = E.S;
    const int nT = S.nT, D = S.D;
    std::vector<double> rows((size_t)nph * nT, 0.0);
    std::vector<unsigned> cu(nph); std::vector<unsigned long long> uid(nph);
    for (int j = 0; j < nph; ++j) {
        std::memcpy(rows.data() + (size_t)j * nT, phantom + (size_t)j * D, sizeof(double) * D);
        if (logL_in_row) rows[(size_t)j * nT + S.l0] = ph_logL[j];
        cu[j] = ph_cluster[j] < 0 ? PC_CUID_NONE : (unsigned)ph_cluster[j]; uid[j] = (unsigned long long)j;
    }
    HIPCHK(hipMemcpy(S.phantom, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.ph_logL, ph_logL, sizeof(double) * nph, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.ph_cuid, cu.data(), sizeof(unsigned) * nph, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.ph_uid, uid.data(), sizeof(unsigned long long) * nph, hipMemcpyHostToDevice));
}

// pchip_cluster_update's set-up: an engine for nlive slots that clusters, and the point set installed in it as a run holds it at the start of an update
pchip_settings cluster_door_settings(const pchip_settings &s, int nlive)
{
    pchip_settings c;
    pchip_settings_default(&c, s.nDims, 0);
    c.nlive = nlive; c.nprior = nlive; c.batch = 1; c.num_repeats = 1; c.do_clustering = 1; c.seed = 1; c.feedback = 0; c.device = s.device; c.ablate = s.ablate;
    c.n_sub_cluster = s.n_sub_cluster; c.sub_cluster_dims = s.sub_cluster_dims;
    return c;
}
void cluster_door_install(Engine &E, const pchip_cluster_in &I, double *init_out, std::vector<int> &cn)
{
    const int nc0 = I.ncluster, nlive = I.nlive, nph = I.nph;
    HIPCHK(hipStreamSynchronize(E.st));                      // (the set-up's own launch writes the per-cluster arrays and the control block)
    if (nc0 > E.S.maxc) E.grow_clusters(nc0);
    if (nph > E.S.Pcap) E.grow_phantoms(nph);
    PcState &S = E.S;
    const int nT = S.nT, D = S.D, Ncap = S.Ncap, maxc = S.maxc;
    // the live slots: rows, values, (cluster, position) labels, and the clusters' lists and sizes made of them
    std::vector<double> rows((size_t)Ncap * nT, 0.0);
    std::vector<int> lpos(Ncap, 0), list((size_t)nc0 * Ncap, 0);
    cn.assign(nc0, 0);
    for (int i = 0; i < nlive; ++i) {
        std::memcpy(rows.data() + (size_t)i * nT, I.live + (size_t)i * D, sizeof(double) * D);
        rows[(size_t)i * nT + S.l0] = I.live_logL[i];
        const int cl = I.live_cluster[i];
        if (cl >= 0) { lpos[i] = cn[cl]; list[(size_t)cl * Ncap + cn[cl]] = i; cn[cl]++; }
    }
    HIPCHK(hipMemcpy(S.live, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.live_logL, I.live_logL, sizeof(double) * nlive, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.live_cluster, I.live_cluster, sizeof(int) * nlive, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.live_pos, lpos.data(), sizeof(int) * nlive, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.cl_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.cl_n, cn.data(), sizeof(int) * nc0, hipMemcpyHostToDevice));
    door_install_phantoms(E, nph, I.phantom, I.ph_logL, I.ph_cluster, true);
    // the clusters' ids, volumes and evidences: fixed and distinct
    std::vector<unsigned> cuid(nc0);
    std::vector<double> init((size_t)5 * nc0 + (size_t)nc0 * nc0), XQ((size_t)nc0 * maxc, 0.0);
    const double sum = 0.5 * nc0 * (nc0 + 1.0);
    for (int k = 0; k < nc0; ++k) {
        cuid[k] = (unsigned)k;
        init[k] = std::log((k + 1.0) / sum); init[nc0 + k] = -1.0 - 0.25 * k; init[2 * nc0 + k] = -2.0 - 0.125 * k;
        init[3 * nc0 + k] = -3.0 - 0.5 * k; init[4 * nc0 + k] = -4.0 - 0.375 * k;
    }
    for (int a = 0; a < nc0; ++a)
        for (int b = 0; b < nc0; ++b) {
            const double v = init[a] + init[b] + (a == b ? std::log(1.5) : 0.0);
            init[(size_t)5 * nc0 + (size_t)a * nc0 + b] = v; XQ[(size_t)a * maxc + b] = v;
        }
    std::memcpy(init_out, init.data(), sizeof(double) * init.size());
    HIPCHK(hipMemcpy(S.cl_uid, cuid.data(), sizeof(unsigned) * nc0, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.logXp, init.data(), sizeof(double) * nc0, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.logZp, init.data() + nc0, sizeof(double) * nc0, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.logZXp, init.data() + 2 * nc0, sizeof(double) * nc0, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.logZp2, init.data() + 3 * nc0, sizeof(double) * nc0, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.logZpXp, init.data() + 4 * nc0, sizeof(double) * nc0, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.XpXq, XQ.data(), sizeof(double) * XQ.size(), hipMemcpyHostToDevice));
    E.h_ctl->ncluster = nc0; E.h_ctl->nphantom = nph; E.h_ctl->next_cluster_uid = (unsigned)nc0;
    HIPCHK(hipMemcpy(S.ctl, E.h_ctl, sizeof(PcCtl), hipMemcpyHostToDevice));
}

// path 1 of pchip_cluster_update (below): R engines, so the guard directly, and every engine's teardown after it
int cluster_door_many(const pchip_settings *s, int R, const pchip_cluster_in *in, pchip_cluster_out *out)
{
    pchip_like like; pchip_prior prior;
    door_builtin_problem(like, prior);
    std::vector<std::unique_ptr<Engine>> E;
    const int rc = door_guard([&] {
        std::vector<std::vector<int>> cn((size_t)R);
        for (int r = 0; r < R; ++r) {
            E.emplace_back(new Engine);
            E[r]->setup(cluster_door_settings(s[r], in[r].nlive), like, prior);
            cluster_door_install(*E[r], in[r], out[r].init, cn[r]);
            E[r]->clus.ensure_scratch();
        }
        hipStream_t st = E[0]->st;                           // (every set's own stream is idle: the installs were blocking copies)
        PcManyRec *d_recs = E[0]->blocks.dev<PcManyRec>((size_t)R);
        // one stage for the records of several sets: laid down, folded and launched as Cohort::flush does for the runs of a round
        auto launch = [&](std::vector<Cohort::Rec> &recs) {
            if (recs.empty()) return;
            std::vector<PcManyRec> hs(recs.size());
            std::vector<const Cohort::Rec *> ord;
            for (size_t i = 0; i < recs.size(); ++i) { Cohort::lay(hs[i], recs[i]); ord.push_back(&recs[i]); }
            HIPCHK(hipMemcpy(d_recs, hs.data(), sizeof(PcManyRec) * hs.size(), hipMemcpyHostToDevice));
            const Cohort::Stage &row = Cohort::stage(recs[0].kind);
            int fold[3];
            Cohort::folds_of(row, ord.data(), ord.data() + ord.size(), fold);
            if (row.many(recs[0], d_recs, (int)recs.size(), fold, st)) engine_fail(PC_RC_LDS, "a cluster too large for the LDS kNN sort");
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
        };
        auto down = [&](std::vector<int> &v, const int *src, size_t n) { v.resize(n); if (n) HIPCHK(hipMemcpy(v.data(), src, sizeof(int) * n, hipMemcpyDeviceToHost)); };
        auto up = [&](int *dst, const std::vector<int> &v) { if (!v.empty()) HIPCHK(hipMemcpy(dst, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice)); };
        // the first pass
        std::vector<FirstPass> fp((size_t)R);
        std::vector<PartRefiner> parts((size_t)R);
        std::vector<Cohort::Rec> recs;
        for (int r = 0; r < R; ++r) {
            Engine &e = *E[r]; auto &cu = e.clus;
            fp[r] = first_pass_descriptors(cn[r]);
            if (fp[r].nd() == 0) continue;
            if (fp[r].o2 > (long long)cu.c_cap * cu.c_cap) engine_fail(PC_RC_DEVICE, "clustering: the clusters' similarity blocks (%lld entries) exceed the scratch of %d points", fp[r].o2, cu.c_cap);
            cu.c_desc_cap = std::max(2 * in[r].ncluster, 64);
            cu.c_desc = e.blocks.dev<int>((size_t)4 * cu.c_desc_cap); cu.c_bout = e.blocks.dev<int>(cu.c_desc_cap);
            cu.c_g_cap = e.S.Ncap;
            cu.c_gdesc = e.blocks.dev<int>((size_t)5 * cu.c_g_cap); cu.c_gpool = e.blocks.dev<int>(cu.c_g_cap); cu.c_glab = e.blocks.dev<int>(cu.c_g_cap); cu.c_gout = e.blocks.dev<int>(cu.c_g_cap);
            up(cu.c_desc, fp[r].desc);
            recs.push_back(rec_clus1(e.S, cu.c_desc, cu.c_Sm, cu.c_knn, cu.c_lab, cu.c_bout, e.sub_dims.empty() ? nullptr : e.c_subdims, fp[r].nd(), fp[r].nmax, (int)e.sub_dims.size()));
        }
        launch(recs);
        for (int r = 0; r < R; ++r) {
            out[r].levels = 0; out[r].scratch_n = 0;
            if (fp[r].nd() == 0) continue;
            auto &cu = E[r]->clus;
            std::vector<int> verdict, lab0;
            down(verdict, cu.c_bout, (size_t)fp[r].nd()); down(lab0, cu.c_lab, (size_t)fp[r].o1);
            if (out[r].scratch_Sm) {
                const size_t n = (size_t)fp[r].desc[1];
                if ((int)n > out[r].scratch_cap) engine_fail(PC_RC_LIMIT, "the first cluster's scratch was asked for with room for %d points; it has %d", out[r].scratch_cap, (int)n);
                out[r].scratch_n = (int)n;
                HIPCHK(hipMemcpy(out[r].scratch_Sm, cu.c_Sm, sizeof(double) * n * n, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(out[r].scratch_knn, cu.c_knn, sizeof(int) * n * n, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(out[r].scratch_lab, cu.c_lab, sizeof(int) * n, hipMemcpyDeviceToHost));
            }
            parts[r].open(fp[r], verdict, lab0);
        }
        // the recursion, level by level: the open parts of every set in one launch
        while (true) {
            recs.clear();
            std::vector<int> who;
            for (int r = 0; r < R; ++r) {
                if (fp[r].nd() == 0 || !parts[r].work_left()) continue;
                Engine &e = *E[r]; auto &cu = e.clus;
                const PartRefiner::Level &lev = parts[r].next_level();
                if (lev.koff > (long long)cu.c_cap * cu.c_cap || std::max(lev.nb, (int)lev.pool.size()) > cu.c_g_cap)
                    engine_fail(PC_RC_DEVICE, "clustering: the parts of a level (%d, %lld list entries) exceed the scratch of %d points", lev.nb, lev.koff, cu.c_cap);
                up(cu.c_gdesc, lev.gdesc); up(cu.c_gpool, lev.pool);
                recs.push_back(rec_clusg(e.S, cu.c_gdesc, cu.c_Sm, cu.c_gpool, cu.c_knn, cu.c_glab, cu.c_gout, lev.nb, lev.mmax));
                who.push_back(r);
            }
            if (recs.empty()) break;
            launch(recs);
            for (int r : who) {
                auto &cu = E[r]->clus;
                std::vector<int> labs, nums;
                down(labs, cu.c_glab, parts[r].lev.pool.size()); down(nums, cu.c_gout, (size_t)parts[r].lev.nb);
                parts[r].take(labs, nums);
                out[r].levels++;
            }
        }
        // every set's final labels: live_pos = a slot's part (1-based) within its cluster, cl_n = the parts of each cluster
        for (int r = 0; r < R; ++r) {
            const pchip_cluster_in &I = in[r]; pchip_cluster_out &O = out[r];
            std::vector<std::vector<int>> final_labels((size_t)I.ncluster); std::vector<int> final_num((size_t)I.ncluster, 1);
            if (fp[r].nd() > 0) parts[r].finish(final_labels, final_num);
            std::vector<int> at((size_t)I.ncluster, 0);
            for (int i = 0; i < I.nlive; ++i) {
                const int c = I.live_cluster[i];
                O.live_cluster[i] = c; O.live_pos[i] = 0;
                if (c >= 0) { O.live_pos[i] = final_num[c] > 1 ? final_labels[c][(size_t)at[c]] : 1; at[c]++; }
            }
            O.ncluster = I.ncluster; O.nsplit = 0;
            for (int c = 0; c < I.ncluster; ++c) O.cl_n[c] = final_num[c];
        }
        return 0;
    });
    for (auto &e : E) e->destroy();
    return rc;
}

}  // namespace

extern "C" {

// kernel-level entry for the parity tests: run K0 + K1 for `nchains` chains, chain c seeded from
// seeds[c] (row of nTotal doubles), all under the same Cholesky factor and contour.
int pchip_slice_chains(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, unsigned batch,
                       int nchains, const double *seeds, const double *chol, double contour, double *babies_out,
                       double *nhats_out, int *nlike_out)
{
    if (like->kind == PCHIP_LIKE_SOURCE || (s->ablate & PC_ABL_RTC_BUILTINS)) {
        std::fprintf(stderr, "polychord_hip: pchip_slice_chains does not take a device source likelihood (or settings.ablate bit 15)\n");
        if (const char *why = pc_quad_batch_refusal("pchip_slice_chains", like, prior, nullptr)) pc_abi_set_last_error(why);
        return 1;
    }
    return with_engine(door_chain_settings(*s, nchains), *like, *prior, [&](Engine &E) {
        PcState &S = E.S;
        const int nT = S.nT, D = S.D, nr = S.nr;
        door_install_chains(E, nchains, seeds, chol, contour);
        const int rc = pc_launch_nhats(&S, batch, nchains, E.st) || pc_launch_slice(&S, batch, nchains, E.st);
        HIPCHK(hipStreamSynchronize(E.st));
        HIPCHK(hipMemcpy(babies_out, S.babies, sizeof(double) * (size_t)nchains * nr * nT, hipMemcpyDeviceToHost));
        if (nhats_out) HIPCHK(hipMemcpy(nhats_out, S.nhat, sizeof(double) * (size_t)nchains * nr * D, hipMemcpyDeviceToHost));
        if (nlike_out) HIPCHK(hipMemcpy(nlike_out, S.ch_nlike, sizeof(int) * nchains, hipMemcpyDeviceToHost));
        return rc;
    });
}

// kernel-level entry for the accuracy tests of the directions (tests/test_directions.py): K0 alone, set up as pchip_slice_chains sets it
// up (one cluster, chain c seeded from row c, the caller's Cholesky factor; the contour is the lowest of the seeds' values), by the launcher a
// run would take:
//   path 0: pc_launch_nhats, the whole kernels (what pchip_slice_chains launches);
//   path 1: pc_launch_nhats_part(1) then (2) on the run's own nhat_raw, as Engine::enqueue_nursery does where pc_nhats_splittable holds;
//   path 2: the same with packed = 1 -- the bases of pc_slice_t.hip (pc_bases_t_ok).
// A path the state does not have: PCHIP_NO_SUCH_PATH, nothing launched.  raw_out (paths 1 and 2): the orthonormal bases part 1 left in
// nhat_raw, brought from the layout of the kernel that wrote them to [chain][basis][vector][coordinate]; vectors no kernel wrote keep
// whatever the block held.  k_slice is not run.
int pchip_directions(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, unsigned batch, int nchains,
                     const double *seeds, const double *chol, int path, double *nhat_out, double *nhat_w_out,
                     double *nhat_Ms_out, double *ch_My_out, int *has_Ms, double *raw_out, int nrows, int nbases)
{
    if (!s || !like || !prior || nchains < 1 || !seeds || !chol || path < 0 || path > 2 || !nhat_out || !nhat_w_out || (path != 0 && !raw_out)) {
        pc_abi_set_last_error("pchip_directions: settings, likelihood, prior, nchains >= 1 seed rows, a Cholesky factor, path 0, 1 or 2, arrays for nhat and nhat_w (and for the raw bases on paths 1 and 2)");
        return 1;
    }
    if (like->kind == PCHIP_LIKE_SOURCE || (s->ablate & PC_ABL_RTC_BUILTINS)) {
        pc_abi_set_last_error("pchip_directions does not take a device source likelihood (or settings.ablate bit 15)");
        return 1;
    }
    if (s->nDims > 256) return PCHIP_NO_SUCH_PATH;
    const pchip_settings c = door_chain_settings(*s, nchains);
    return with_engine(c, *like, *prior, [&](Engine &E) {
        PcState &S = E.S;
        const int nT = S.nT, D = S.D, nr = S.nr, nb = S.nb_total;
        int rc = 0;
        if (nrows != nr || nbases != nb) {
            pc_abi_set_last_error("pchip_directions: the caller's arrays are for another number of directions or bases than the settings give");
            rc = 1;
        } else if ((path != 0 && !pc_nhats_splittable(&S)) || (path == 2 && !pc_bases_t_ok(&S))) rc = PCHIP_NO_SUCH_PATH;
        if (has_Ms) *has_Ms = S.nhat_Ms != nullptr ? 1 : 0;
        if (rc) return rc;
        double contour = seeds[S.l0];
        for (int i = 1; i < nchains; ++i) contour = std::min(contour, seeds[(size_t)i * nT + S.l0]);
        door_install_chains(E, nchains, seeds, chol, contour);
        if (path == 0) rc = pc_launch_nhats(&S, batch, nchains, E.st) ? PCHIP_NO_SUCH_PATH : 0;
        else rc = (pc_launch_nhats_part(&S, batch, nchains, 1, E.st, pc_part1_kind(path == 2, c.ablate)) || pc_launch_nhats_part(&S, batch, nchains, 2, E.st, 0)) ? PCHIP_NO_SUCH_PATH : 0;
        HIPCHK(hipStreamSynchronize(E.st));
        HIPCHK(hipGetLastError());
        if (rc) return rc;
        HIPCHK(hipMemcpy(nhat_out, S.nhat, sizeof(double) * (size_t)nchains * nr * D, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nhat_w_out, S.nhat_w, sizeof(double) * (size_t)nchains * nr, hipMemcpyDeviceToHost));
        if (S.nhat_Ms && nhat_Ms_out) HIPCHK(hipMemcpy(nhat_Ms_out, S.nhat_Ms, sizeof(double) * (size_t)nchains * nr * D, hipMemcpyDeviceToHost));
        if (S.ch_My && ch_My_out) HIPCHK(hipMemcpy(ch_My_out, S.ch_My, sizeof(double) * (size_t)nchains * D, hipMemcpyDeviceToHost));
        if (path == 0) return 0;
        // a basis block as its kernel laid it out: k_nhats<., 64, 1> and the packed bases vector-major, D doubles a vector; k_nhats_q<8 | 16, 1>
        // thread by thread, i.e. vector-major with rows of 32 | 64; k_basis in k_whiten's pair layout, 32 x 512 doubles
        const size_t blk = D <= 24 ? (size_t)D * D : D <= 32 ? (size_t)1024 : D <= 64 ? (size_t)4096 : (size_t)32 * 512;
        std::vector<double> raw((size_t)nchains * nb * blk);
        HIPCHK(hipMemcpy(raw.data(), S.nhat_raw, sizeof(double) * raw.size(), hipMemcpyDeviceToHost));
        for (size_t cb = 0; cb < (size_t)nchains * nb; ++cb) {
            const double *in = raw.data() + cb * blk;
            double *out = raw_out + cb * (size_t)D * D;
            for (int v = 0; v < D; ++v)
                for (int d = 0; d < D; ++d) {
                    size_t at;
                    if (D <= 24) at = (size_t)v * D + d;
                    else if (D <= 64) at = (size_t)v * (D <= 32 ? 32 : 64) + d;
                    else { const int n = 2 * (d >> 3) + (d & 1), lk = (d & 7) >> 1; at = (size_t)n * 512 + 64 * (v >> 4) + 16 * lk + (v & 15); }
                    out[(size_t)v * D + d] = in[at];
                }
        }
        return 0;
    });
}

// kernel-level entry beside pchip_directions (tests/test_bases_wave.py): the deck records part 1 of the split launch leaves behind the bases of
// a nursery (pc_deck_record, pc_seed.h), 66 ints a chain exactly as they lie there.  An engine as pchip_directions'; part 1 only, by the kernel
// a run on its own takes (settings.ablate bit 19: k_nhats<.., 64, 1>).  The caller's array goes into the block first: what comes back where
// the kernel writes no record (num_repeats > 64) is what the caller put there.
int pchip_deck_records(const pchip_settings *s, const pchip_like *like, const pchip_prior *prior, unsigned batch, int nchains, int *records_out)
{
    if (!s || !like || !prior || nchains < 1 || !records_out) {
        pc_abi_set_last_error("pchip_deck_records: settings, likelihood, prior, nchains >= 1 and an array of 66 ints a chain");
        return 1;
    }
    if (like->kind == PCHIP_LIKE_SOURCE || (s->ablate & PC_ABL_RTC_BUILTINS)) {
        pc_abi_set_last_error("pchip_deck_records does not take a device source likelihood (or settings.ablate bit 15)");
        return 1;
    }
    if (s->nDims > 24) return PCHIP_NO_SUCH_PATH;      // (no records behind the bases of the larger kernels)
    const pchip_settings c = door_chain_settings(*s, nchains);
    return with_engine(c, *like, *prior, [&](Engine &E) {
        PcState &S = E.S;
        if (!pc_nhats_splittable(&S) || S.ngrade > 1) return PCHIP_NO_SUCH_PATH;
        int *rec = (int *)(S.nhat_raw + (size_t)S.B * S.nb_total * S.D * S.D);      // pc_deck_record(S, 0)
        HIPCHK(hipMemcpy(rec, records_out, sizeof(int) * (size_t)nchains * 66, hipMemcpyHostToDevice));
        const int rc = pc_launch_nhats_part(&S, batch, nchains, 1, E.st, pc_part1_kind(false, c.ablate)) ? PCHIP_NO_SUCH_PATH : 0;
        HIPCHK(hipStreamSynchronize(E.st));
        HIPCHK(hipGetLastError());
        if (rc == 0) HIPCHK(hipMemcpy(records_out, rec, sizeof(int) * (size_t)nchains * 66, hipMemcpyDeviceToHost));
        return rc;
    });
}

// kernel-level entry for the parity tests: the device transform of a prior table at n hypercube points
int pchip_prior_transform(const pchip_prior *prior, int nDims, int n, const double *cube, double *theta, int device)
{
    if (!prior || prior->kind != PCHIP_PRIOR_TABLE || n < 1 || !cube || !theta) { pc_abi_set_last_error("pchip_prior_transform: a prior table (kind 2) and n >= 1 points"); return 1; }
    PcPriorTable T;
    const std::string err = pc_prior_table_build(nDims, prior->table, prior->hyper, T);
    if (!err.empty()) { pc_abi_set_last_error(err.c_str()); return 1; }
    if (nDims > 256) return 3;
    return with_blocks(device, [&](RunBlocks &blocks) {
        const std::vector<double> tp = T.dev_par(); const std::vector<int> ti = T.dev_int();
        const size_t nd = (size_t)n * nDims;
        double *d_tp = blocks.dev<double>(tp.size()), *d_c = blocks.dev<double>(nd), *d_t = blocks.dev<double>(nd); int *d_ti = blocks.dev<int>(ti.size());
        HIPCHK(hipMemcpy(d_tp, tp.data(), sizeof(double) * tp.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ti, ti.data(), sizeof(int) * ti.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_c, cube, sizeof(double) * nd, hipMemcpyHostToDevice));
        PcState S;
        std::memset(&S, 0, sizeof(S));
        S.D = nDims; S.prior.kind = PCHIP_PRIOR_TABLE; S.prior.lo = d_tp; S.prior.hi = (const double *)d_ti; S.src_pad = (int)T.mask;
        if (pc_launch_prior_transform(&S, n, d_c, d_t, nullptr)) return 2;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(theta, d_t, sizeof(double) * nd, hipMemcpyDeviceToHost));
        return 0;
    });
}

// kernel-level entry for tests/test_park_pack.py: the pack of the device batch callback (k_park_index, k_park_rows) on host arrays
int pchip_park_pack(int nchains, int nDims, const int *need, const double *prop, int *rank, int *count, double *cube, int device)
{
    if (nchains < 1 || nDims < 1 || !need || !prop || !rank || !count || !cube) { pc_abi_set_last_error("pchip_park_pack: nchains >= 1 flags and rows of nDims >= 1, and room for the ranks, the count and the rows"); return 1; }
    return with_blocks(device, [&](RunBlocks &blocks) {
        const size_t nd = (size_t)nchains * nDims;
        int *d_need = blocks.dev<int>(nchains), *d_rank = blocks.dev<int>(nchains), *d_count = blocks.dev<int>(1);
        double *d_prop = blocks.dev<double>(nd), *d_cube = blocks.dev<double>(nd);
        int *h_count = blocks.pin<int>(1);                  // (a pinned block of the cache is mapped, as the engine's own count word is)
        HIPCHK(hipMemcpy(d_need, need, sizeof(int) * nchains, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_prop, prop, sizeof(double) * nd, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_cube, cube, sizeof(double) * nd, hipMemcpyHostToDevice));      // (the caller's `cube` goes up first: the rows from count on come back as they were)
        void *dp = nullptr;
        *h_count = -1;
        HIPCHK(hipHostGetDevicePointer(&dp, h_count, 0));
        pc_launch_park_pack(nchains, nDims, d_need, 1, d_prop, d_rank, d_count, (int *)dp, d_cube, nullptr);
        int dc = -2;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(rank, d_rank, sizeof(int) * nchains, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&dc, d_count, sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cube, d_cube, sizeof(double) * nd, hipMemcpyDeviceToHost));
        *count = *(volatile int *)h_count;
        return dc == *count ? 0 : 2;         // the device word and the pinned word are one number
    });
}

// kernel-level entry for tests/test_par_accept.py: the acceptance of the parallel contraction (k_par_accept: par_search, par_rank, par_accept of
// pc_par.hip) on host arrays
int pchip_par_accept(int n, const double *snapshot_logL, int T, const double *cand_logL, const unsigned char *valid, int serial,
                     unsigned char *accept, int device)
{
    if (n < 1 || n > 8192 || T < 1 || T > 1024 || !snapshot_logL || !cand_logL || !valid || !accept) {
        pc_abi_set_last_error("pchip_par_accept: 1 <= n <= 8192 ascending snapshot values, 1 <= T <= 1024 candidates with their flags, and room for T answers");
        return 1;
    }
    for (int i = 1; i < n; ++i) if (!(snapshot_logL[i - 1] <= snapshot_logL[i])) { pc_abi_set_last_error("pchip_par_accept: the snapshot is not ascending"); return 1; }
    return with_blocks(device, [&](RunBlocks &blocks) {
        double *d_snap = blocks.dev<double>(n), *d_cand = blocks.dev<double>(T);
        unsigned char *d_valid = blocks.dev<unsigned char>(T), *d_acc = blocks.dev<unsigned char>(T);
        HIPCHK(hipMemcpy(d_snap, snapshot_logL, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_cand, cand_logL, sizeof(double) * (size_t)T, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_valid, valid, (size_t)T, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d_acc, 0xEE, (size_t)T));
        if (pc_launch_par_accept(n, d_snap, T, d_cand, d_valid, serial, d_acc, nullptr)) return 2;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(accept, d_acc, (size_t)T, hipMemcpyDeviceToHost));
        return 0;
    });
}

// kernel-level entry for tests/test_park_pack_many.py: the pack of a group of runs (k_park_index_many, k_park_rows_many) on host arrays, the
// runs' flags, proposals and ranks one run behind the other
int pchip_park_pack_many(int nruns, const int *nchains, int nDims, const int *need, const double *prop, int *rank, int *counts, int *total,
                         double *cube, int device)
{
    if (nruns < 1 || nruns > PC_PARK_MAX_RUNS || nDims < 1 || !nchains || !need || !prop || !rank || !counts || !total || !cube) {
        pc_abi_set_last_error("pchip_park_pack_many: 1 <= nruns <= 64 runs of nchains[r] >= 1 flags and rows of nDims >= 1, and room for the ranks, the counts, the total and the rows");
        return 1;
    }
    size_t all = 0; int max_chains = 0;
    for (int r = 0; r < nruns; ++r) {
        if (nchains[r] < 1) { pc_abi_set_last_error("pchip_park_pack_many: every run has at least one chain"); return 1; }
        all += (size_t)nchains[r]; max_chains = std::max(max_chains, nchains[r]);
    }
    return with_blocks(device, [&](RunBlocks &blocks) {
        const size_t nd = all * nDims;
        int *d_need = blocks.dev<int>(all), *d_rank = blocks.dev<int>(all), *d_count = blocks.dev<int>(PC_PARK_MAX_RUNS);
        double *d_prop = blocks.dev<double>(nd), *d_cube = blocks.dev<double>(nd);
        int *h_count = blocks.pin<int>(PC_PARK_MAX_RUNS + 1); PcParkRun *h_runs = blocks.pin<PcParkRun>(PC_PARK_MAX_RUNS);      // (pinned blocks of the cache are mapped, as the engine's own are)
        HIPCHK(hipMemcpy(d_need, need, sizeof(int) * all, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_prop, prop, sizeof(double) * nd, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_cube, cube, sizeof(double) * nd, hipMemcpyHostToDevice));      // (the caller's `cube` goes up first: the rows from the total on come back as they were)
        size_t o = 0;
        for (int r = 0; r < nruns; ++r) { h_runs[r] = PcParkRun{d_need + o, d_prop + o * nDims, d_rank + o, nchains[r], 1}; o += (size_t)nchains[r]; }
        for (int r = 0; r <= nruns; ++r) h_count[r] = -1;
        void *dp = nullptr, *dr = nullptr;
        HIPCHK(hipHostGetDevicePointer(&dp, h_count, 0));
        HIPCHK(hipHostGetDevicePointer(&dr, h_runs, 0));
        if (pc_launch_park_pack_many(nruns, (const PcParkRun *)dr, max_chains, nDims, d_count, (int *)dp, d_cube, nullptr)) return 2;
        std::vector<int> dc((size_t)nruns, -2);
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(rank, d_rank, sizeof(int) * all, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dc.data(), d_count, sizeof(int) * nruns, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cube, d_cube, sizeof(double) * nd, hipMemcpyDeviceToHost));
        long sum = 0; int rc = 0;
        for (int r = 0; r < nruns; ++r) { counts[r] = ((volatile int *)h_count)[r]; sum += counts[r]; if (dc[(size_t)r] != counts[r]) rc = 2; }      // the device words and the pinned words are the same numbers
        *total = ((volatile int *)h_count)[nruns];
        return sum != *total ? 2 : rc;
    });
}

// kernel-level entry for the accuracy tests of the update (tests/test_update_factors.py): covariance and Cholesky factor of given live
// and phantom rows by the launchers of Engine::do_update's non-deferred branch -- no hooks, no clustering, no resume file.
//   path 1: pc_launch_update_fused (one cluster, nDims <= 128, nph >= 1; pool mode unless settings.ablate has PC_ABL_NO_POOL; the chain
//           with PC_ABL_UPDATE_CHAIN), the moments about `shift` (NULL: the cube centre);
//   path 0: pc_launch_clean, the buffers swapped, the thresholds reset, pc_launch_covmats -- with one cluster on the row count from
//           before the clean (the kernels clamp to the device's count, as in a run nobody watches), with more on the count after it.
int pchip_update_factors(const pchip_settings *s, int ncluster, int nlive, const double *live, const int *live_cluster,
                         int nph, const double *phantom, const double *ph_logL, const int *ph_cluster, const double *threshold,
                         const double *shift, int path, double *cov, double *chol, int *count, double *shift_out, int *chol_suspect)
{
    if (!s || s->nDims < 1 || ncluster < 1 || nlive < 1 || !live || !live_cluster || nph < 0 || (nph > 0 && (!phantom || !ph_logL || !ph_cluster)) ||
        !threshold || !cov || !chol || !count || (path != 0 && path != 1)) {
        pc_abi_set_last_error("pchip_update_factors: nDims >= 1, ncluster >= 1, nlive >= 1 rows with their clusters, nph >= 0 rows with logL and cluster, a threshold per cluster, path 0 or 1, arrays for cov, chol and the counts");
        return 1;
    }
    if (s->nDims > 256) return 3;
    if (path == 1 && (ncluster != 1 || s->nDims > 128 || nph < 1)) { pc_abi_set_last_error("pchip_update_factors: the fused update (path 1) takes one cluster, nDims <= 128 and at least one phantom row"); return 1; }
    for (int i = 0; i < nlive; ++i) if (live_cluster[i] < 0 || live_cluster[i] >= ncluster) { pc_abi_set_last_error("pchip_update_factors: a live row's cluster is 0 ... ncluster - 1"); return 1; }
    for (int j = 0; j < nph; ++j) if (ph_cluster[j] < -1 || ph_cluster[j] >= ncluster) { pc_abi_set_last_error("pchip_update_factors: a phantom row's cluster is -1 (no phantom) or 0 ... ncluster - 1"); return 1; }
    pchip_settings c;
    pchip_settings_default(&c, s->nDims, 0);
    c.nlive = nlive; c.nprior = nlive; c.batch = 1; c.num_repeats = 1; c.do_clustering = 0; c.seed = 1; c.device = s->device; c.ablate = s->ablate;
    pchip_like like; pchip_prior prior;
    door_builtin_problem(like, prior);
    return with_engine(c, like, prior, [&](Engine &E) {
        PcState &S = E.S;
        const int nT = S.nT, D = S.D, DD = D * D;
        HIPCHK(hipStreamSynchronize(E.st));                      // (the set-up's own launch writes the per-cluster arrays and the control block)
        if (ncluster > S.maxc) E.grow_clusters(ncluster);
        if (nph > S.Pcap) E.grow_phantoms(nph);
        std::vector<double> rows((size_t)nlive * nT, 0.0);
        for (int i = 0; i < nlive; ++i) std::memcpy(rows.data() + (size_t)i * nT, live + (size_t)i * D, sizeof(double) * D);
        HIPCHK(hipMemcpy(S.live, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(S.live_cluster, live_cluster, sizeof(int) * nlive, hipMemcpyHostToDevice));
        door_install_phantoms(E, nph, phantom, ph_logL, ph_cluster, false);
        std::vector<unsigned> cuid(ncluster);
        for (int k = 0; k < ncluster; ++k) cuid[k] = (unsigned)k;
        HIPCHK(hipMemcpy(S.cl_uid, cuid.data(), sizeof(unsigned) * ncluster, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(S.death_thr, threshold, sizeof(double) * ncluster, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(&S.ctl->ncluster, &ncluster, sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(&S.ctl->nphantom, &nph, sizeof(int), hipMemcpyHostToDevice));
        E.h_ctl->ncluster = ncluster; E.h_ctl->nphantom = nph;
        if (path == 1) {
            S.pool = (s->ablate & PC_ABL_NO_POOL) ? 0 : 1;
            const size_t need = (size_t)pc_update_fused_blocks(&S, nph) * pc_update_fused_entries(&S);
            E.upd_part_cap = need; E.upd_part = E.blocks.dev<double>(need);
            E.upd_shift = E.blocks.dev<double>(D);
            std::vector<double> sh(D, 0.5);
            if (shift) sh.assign(shift, shift + D);
            HIPCHK(hipMemcpy(E.upd_shift, sh.data(), sizeof(double) * D, hipMemcpyHostToDevice));
            pc_launch_update_fused(&S, nph, E.keep, E.blk, E.d_total, E.ph2, E.phL2, E.phC2, E.phU2, E.upd_part, E.upd_shift, 0, E.st);
            HIPCHK(hipStreamSynchronize(E.st));
            HIPCHK(hipGetLastError());
            // the rows that were counted: the count entries of the groups' records (k_upd_fold), whole numbers in doubles
            const int G = pc_update_fused_grid(&S, nph, 0), ng = (G + 15) / 16, Ee = pc_update_fused_entries(&S), npair = D * (D + 1) / 2;
            std::vector<double> rec((size_t)ng * Ee);
            HIPCHK(hipMemcpy(rec.data(), E.upd_part + (size_t)G * Ee, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
            double n = 0.0;
            for (int g = 0; g < ng; ++g) n += rec[(size_t)g * Ee + npair + D];
            count[0] = (int)n;
            if (shift_out) HIPCHK(hipMemcpy(shift_out, E.upd_shift, sizeof(double) * D, hipMemcpyDeviceToHost));
        } else {
            S.pool = 0;
            pc_launch_clean(&S, nph, E.keep, E.blk, E.d_total, E.ph2, E.phL2, E.phC2, E.phU2, nullptr, E.st);
            int total = nph;
            if (ncluster > 1) { HIPCHK(hipMemcpyAsync(&total, E.d_total, sizeof(int), hipMemcpyDeviceToHost, E.st)); HIPCHK(hipStreamSynchronize(E.st)); }
            std::swap(S.phantom, E.ph2); std::swap(S.ph_logL, E.phL2); std::swap(S.ph_cuid, E.phC2); std::swap(S.ph_uid, E.phU2);
            pc_launch_reset_thresholds(&S, E.st);
            E.covmats(total, ncluster);
            HIPCHK(hipStreamSynchronize(E.st));
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy(count, E.count, sizeof(int) * ncluster, hipMemcpyDeviceToHost));
            if (shift_out) for (int d = 0; d < D; ++d) shift_out[d] = shift ? shift[d] : 0.5;      // (the steps take no shift)
        }
        HIPCHK(hipMemcpy(cov, S.cov, sizeof(double) * (size_t)ncluster * DD, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(chol, S.chol, sizeof(double) * (size_t)ncluster * DD, hipMemcpyDeviceToHost));
        if (chol_suspect) HIPCHK(hipMemcpy(chol_suspect, &S.ctl->chol_suspect, sizeof(int), hipMemcpyDeviceToHost));
        return 0;
    });
}

// kernel-level entry for the tests of the clustering kernels (tests/test_clustering_kernels.py): a given point set with its clusters, list
// positions and phantoms, installed as a run holds them at the start of an update; then the update's clustering as Engine::do_update makes
// it -- no hooks, no resume file, nothing launched that a run does not launch.
//   path 0: ClusterUpdate::do_clustering by the one-run launchers (with sub-dimensions: the sub pass, then the full pass).
//   path 1: the launchers of the runs in step, without fibers: the first pass of all sets in one pc_launch_knn_cluster_batch_many, every
//           level of all sets' recursions in one pc_launch_knn_cluster_sub_many -- the records made by rec_clus1 / rec_clusg, laid down and
//           folded by the cohort's own code (Cohort::lay, Cohort::folds_of) and launched through its table of stages; the host side is
//           first_pass_descriptors and PartRefiner.  One pass per set (a set with sub-dimensions: the sub pass), no add_cluster.
// The first pass's scratch of its first cluster leaves through ClusterTap (pc_split.h) where the caller asks for it.
int pchip_cluster_update(const pchip_settings *s, int nsets, const pchip_cluster_in *in, pchip_cluster_out *out, int path)
{
    if (!s || !in || !out || nsets < 1) { pc_abi_set_last_error("pchip_cluster_update: settings, point sets and results for nsets >= 1 sets"); return 1; }
    for (int r = 0; r < nsets; ++r) {
        const pchip_cluster_in &I = in[r]; const pchip_cluster_out &O = out[r];
        if (s[r].nDims < 1 || I.ncluster < 1 || I.nlive < 1 || !I.live || !I.live_logL || !I.live_cluster || I.nph < 0 || (I.nph > 0 && (!I.phantom || !I.ph_logL || !I.ph_cluster))) {
            pc_abi_set_last_error("pchip_cluster_update: nDims >= 1, ncluster >= 1, nlive >= 1 slots with coordinates, logL and cluster, nph >= 0 rows with coordinates, logL and cluster");
            return 1;
        }
        if (O.maxc < I.ncluster || O.nsplit_cap < 0 || !O.live_cluster || !O.live_pos || !O.cl_list || !O.cl_n || !O.imin_slot || !O.ph_count || !O.cl_uid || !O.logLp || !O.lse_ref ||
            !O.lse_sum || !O.logXp || !O.logZp || !O.logZXp || !O.logZp2 || !O.logZpXp || !O.XpXq || (I.nph > 0 && !O.ph_cluster) ||
            (O.nsplit_cap > 0 && (!O.split_child || !O.split_parent || !O.split_logfrac)) || !O.init) {
            pc_abi_set_last_error("pchip_cluster_update: every array of the result but the scratch is needed, with room for maxc >= ncluster clusters");
            return 1;
        }
        const int nscr = (O.scratch_Sm != nullptr) + (O.scratch_knn != nullptr) + (O.scratch_lab != nullptr);
        if ((nscr != 0 && nscr != 3) || (nscr == 3 && O.scratch_cap < 1)) { pc_abi_set_last_error("pchip_cluster_update: the scratch is asked for with all three arrays and scratch_cap >= 1, or not at all"); return 1; }
        for (int i = 0; i < I.nlive; ++i) if (I.live_cluster[i] < -1 || I.live_cluster[i] >= I.ncluster) { pc_abi_set_last_error("pchip_cluster_update: a live slot's cluster is -1 (dead) or 0 ... ncluster - 1"); return 1; }
        for (int j = 0; j < I.nph; ++j) if (I.ph_cluster[j] < -1 || I.ph_cluster[j] >= I.ncluster) { pc_abi_set_last_error("pchip_cluster_update: a phantom row's cluster is -1 (no phantom) or 0 ... ncluster - 1"); return 1; }
        if (s[r].nDims > 256) return 3;
    }
    if (path == 1) return cluster_door_many(s, nsets, in, out);
    if (path != 0 || nsets != 1) return PCHIP_NO_SUCH_PATH;
    const pchip_cluster_in &I = in[0]; pchip_cluster_out &O = out[0];
    const int nc0 = I.ncluster, nlive = I.nlive, nph = I.nph;
    pchip_like like; pchip_prior prior;
    door_builtin_problem(like, prior);
    return with_engine(cluster_door_settings(*s, nlive), like, prior, [&](Engine &E) {
        std::vector<int> cn;
        cluster_door_install(E, I, O.init, cn);
        const int Ncap = E.S.Ncap;
        // the update's clustering, as Engine::do_update makes it
        ClusterTap tap{O.scratch_Sm, O.scratch_knn, O.scratch_lab, O.scratch_cap, 0};
        ClusterTap *tp = O.scratch_Sm ? &tap : nullptr;
        if (E.sub_dims.empty()) E.clus.do_clustering(cn, nullptr, 0, nullptr, tp);
        else {
            std::vector<int> map1, map2;
            bool found = E.clus.do_clustering(cn, E.c_subdims, (int)E.sub_dims.size(), &map1, tp);
            if (found) cn.clear();
            found = E.clus.do_clustering(cn, nullptr, 0, &map2) || found;
            cluster_map_compose(map1, map2);
            if (found && !E.cfg.epoch_discard) E.clus.remap_nursery(map1, nc0);
        }
        HIPCHK(hipStreamSynchronize(E.st));
        HIPCHK(hipGetLastError());
        // the state after it (E.S: a split may have moved the per-cluster arrays)
        const int nc = E.h_ctl->ncluster, mc = E.S.maxc, nsp = (int)E.split_child.size();
        O.ncluster = nc; O.nsplit = nsp; O.levels = (int)E.clus.levels; O.scratch_n = tap.n;
        if (nc > O.maxc || nsp > O.nsplit_cap) engine_fail(PC_RC_LIMIT, "pchip_cluster_update: %d clusters and %d genealogy entries after the update, the caller's arrays hold %d and %d", nc, nsp, O.maxc, O.nsplit_cap);
        auto down = [&](auto *dst, const auto *src, size_t n) { if (n) HIPCHK(hipMemcpy(dst, src, sizeof(*dst) * n, hipMemcpyDeviceToHost)); };
        down(O.live_cluster, E.S.live_cluster, (size_t)nlive); down(O.live_pos, E.S.live_pos, (size_t)nlive);
        down(O.cl_n, E.S.cl_n, (size_t)nc); down(O.imin_slot, E.S.imin_slot, (size_t)nc); down(O.cl_uid, E.S.cl_uid, (size_t)nc);
        down(O.logLp, E.S.logLp, (size_t)nc); down(O.lse_ref, E.S.lse_ref, (size_t)nc); down(O.lse_sum, E.S.lse_sum, (size_t)nc);
        down(O.logXp, E.S.logXp, (size_t)nc); down(O.logZp, E.S.logZp, (size_t)nc); down(O.logZXp, E.S.logZXp, (size_t)nc);
        down(O.logZp2, E.S.logZp2, (size_t)nc); down(O.logZpXp, E.S.logZpXp, (size_t)nc);
        for (int a = 0; a < nc; ++a) down(O.XpXq + (size_t)a * O.maxc, E.S.XpXq + (size_t)a * mc, (size_t)nc);
        for (int k = 0, at = 0; k < nc; ++k) {
            if (O.cl_n[k] < 0 || at + O.cl_n[k] > nlive) engine_fail(PC_RC_DEVICE, "pchip_cluster_update: the clusters' sizes after the update do not add up to the live slots");
            down(O.cl_list + at, E.S.cl_list + (size_t)k * Ncap, (size_t)O.cl_n[k]); at += O.cl_n[k];
        }
        for (int k = 0; k < nc; ++k) O.ph_count[k] = -1;
        if (E.nsplits > 0) down(O.ph_count, E.clus.c_cnt, (size_t)nc);
        if (nph > 0) {
            std::vector<unsigned> cu(nph);
            down(cu.data(), E.S.ph_cuid, (size_t)nph);
            for (int j = 0; j < nph; ++j) {
                O.ph_cluster[j] = -1;
                for (int k = 0; k < nc; ++k) if (cu[j] == O.cl_uid[k]) O.ph_cluster[j] = k;
            }
        }
        for (int k = 0; k < nsp; ++k) { O.split_child[k] = E.split_child[k]; O.split_parent[k] = E.split_parent[k]; O.split_logfrac[k] = E.split_logfrac[k]; }
        return 0;
    });
}

}  // extern "C"
