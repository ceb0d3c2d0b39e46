// pc_cohort.h -- the runs of a device in step: what each run would launch in a phase of the round, written down and launched ONCE for all.
//
// Included by pc_engine.hip alone (and by tools/dev/cohort_record.hip, which stands recorders in for everything below and compares the
// launches with those of the commit before this header existed: tests/test_cohort_record.py).  The including file provides, before the
// include: pc_state.h and pc_launch.h; the HIP stream, event and copy calls, and HIPCHK around them; and these services:
//   template <class T> T *halloc(size_t) / void hfree(void *)      pinned host blocks
//   template <class T> T *dalloc(size_t) / void dfree(T *&)        device blocks
//   hpool().get_sync_event() / hpool().put_sync_event(hipEvent_t)  events to wait on
//   pc_copy_many(const std::vector<std::array<uintptr_t, 3>> &, hipStream_t)      {dst, src, bytes} copies in one kernel
// It does not see Engine.
//
// A stage of the runs in step is three things, and a new one is added by adding the three:
//   its names       the slots of Rec::p / Rec::ia it uses (PC_REC_* next to PcManyRec in pc_state.h: the _many kernels read them by the same
//                   names) and of Rec::a (PC_REC_A_* below: host only)
//   a constructor   rec_<stage>(...) below: named parameters in, a record out; no caller names a slot
//   a row           of Cohort::stage()'s table, at its place in the launch order (= the order of the CK_* enumerators): the one-run launch, the launch
//                   for a group of runs, and the integers of the group's records the latter wants folded into one
#pragma once
#include <vector>
#include <array>
#include <functional>
#include <algorithm>
#include <cstring>
#include <cstdint>

enum { CK_COMPACT = 0, CK_RESET, CK_CLUS1, CK_CLUSG, CK_BASES, CK_NHATS_G, CK_SLICE, CK_SLICE_G, CK_TICK, CK_BASES_NEXT, CK_SORT, CK_NN, CK_CONSUME, CK_CONSUME_CL, CK_APPLY, CK_UPDATE, CK_FINAL, CK_N };      // (in the order they are launched)
// (_G: any device likelihood, the wavefront-per-chain kernels of a run on its own with the run in the grid; TICK: the device batch callback, one tick of
//  the chains that wait for an answer -- several a nursery, each in a flush of its own (pc_step.h); NN / CONSUME_CL: runs with several clusters)

// Rec::a, what the runs of one launch must share: the chains of the nursery (directions, sampling, apply) and whether k_slice makes seeds +
// whitening itself (CK_SLICE_G); the fused update's grid and its deferred flag; more than 64 clusters (CK_CONSUME_CL)
enum { PC_REC_A_NCHAINS = 0, PC_REC_A_FUSED = 1 };
enum { PC_REC_A_GRID = 0, PC_REC_A_DEFERRED = 1 };
enum { PC_REC_A_WIDE = 0 };

struct Cohort {
    hipStream_t st = nullptr;
    hipStream_t st2 = nullptr;          // the bases of the NEXT nursery, next to this one's sampling and contraction
    hipEvent_t ev_up = nullptr, ev_next = nullptr; bool next_pending = false;
    // bases drawn TWO nurseries ahead: a sampling launch waits for the launch that drew ITS bases (numbered), not for the second stream's
    // latest -- with one event for the latest, sixteen runs' k_slice_t waited 140 us per round without an update for the 250 us of
    // deviates + bases launched a round before
    hipEvent_t ev_seq[4] = {nullptr, nullptr, nullptr, nullptr}; unsigned long long seq_launched = 0, seq_waited = 0; bool seq_open = false;
    int seq_for_next() const { return (int)(seq_launched + 1); }      // (the number the bases written down now will be launched under)
    // a: what the runs of one launch must share; p, ia: each run's own (PcManyRec); note: host only, where flush() tells the run what became of a
    // sampling record (null: nobody asks)
    struct Note { long shared = 0; int failed = 0; };      // shared: sampling records launched once for several runs; failed: ... that no launcher took
    struct Rec { int kind; PcState S; void *p[10]; long long a[4]; int ia[6]; Note *note; };
    // a row of the table of stages.  `one`: the launch for one run (what a run on its own makes at this point, where Engine::stage is used);
    // `many`: for cnt runs whose records start at d, f the first of them, fold[t] the fold of ia[folds[t].slot] over them; both return the
    // launcher's code (0: launched)
    enum { FOLD_END = 0, FOLD_MAX, FOLD_ANY /* 1 if the slot is > 0 in any record */ };
    struct Stage {
        int kind; const char *name;
        int (*one)(const Rec &r, hipStream_t st);
        int (*many)(const Rec &f, const PcManyRec *d, int cnt, const int *fold, hipStream_t st);
        struct { int slot, how; } folds[3];
    };
    static const Stage &stage(int kind);
    static constexpr bool stages_in_order(const Stage (&rows)[CK_N]) { for (int k = 0; k < CK_N; ++k) if (rows[k].kind != k || !rows[k].one || !rows[k].many) return false; return true; }
    std::vector<Rec> pend;
    static constexpr int RING = 4;
    PcManyRec *h_stage[RING] = {}, *d_recs[RING] = {};
    // a slot's records are read by the kernels launched from it: its events are recorded behind the LAST of them, on both streams
    hipEvent_t ev[RING] = {}, ev2[RING] = {}; bool ev_used[RING] = {}, ev2_used[RING] = {};
    size_t cap = 0; int ring = 0;
    void slot_wait(int k)
    {
        if (ev_used[k]) { HIPCHK(hipEventSynchronize(ev[k])); ev_used[k] = false; }
        if (ev2_used[k]) { HIPCHK(hipEventSynchronize(ev2[k])); ev2_used[k] = false; }
    }
    // the bases of this nursery were drawn on the second stream: whatever reads them on the main stream comes behind them
    void wait_next() { if (next_pending) { HIPCHK(hipStreamWaitEvent(st, ev_next, 0)); next_pending = false; } }
    long n_fused = 0, n_single = 0;
    // the runs' copies to the host (dead rows, results) share two streams of the cohort, on hardware queues other than the two its
    // kernels use: a copy stream per run came from the pool, on whatever queue -- and where copies are shader blits (the HIP runtime
    // PyTorch ships: 48 us each) a round's kernels queued behind them
    hipStream_t stc[2] = {nullptr, nullptr}; int n_stc = 0;
    // copies to the host that belong behind what has been written down: made at the end of flush(), in the order they were asked for
    std::vector<std::function<void()>> post;
    // ... and copies to the device that what is written down reads: made at the start of flush()
    std::vector<std::function<void()>> pre;
    void rec(const Rec &r) { pend.push_back(r); }
    // a record as the _many kernels read it; and what a stage's launch for the records [first, last) wants folded of their integers
    // (flush below, and the kernel-level door pchip_cluster_update, which launches the clustering stages for given point sets)
    static void lay(PcManyRec &d, const Rec &r) { d.S = r.S; std::memcpy(d.p, r.p, sizeof(r.p)); std::memcpy(d.ia, r.ia, sizeof(r.ia)); }
    static void folds_of(const Stage &row, const Rec *const *first, const Rec *const *last, int fold[3])
    {
        fold[0] = fold[1] = fold[2] = 0;
        for (int t = 0; t < 3 && row.folds[t].how != FOLD_END; ++t)
            for (const Rec *const *x = first; x != last; ++x) {
                const int v = (*x)->ia[row.folds[t].slot];
                fold[t] = row.folds[t].how == FOLD_MAX ? std::max(fold[t], v) : (fold[t] | (v > 0));
            }
    }
    // ... the copies among them as (destination, source, bytes): one kernel for all of them (k_copy_batch), not a hipMemcpyAsync each
    std::vector<std::array<uintptr_t, 3>> post_copies, pre_copies;
    // everything written down and asked for is forgotten, nothing of it launched (the flush it waited for will not come)
    void drop_pending() { pre.clear(); post.clear(); pend.clear(); pre_copies.clear(); post_copies.clear(); }
    void run_post()
    {
        if (!post_copies.empty()) { std::vector<std::array<uintptr_t, 3>> c; c.swap(post_copies); pc_copy_many(c, st); }
        if (post.empty()) return;
        std::vector<std::function<void()>> p; p.swap(post); for (auto &f : p) f();
    }
    void run_pre()
    {
        if (!pre_copies.empty()) { std::vector<std::array<uintptr_t, 3>> c; c.swap(pre_copies); pc_copy_many(c, st); }
        if (pre.empty()) return;
        std::vector<std::function<void()>> p; p.swap(pre); for (auto &f : p) f();
    }
    void flush()
    {
        run_pre();
        if (pend.empty()) { run_post(); return; }
        const size_t n = pend.size();
        if (n > cap) {
            for (int k = 0; k < RING; ++k) {
                slot_wait(k);      // (kernels of earlier flushes may still be reading the old records, on either stream)
                // (from the block caches and the event pool: asking the driver -- and giving back to it at the end -- was 2 ms per call)
                if (h_stage[k]) hfree(h_stage[k]);
                if (d_recs[k]) dfree(d_recs[k]);
                h_stage[k] = halloc<PcManyRec>(2 * n);
                d_recs[k] = dalloc<PcManyRec>(2 * n);
                if (!ev[k]) ev[k] = hpool().get_sync_event();
                if (!ev2[k] && st2) ev2[k] = hpool().get_sync_event();
            }
            cap = 2 * n;
        }
        const int slot = ring++ % RING;
        slot_wait(slot);
        PcManyRec *hs = h_stage[slot], *dr = d_recs[slot];
        // records in launch order: by kind, and inside a kind by the arguments all runs of a launch must share
        std::vector<const Rec *> ord; ord.reserve(n);
        for (const Rec &r : pend) ord.push_back(&r);
        auto shape_less = [](const Rec *x, const Rec *y) {
            if (x->kind != y->kind) return x->kind < y->kind;
            const int c = std::memcmp(x->a, y->a, sizeof(x->a));
            if (c != 0) return c < 0;
            if (x->S.Ncap != y->S.Ncap) return x->S.Ncap < y->S.Ncap;
            if (x->S.B != y->S.B) return x->S.B < y->S.B;
            if (x->S.pool != y->S.pool) return x->S.pool < y->S.pool;
            if ((x->S.prior.lo == nullptr) != (y->S.prior.lo == nullptr)) return (x->S.prior.lo == nullptr) < (y->S.prior.lo == nullptr);
            // (one launch, one kernel: the runs share the likelihood's kind, its source handle and the prior's kind -- those of one call always do)
            if (x->S.like.kind != y->S.like.kind) return x->S.like.kind < y->S.like.kind;
            if (x->S.src_id != y->S.src_id) return x->S.src_id < y->S.src_id;
            return x->S.prior.kind < y->S.prior.kind;
        };
        std::stable_sort(ord.begin(), ord.end(), shape_less);
        for (size_t i = 0; i < n; ++i) lay(hs[i], *ord[i]);
        HIPCHK(hipMemcpyAsync(dr, hs, sizeof(PcManyRec) * n, hipMemcpyHostToDevice, st));
        bool up_marked = false, used_st2 = false;
        for (size_t i = 0; i < n;) {
            size_t j = i + 1;
            while (j < n && !shape_less(ord[i], ord[j]) && !shape_less(ord[j], ord[i])) ++j;
            const Rec &f = *ord[i];
            const int cnt = (int)(j - i), k = f.kind;
            const Stage &row = stage(k);
            hipStream_t q = st;
            if (k == CK_BASES_NEXT && st2) {         // on the second stream, behind the upload of the records
                if (!up_marked) { HIPCHK(hipEventRecord(ev_up, st)); up_marked = true; }
                HIPCHK(hipStreamWaitEvent(st2, ev_up, 0));
                q = st2; used_st2 = true;
            }
            if (k == CK_SLICE || k == CK_SLICE_G) {             // (its bases were drawn over there)
                int need = 0; bool numbered = st2 != nullptr;
                for (size_t x = i; x < j; ++x) { numbered = numbered && ord[x]->ia[PC_REC_I_BASES_SEQ] > 0; need = std::max(need, ord[x]->ia[PC_REC_I_BASES_SEQ]); }
                if (numbered && (unsigned long long)need <= seq_launched) {
                    if ((unsigned long long)need > seq_waited) { HIPCHK(hipStreamWaitEvent(st, ev_seq[need & 3], 0)); seq_waited = (unsigned long long)need; }
                } else wait_next();
            }
            int fold[3];
            folds_of(row, ord.data() + i, ord.data() + j, fold);
            if (row.many(f, dr + i, cnt, fold, q) == 0) {
                n_fused += cnt;
                if (cnt > 1) for (size_t x = i; x < j; ++x) if (ord[x]->note) ord[x]->note->shared++;
            }
            else for (size_t x = i; x < j; ++x) { if (row.one(*ord[x], q) != 0 && ord[x]->note) ord[x]->note->failed = 1; n_single++; }
            if (k == CK_BASES_NEXT && st2) {
                HIPCHK(hipEventRecord(ev_next, st2)); next_pending = true;
                if (!seq_open) { seq_launched++; seq_open = true; }
                if (!ev_seq[seq_launched & 3]) ev_seq[seq_launched & 3] = hpool().get_sync_event();
                HIPCHK(hipEventRecord(ev_seq[seq_launched & 3], st2));
            }
            i = j;
        }
        HIPCHK(hipEventRecord(ev[slot], st)); ev_used[slot] = true;
        if (used_st2 && ev2[slot]) { HIPCHK(hipEventRecord(ev2[slot], st2)); ev2_used[slot] = true; }
        pend.clear();
        seq_open = false;
        run_post();
    }
    void destroy()
    {
        for (int k = 0; k < 4; ++k) if (ev_seq[k]) { hpool().put_sync_event(ev_seq[k]); ev_seq[k] = nullptr; }
        for (int k = 0; k < RING; ++k) {
            if (ev_used[k]) (void)hipEventSynchronize(ev[k]);
            if (ev2_used[k]) (void)hipEventSynchronize(ev2[k]);
            if (ev[k]) hpool().put_sync_event(ev[k]);
            if (ev2[k]) hpool().put_sync_event(ev2[k]);
            ev2[k] = nullptr; ev2_used[k] = false;
            if (h_stage[k]) hfree(h_stage[k]);
            if (d_recs[k]) dfree(d_recs[k]);
            ev[k] = nullptr; h_stage[k] = nullptr; d_recs[k] = nullptr; ev_used[k] = false;
        }
        cap = 0;
    }
};

// ---- the constructors: one per stage (the two clean / update stages and the sampling stages share theirs where the slots are the same)
inline Cohort::Rec rec_of(int kind, const PcState &S)
{
    Cohort::Rec r;
    r.kind = kind; r.S = S;
    for (void *&x : r.p) x = nullptr;
    for (long long &x : r.a) x = 0;
    for (int &x : r.ia) x = 0;
    r.note = nullptr;
    return r;
}
// the phantom clean (an update by steps, the compaction of the pool) over the nph rows in use
inline Cohort::Rec rec_compact(const PcState &S, unsigned char *keep, int *blk, int *total, double *ph2, double *phL2, unsigned *phC2, unsigned long long *phU2, int nph)
{
    Cohort::Rec r = rec_of(CK_COMPACT, S);
    r.p[PC_REC_KEEP] = keep; r.p[PC_REC_BLK] = blk; r.p[PC_REC_TOTAL] = total; r.p[PC_REC_PH2] = ph2; r.p[PC_REC_PHL2] = phL2; r.p[PC_REC_PHC2] = phC2; r.p[PC_REC_PHU2] = phU2;
    r.ia[PC_REC_I_ROWS] = nph; r.ia[PC_REC_I_BLOCKS] = (nph + 255) / 256;
    return r;
}
// the fused update of one cluster; grid: pc_update_fused_grid for (nph, deferred), which the runs of a launch share (a run on its own: not read)
inline Cohort::Rec rec_update(const PcState &S, unsigned char *keep, int *blk, int *total, double *ph2, double *phL2, unsigned *phC2, unsigned long long *phU2,
                              double *part, double *shift, int grid, bool deferred, int nph)
{
    Cohort::Rec r = rec_compact(S, keep, blk, total, ph2, phL2, phC2, phU2, nph);
    r.kind = CK_UPDATE;
    r.p[PC_REC_PART] = part; r.p[PC_REC_SHIFT] = shift;
    r.a[PC_REC_A_GRID] = grid; r.a[PC_REC_A_DEFERRED] = deferred ? 1 : 0;
    return r;
}
inline Cohort::Rec rec_reset(const PcState &S) { return rec_of(CK_RESET, S); }
// the first clustering pass over nd whole clusters, the largest of nmax points; dims / nd_sub: the sub-dimension pass's coordinates (0: the full space)
inline Cohort::Rec rec_clus1(const PcState &S, int *desc, double *Sm, int *knn, int *lab, int *out, const int *dims, int nd, int nmax, int nd_sub)
{
    Cohort::Rec r = rec_of(CK_CLUS1, S);
    r.p[PC_REC_DESC] = desc; r.p[PC_REC_SM] = Sm; r.p[PC_REC_KNN] = knn; r.p[PC_REC_LAB] = lab; r.p[PC_REC_OUT] = out; r.p[PC_REC_DIMS] = (void *)dims;
    r.ia[PC_REC_I_ND] = nd; r.ia[PC_REC_I_NMAX] = nmax; r.ia[PC_REC_I_ND_SUB] = nd_sub;
    return r;
}
// one level of the recursion over nb parts of clusters, the largest of mmax points
inline Cohort::Rec rec_clusg(const PcState &S, int *desc, double *Sm, int *pool, int *knn, int *lab, int *out, int nb, int mmax)
{
    Cohort::Rec r = rec_of(CK_CLUSG, S);
    r.p[PC_REC_G_DESC] = desc; r.p[PC_REC_G_SM] = Sm; r.p[PC_REC_G_POOL] = pool; r.p[PC_REC_G_KNN] = knn; r.p[PC_REC_G_LAB] = lab; r.p[PC_REC_G_OUT] = out;
    r.ia[PC_REC_I_NB] = nb; r.ia[PC_REC_I_MMAX] = mmax;
    return r;
}
// what a nursery's launches share: its number and its chains (kind: CK_BASES, CK_BASES_NEXT, CK_NHATS_G, CK_APPLY)
inline Cohort::Rec rec_nursery(int kind, const PcState &S, unsigned batch, int nchains)
{
    Cohort::Rec r = rec_of(kind, S);
    r.ia[PC_REC_I_BATCH] = (int)batch; r.a[PC_REC_A_NCHAINS] = nchains;
    return r;
}
inline Cohort::Rec rec_bases(const PcState &S, unsigned batch, int nchains) { return rec_nursery(CK_BASES, S, batch, nchains); }
inline Cohort::Rec rec_bases_next(const PcState &S, unsigned batch, int nchains) { return rec_nursery(CK_BASES_NEXT, S, batch, nchains); }
inline Cohort::Rec rec_nhats_g(const PcState &S, unsigned batch, int nchains) { return rec_nursery(CK_NHATS_G, S, batch, nchains); }
inline Cohort::Rec rec_apply(const PcState &S, unsigned batch, int nchains) { return rec_nursery(CK_APPLY, S, batch, nchains); }
// the sampling; bases_seq: the number of the launch that drew the nursery's bases on the second stream (0: drawn in line)
inline Cohort::Rec rec_slice(const PcState &S, unsigned batch, int nchains, int bases_seq)
{
    Cohort::Rec r = rec_nursery(CK_SLICE, S, batch, nchains);
    r.ia[PC_REC_I_BASES_SEQ] = bases_seq;
    return r;
}
inline Cohort::Rec rec_slice_g(const PcState &S, unsigned batch, int nchains, bool fused, int bases_seq, Cohort::Note *note = nullptr)
{
    Cohort::Rec r = rec_nursery(CK_SLICE_G, S, batch, nchains);
    r.a[PC_REC_A_FUSED] = fused ? 1 : 0; r.ia[PC_REC_I_BASES_SEQ] = bases_seq;
    r.note = note;
    return r;
}
// one tick of a nursery through the device batch callback: the chains' records, start points, decks and parked proposals, the answers of the
// last call (the group's one block) and the ranks of the last pack (rows of that block); first: the nursery's first tick
inline Cohort::Rec rec_tick(const PcState &S, unsigned batch, int nchains, void *cs, double *x0s, int *decks, double *prop, const double *ev_logL,
                            const double *ev_theta, const double *ev_phi, const int *rank, bool first)
{
    Cohort::Rec r = rec_nursery(CK_TICK, S, batch, nchains);
    r.p[PC_REC_T_CS] = cs; r.p[PC_REC_T_X0] = x0s; r.p[PC_REC_T_DECK] = decks; r.p[PC_REC_T_PROP] = prop;
    r.p[PC_REC_T_LOGL] = (void *)ev_logL; r.p[PC_REC_T_THETA] = (void *)ev_theta; r.p[PC_REC_T_PHI] = (void *)ev_phi; r.p[PC_REC_T_RANK] = (void *)rank;
    r.ia[PC_REC_I_FIRST] = first ? 1 : 0;
    return r;
}
inline Cohort::Rec rec_sort(const PcState &S) { return rec_of(CK_SORT, S); }
inline Cohort::Rec rec_nn(const PcState &S, int nursery_left)
{
    Cohort::Rec r = rec_of(CK_NN, S);
    r.ia[PC_REC_I_NLEFT] = nursery_left;
    return r;
}
inline Cohort::Rec rec_consume(const PcState &S) { return rec_of(CK_CONSUME, S); }
inline Cohort::Rec rec_consume_cl(const PcState &S, bool wide)
{
    Cohort::Rec r = rec_of(CK_CONSUME_CL, S);
    r.a[PC_REC_A_WIDE] = wide ? 1 : 0;
    return r;
}
inline Cohort::Rec rec_final(const PcState &S) { return rec_of(CK_FINAL, S); }

// ---- the table of stages, in launch order
#define PC_ONE [](const Cohort::Rec &r, hipStream_t st) -> int
#define PC_MANY [](const Cohort::Rec &f, const PcManyRec *d, int cnt, const int *fold, hipStream_t st) -> int
inline const Cohort::Stage &Cohort::stage(int kind)
{
    static constexpr Stage rows[CK_N] = {
        { CK_COMPACT, "compact",
          PC_ONE { pc_launch_clean(&r.S, r.ia[PC_REC_I_ROWS], (unsigned char *)r.p[PC_REC_KEEP], (int *)r.p[PC_REC_BLK], (int *)r.p[PC_REC_TOTAL], (double *)r.p[PC_REC_PH2],
                                   (double *)r.p[PC_REC_PHL2], (unsigned *)r.p[PC_REC_PHC2], (unsigned long long *)r.p[PC_REC_PHU2], nullptr, st); return 0; },
          PC_MANY { return pc_launch_clean_many(d, cnt, fold[0], st); },
          { { PC_REC_I_BLOCKS, FOLD_MAX } } },
        { CK_RESET, "reset",
          PC_ONE { pc_launch_reset_thresholds(&r.S, st); return 0; },
          PC_MANY { return pc_launch_reset_thresholds_many(&f.S, d, cnt, st); }, {} },
        { CK_CLUS1, "clus1",
          PC_ONE { return pc_launch_knn_cluster_batch_dev(&r.S, (const int *)r.p[PC_REC_DESC], r.ia[PC_REC_I_ND], r.ia[PC_REC_I_NMAX], (double *)r.p[PC_REC_SM], (int *)r.p[PC_REC_KNN],
                                                          (int *)r.p[PC_REC_LAB], (int *)r.p[PC_REC_OUT], (const int *)r.p[PC_REC_DIMS], r.ia[PC_REC_I_ND_SUB], st); },
          PC_MANY { return pc_launch_knn_cluster_batch_many(&f.S, d, cnt, fold[0], fold[1], fold[2], st); },
          { { PC_REC_I_ND, FOLD_MAX }, { PC_REC_I_NMAX, FOLD_MAX }, { PC_REC_I_ND_SUB, FOLD_ANY } } },
        { CK_CLUSG, "clusg",
          PC_ONE { return pc_launch_knn_cluster_sub((const int *)r.p[PC_REC_G_DESC], r.ia[PC_REC_I_NB], r.ia[PC_REC_I_MMAX], (const double *)r.p[PC_REC_G_SM], (const int *)r.p[PC_REC_G_POOL],
                                                    (int *)r.p[PC_REC_G_KNN], (int *)r.p[PC_REC_G_LAB], (int *)r.p[PC_REC_G_OUT], st); },
          PC_MANY { return pc_launch_knn_cluster_sub_many(d, cnt, fold[0], fold[1], st); },
          { { PC_REC_I_NB, FOLD_MAX }, { PC_REC_I_MMAX, FOLD_MAX } } },
        { CK_BASES, "bases",
          PC_ONE { return pc_launch_nhats_part(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], 1, st, 1); },
          PC_MANY { return pc_launch_bases_t_many(&f.S, d, cnt, 0u, (int)f.a[PC_REC_A_NCHAINS], st); }, {} },
        { CK_NHATS_G, "nhats_g",
          PC_ONE { return pc_launch_nhats(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], st); },
          PC_MANY { return pc_launch_nhats_many(&f.S, d, cnt, (int)f.a[PC_REC_A_NCHAINS], st); }, {} },
        { CK_SLICE, "slice",
          PC_ONE { return pc_launch_slice_t(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], st); },
          PC_MANY { return pc_launch_slice_t_many(&f.S, d, cnt, 0u, (int)f.a[PC_REC_A_NCHAINS], st); }, {} },
        { CK_SLICE_G, "slice_g",
          PC_ONE { return r.a[PC_REC_A_FUSED] ? pc_launch_slice_fused(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], st)
                                              : pc_launch_slice(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], st); },
          // (the user's own problem -- a device prior, a source likelihood --: the launcher with the prior kind in its variants and the terms form's LDS)
          PC_MANY { return (f.S.prior.kind >= 2 || f.S.like.kind == PC_LIKE_SOURCE)
                               ? pc_launch_slice_step(&f.S, d, cnt, (int)f.a[PC_REC_A_NCHAINS], (int)f.a[PC_REC_A_FUSED], st)
                               : pc_launch_slice_many(&f.S, d, cnt, (int)f.a[PC_REC_A_NCHAINS], (int)f.a[PC_REC_A_FUSED], st); }, {} },
        { CK_TICK, "tick",
          PC_ONE { pc_launch_slice_tick_dev(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], r.p[PC_REC_T_CS], (double *)r.p[PC_REC_T_X0], (int *)r.p[PC_REC_T_DECK],
                                            (double *)r.p[PC_REC_T_PROP], (const double *)r.p[PC_REC_T_LOGL], (const double *)r.p[PC_REC_T_THETA], (const double *)r.p[PC_REC_T_PHI],
                                            r.ia[PC_REC_I_FIRST], (const int *)r.p[PC_REC_T_RANK], st); return 0; },
          PC_MANY { return pc_launch_slice_tick_many(d, cnt, (int)f.a[PC_REC_A_NCHAINS], st); }, {} },
        { CK_BASES_NEXT, "bases_next",
          PC_ONE { return pc_launch_nhats_part(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], 1, st, 1); },
          PC_MANY { return pc_launch_bases_t_many(&f.S, d, cnt, 0u, (int)f.a[PC_REC_A_NCHAINS], st); }, {} },
        { CK_SORT, "sort",
          PC_ONE { return pc_launch_sort_live(&r.S, st); },
          PC_MANY { return pc_launch_sort_live_many(&f.S, d, cnt, st); }, {} },
        { CK_NN, "nn",      // (the run's CK_SORT of this round has been launched: kinds go in order)
          PC_ONE { pc_launch_nn_lists(&r.S, r.ia[PC_REC_I_NLEFT], 1, st); return 0; },
          PC_MANY { return pc_launch_nn_lists_many(&f.S, d, cnt, fold[0], 1, st); },
          { { PC_REC_I_NLEFT, FOLD_MAX } } },
        { CK_CONSUME, "consume",
          PC_ONE { return pc_launch_consume_par(&r.S, st); },
          PC_MANY { return pc_launch_consume_par_many(&f.S, d, cnt, st); }, {} },
        { CK_CONSUME_CL, "consume_cl",
          PC_ONE { return pc_launch_consume_cl(&r.S, r.a[PC_REC_A_WIDE] ? 65 : 2, st); },
          PC_MANY { return pc_launch_consume_cl_many(&f.S, d, cnt, (int)f.a[PC_REC_A_WIDE], st); }, {} },
        { CK_APPLY, "apply",
          PC_ONE { pc_launch_apply(&r.S, (unsigned)r.ia[PC_REC_I_BATCH], (int)r.a[PC_REC_A_NCHAINS], st); return 0; },
          PC_MANY { return pc_launch_apply_many(&f.S, d, cnt, 0u, (int)f.a[PC_REC_A_NCHAINS], st); }, {} },
        { CK_UPDATE, "update",
          PC_ONE { pc_launch_update_fused(&r.S, r.ia[PC_REC_I_ROWS], (unsigned char *)r.p[PC_REC_KEEP], (int *)r.p[PC_REC_BLK], (int *)r.p[PC_REC_TOTAL], (double *)r.p[PC_REC_PH2],
                                          (double *)r.p[PC_REC_PHL2], (unsigned *)r.p[PC_REC_PHC2], (unsigned long long *)r.p[PC_REC_PHU2], (double *)r.p[PC_REC_PART],
                                          (double *)r.p[PC_REC_SHIFT], (int)r.a[PC_REC_A_DEFERRED], st); return 0; },
          PC_MANY { return pc_launch_update_fused_many(&f.S, d, cnt, fold[0], (int)f.a[PC_REC_A_GRID], (int)f.a[PC_REC_A_DEFERRED], st); },
          { { PC_REC_I_BLOCKS, FOLD_MAX } } },
        { CK_FINAL, "final",
          PC_ONE { return pc_launch_final_par(&r.S, st); },
          PC_MANY { return pc_launch_final_par_many(d, cnt, st); }, {} },
    };
    static_assert(stages_in_order(rows), "a row of the table is not at its kind's place");
    return rows[kind];
}
#undef PC_ONE
#undef PC_MANY
