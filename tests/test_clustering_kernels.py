"""The clustering kernels of an update alone (pc_cluster.hip, with the host's recursion and bookkeeping in pc_split.h), through the
kernel-level door pchip_cluster_update: ties, duplicates, tile edges, LDS above 64 KB, batches of clusters, sub-dimensions, the
per-cluster statistics and the phantoms' new homes.

REFERENCES, in this order of authority:
 1. the Fortran's own answer, tests/golden/ref_clustering.json: calculate_similarity_matrix, NN_clustering and (sets of at most 64 points)
    compute_knn with k = min(n, 20) of the reference, called by oracle/ref_clustering.f90 on the point sets of point_sets() below; the
    fixture keeps a checksum of every set's coordinates, so a drifting generator fails here (oracle/gen_golden.py clustering);
 2. a restatement written out below (Restated): neighbour order a stable sort by (distance, index); the n = 2 .. k0 loop with its trip count
    fixed at entry; components of "i's first entry in j's n-list, or j's in i's"; relabel by first appearance; exit on one cluster or on
    unchanged labels; then the recursion of clustering.f90:80-95, literally.  On lattice sets it works on exact integer squared distances;
 3. the oracle's pc_similarity and pc_nn_clustering (oracle/pc_oracle.c).

POINT SETS.  Lattice sets have coordinates k / 1024, 0 <= k < 1024: every product and sum of the similarity is exact in fp64 in any order,
with or without FMA, so the Fortran's matmul, the oracle and the kernel give the same bits and ties are exact ties.  Continuous sets
(rng.random) are compared bit for bit with the oracle only (both sum un-fused in dimension order); against the Fortran their labels only,
under the SEPARATION condition asserted for every such set: among each point's first 20 neighbours no two distances lie within 1e-12
relative of each other, which makes the neighbour order independent of the order of summation.

BOUNDS.  Integers, similarities, minima and maxima are compared exactly.  Two figures take a bound:
  lse_sum      against long double within (n + 3 + max|l - ref|) u relative: gamma_{n-1} of the positive sum, one rounding of the difference
               scaled by its size, and 2 ulp for exp.  The 2 ulp are the one figure here that is not derived: ROCm documents 1 ulp for exp
               in double precision; the second is allowance.
  sum of exp(logXp) over the children of a split == exp(logXp) of the parent: within 4u relative in the batch case, the figure set for it;
               elsewhere within the bound Update.split derives from the operations (eight children of four points each miss 4u by 2u:
               the logarithms' own roundings, which the reference has as well).
The volumes themselves (logXp = parent + split_logfrac) are restated operation for operation with the host's libm and compared exactly.

FOUND.  FUSED: the similarity bodies of pc_cluster.hip formed their products and sums with __dmul_rn / __dadd_rn "kept un-fused in dimension
order"; in the HIP headers those are a plain * and +, and the compiler contracted them (three v_fmac_f64 in k_similarity_b's ISA).  Against
the oracle's pc_similarity, before the fix, on the continuous sets: seam1_255 25 948 of 65 025 entries differ, at most 7.3e-13 relative;
seam1_1023 442 584 of 1 046 529, 8.3e-12; seam2_1025 377 722 of 1 050 625, 2.3e-11; seam2_2049 1 484 894 of 4 198 401, 4.3e-10 (the sum
cancels for near points).  No row's neighbour order and no label changed on these sets; on live points 1e-5 apart it can.  The lattice
sets could not see it (every operation is exact there).  Fixed in the bodies with #pragma clang fp contract(off): v_mul_f64 + v_add_f64
now, and the blocks are the oracle's bit for bit.
UNREACHABLE: no split makes a part of one or two points (test_depth_sets_reach_what_they_are_named_after says why), so the singleton branch
of PartRefiner::split_by and a launch with m = 2 are not reached by any set here, the "blobs of 1 and 2 points" included.
NOT REACHED: k_remap_chains (the door's nursery is empty) and k_ph_rehome_r<12 ... 28>.

GPU TIME.  Every GPU case is one door call (the sets in step: one call by path 1 and one by path 0 per set).  Measured on an MI355X: the 69
GPU cases of this file take 3.6 s together, the slowest 0.74 s (5500 points, of which the oracle's clustering on the host is about 0.5 s).
"""
import ctypes as C
import hashlib
import json
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_clustering.json")
LATT = 1024
U = 2.0 ** -53
KNN_MAX_N, FORTRAN_MAX_N = 64, 2100


# ---- the point sets -----------------------------------------------------------------------------------------------------------------------

def _cells(rng, n, lo, hi, D=2):
    """n distinct lattice points with integer coordinates in [lo, hi)^D"""
    w = hi - lo
    pick = rng.choice(w ** D, size=n, replace=False)
    return np.stack([(pick // w ** d) % w + lo for d in range(D)], axis=1).astype(np.int64)


def _lat(k):
    return np.ascontiguousarray(np.asarray(k, dtype=np.int64) / float(LATT))


def _blob1(n, seed):
    return _lat(_cells(np.random.default_rng(seed), n, 448, 576))


def _blob2(n, seed):
    rng = np.random.default_rng(seed)
    a = (n + 1) // 2
    return _lat(np.concatenate([_cells(rng, a, 0, 64), _cells(rng, n - a, 900, 964)]))


def _grid(*shape, step=16, drop_cols=(), seed=0):
    """a regular grid with its rows in a fixed random order: which of a point's equally near neighbours comes first is the index's decision
    (in natural order either tie-break chains the whole grid at nn = 2, and a wrong one would not show in the partition)"""
    ax = [np.arange(m) for m in shape]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, len(shape))
    g = g[~np.isin(g[:, 0], drop_cols)]
    return _lat(g[np.random.default_rng(seed).permutation(len(g))] * step + 100)


def _dup_blobs():
    rng = np.random.default_rng(11)
    a, b = _cells(rng, 9, 100, 140), _cells(rng, 8, 800, 840)
    base = np.concatenate([a, b])
    return _lat(np.concatenate([base, base[[2, 5, 11, 16]], base[[5]]]))      # copies at the end; base[5] three times in all


def _chain():
    """groups of 2, 3, ..., 11 collinear points one lattice step apart; the gap behind the group of g points is 12 + g steps: at nn = g + 1
    the group of g reaches the group behind it, so every pass nn = 2 .. 10 of the first level changes the labels"""
    xs, at = [], 8
    for g in range(2, 12):
        xs += list(range(at, at + g))
        at += g - 1 + 12 + g
    k = np.zeros((len(xs), 2), dtype=np.int64)
    k[:, 0] = xs; k[:, 1] = 512
    return _lat(k)


def _nested(sizes):
    """2 x 2 x 2 nested blobs along a line in 2-D: offsets 512, 128, 32 lattice steps; the blobs' points a step apart, sizes[b] of them"""
    pts = []
    for b in range(8):
        x0 = 8 + 512 * (b >> 2) + 128 * ((b >> 1) & 1) + 32 * (b & 1)
        pts += [(x0 + (i & 1), 300 + (i >> 1)) for i in range(sizes[b])]
    return _lat(pts)


def _two_blobs_cont(n, seed, D=3):
    rng = np.random.default_rng(seed)
    a = n // 3
    x = rng.random((n, D))
    x[:a] = 0.2 * x[:a]
    x[a:] = 0.7 + 0.3 * x[a:]
    return np.ascontiguousarray(x)


def _one_blob_cont(n, seed, D=3):
    return np.ascontiguousarray(0.25 + 0.5 * np.random.default_rng(seed).random((n, D)))


SEAMS = (255, 256, 257, 1023, 1024, 1025, 2049)
SMALL = (3, 4, 9, 10, 11, 19, 20, 21)
SEAM_SEED2 = {255: 1, 256: 2, 257: 3, 1023: 4, 1024: 5, 1025: 6, 2049: 7}
SEAM_SEED1 = {255: 21, 256: 22, 257: 23, 1023: 24, 1024: 25, 1025: 26, 2049: 27}


def _batch_parts():
    """the clusters of the batch case: sizes 1, 2, 3, 40 (three far groups), 2, 300 (a jittered grid), 64 (two far groups)"""
    rng = np.random.default_rng(5)
    c40 = np.concatenate([_cells(rng, 13, 0, 24), _cells(rng, 13, 480, 504), _cells(rng, 14, 960, 984)])[rng.permutation(40)]
    g = np.stack(np.meshgrid(np.arange(20), np.arange(15), indexing="ij"), axis=-1).reshape(-1, 2) * 12 + 300
    c300 = g + rng.integers(0, 3, size=g.shape)
    c64 = np.concatenate([_cells(rng, 30, 40, 72), _cells(rng, 34, 900, 932)])[rng.permutation(64)]
    return [_lat(_cells(rng, 1, 200, 210)), _lat(_cells(rng, 2, 700, 720)), _lat(_cells(rng, 3, 600, 640)), _lat(c40), _lat(_cells(rng, 2, 10, 900)),
            _lat(c300), _lat(c64)]


def _subdim_sets():
    """D = 6, sub-dimensions (4, 1) in that order.  A: two groups far apart on coordinates 4 and 1 that a third, wide coordinate smears in the
    full space; B: one blob on (4, 1), two groups far apart on coordinate 0"""
    rng = np.random.default_rng(9)
    n = 24
    a = np.zeros((n, 6), dtype=np.int64)
    a[:, [0, 2, 3, 5]] = rng.integers(0, 1024, size=(n, 4))
    grp = np.arange(n) % 2
    sub = np.concatenate([_cells(rng, n // 2, 100, 116), _cells(rng, n // 2, 300, 316)])
    a[grp == 0, 4], a[grp == 0, 1] = sub[:n // 2, 0], sub[:n // 2, 1]
    a[grp == 1, 4], a[grp == 1, 1] = sub[n // 2:, 0], sub[n // 2:, 1]
    b = np.zeros((n, 6), dtype=np.int64)
    sb = _cells(rng, n, 500, 520)
    b[:, 4], b[:, 1] = sb[:, 0], sb[:, 1]
    b[:, [2, 3, 5]] = rng.integers(500, 516, size=(n, 3))
    b[:, 0] = np.where(grp == 0, rng.integers(0, 16, size=n), rng.integers(1000, 1016, size=n))
    return _lat(a), _lat(b), grp


def _subdim_dups():
    """distinct in D = 4, coinciding pairwise on the sub-dimensions (0, 2)"""
    rng = np.random.default_rng(13)
    half = _cells(rng, 7, 100, 600, D=4)
    twin = half.copy()
    twin[:, [1, 3]] = _cells(rng, 7, 100, 600)
    return _lat(np.concatenate([half, twin]))


def point_sets():
    """name -> coordinates [n][D] of every set the Fortran is asked about (oracle/gen_golden.py) -- from fixed seeds"""
    sets = {}
    for n in SMALL:
        sets[f"blob1_{n}"] = _blob1(n, 100 + n)
        sets[f"blob2_{n}"] = _blob2(n, 200 + n)
    sets["tie_grid6x6"] = _grid(6, 6, seed=61)
    sets["tie_grid12x5_gap"] = _grid(12, 5, drop_cols=(5, 6, 7), seed=62)
    sets["tie_grid4x4x4"] = _grid(4, 4, 4, seed=63)
    sets["dup_all5"] = _lat(np.tile([[300, 700]], (5, 1)))
    sets["dup_blobs"] = _dup_blobs()
    rng = np.random.default_rng(12)
    tr = _cells(rng, 7, 200, 260)
    sets["dup_triple"] = _lat(np.concatenate([tr, tr[[3]], tr[[3]]]))
    sets["dup_first0"] = _lat(np.concatenate([tr, tr[[0]]]))
    for k in ("dup_all5", "dup_blobs", "dup_triple", "dup_first0"):
        sets[k + "_rev"] = np.ascontiguousarray(sets[k][::-1])
    sd = _subdim_dups()
    sets["dup_subdims_proj"] = np.ascontiguousarray(sd[:, [0, 2]])
    sets["chain_2_to_11"] = _chain()
    sets["nested_4"] = _nested([4] * 8)
    sets["nested_1_2"] = _nested([1, 2, 2, 1, 4, 2, 1, 3])
    sets["nested_deep"] = _nested([3, 5, 4, 5, 3, 4, 3, 2])
    for n in SEAMS:
        sets[f"seam2_{n}"] = _two_blobs_cont(n, SEAM_SEED2[n])
        sets[f"seam1_{n}"] = _one_blob_cont(n, SEAM_SEED1[n])
    for k, x in enumerate(_batch_parts()):
        if x.shape[0] > 2:
            sets[f"batch_c{k}"] = x
    a, b, grp = _subdim_sets()
    sets["subdim_a_proj"] = np.ascontiguousarray(a[:, [4, 1]])
    sets["subdim_a_full_g0"], sets["subdim_a_full_g1"] = np.ascontiguousarray(a[grp == 0]), np.ascontiguousarray(a[grp == 1])
    sets["subdim_b_proj"] = np.ascontiguousarray(b[:, [4, 1]])
    sets["subdim_b_full"] = b
    return sets


def is_lattice(x):
    k = x * LATT
    return bool(np.all(k == np.round(k)) and np.all(k >= 0) and np.all(k < LATT))


def checksum(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype="<f8").tobytes()).hexdigest()[:16]


def lds_blobs():
    """n = 5500, D = 2, two far blobs (continuous): dynamic LDS above 64 KB in the sort and in the clustering kernel; the oracle alone"""
    return _two_blobs_cont(5500, 31, D=2)


# ---- reference 2: the restatement -----------------------------------------------------------------------------------------------------------

def similarity_int(x):
    """lattice sets: S * 1024^2 as exact integers"""
    k = np.round(x * LATT).astype(np.int64)
    d = k[:, None, :] - k[None, :, :]
    return np.einsum("abd,abd->ab", d, d)


def similarity_fp(x):
    """r_a + r_b - 2 x_a.x_b with un-fused products and sums in dimension order (calculate.f90:94-109 as the engine and the oracle sum it)"""
    n, D = x.shape
    r = np.zeros(n)
    s = np.zeros((n, n))
    for d in range(D):
        r = r + x[:, d] * x[:, d]
        s = s + x[:, d][:, None] * x[:, d][None, :]
    return (r[:, None] + r[None, :]) - 2.0 * s


def neighbour_order(S, spoiled=False):
    """all n neighbours of every point by (distance, index): compute_knn's insertion rule (clustering.f90:156-172).  spoiled: ties by the HIGHER index"""
    if spoiled:
        n = S.shape[0]
        return (n - 1 - np.argsort(S[:, ::-1], axis=1, kind="stable")).astype(np.int64)
    return np.argsort(S, axis=1, kind="stable").astype(np.int64)


def _relabel(lab):
    """utils.F90:713-749: 1, 2, ... in order of first appearance"""
    seen, out = {}, np.empty(len(lab), dtype=np.int64)
    for i, v in enumerate(lab):
        out[i] = seen.setdefault(int(v), len(seen) + 1)
    return out, len(seen)


def _components(knn, nn):
    """do_clustering_k + neighbours() (clustering.f90:100-130, :178-188): i and j are joined when i's first entry is among j's first nn, or j's
    among i's -- plain union-find, the label a component's smallest member"""
    n = knn.shape[0]
    first = knn[:, 0]
    by_first = {}
    for i in range(n):
        by_first.setdefault(int(first[i]), []).append(i)
    par = list(range(n))

    def find(a):
        while par[a] != a:
            par[a] = par[par[a]]
            a = par[a]
        return a
    for j in range(n):
        for t in knn[j, :nn]:
            for i in by_first.get(int(t), ()):
                a, b = find(i), find(j)
                if a != b:
                    par[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


class Restated:
    """NN_clustering (clustering.f90:15-97) of a similarity matrix.  labels, num: the answer; first: the first level's labels; passes: the nn the
    first level ran; why: how it ended ('one', 'same', 'trip'); levels: levels of the recursion below the first in which a part of more than one
    point is clustered again -- what PartRefiner launches (pc_split.h); part_sizes: the sizes of the parts every split made, at any level"""

    def __init__(self, S, spoiled=False):
        n = S.shape[0]
        self.passes, self.why, self.levels, self.part_sizes = [], "trip", 0, []
        if n <= 1:
            self.labels, self.num, self.first, self.why = np.ones(n, dtype=np.int64), 1, np.ones(n, dtype=np.int64), "one"
            return
        knn = neighbour_order(S, spoiled)
        k = min(n, 10)
        old = np.arange(1, n + 1)
        lab, num = old.copy(), n
        for nn in range(2, k + 1):                     # (the trip count is fixed at entry: k may double inside, the loop does not go on)
            self.passes.append(nn)
            lab, num = _relabel(_components(knn, nn))
            if num == 1:
                self.why = "one"
                break
            if np.array_equal(lab, old):
                self.why = "same"
                break
            old = lab
        self.first = lab.copy()
        if num > 1:
            self.part_sizes = [int(v) for v in np.bincount(lab)[1:]]
            ic, deepest, any_open = 1, 0, False
            while ic <= num:
                pts = np.flatnonzero(lab == ic)
                sub = Restated(S[np.ix_(pts, pts)], spoiled)
                if len(pts) > 1:
                    any_open, deepest = True, max(deepest, sub.levels)
                self.part_sizes += sub.part_sizes
                lab[pts] = num + sub.labels
                if sub.num == 1:
                    ic += 1
                lab, num = _relabel(lab)
            self.levels = 1 + deepest if any_open else 0
        self.labels, self.num = lab, num


def separation(S, k=20):
    """the smallest relative gap between two neighbouring distances among each point's first k neighbours (the point itself left out)"""
    d = np.sort(S, axis=1)[:, 1:k + 1]
    gap = np.diff(d, axis=1) / np.maximum(np.abs(d[:, 1:]), 1e-300)
    return float(gap.min()) if gap.size else float("inf")


# ---- references 1 and 3, and what the tests share ------------------------------------------------------------------------------------------

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def fixture():
    return cached("fixture", lambda: json.load(open(FIXTURE)))


def sets():
    return cached("sets", point_sets)


def oracle_cluster(x):
    """reference 3: (similarity matrix, labels, number of clusters) of the oracle"""
    from tests import oracle_api as orc
    lib = orc.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, D = x.shape
    S = np.zeros((n, n))
    lib.pc_similarity(orc.dptr(x), n, D, D, orc.dptr(S))
    lab = np.zeros(n, dtype=np.int32)
    num = lib.pc_nn_clustering(orc.dptr(S), n, lab.ctypes.data_as(C.POINTER(C.c_int)))
    return S, lab.astype(np.int64), int(num)


def restated(x, spoiled=False):
    """reference 2 on a point set: on exact integers where the set is a lattice set"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return Restated(similarity_int(x) if is_lattice(x) else similarity_fp(x), spoiled)


def reference(name):
    """(Restated, oracle's (S, labels, num)) of a named set, made once"""
    return cached(("ref", name), lambda: (restated(sets()[name]), oracle_cluster(sets()[name])))


def lds_reference():
    def make():
        x = lds_blobs()
        S, lab, num = oracle_cluster(x)
        return x, separation(S), lab, num
    return cached("lds", make)


ALL_SETS = sorted(point_sets().keys())


# ---- the reference's bookkeeping, restated (do_clustering, clustering.f90:253-324; add_cluster, run_time_info.f90:303-505) -------------------

def _logsumexp(v):
    mx = max(v)
    return mx + math.log(sum(math.exp(a - mx) for a in v))


class Update:
    """The state of an update as the reference keeps it: the clusters' slots in list order, ids, volumes and evidences, the phantoms' clusters.
    split(ic, labels, num) is add_cluster: the split cluster leaves, those behind it move up, its parts go to the end in label order, position =
    rank in list order; every phantom that is still there goes to the cluster of its nearest live point, the first in (cluster, position) order
    among equals, and stays only above that cluster's contour; volumes and evidences are shared out by live points + phantoms, with the
    operations of the reference in their order (Python's floats and math are the host's doubles and libm)."""

    def __init__(self, live, logL, cluster, ncluster, init, XQ0, phantom=None, ph_logL=None, ph_cluster=None):
        self.x = np.round(np.asarray(live) * LATT).astype(np.int64) if is_lattice(np.asarray(live)) else None
        self.logL = np.asarray(logL, dtype=np.float64)
        self.cl = [[int(s) for s in np.flatnonzero(np.asarray(cluster) == c)] for c in range(ncluster)]
        self.uid = list(range(ncluster)); self.next_uid = ncluster
        self.val = [list(map(float, init[k])) for k in range(5)]          # logXp, logZp, logZXp, logZp2, logZpXp
        self.XQ = [list(map(float, row)) for row in XQ0]
        self.splits = []                                                   # (child uid, parent uid, logfrac)
        self.ph = None if phantom is None or len(phantom) == 0 else np.round(np.asarray(phantom) * LATT).astype(np.int64)
        self.ph_logL = None if self.ph is None else np.asarray(ph_logL, dtype=np.float64)
        self.ph_cl = None if self.ph is None else [int(c) for c in ph_cluster]
        self.nsplit_calls, self.vol_bound = 0, {}

    def contour(self, c):
        return min(self.logL[s] for s in self.cl[c]) if self.cl[c] else None

    def split(self, ic, labels, num):
        self.nsplit_calls += 1
        nc, nold = len(self.cl), len(self.cl) - 1
        parent = self.cl.pop(ic); puid = self.uid.pop(ic)
        new = [[] for _ in range(num)]
        for a, s in enumerate(parent):
            new[int(labels[a]) - 1].append(s)
        assert all(new)
        self.cl.extend(new)
        par = [v.pop(ic) for v in self.val]
        rowpq = [self.XQ[ic][q] for q in range(nc) if q != ic]; Xp2 = self.XQ[ic][ic]
        self.XQ = [[self.XQ[a][b] for b in range(nc) if b != ic] for a in range(nc) if a != ic]
        kids = list(range(self.next_uid, self.next_uid + num)); self.next_uid += num
        self.uid.extend(kids)
        # the phantoms: cluster numbers follow the list; then each goes to its nearest live point's cluster
        if self.ph is not None:
            pts, keys = [], []
            for c, lst in enumerate(self.cl):
                for p, s in enumerate(lst):
                    pts.append(self.x[s]); keys.append((c, p))
            pts = np.array(pts)
            for j in range(len(self.ph_cl)):
                if self.ph_cl[j] < 0:
                    continue
                d2 = ((pts - self.ph[j]) ** 2).sum(axis=1)
                c = min(keys[i] for i in np.flatnonzero(d2 == d2.min()))[0]
                self.ph_cl[j] = c if self.ph_logL[j] > self.contour(c) else -1
        nph = [0] * len(self.cl)
        for c in (self.ph_cl or ()):
            if c >= 0:
                nph[c] += 1
        # the evidence split (run_time_info.f90:458-503)
        ni = [float(len(self.cl[nold + k]) + nph[nold + k]) for k in range(num)]
        logni = [math.log(v + 0.0) for v in ni]; logni1 = [math.log(v + 1.0) for v in ni]
        logn = _logsumexp(logni)
        logn1 = logn + math.log(math.exp(0.0 - logn) + 1.0) if logn > 0.0 else 0.0 + math.log(math.exp(logn - 0.0) + 1.0)
        Xp, Zp, ZXp, Zp2, ZpXp = par
        # how far the children's volumes may be from adding up to the parent's, relative, in units of u: a child's logXp = (Xp + log n_k) - logn
        # carries 2 |log n_k| (the logarithm, 1 ulp), the error of logn = mx + log(sum exp(log n_k - mx)) -- num + 3 for the sum of
        # exponentials, whose logarithm is taken of a number in [1, num], 2 |logn - mx| for that logarithm, |logn| for the addition -- and one
        # rounding of either addition; its exponential carries that absolute error as a relative one.  The 5 are the exponentials the
        # test itself takes (1 ulp each, both sides) and the rounding of its sum.
        self.vol_bound[puid] = 5 + max(2 * abs(logni[k]) + num + 3 + 2 * abs(logn - max(logni)) + abs(logn) + abs(Xp + logni[k]) + abs(Xp + logni[k] - logn)
                                       for k in range(num))
        for k in range(num):
            self.splits.append((kids[k], puid, logni[k] - logn))
            self.val[0].append(Xp + logni[k] - logn); self.val[1].append(Zp + logni[k] - logn); self.val[2].append(ZXp + logni[k] - logn)
            self.val[3].append(Zp2 + logni[k] + logni1[k] - logn - logn1); self.val[4].append(ZpXp + logni[k] + logni1[k] - logn - logn1)
        for row in self.XQ:
            row.extend([0.0] * num)
        for k in range(num):
            self.XQ.append([0.0] * (nold + num))
        for k in range(num):
            for q in range(nold):
                self.XQ[nold + k][q] = rowpq[q] + logni[k] - logn; self.XQ[q][nold + k] = self.XQ[nold + k][q]
        for a in range(num):
            for b in range(num):
                self.XQ[nold + a][nold + b] = (Xp2 + logni[a] + logni1[a] - logn - logn1) if a == b else (Xp2 + logni[a] + logni[b] - logn - logn1)
        self.ph_count = nph

    def do_clustering(self, label_fn):
        """one pass over the clusters there are (do_clustering): label_fn(slots in list order) -> (labels, num) for clusters of more than two points"""
        nold, ic = len(self.cl), 0
        todo = [label_fn(list(c)) if len(c) > 2 else (None, 1) for c in self.cl]
        for j in range(nold):
            if todo[j][1] > 1:
                self.split(ic, *todo[j])
            else:
                ic += 1


def labels_by_restatement(live, dims=None):
    live = np.asarray(live)

    def fn(slots):
        x = live[slots] if dims is None else live[np.ix_(slots, list(dims))]
        r = restated(x)
        return r.labels, r.num
    return fn


def check_state(g, want, nlive, vol_units=None):
    """the door's state after the update against the restated bookkeeping: integers exactly, and the doubles too.  vol_units: the bound, in
    units of u, on how far the children's volumes are from adding up to their parent's (None: the bound Update.split works out)"""
    nc = len(want.cl)
    assert g["ncluster"] == nc
    lc = np.full(nlive, -1, dtype=np.int64); lp = np.zeros(nlive, dtype=np.int64)
    for c, lst in enumerate(want.cl):
        for p, s in enumerate(lst):
            lc[s], lp[s] = c, p
    live = lc >= 0
    assert np.array_equal(g["live_cluster"], lc)
    assert np.array_equal(np.asarray(g["live_pos"])[live], lp[live])
    assert list(g["cl_n"]) == [len(c) for c in want.cl]
    for c in range(nc):
        assert list(g["cl_list"][c]) == want.cl[c], c
    assert list(g["cl_uid"]) == want.uid and len(set(want.uid)) == nc
    assert g["nsplit"] == len(want.splits)
    assert [(int(a), int(b)) for a, b in zip(g["split_child"], g["split_parent"])] == [(a, b) for a, b, _ in want.splits]
    assert [float(v) for v in g["split_logfrac"]] == [f for _, _, f in want.splits]
    for k, name in enumerate(("logXp", "logZp", "logZXp", "logZp2", "logZpXp")):
        assert [float(v) for v in g[name]] == want.val[k], name
    assert np.array_equal(g["XpXq"], np.array(want.XQ).reshape(nc, nc))
    # every child of a split: logXp = parent + logfrac restated above, exactly; and the children's volumes add up to the parent's
    vol = {u: v for u, v in zip(range(len(g["init"][0])), g["init"][0])}
    for child, parent, _ in want.splits:
        vol[child] = None
    final = dict(zip(want.uid, want.val[0]))
    by_parent = {}
    for child, parent, frac in want.splits:
        by_parent.setdefault(parent, []).append(child)
    for parent, kids in by_parent.items():
        if parent in vol and vol[parent] is not None and all(k in final for k in kids):
            tot = math.fsum(math.exp(final[k]) for k in kids)
            units = want.vol_bound[parent] if vol_units is None else vol_units
            assert abs(tot - math.exp(vol[parent])) <= units * U * math.exp(vol[parent]), (parent, tot, math.exp(vol[parent]), units)


def run_door(x, cluster=None, scratch=True, **kw):
    from polychordlite_amd import _ctypes_api as api
    x = np.asarray(x)
    n = x.shape[0]
    cl = np.zeros(n, dtype=np.int32) if cluster is None else np.asarray(cluster, dtype=np.int32)
    st = dict(live=x, cluster=cl, **kw)
    if scratch:
        first = [c for c in range(int(cl.max()) + 1) if np.count_nonzero(cl == c) > 2]
        st["scratch"] = int(np.count_nonzero(cl == first[0])) if first else 0
    out = api.cluster_update([st], path=0)
    assert out is not None
    return out[0]


def show(case, g, path="path 0: one-run launchers"):
    print(f"\n  {case}: {g['ncluster']} clusters after the update, {g['nsplit']} new, {g['levels']} levels of the recursion, {path}", end="")


# ---- the CPU half ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL_SETS)
def test_references_agree(name):
    """fixture == restatement == oracle on every set; the generator's checksum; exact similarities on lattice sets; separation on the others"""
    x = sets()[name]
    f = fixture()[name]
    assert (f["n"], f["D"]) == x.shape and f["checksum"] == checksum(x), "the generator drifted from the fixture"
    r, (S, olab, onum) = reference(name)
    assert np.array_equal(similarity_fp(x), S)
    if is_lattice(x):
        assert np.array_equal(similarity_int(x) / float(LATT * LATT), S)          # (an integer below 2^53 over a power of two: exact)
    else:
        sep = separation(S)
        assert sep > 1e-12, f"{name}: two of a point's first 20 distances within {sep:.2e} relative: replace the set"
    assert f["ncl"] == r.num == onum
    assert f["labels"] == list(r.labels) == list(olab)
    if x.shape[0] <= KNN_MAX_N:
        k = f["k"]
        assert k == min(x.shape[0], 20)
        fk = np.array(f["knn"]).reshape(x.shape[0], k) - 1
        order = neighbour_order(similarity_int(x) if is_lattice(x) else S)
        assert np.array_equal(fk, order[:, :k])
        from tests import oracle_api as orc
        ok = np.zeros((x.shape[0], k), dtype=np.int32)
        orc.load().pc_compute_knn(orc.dptr(S), x.shape[0], k, ok.ctypes.data_as(C.POINTER(C.c_int)))
        assert np.array_equal(ok, fk)


def test_fixture_is_complete_and_small():
    f = fixture()
    assert sorted(f) == [k for k in ALL_SETS if sets()[k].shape[0] <= FORTRAN_MAX_N] == ALL_SETS
    assert os.path.getsize(FIXTURE) < 100 * 1024
    assert all(("knn" in v) == (v["n"] <= KNN_MAX_N) for v in f.values())


def test_chain_runs_nine_first_level_passes():
    r, _ = reference("chain_2_to_11")
    assert r.passes == list(range(2, 11)) and r.why == "trip" and r.num > 1


def test_depth_sets_reach_what_they_are_named_after():
    assert reference("nested_deep")[0].levels == 3 and reference("nested_4")[0].num == 8
    r = reference("nested_1_2")[0]
    assert r.levels == 2 and r.num == 4
    # Blobs of 1 and 2 points do NOT give parts of 1 or 2 points: at nn >= 2 every point is joined to its nearest neighbour, and a level
    # ends on unchanged labels at nn >= 3 at the earliest, where a component holds at least three points (or on one cluster).  So the
    # singleton branch and the m = 2 launches of PartRefiner::split_by cannot be reached from NN_clustering's own labels, on any set:
    for name in ALL_SETS:
        assert min(reference(name)[0].part_sizes, default=3) >= 3, name


def test_small_sets_take_both_branches_of_k():
    """k = m below 10 and the fixed trip count at 10: some small set must split and some must not, on either side of 10"""
    nums = {n: (reference(f"blob1_{n}")[0].num, reference(f"blob2_{n}")[0].num) for n in SMALL}
    assert any(max(v) > 1 for n, v in nums.items() if n < 10) and any(max(v) > 1 for n, v in nums.items() if n >= 10)
    assert any(min(v) == 1 for v in nums.values())


@pytest.mark.parametrize("name", ["tie_grid6x6", "tie_grid12x5_gap", "tie_grid4x4x4"])
def test_spoiled_tie_break_is_noticed(name):
    """neighbour ties broken by the HIGHER index: the lists leave the Fortran's, in neighbours 2 ... 5, and the partition changes at some nn"""
    x = sets()[name]
    f = fixture()[name]
    S = similarity_int(x)
    good, bad = neighbour_order(S), neighbour_order(S, spoiled=True)
    fk = np.array(f["knn"]).reshape(x.shape[0], f["k"]) - 1
    assert np.array_equal(good[:, :f["k"]], fk) and not np.array_equal(bad[:, 1:5], fk[:, 1:5])
    assert np.array_equal(np.sort(S[np.arange(len(S))[:, None], bad], axis=1), S[np.arange(len(S))[:, None], bad])      # (still sorted by distance)
    differs = [nn for nn in range(2, 11) if not np.array_equal(_relabel(_components(good, nn))[0], _relabel(_components(bad, nn))[0])]
    print(f"\n  {name}: the spoiled order changes the partition at nn = {differs}", end="")
    assert differs


def test_lds_set_meets_the_separation_condition():
    x, sep, lab, num = lds_reference()
    assert sep > 1e-12 and x.shape == (5500, 2)


def test_door_refuses_without_launching():
    """paths that do not exist and bad arguments are answered before a device is looked for"""
    from polychordlite_amd import _ctypes_api as api
    x = sets()["blob1_9"]
    st = dict(live=x, cluster=np.zeros(9, dtype=np.int32))
    assert api.cluster_update([st], path=2) is None and api.cluster_update([st], path=7) is None and api.cluster_update([st, st], path=0) is None
    with pytest.raises(api.ClusterUpdateError) as e:
        api.cluster_update([dict(live=x, cluster=np.full(9, 3, dtype=np.int32), ncluster=2)], path=0)
    assert e.value.code == 1 and "cluster" in str(e.value)


# ---- the GPU half: every case one door call --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_SETS)
def test_gpu_one_cluster(name):
    """a named set as the one cluster of an update: the first pass's similarity block bit for bit, all m neighbours of every row, the first
    level's labels, the parts, the levels launched and the state after the update"""
    x = sets()[name]
    n = x.shape[0]
    r, (S, olab, onum) = reference(name)
    g = run_door(x)
    show(name, g)
    assert g["scratch_n"] == n
    assert np.array_equal(g["Sm"], S)                                      # bit for bit the oracle's (on lattice sets: the integers', test_references_agree)
    order = neighbour_order(similarity_int(x) if is_lattice(x) else S)
    assert np.array_equal(g["knn"], order)
    assert np.array_equal(g["lab"], r.first)
    f = fixture()[name]
    want = Update(x, np.zeros(n), np.zeros(n, dtype=int), 1, g["init"], g["XpXq0"])
    want.do_clustering(lambda slots: (np.array(f["labels"]), f["ncl"]))
    check_state(g, want, n)
    assert g["ncluster"] == f["ncl"] and g["levels"] == r.levels


@pytest.mark.gpu
def test_gpu_lds_above_64k():
    """5500 points: k_knn_sort_b and k_nn_cluster_b (and the _sub kernels on the larger part) with more than 64 KB of dynamic LDS; the oracle alone"""
    x, sep, lab, num = lds_reference()
    g = run_door(x, scratch=False)
    show("lds_5500", g)
    want = Update(x, np.zeros(5500), np.zeros(5500, dtype=int), 1, g["init"], g["XpXq0"])
    want.do_clustering(lambda slots: (lab, num))
    assert num == 2
    check_state(g, want, 5500)


@pytest.mark.gpu
def test_gpu_lds_refusal_launches_nothing():
    """8193 points want 196608 bytes for the sort: the launcher declines, the engine answers with its LDS code (PC_RC_LDS = 4)"""
    from polychordlite_amd import _ctypes_api as api
    x = (np.arange(8193, dtype=np.float64) / 8193.0).reshape(-1, 1)
    with pytest.raises(api.ClusterUpdateError) as e:
        run_door(x, scratch=False)
    assert e.value.code == 4


def batch_case():
    parts = _batch_parts()
    live = np.concatenate(parts)
    cluster = np.concatenate([np.full(len(p), c, dtype=np.int32) for c, p in enumerate(parts)])
    # the clusters' slots interleave; inside a cluster the rows keep their order, which is the list order the fixture's labels are for
    slots = np.random.default_rng(6).permutation(len(live))
    out, ocl, at = np.empty_like(live), np.empty_like(cluster), 0
    for c, p in enumerate(parts):
        mine = np.sort(slots[at:at + len(p)]); at += len(p)
        out[mine], ocl[mine] = p, c
    return np.ascontiguousarray(out), ocl


@pytest.mark.gpu
def test_gpu_batch_of_clusters():
    """seven clusters of 1, 2, 3, 40, 2, 300 and 64 points in one update: descriptors only for those above two points, early exits where
    nmax belongs to another cluster, two splits (five new clusters) and their bookkeeping in the reference's order"""
    live, cluster = batch_case()
    g = run_door(live, cluster)
    show("batch", g)
    want = Update(live, np.zeros(len(live)), cluster, 7, g["init"], g["XpXq0"])
    fx = fixture()
    by_size = {3: "batch_c2", 40: "batch_c3", 300: "batch_c5", 64: "batch_c6"}

    def fn(slots):
        f = fx[by_size[len(slots)]]
        assert f["checksum"] == checksum(live[slots])
        return np.array(f["labels"]), f["ncl"]
    want.do_clustering(fn)
    assert [len(c) for c in want.cl[:5]] == [1, 2, 3, 2, 300] and len(want.cl) == 10 and want.nsplit_calls == 2
    check_state(g, want, len(live), vol_units=4)                          # (the children's volumes within 4u of the parent's: the figure set for this case)
    assert len(set(g["cl_uid"])) == 10 and set(g["cl_uid"][5:]) == {7, 8, 9, 10, 11}
    assert g["scratch_n"] == 3                                              # (the first cluster the pass looks at is the one of three points)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a", "b", "dups"])
def test_gpu_sub_dimensions(which):
    """a: the sub-space (4, 1) separates two groups the full space does not; b: the full pass splits what the sub pass left; dups: points
    distinct in D = 4 that coincide pairwise on (0, 2) -- the duplicate branch inside the sub pass"""
    if which == "dups":
        live, dims = _subdim_dups(), (0, 2)
    else:
        a, b, grp = _subdim_sets()
        live, dims = (a if which == "a" else b), (4, 1)
    n = len(live)
    g = run_door(live, sub_dims=dims)
    show(f"subdim_{which}", g, "path 0: sub pass, then full pass")
    proj = np.ascontiguousarray(live[:, list(dims)])
    S, _, _ = oracle_cluster(proj)
    assert np.array_equal(g["Sm"], S) and np.array_equal(g["knn"], neighbour_order(similarity_int(proj)))      # (the sub-space block)
    want = Update(live, np.zeros(n), np.zeros(n, dtype=int), 1, g["init"], g["XpXq0"])
    want.do_clustering(labels_by_restatement(live, dims))
    after_sub = len(want.cl)
    want.do_clustering(labels_by_restatement(live))
    check_state(g, want, n)
    if which == "a":
        assert after_sub == 2 == len(want.cl) and restated(live).num == 1
    if which == "b":
        assert after_sub == 1 and len(want.cl) == 2
    if which == "dups":
        assert after_sub == fixture()["dup_subdims_proj"]["ncl"] == 2


def stats_case():
    parts = _batch_parts()
    live = np.concatenate([parts[6], parts[5]])
    cluster = np.concatenate([np.zeros(64, dtype=np.int32), np.full(300, 2, dtype=np.int32)])
    rng = np.random.default_rng(8)
    logL = -600.0 * rng.random(364)
    lab = restated(parts[6]).labels
    for part in (1, 2):                                                      # two equal minima in either part of the cluster that splits
        s = np.flatnonzero(lab == part)
        logL[s[5]] = logL[s[2]] = logL[s].min() - 1.0
    logL[64 + 7] = logL[64 + 200] = logL[64:].min() - 0.5                    # ... and in the cluster that stays
    logL[64 + 100] = logL[64 + 250] = 0.25                                   # two equal maxima
    return live, cluster, logL


@pytest.mark.gpu
def test_gpu_cluster_stats():
    """k_cluster_stats after a split: the contour exactly, its slot by list position among equal minima, an empty cluster, the live
    log-sum-exp against long double within (n + 3 + max|l - ref|) u (the 2 ulp for exp in it are not derived, see the file's docstring)"""
    live, cluster, logL = stats_case()
    g = run_door(live, cluster, logL=logL, ncluster=3)
    show("stats", g)
    want = Update(live, logL, cluster, 3, g["init"], g["XpXq0"])
    want.do_clustering(labels_by_restatement(live))
    check_state(g, want, len(live))
    assert [len(c) for c in want.cl] == [0, 300] + [len(c) for c in want.cl[2:]] and len(want.cl) == 4
    for c, lst in enumerate(want.cl):
        if not lst:
            assert g["logLp"][c] == 1.7976931348623157e308 and g["imin_slot"][c] == -1 and g["lse_ref"][c] == 0.0 and g["lse_sum"][c] == 0.0
            continue
        l = logL[lst]
        assert g["logLp"][c] == l.min() and np.count_nonzero(l == l.min()) == 2
        assert g["imin_slot"][c] == lst[int(np.argmin(l))]                   # (argmin: the first in list order)
        assert g["lse_ref"][c] == l.max()
        ld = np.longdouble
        ref = np.sum(np.exp(l.astype(ld) - ld(l.max())))
        bound = (len(l) + 3 + np.abs(l - l.max()).max()) * U
        err = abs(ld(g["lse_sum"][c]) - ref) / ref
        print(f"\n    cluster {c}: n = {len(l)}, lse_sum error {float(err) / U:.2f} u, bound {bound / U:.0f} u", end="")
        assert err <= bound and np.abs(l - l.max()).max() > 500


def phantom_case(D):
    """two chains of 100 points a lattice step apart along coordinate 0 (one cluster that splits in two), a third cluster of five, eight
    dead slots: 213 slots; 130 phantoms: on the bisector of the two parts, near each, at and just above the new contours, some gone before"""
    rng = np.random.default_rng(40 + D)
    k = np.full((213, D), 500, dtype=np.int64)
    x0 = np.concatenate([np.arange(101, 201), np.arange(400, 500), np.arange(900, 905), np.zeros(8, dtype=np.int64)])
    cl = np.concatenate([np.zeros(200, dtype=np.int32), np.ones(5, dtype=np.int32), np.full(8, -1, dtype=np.int32)])
    perm = rng.permutation(213)
    k[:, 0] = x0; k, cl = k[perm], cl[perm]
    logL = -50.0 * rng.random(213)
    ph = np.full((130, D), 500, dtype=np.int64)
    ph[:, 0] = rng.integers(90, 520, size=130)
    ph[:10, 0] = 300                                                       # the bisector of x0 = 200 and x0 = 400
    if D > 1:
        ph[5:10, D - 1] = 503                                              # ... also off the line: still equally far from both
        ph[10:, 1:] += rng.integers(-3, 4, size=(120, D - 1))
    ph[100:110, 0] = rng.integers(880, 930, size=10)
    pc = np.where(np.arange(130) % 3 == 0, 1, 0).astype(np.int32)
    pc[120:] = -1                                                          # gone before the update
    pl = 10.0 * rng.random(130)                                            # above every contour
    lo_a, lo_b = logL[(cl == 0) & (k[:, 0] <= 200)].min(), logL[(cl == 0) & (k[:, 0] >= 400)].min()
    ph[20:24, 0], ph[24:28, 0] = 150, 450
    pl[20:22], pl[22:24] = lo_a, np.nextafter(lo_a, np.inf)                 # at the contour: dropped (strict >); just above: kept
    pl[24:26], pl[26:28] = lo_b, np.nextafter(lo_b, np.inf)
    pl[28:34] = -60.0                                                      # below every contour
    return _lat(k), cl, logL, _lat(ph), pl, pc


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 4, 5, 32, 33, 40])
def test_gpu_phantoms_find_their_homes(D):
    """k_ph_rehome_r<4 | 8 | 32> padded (1, 5) and full (4, 32), k_ph_rehome (33, 40): exact distances on the lattice, ties to the lower
    (cluster, position) key, the strict contour, rows that were gone, a ragged block of phantoms, dead slots, k_ph_count's counts"""
    live, cl, logL, ph, pl, pc = phantom_case(D)
    g = run_door(live, cl, logL=logL, ncluster=2, phantom=ph, ph_logL=pl, ph_cluster=pc)
    show(f"phantoms_D{D}", g, "path 0: one-run launchers, " + ("k_ph_rehome" if D > 32 else f"k_ph_rehome_r<{4 * ((D + 3) // 4)}>"))
    want = Update(live, logL, cl, 2, g["init"], g["XpXq0"], ph, pl, pc)
    want.do_clustering(labels_by_restatement(live))
    assert len(want.cl) == 3 and [len(c) for c in want.cl] == [5, 100, 100]
    check_state(g, want, 213)
    got = list(g["ph_cluster"])
    assert got == want.ph_cl
    assert got[:10] == [1] * 10                                            # the bisector: the part with the lower key
    a = 1 if live[want.cl[1][0], 0] < 0.25 else 2                          # the part of the chain 101 .. 200
    assert got[20:28] == [-1, -1, a, a, -1, -1, 3 - a, 3 - a] and got[28:34] == [-1] * 6 and got[120:] == [-1] * 10
    assert list(g["ph_count"]) == want.ph_count == [got.count(c) for c in range(3)]


def parts_by_cluster(live_cluster_after, cluster, ncluster):
    """path 0's state after the update as path 1 states its answer: a slot's part within its cluster, numbered by first appearance in list
    order, and the parts of each cluster"""
    lab, nums = np.zeros(len(cluster), dtype=np.int64), []
    for c in range(ncluster):
        slots = np.flatnonzero(np.asarray(cluster) == c)
        lab[slots], num = _relabel(np.asarray(live_cluster_after)[slots]) if len(slots) else (0, 1)
        nums.append(max(num, 1))
    return lab, nums


@pytest.mark.gpu
def test_gpu_sets_in_step():
    """path 1: three sets in one call -- the batch of seven clusters, the sub-dimension set (the only one with dims: the mixed branch of
    k_similarity_b_many_sub) and the two blobs of 1025 points; ragged nd_max / nmax / nb_max.  Labels and counts equal path 0's, set for set"""
    from polychordlite_amd import _ctypes_api as api
    live_b, cl_b = batch_case()
    a, _, _ = _subdim_sets()
    x = sets()["seam2_1025"]
    cases = [dict(live=live_b, cluster=cl_b, ncluster=7), dict(live=a, cluster=np.zeros(len(a), dtype=np.int32), sub_dims=(4, 1), scratch=len(a)),
             dict(live=x, cluster=np.zeros(1025, dtype=np.int32), scratch=1025)]
    many = api.cluster_update(cases, path=1)
    assert many is not None and len(many) == 3
    # the mixed launch: the set with dims has the sub-space block, the set without them the full-space one, both bit for bit the oracle's
    assert np.array_equal(many[1]["Sm"], oracle_cluster(np.ascontiguousarray(a[:, [4, 1]]))[0]) and np.array_equal(many[2]["Sm"], reference("seam2_1025")[1][0])
    assert np.array_equal(many[2]["knn"], neighbour_order(reference("seam2_1025")[1][0]))
    for k, (st, g1) in enumerate(zip(cases, many)):
        g0 = api.cluster_update([st], path=0)[0]
        nc = st.get("ncluster", 1)
        lab, nums = parts_by_cluster(g0["live_cluster"], st["cluster"], nc)
        print(f"\n  set {k}: {sum(nums)} parts in {nc} clusters, {g1['levels']} levels of the recursion, path 1: _many launchers (path 0: {g0['levels']} levels)", end="")
        assert list(g1["cl_n"]) == nums and np.array_equal(g1["live_pos"], lab) and np.array_equal(g1["live_cluster"], st["cluster"])
        assert g1["levels"] == g0["levels"] or "sub_dims" in st
    assert [sum(m["cl_n"]) for m in many] == [10, 2, 2]
    # ... and a launch in which no set has dims (k_similarity_b_many): two small sets against the Fortran's labels
    pair = api.cluster_update([dict(live=sets()[k], cluster=np.zeros(len(sets()[k]), dtype=np.int32)) for k in ("blob2_9", "blob2_21")], path=1)
    for k, g in zip(("blob2_9", "blob2_21"), pair):
        assert list(g["live_pos"]) == fixture()[k]["labels"] and list(g["cl_n"]) == [fixture()[k]["ncl"]]
