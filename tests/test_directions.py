"""The directions a slice moves along -- Gaussian deviates, Gram-Schmidt into an orthonormal basis, whitening with the cluster's Cholesky
factor (n^ = L q / |L q|, nhat_w = 3 |L q|) -- against a long double reference, through the kernel-level door pchip_directions, which runs
K0 alone by the launcher a run takes:
  path 0  pc_launch_nhats, the whole kernels: k_nhats<8|16|24> up to 24 dimensions, k_nhats_q<8|16> up to 64, k_nhats_q<32> up to 128
          (two tile buffers up to 112, one beyond), k_nhats_big up to 256;
  path 1  pc_launch_nhats_part(1) then (2), what Engine::enqueue_nursery launches where pc_nhats_splittable holds: k_nhats<., 64, 1|2>,
          k_nhats_q<8|16, 1|2>, and for 64 < nDims <= 128 k_basis<5..8> + k_whiten<5..8> on the fp64 matrix cores;
  path 2  path 1 with the packed bases of pc_slice_t.hip (k_deviates_t + k_bases_packed<8|16|24>), one grade, nDims 2 ... 24.

THE INPUTS come from the oracle (pc_direction_inputs): the deviates generate_nhats draws, in drawing order, and its unshuffled fp64
directions before whitening.  The kernels draw the same deviates from the same Philox stream.

THE REFERENCE is written out here in np.longdouble: per (chain, grade, basis) modified Gram-Schmidt of the fp64 deviates in the reference's
order (random_utils.F90:381-437 as the oracle restates it: normalise, project on the finished vectors one after the other, normalise) gives
Q_ref; kappa = the 2-norm condition number of the basis' row-normalised deviate matrix, all nDims vectors of it also where a truncated
basis uses three.  (With kappa of the three used vectors alone, about 1, kappa u is no scale for them: the rounding of a norm over 255
coordinates is 8 u, the oracle's own e_orth there, and that one number would have been C_ref for every full basis as well.)

THE DEVICE'S OWN BASIS of every variant comes from a run with chol = identity: then t = L q = q exactly, n^ = fl(q fl(1 / w)) and
nhat_w = fl(3 w), so Q_dev = n^ nhat_w / 3 in long double is the device's q to 3 u relative (u = 2^-53).  On paths 1 and 2 the raw basis that
part 1 left in nhat_raw, unpacked by the door, must agree with it to those 3 u; the coordinates in front of a grade must be exactly 0.0.

(a) THE BASIS.  e_orth = max |Q_dev Q_dev^T - I| and e_fwd = max |Q_dev - Q_ref| in long double, no sign fixing, as ratios to kappa u.  The
    constant of "c kappa u" is not derivable (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 19.13: "a modest
    constant"), so it is measured on the reference algorithm, never on the code under test: C_ref = the worst ratio of the ORACLE's fp64
    basis over all cases of this file, one for each quantity, computed in the session on the CPU.  A kernel passes with both ratios
    <= 4 C_ref: two bits for another summation order (four partial sums, DPP sums, matrix-core accumulation), FMA contraction and the panel
    scheme of k_basis / k_nhats_big (modified Gram-Schmidt inside a panel of sixteen, block classical across panels).  A loss of
    orthogonality like kappa^2 u shows as a ratio that grows with kappa: every shape above 64 dimensions runs a second key whose four chains
    hold the worst-conditioned basis among the keys 1 ... 32 (asserted: kappa >= 10 x the median).  And e_orth < 1e-9 outright.
(b) THE WHITENING, separated from (a): the device's own Q_dev and a hard factor -- the Cholesky factor of 0.05^2 R diag(lam) R^T, R random
    orthogonal, lam geometric from 1 to 1e-8 (test_update_factors.cloud's covariance), strict upper triangle exactly 0.0.  In long double
    t = L q, w = |t|, n^ = t / w.  Derived, not tuned (Higham sections 3.1 and 3.5, gamma_k = k u / (1 - k u)):
      |t^ - t|_a <= d_a = gamma_{D+5} (|L| |q|)_a      any order of the sum, any use of FMA; + 5 = the 3 u of Q_dev and the roundings left;
      |w^ - w|   <= b_w = |d|_2 + gamma_{D+2} (w + |d|_2)      the triangle inequality and the norm's own summation;
      |n^_a - t_a / w| <= d_a / (w - b_w) + |t_a| b_w / (w (w - b_w)) + gamma_3 (|t_a| + d_a) / (w - b_w)      (reciprocal, product);
      |nhat_w - 3 w| <= 3 b_w + 3 u (w + b_w).
    Correlated Gaussian, 64 < nDims <= 128 (the run forms nhat_Ms, ch_My): with the device's own n^, span = hi - lo and
    y0 = (lo + (hi - lo) cube) - mean exactly as k_whiten defines them (box (-1, 3): span = 4, both exact in fp64),
      |nhat_Ms - M (span o n^)|_a <= gamma_{D+5} (|M| |span o n^|)_a,      |ch_My - M y0|_a <= gamma_{D+5} (|M| |y0|)_a.
    Every ratio error / bound must be <= 1.
(c) STRUCTURE.  All num_repeats rows of every chain written (the blocks are poisoned under the tests' PC_POISON), finite, of unit norm to
    4 u (test_rows_have_unit_norm_to_4u; NORM below) and to gamma_D / 2 + gamma_3, what any order of the norm's sum keeps
    (test_device_directions); every row is compared with ITS vector of the reference, so a truncated last basis leaves the rows behind it
    to the next grade; two chains, and two keys, give different bases.
(d) THE SAME BITS where the code claims them: the two halves of k_nhats / k_nhats_q are the template of the whole kernel and
    pc_slice_t.hip calls the packed bases "the same bases", so paths 0, 1 and 2 must be np.array_equal up to 64 dimensions (nhat, nhat_w,
    and the raw bases of paths 1 and 2).  Between 65 and 128 path 0 (k_nhats_q<32>) and path 1 (k_basis) are different arithmetic: each
    answers to (a) and (b) on its own.
Paths that do not exist return PCHIP_NO_SUCH_PATH: path 2 with nDims 1, above 24 or with grades; paths 1 and 2 above 128 dimensions and
with two grades above 24.  (Two grades within 24 dimensions -- [12, 8] -- DO split: pc_nhats_splittable asks for one grade only above 24,
and a graded run of that size takes k_nhats<24, 64, 1|2>.  That case runs paths 0 and 1 and holds them to the same bits.)

CASES: four chains, num_repeats = nDims + 3 (two bases, the second truncated to three vectors), two keys.  Which reaches which:
  nDims 1, 2, 8      k_nhats<8> whole and halves (path 1 from 1 on), k_bases_packed<8> (2, 8)
  nDims 9, 16        k_nhats<16>, k_bases_packed<16>                      nDims 17, 24       k_nhats<24>, k_bases_packed<24>
  nDims 25, 32       k_nhats_q<8> whole and halves                        nDims 33, 64       k_nhats_q<16> whole and halves
  path 1: 65, 80 -> k_basis<5> + k_whiten<5>; 81, 96 -> <6>; 97, 112 -> <7>; 113, 127, 128 -> <8> (a ragged and a full last panel each)
  path 0: 65, 112 -> k_nhats_q<32> with two tile buffers; 113, 128 -> with one
  correlated Gaussian 65, 100, 128, paths 0 and 1: the M products of k_nhats_q<32> and of k_whiten<5|7|8>
  nDims 129 (a one-vector last panel), 130, 144 (a full last panel), 255 (the remainder loop of the dot product), 256: k_nhats_big
  two grades [12, 8] k_nhats<24> (paths 0, 1), [30, 10] k_nhats_q<16>, [60, 40] k_nhats_q<32>, [100, 50] k_nhats_big: (a)-(c) within the
  grade's subspace.

THE CPU HALF applies the same reference and bounds to the oracle's fp64 directions and to a plain fp64 L q (the bounds are attainable),
computes and prints C_ref, and holds a deliberately spoiled basis -- classical Gram-Schmidt of all vectors at once -- which must FAIL (a).

SEEN ON AN MI355X (pytest -s prints every case; DESIGN.md section 5d has the table), worst e_orth, e_fwd in kappa u | n^, nhat_w, M.s, M.y as
error / bound | norm in u, with C_ref = 1.70, 0.95 (the oracle at nDims 2; 1.14, 0.65 on full bases from 8 dimensions on):
  k_nhats<8>, halves, k_bases_packed<8> at nDims 2 (kappa <= 25)          4.11  2.11 | 0.095 0.164             | 1.6
  k_nhats<8|16|24>, halves, k_bases_packed, nDims 8 ... 24, [12, 8]        0.97  0.62 | 0.091 0.090             | 2.1
  k_nhats_q<8|16>, halves, nDims 25 ... 64, [30, 10] (kappa <= 5.1e4)      0.54  0.38 | 0.040 0.024             | 2.4
  k_nhats_q<32>, nDims 65 ... 128, [60, 40] (kappa <= 5.3e4)               0.43  0.33 | 0.033 0.015 0.060 0.013 | 2.8
  k_basis<5..8> + k_whiten<5..8>, nDims 65 ... 128 (kappa <= 2.3e5)        0.68  0.46 | 0.035 0.011 0.078 0.009 | 2.7
  k_nhats_big, nDims 129 ... 256, [100, 50] (kappa <= 2.5e5)               0.66  0.48 | 0.021 0.005             | 1.9
Nothing grows with kappa: the panel kernels (k_basis, k_nhats_big) keep to kappa u like the pivot-by-pivot ones, with a constant 1.4 x
larger.  Every equality of (d) holds.  On the CPU: the oracle is C_ref by definition, a plain fp64 L q <= 0.11 and 0.15 of the bounds,
classical Gram-Schmidt of the four full 256-dimensional bases of the second key 4 ... 38 and 1.2 ... 7.6 kappa u.

NORM.  test_rows_have_unit_norm_to_4u found k_nhats_big at | |n^| - 1 | = 4.03 u (nDims 255), 4.21 u (256), 4.09 u (grades [100, 50]) and
3.6 u up to 144 dimensions: w = sqrt(sum t_a^2) was summed over up to 256 squares on two accumulators, 3 ... 4 u of rounding in the sum
alone.  The kernel's sum is compensated now (the product's error by FMA, the addition's by TwoSum): 1.9 u, below the matrix-core
kernels, which split the same sum over four lanes (2.8 u)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import oracle_api as orc
from tests.test_update_factors import LD, U, _need_long_double, _ratio, gam

BATCH, NCH, KEY1, KEY2_SMALL = 5, 4, 11, 12
MARGIN = 4


class Shape:
    def __init__(self, D, paths, grades=None, kind="gaussian"):
        self.D, self.paths, self.grades, self.kind = D, paths, grades, kind
        self.absent = tuple(p for p in (0, 1, 2) if p not in paths)
        self.reps = [d + 3 for d in self._dg()]
        self.nr = sum(self.reps)
        self.id = ("corr" if kind != "gaussian" else "") + ("+".join(str(g) for g in grades) if grades else str(D)) + "-p" + "".join(str(p) for p in paths)

    def _dg(self):
        if not self.grades:
            return [self.D]
        off = np.concatenate([[0], np.cumsum(self.grades)[:-1]])
        return [self.D - int(o) for o in off]

    def key(self):
        return (self.D, tuple(self.grades) if self.grades else ())

    def family(self, path):
        D = self.D
        if path == 2:
            return "k_bases_packed"
        if D <= 24:
            return "k_nhats" if path == 0 else "k_nhats halves"
        if D <= 64:
            return "k_nhats_q<8|16>" if path == 0 else "k_nhats_q<8|16> halves"
        if D <= 128:
            return "k_nhats_q<32>" if path == 0 else "k_basis+k_whiten"
        return "k_nhats_big"


SHAPES = ([Shape(1, (0, 1))] + [Shape(D, (0, 1, 2)) for D in (2, 8, 9, 16, 17, 24)] + [Shape(D, (0, 1)) for D in (25, 32, 33, 64)]
          + [Shape(D, (1,)) for D in (80, 81, 96, 97, 127)] + [Shape(D, (0, 1)) for D in (65, 112, 113, 128)]
          + [Shape(D, (0, 1), kind="corr_gaussian") for D in (65, 100, 128)] + [Shape(D, (0,)) for D in (129, 130, 144, 255, 256)]
          + [Shape(20, (0, 1), grades=(12, 8)), Shape(40, (0,), grades=(30, 10)), Shape(100, (0,), grades=(60, 40)),
             Shape(150, (0,), grades=(100, 50))])
# a shape that runs path 1 only still must not have path 2; path 0 exists for all of them and is simply not part of the case
for _s in SHAPES:
    if _s.paths == (1,):
        _s.absent = (2,)


# ---------------------------------------------------------------------------------------------------------------- reference
def mgs_ld(G):
    """modified Gram-Schmidt of the rows of G in long double, the reference's order: every vector normalised, then vector i loses its
    components along the finished vectors 0 ... i - 1 one after the other and is normalised (row oriented: the same operations)"""
    V = np.array(G, dtype=LD)
    V /= np.sqrt((V * V).sum(1))[:, None]
    for j in range(len(V)):
        V[j] /= np.sqrt((V[j] * V[j]).sum())
        if j + 1 < len(V):
            V[j + 1:] -= np.outer(V[j + 1:] @ V[j], V[j])
    return V


def cgs_f64(G):
    """the spoiled basis: CLASSICAL Gram-Schmidt in fp64, all coefficients of a vector taken from the vector as it was drawn"""
    V = G / np.linalg.norm(G, axis=1)[:, None]
    Q = np.zeros_like(V)
    for i in range(len(V)):
        v = V[i] - (Q[:i] @ V[i]) @ Q[:i]
        Q[i] = v / np.linalg.norm(v)
    return Q


class Block:
    """one basis of one chain: rows [r0, r0 + nvec) of the chain's directions, coordinates off ... D - 1"""

    def __init__(self, chain, grade, basis, gb, off, r0, G, nvec, Qorc):
        self.chain, self.grade, self.basis, self.gb, self.off, self.r0, self.nvec = chain, grade, basis, gb, off, r0, nvec      # (gb: the basis' number over all grades)
        self.kappa = float(np.linalg.cond(G / np.linalg.norm(G, axis=1)[:, None]))     # (of the basis as drawn, also where only three of its vectors are used)
        self.G = G
        self.Qref = mgs_ld(G[:nvec])
        self.Qorc = Qorc

    def ratios(self, Q):
        """(e_orth, e_fwd) / (kappa u) and e_orth of a basis Q [nvec][Dg]"""
        Q = np.asarray(Q, dtype=LD)
        assert Q.shape == self.Qref.shape
        e_orth = np.abs(Q @ Q.T - np.eye(self.nvec, dtype=LD)).max()
        e_fwd = np.abs(Q - self.Qref).max()
        ku = LD(self.kappa) * U
        return float(e_orth / ku), float(e_fwd / ku), float(e_orth)


def _osettings(D, grades, reps, seed):
    so = orc.settings(D, 0, num_repeats=reps[0], seed=seed)
    keep = orc.set_grades(so, list(grades), [float(r) for r in reps]) if grades else None
    return so, keep


@functools.lru_cache(maxsize=None)
def worst_key(D):
    """the key among 1 ... 32 whose chains 0 ... 3 hold the worst-conditioned first basis (-> key, its kappa, the median of all 128)"""
    so, _ = _osettings(D, None, [D], 1)
    kap = np.zeros((32, NCH))
    for k in range(32):
        for c in range(NCH):
            dev, _ = orc.direction_inputs(so, k + 1, BATCH, c, want_raw=False)
            G = dev.reshape(D, D)
            kap[k, c] = np.linalg.cond(G / np.linalg.norm(G, axis=1)[:, None])
    return int(np.argmax(kap.max(1))) + 1, float(kap.max()), float(np.median(kap))


def keys_of(shape):
    return (KEY1, worst_key(shape.D)[0] if shape.D > 64 else KEY2_SMALL)


@functools.lru_cache(maxsize=None)
def reference(D, grades, key):
    """the blocks of all four chains for one key (the bases depend on the key, the nursery, the chain and the grades alone)"""
    dg = [D] if not grades else [D - int(o) for o in np.concatenate([[0], np.cumsum(grades)[:-1]])]
    reps = [d + 3 for d in dg]
    so, keep = _osettings(D, grades, reps, key)
    blocks = []
    for c in range(NCH):
        dev, raw = orc.direction_inputs(so, key, BATCH, c)
        pos = r0 = gb = 0
        for g, (Dg, nrg) in enumerate(zip(dg, reps)):
            off = D - Dg
            for b in range(-(-nrg // Dg)):
                G = dev[pos:pos + Dg * Dg].reshape(Dg, Dg)
                pos += Dg * Dg
                nvec = min(Dg, nrg - b * Dg)
                rows = raw[r0 + b * Dg:r0 + b * Dg + nvec]
                assert np.all(rows[:, :off] == 0.0)
                blocks.append(Block(c, g, b, gb, off, r0 + b * Dg, G, nvec, rows[:, off:].copy()))
                gb += 1
            r0 += nrg
        assert pos == dev.size and r0 == raw.shape[0]
    return blocks


@functools.lru_cache(maxsize=None)
def c_ref():
    """the worst (e_orth, e_fwd) / (kappa u) of the oracle's fp64 bases over all cases of this file"""
    _need_long_double()
    worst = [0.0, 0.0]
    for key in sorted({s.key() for s in SHAPES}):
        shape = next(s for s in SHAPES if s.key() == key)
        for k in keys_of(shape):
            for blk in reference(*key, k):
                ro, rf, _ = blk.ratios(blk.Qorc)
                worst = [max(worst[0], ro), max(worst[1], rf)]
    return tuple(worst)


def hard_factor(D):
    """the Cholesky factor of 0.05^2 R diag(lam) R^T, lam geometric from 1 to 1e-8 (test_update_factors.cloud), strict upper triangle 0.0"""
    rng = np.random.default_rng(7000 + D)
    R, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = 1e8 ** (-np.arange(D) / max(D - 1, 1))
    cov = 0.05 ** 2 * (R * lam) @ R.T
    L = np.ascontiguousarray(np.linalg.cholesky(0.5 * (cov + cov.T)))
    assert np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0)
    return L


# ---------------------------------------------------------------------------------------------------------------- bounds
def whiten_ratios(Q, L, nhat, w3):
    """worst error / bound of n^ [n][D] and nhat_w [n] against t = L q of the rows of Q [n][D] (long double)"""
    D = L.shape[0]
    Q = np.asarray(Q, dtype=LD); Ll = L.astype(LD)
    T = Q @ Ll.T
    d = gam(D + 5) * (np.abs(Q) @ np.abs(Ll).T)
    w = np.sqrt((T * T).sum(1)); dn = np.sqrt((d * d).sum(1))
    bw = dn + gam(D + 2) * (w + dn)
    wl = w - bw
    assert np.all(wl > 0)
    bn = d / wl[:, None] + np.abs(T) * (bw / (w * wl))[:, None] + gam(3) * (np.abs(T) + d) / wl[:, None]
    return (_ratio(np.abs(nhat.astype(LD) - T / w[:, None]), bn), _ratio(np.abs(w3.astype(LD) - 3 * w), 3 * bw + 3 * U * (w + bw)))


def matvec_ratio(M, X, got):
    """worst error / bound of the rows of got against M x of the rows of X (fp64 values, products in long double)"""
    D = M.shape[0]
    Ml, Xl = M.astype(LD), X.astype(LD)
    return _ratio(np.abs(got.astype(LD) - Xl @ Ml.T), gam(D + 5) * (np.abs(Xl) @ np.abs(Ml).T))


def pad(blk, Q, D):
    out = np.zeros((blk.nvec, D), dtype=LD)
    out[:, blk.off:] = Q
    return out


# ---------------------------------------------------------------------------------------------------------------- the CPU half
def test_oracle_bases_and_a_plain_product_keep_the_bounds_and_a_spoiled_basis_does_not():
    _need_long_double()
    co, cf = c_ref()
    print(f"\ndirections C_ref: e_orth <= {co:.3f} kappa u, e_fwd <= {cf:.3f} kappa u (the oracle's fp64 bases, {len(SHAPES)} shapes, two keys)")
    assert 0 < co < 64 and 0 < cf < 64            # "a modest constant"
    worst_w = [0.0, 0.0]
    for D in sorted({s.D for s in SHAPES if s.D > 64}):
        key, kmax, kmed = worst_key(D)
        print(f"directions nDims {D}: key {key} holds kappa = {kmax:.3g}, median {kmed:.3g}")
        assert kmax >= 10 * kmed, (D, kmax, kmed)
    for key in sorted({s.key() for s in SHAPES}):
        shape = next(s for s in SHAPES if s.key() == key)
        L = hard_factor(shape.D)
        for k in keys_of(shape):
            for blk in reference(*key, k):
                assert blk.ratios(blk.Qorc)[2] < 1e-9
                q = np.zeros((blk.nvec, shape.D)); q[:, blk.off:] = blk.Qorc
                t = q @ L.T                                                   # a plain fp64 L q
                w = np.sqrt((t * t).sum(1))
                rn, rw = whiten_ratios(q, L, t / w[:, None], 3.0 * w)
                worst_w = [max(worst_w[0], rn), max(worst_w[1], rw)]
    print(f"directions plain fp64 L q: n^ error / bound <= {worst_w[0]:.3f}, nhat_w <= {worst_w[1]:.3f}")
    assert worst_w[0] <= 1 and worst_w[1] <= 1
    # the harness sees the failure it exists for: classical Gram-Schmidt of the full bases of 256 dimensions under the second key.  (On
    # Gaussian deviates classical Gram-Schmidt stays near kappa u as well -- kappa comes from ONE small singular value, nothing squares it --
    # with a constant of 2 ... 40 where the reference's order has 0.3 ... 0.9: the margin of 4 lies between the two.)
    spoiled = [(blk.ratios(cgs_f64(blk.G)), blk.kappa) for blk in reference(256, (), worst_key(256)[0]) if blk.nvec == 256]
    for (ro, rf, eo), kap in spoiled:
        print(f"directions spoiled basis (classical Gram-Schmidt, nDims 256, kappa {kap:.3g}): e_orth = {ro:.3g} kappa u, e_fwd = {rf:.3g} kappa u")
    ro, rf = max(r[0][0] for r in spoiled), max(r[0][1] for r in spoiled)
    assert ro > 2 * MARGIN * co and rf > MARGIN * cf
    # ... and a whitening product with one element of L dropped is outside its bound
    blk = reference(128, (), KEY1)[0]
    q = blk.Qorc; L = hard_factor(128); Lb = L.copy(); Lb[77, 3] = 0.0
    t = q @ Lb.T; w = np.sqrt((t * t).sum(1))
    assert max(whiten_ratios(q, L, t / w[:, None], 3.0 * w)) > 1


# ---------------------------------------------------------------------------------------------------------------- the device
def _problem(api, shape):
    olib = orc.load()
    D = shape.D
    if shape.kind == "gaussian":
        L, P, keep = api.make_problem("gaussian", D, 0)
        Lo, Po, keep2 = orc.make_problem("gaussian", D)
        return L, P, (keep, keep2), Lo, None, np.zeros(D), np.ones(D), None
    ic = np.zeros((D, D)); ld = C.c_double()
    olib.pc_random_invcov(12345, D, C.c_double(0.1), orc.dptr(ic), C.byref(ld))
    assert np.array_equal(ic, ic.T)
    mean = np.full(D, 0.5)
    L, P, keep = api.make_problem("corr_gaussian", D, 0, -1.0, 3.0, invcov=ic, mean=mean, logdet=ld.value)
    Lo, Po, keep2 = orc.make_problem("corr_gaussian", D, -1.0, 3.0, invcov=ic, mean=mean, logdet=ld.value)
    return L, P, (keep, keep2), Lo, ic, np.full(D, -1.0), np.full(D, 3.0), mean


def _start_rows(shape, Lo, lo, hi):
    olib = orc.load()
    D = shape.D; nT = 2 * D + 2
    rng = np.random.default_rng(31 * D + 5)
    rows = np.zeros((NCH, nT))
    for c in range(NCH):
        cube = 0.5 + 0.04 * rng.standard_normal(D)
        th = np.ascontiguousarray(lo + (hi - lo) * cube)
        phi = np.zeros(1)
        rows[c, :D] = cube; rows[c, D:2 * D] = th
        rows[c, nT - 1] = olib.pc_like_eval(C.byref(Lo), orc.dptr(th), D, orc.dptr(phi), 0)
    return rows


@pytest.fixture(scope="module")
def cref():
    return c_ref()


_MEASURED = {}


def _measure(api, cref, shape):
    """every run of a shape (two keys, its paths, the identity and the hard factor) held to (a), (b), (c) and (d); -> the largest
    | |n^| - 1 | / u of its rows (once per session: both tests of a shape read it)"""
    if shape.id in _MEASURED:
        return _MEASURED[shape.id]
    _need_long_double()
    co, cf = cref
    D, nr = shape.D, shape.nr
    Lk, Pk, keep, Lo, M, lo, hi, mean = _problem(api, shape)
    rows = _start_rows(shape, Lo, lo, hi)
    eye, Lh = np.eye(D), hard_factor(D)
    norm_u = 0.0
    first = {}
    for key in keys_of(shape):
        s = api.Settings(); api.load().pchip_settings_default(C.byref(s), D, 0)
        s.num_repeats, s.seed = shape.reps[0], key
        gk = api.set_grades(s, list(shape.grades), shape.reps) if shape.grades else None
        blocks = reference(*shape.key(), key)
        outs = {}
        for path in shape.absent:
            assert api.directions(s, Lk, Pk, BATCH, rows, eye, path) is None, f"path {path} must not exist"
        for path in shape.paths:
            a = api.directions(s, Lk, Pk, BATCH, rows, eye, path)
            h = api.directions(s, Lk, Pk, BATCH, rows, Lh, path)
            assert a is not None and h is not None, f"path {path} must exist"
            outs[path] = (a, h)
            wr = [0.0] * 8
            for o in (a, h):                                                  # (c) every row written, finite, of unit norm
                assert o["nhat"].shape == (NCH, nr, D) and np.all(np.isfinite(o["nhat"])) and np.all(np.isfinite(o["nhat_w"])) and np.all(o["nhat_w"] > 0)
                dev = np.abs(np.sqrt((o["nhat"].astype(LD) ** 2).sum(-1)) - 1).max()
                wr[7] = max(wr[7], float(dev / U))
                assert dev <= gam(D) / 2 + gam(3), float(dev / U)             # (what any order of the norm's sum keeps; the 4 u: the test below)
            kmax = 0.0
            for blk in blocks:
                c, r = blk.chain, slice(blk.r0, blk.r0 + blk.nvec)
                for o in (a, h):
                    assert np.all(o["nhat"][c, r, :blk.off] == 0.0)          # a grade's vectors carry zeros in front
                Qd = a["nhat"][c, r].astype(LD) * (a["nhat_w"][c, r].astype(LD) / 3)[:, None]
                if path != 0:                                                # the raw basis part 1 left behind is that basis
                    raw = a["raw"][c, blk.gb, :blk.nvec]
                    assert np.all(raw[:, :blk.off] == 0.0)
                    wr[6] = max(wr[6], _ratio(np.abs(raw.astype(LD) - Qd), 3 * U * np.abs(raw).astype(LD)))
                    assert np.array_equal(raw, h["raw"][c, blk.gb, :blk.nvec])   # (the bases do not depend on the factor)
                ro, rf, eo = blk.ratios(Qd[:, blk.off:])                     # (a)
                wr[0], wr[1] = max(wr[0], ro), max(wr[1], rf)
                kmax = max(kmax, blk.kappa)
                assert eo < 1e-9
                assert ro <= MARGIN * co and rf <= MARGIN * cf, (shape.family(path), blk.chain, blk.grade, blk.basis, blk.kappa, ro, rf, co, cf)
                rn, rw = whiten_ratios(Qd, Lh, h["nhat"][c, r], h["nhat_w"][c, r])      # (b)
                wr[2], wr[3] = max(wr[2], rn), max(wr[3], rw)
            assert wr[6] <= 1, wr[6]
            if shape.kind != "gaussian":
                for o in (a, h):
                    assert o["nhat_Ms"] is not None and np.all(np.isfinite(o["nhat_Ms"])) and np.all(np.isfinite(o["ch_My"]))
                    wr[4] = max(wr[4], matvec_ratio(M, ((hi - lo) * o["nhat"]).reshape(-1, D), o["nhat_Ms"].reshape(-1, D)))
                    wr[5] = max(wr[5], matvec_ratio(M, (lo + (hi - lo) * rows[:, :D]) - mean, o["ch_My"]))
            else:
                assert a["nhat_Ms"] is None and a["ch_My"] is None
            print(f"\ndirections {shape.family(path):>22} {shape.id:>12} key {key:2d} path {path} kappa <= {kmax:9.3g}: e_orth {wr[0]:.3f} e_fwd {wr[1]:.3f} kappa u"
                  f" (4 C_ref {MARGIN * co:.3f} {MARGIN * cf:.3f}) | n^ {wr[2]:.3f} nhat_w {wr[3]:.3f} M.s {wr[4]:.3f} M.y {wr[5]:.3f} of the bound | raw {wr[6]:.3f} of 3u | norm {wr[7]:.2f} u", end="")
            assert max(wr[2:6]) <= 1, wr
            norm_u = max(norm_u, wr[7])
            assert not np.array_equal(a["nhat"][0], a["nhat"][1])            # (c) two chains give different bases
        if D <= 64:                                                           # (d) the same bits
            p0 = shape.paths[0]
            for p in shape.paths[1:]:
                for i in (0, 1):
                    assert np.array_equal(outs[p][i]["nhat"], outs[p0][i]["nhat"]) and np.array_equal(outs[p][i]["nhat_w"], outs[p0][i]["nhat_w"]), (p0, p)
            if 2 in shape.paths:
                assert np.array_equal(outs[1][0]["raw"], outs[2][0]["raw"])
        first[key] = outs[shape.paths[0]][0]["nhat"]
    ka, kb = keys_of(shape)
    assert not np.array_equal(first[ka], first[kb])                           # two keys give different bases
    _MEASURED[shape.id] = norm_u
    return norm_u


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
def test_device_directions(engine, cref, shape):
    _measure(engine, cref, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
def test_rows_have_unit_norm_to_4u(engine, cref, shape):
    """(c), the figure as set: | |n^| - 1 | <= 4 u for every row of every run of the shape.
    (k_nhats_big missed it at nDims 255, 256 and [100, 50] until its norm was summed with compensation -- NORM at the top of the file)"""
    worst = _measure(engine, cref, shape)
    print(f"\ndirections {shape.id}: | |n^| - 1 | <= {worst:.2f} u", end="")
    assert worst <= 4, worst
