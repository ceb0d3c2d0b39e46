"""The reference's adaptive prior types (11 .. 15: adaptive_sorted_uniform / _gaussian / _half_gaussian / _exponential and
nn_adaptive_layer_gaussian, priors.f90:363-488) in a prior table: the host function against the reference's priors_module and against a
numpy restatement, the ini door, validation, the public names, the kernels' run-time compilation; on the GPU the device transform against
the host function, engine against oracle and against the reference binary, an analytic evidence, runs in step, the device maximiser and
the doors."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_device_priors import GAUSS_SRC, _evidence_check, _settings, _stats_logz, _table_variants, _table_vs_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTIVE = {"adaptive_sorted_uniform": 11, "adaptive_sorted_gaussian": 12, "adaptive_sorted_half_gaussian": 13,
            "adaptive_sorted_exponential": 14, "nn_adaptive_layer_gaussian": 15}
BASE = {11: "uniform", 12: "gaussian", 13: "half_gaussian", 14: "exponential", 15: "gaussian"}
# prior parameters of a block's k-th parameter, different for every member (the count's and the layer's are read and ignored)
PARS = {"adaptive_sorted_uniform": lambda k: (-1.0 + 0.25 * k, 2.0 + 0.5 * k), "adaptive_sorted_gaussian": lambda k: (0.1 * k, 1.0 + 0.5 * k),
        "adaptive_sorted_half_gaussian": lambda k: (-0.2 * k, 0.5 + 0.25 * k), "adaptive_sorted_exponential": lambda k: (0.5 + k,),
        "nn_adaptive_layer_gaussian": lambda k: (0.3 * k, 0.75 + 0.25 * k)}
# 5-D Gaussian likelihood (0.5, 0.1) under one adaptive_sorted_uniform (0, 1) block of five: the count is uniform on (0.5, 4.5) and sees
# half a Gaussian; a product of identical factors integrates the same over sorted and unsorted members, whatever nfunc
LOGZ_BLOCK5 = math.log(0.5 * math.erf(4.0 / (0.1 * math.sqrt(2.0))) / 4.0) + 4.0 * math.log(math.erf(0.5 / (0.1 * math.sqrt(2.0))))


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _block(kind, n, block=1):
    return [(kind, block, PARS[kind](k)) for k in range(n)]


def _num(t):
    return ADAPTIVE.get(t, t) if isinstance(t, str) else t


def _adaptive_blocks(entries):
    """(first parameter, number of parameters, type number) of every adaptive block of a table"""
    out, i = [], 0
    while i < len(entries):
        t = _num(entries[i][0])
        if not isinstance(t, int) or t < 11:
            i += 1
            continue
        j = i
        while j < len(entries) and _num(entries[j][0]) == t and entries[j][1] == entries[i][1]:
            j += 1
        out.append((i, j - i, t))
        i = j
    return out


def _count_columns(entries):
    """(parameter index of the count, n - 1 = its number of members) of every adaptive block"""
    return [(i + (t == 15), n - 1 - (t == 15)) for i, n, t in _adaptive_blocks(entries)]


def _edge_values(n1):
    """every bin edge x_1 = k / (n - 1), its two neighbours, and the largest double below 1"""
    v = []
    for k in range(n1 + 1):
        e = k / n1
        v += [e, np.nextafter(e, 0.0), np.nextafter(e, 1.0)]
    return [x for x in v if 0.0 <= x < 1.0] + [1.0 - 2.0 ** -53]


def _nfunc(x, n1):
    """priors.f90:378-380 with the defined clamp: every operation rounded on its own (numpy scalars do not fuse)"""
    t = np.float64(0.5) + np.float64(x) * np.float64(n1)
    return min(max(int(t + np.float64(0.5)), 1), n1)


def _root(x, j):
    if 1.0 - 2.0 ** -33 < x < 1.0 and j <= 256:                 # the exactness rule of pc_sorted_root
        k = int((1.0 - x) * 2.0 ** 53)
        return 1.0 - float((2 * k + j) // (2 * j)) * 2.0 ** -53
    return float(np.power(np.float64(x), np.float64(1.0) / np.float64(j)))


def _base(lib, base, y, pp):
    if base == "uniform":
        return pp[0] + (pp[1] - pp[0]) * y
    if base == "gaussian":
        return pp[0] + pp[1] * lib.polychord_hip_inv_normal_cdf(y)
    if base == "half_gaussian":
        return pp[0] + pp[1] * lib.polychord_hip_inv_normal_cdf(0.5 + 0.5 * y)
    return -math.log(1.0 - y) / pp[0]


def _restated(lib, entries, hyper, cube):
    """the five adaptive types restated (a table of adaptive blocks only): (theta, [nfunc of every block])"""
    x = [cube[h] for h in hyper]
    th, nfs = [0.0] * len(entries), []
    for i, n, t in _adaptive_blocks(entries):
        base, c = BASE[t], i
        if t == 15:
            th[i] = 0.5 + 2.0 * x[i]
            base, c, n = ("half_gaussian" if th[i] < 1.5 else "gaussian"), i + 1, n - 1
        th[c] = float(np.float64(0.5) + np.float64(x[c]) * np.float64(n - 1))
        nf = _nfunc(x[c], n - 1)
        nfs.append(nf)
        y = list(x[c + 1:c + n])
        prev = 1.0
        for s in range(nf, 0, -1):
            prev = prev * _root(y[s - 1], s)
            y[s - 1] = prev
        for s in range(1, n):
            th[c + s] = _base(lib, base, y[s - 1], entries[c + s][2])
    return np.array(th), nfs


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_host_function_matches_the_reference(golden):
    """polychord_hip_table_prior against the reference's priors_module at the fixture's cube points (tools/dev/gen_ref_adaptive_priors.py):
    types 11 .. 14 at n = 2 and 5 with a point in every nfunc bin, type 15 at n = 4 on both sides of the layer boundary; the bound of
    test_table_prior_matches_the_reference"""
    api, lib = _lib()
    fx = golden["ref_adaptive_priors"]["transforms"]
    assert {r["type"] for r in fx} == set(ADAPTIVE) and {(r["type"], len(r["cube"])) for r in fx} >= {(t, n) for t in list(ADAPTIVE)[:4] for n in (2, 5)}
    for r in fx:
        api.set_table_prior([(r["type"], 1, p) for p in r["par"]])
        theta = api.table_prior(r["cube"])
        assert np.allclose(theta, r["theta"], rtol=1e-13, atol=1e-15), (r["type"], r["cube"], theta, r["theta"])


@pytest.mark.parametrize("kind", list(ADAPTIVE))
def test_host_function_matches_a_restatement(kind):
    """2 000 seeded points per type and block size, identity and permuted order, against the numpy restatement above (rtol 1e-13, atol 1e-15);
    among them every bin edge x_1 = k / (n - 1) with its two neighbours and x_1 = 1 - 2^-53, where nfunc must be n - 1.  The restatement forms
    nfunc with numpy scalars, each operation rounded on its own; a host nfunc that differs at any point sorts another number of members and
    misses the bound by orders of magnitude."""
    api, lib = _lib()
    lib.polychord_hip_inv_normal_cdf.restype = C.c_double
    lib.polychord_hip_inv_normal_cdf.argtypes = [C.c_double]
    rng = np.random.default_rng(11)
    extra = 1 if kind == "nn_adaptive_layer_gaussian" else 0
    for n1 in (1, 2, 3, 4):
        n = n1 + 1 + extra
        entries = _block(kind, n)
        cubes = rng.random((2000, n))
        edges = _edge_values(n1)
        for order in ("identity", "permuted"):
            hyper = list(range(n)) if order == "identity" else [int(v) for v in rng.permutation(n)]
            cubes[:len(edges), hyper[extra]] = edges
            if extra:                                       # the layer boundary theta_1 = 1.5 and its neighbours
                cubes[:3, hyper[0]] = [0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)]
            api.set_table_prior(entries, None if order == "identity" else hyper)
            for row, cube in enumerate(cubes):
                host = api.table_prior(cube)
                want, (nf,) = _restated(lib, entries, hyper, cube)
                if row < len(edges) and edges[row] == 1.0 - 2.0 ** -53:
                    assert nf == n1, (kind, n, nf)
                assert np.allclose(host, want, rtol=1e-13, atol=1e-15), (kind, n, order, row, nf, cube.tolist(), host, want)


def test_ini_prior_with_an_adaptive_block_and_two_speeds_is_the_table(tmp_path):
    """polychord_hip_ini_prior on an ini text whose adaptive block has its count in the slow grade and its members in the fast one equals
    the table set by hand with the hypercube order of priors.f90:708-737"""
    api, lib = _lib()
    f = lib.polychord_hip_ini_prior
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    ini = tmp_path / "a.ini"
    lines = ["nlive = 50", "num_repeats = 5", "grade_frac = 2 4", "",
             "P : m1 | m_1 | 2 | gaussian | 1 | 0.5 0.5",
             "P : n | n | 1 | adaptive_sorted_exponential | 2 | 2.0"] + \
            [f"P : a{k} | a_{k} | 2 | adaptive_sorted_exponential | 2 | {1.0 + k}" for k in range(1, 4)] + \
            ["P : u | u | 1 | uniform | 3 | 0.0 2.0"]
    ini.write_text("\n".join(lines) + "\n")
    entries = [("gaussian", 1, (0.5, 0.5)), ("adaptive_sorted_exponential", 2, (2.0,))] + \
              [("adaptive_sorted_exponential", 2, (1.0 + k,)) for k in range(1, 4)] + [("uniform", 3, (0.0, 2.0))]
    hyper = [2, 0, 3, 4, 5, 1]                              # the slow parameters (n, u) first, then the fast ones in file order
    api.set_table_prior(entries, hyper)
    rng = np.random.default_rng(5)
    for cube in rng.random((50, 6)):
        th = np.empty(6)
        assert f(str(ini).encode(), api.dptr(np.ascontiguousarray(cube)), api.dptr(th), 6) == 6
        assert np.array_equal(th, api.table_prior(cube)), (cube, th)


BAD_ADAPTIVE = [  # (entries, what the message must name)
    ([("uniform", (0, 1)), ("adaptive_sorted_uniform", 1, (0, 1))], ("parameter 2", "block of 1")),
    ([("nn_adaptive_layer_gaussian", 1, (0, 1))] * 2, ("parameter 1", "block of 2")),
    ([("adaptive_sorted_uniform", 1, (0, 1)), ("adaptive_sorted_uniform", 1, (0, 1, 2))], ("parameter 2", "exactly 2")),
    ([("adaptive_sorted_exponential", 1, (1.0, 2.0)), ("adaptive_sorted_exponential", 1, (1.0,))], ("parameter 1", "exactly 1")),
    ([("adaptive_sorted_gaussian", 1, (0, 1)), ("adaptive_sorted_gaussian", 1, (0,))], ("parameter 2", "exactly 2")),
    ([("adaptive_sorted_gaussian", 1, (0, 1)), ("adaptive_sorted_gaussian", 1, (0.0, 0.0))], ("parameter 2", "sigma")),
    ([("nn_adaptive_layer_gaussian", 1, (0, 1))] * 3 + [("nn_adaptive_layer_gaussian", 1, (0.0, -1.0))], ("parameter 4", "sigma")),
    ([("adaptive_sorted_half_gaussian", 1, (0, 1))] * 2 + [("adaptive_sorted_half_gaussian", 1, (0.0, -2.0))], ("parameter 3", "sigma")),
    ([("adaptive_sorted_exponential", 1, (1.0,)), ("adaptive_sorted_exponential", 1, (0.0,))], ("parameter 2", "rate")),
    ([("adaptive_sorted_uniform", 1, (0, 1))] * 2 + [("uniform", 1, (0, 1)), ("adaptive_sorted_uniform", 1, (0, 1))], ("parameter 4", "consecutive")),
]


def test_validation_names_the_parameter():
    api, lib = _lib()
    for entries, words in BAD_ADAPTIVE:
        with pytest.raises(ValueError) as e:
            api.set_table_prior(entries)
        for w in words:
            assert w in str(e.value), (entries, str(e.value))
    # the count's (and the layer's) values are read and ignored: a sigma of zero there is no error; two blocks of one type by block number
    api.set_table_prior([("adaptive_sorted_gaussian", 1, (0.0, 0.0)), ("adaptive_sorted_gaussian", 1, (0.0, 1.0))] +
                        [("nn_adaptive_layer_gaussian", 1, (0.0, -1.0))] * 2 + [("nn_adaptive_layer_gaussian", 1, (0.0, 1.0))] +
                        [("adaptive_sorted_gaussian", 2, (0.0, 1.0))] * 2)
    assert lib.polychord_hip_last_error() is None


def test_public_names_and_the_table_prior_object():
    api, lib = _lib()
    assert api.ADAPTIVE_PRIOR_TYPES == ADAPTIVE and not set(api.ADAPTIVE_PRIOR_TYPES) & set(api.PRIOR_TYPES)
    hdr = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    for name, num in api.ADAPTIVE_PRIOR_TYPES.items():
        assert re.search(r"PCHIP_PT_%s = %d\b" % (name.upper(), num), hdr), name
    assert not re.search(r"adaptive types[^.]*not supported", hdr)
    f90 = open(os.path.join(ROOT, "bindings", "fortran", "polychord_hip.f90")).read()
    for name, num in api.ADAPTIVE_PRIOR_TYPES.items():
        assert re.search(r"PCHIP_PT_%s = %d\b" % (name.upper(), num), f90), name
    from polychordlite_amd.pypolychord.device_likelihoods import TablePrior
    for name in ADAPTIVE:
        assert name in TablePrior.__doc__, name
    entries = [("uniform", (0.0, 2.0))] + _block("adaptive_sorted_uniform", 5)
    p = TablePrior(entries)
    cube = [0.25, 0.6, 0.9, 0.8, 0.1, 0.3]                  # nfunc = INT(1 + 4 * 0.6) = 3
    th = p(cube)
    api.set_table_prior(entries)
    assert np.array_equal(th, api.table_prior(cube))
    assert th[0] == 0.5 and th[1] == 0.5 + 0.6 * 4 and th[2] < th[3] < th[4]
    # (by number as well as by name)
    api.set_table_prior([("uniform", (0.0, 2.0))] + [(11, 1, e[2]) for e in entries[1:]])
    assert np.array_equal(th, api.table_prior(cube))
    with pytest.raises(ValueError):
        TablePrior([("adaptive_sorted_uniform", 1, (0, 1))])([0.5])


def _kernel_names():
    """adaptive tables have a template value of their own in the sampling kernels (PT = 2: the PT = 1 kernels of the other tables stay what
    they were): the twin of every table variant of k_slice, of the runs in step; and the kernels with one text for every table -- the
    live set's, the transform door's, the maximiser's"""
    one = _table_variants() + [f"k_slice_many<1, {nrows}, false, 1, {fw}, 0, 1>" for nrows, fw in ((1, 0), (2, 0), (4, 0), (1, 8), (1, 16), (2, 24))]
    two = [re.sub(r", 1>$", ", 2>", n) for n in one if n.startswith("k_slice")]
    assert len(two) == 13 + 6 and all(n.endswith(", 0, 2>") for n in two)
    return one + two + [f"k_prior_transform<{d}>" for d in (1, 2, 4)] + ["k_maximise<1>"]


@pytest.mark.parametrize("with_source", [False, True])
def test_every_kernel_of_a_table_compiles_for_gfx950(with_source):
    api, lib = _lib()
    src = open(os.path.join(ROOT, "polychordlite_amd", "csrc", "pc_sample.hip")).read()
    assert "PC_PT_ADAPTIVE" in src and "__dmul_rn" in src     # (the rounding of nfunc is spelt out, not left to contraction)
    rows = re.findall(r"\bX\(([^()]*)\)", src)               # every PT = 2 name is a row of the launchers' variant tables
    for n in _kernel_names():
        if n.endswith(", 2>"):
            assert n[n.index("<") + 1:-1] in rows, n
    h = api.source_create(GAUSS_SRC) if with_source else 0
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(_kernel_names()).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    if h:
        lib.pchip_source_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _mixed20():
    return ([("uniform", 1, (-1.0, 2.0))] + _block("adaptive_sorted_uniform", 4, 10) + [("gaussian", 1, (0.3, 2.0))] +
            _block("adaptive_sorted_gaussian", 3, 20) + [("sorted_uniform", 30, (0.0, 10.0))] * 2 + _block("adaptive_sorted_half_gaussian", 2, 40) +
            [("log_uniform", 1, (1e-3, 5.0))] + _block("nn_adaptive_layer_gaussian", 4, 50) + _block("adaptive_sorted_exponential", 2, 60))


G62 = [("gaussian", 1, (0.5, 0.2))] * 62
TAIL2 = [("half_gaussian", 1, (0.4, 0.2)), ("exponential", 1, (3.0,))]
# the count at index 62, the members at 63 .. 67: lane 63's first coordinate and lanes 0 .. 3's second
BOUNDARY70 = G62 + _block("adaptive_sorted_gaussian", 6, 7) + TAIL2
# the layer at 61, the count at 62, the members at 63 .. 67
BOUNDARY70_NN = G62[:61] + _block("nn_adaptive_layer_gaussian", 7, 7) + TAIL2


def _transform_cases():
    cases = [(f"{kind}_n{n}", _block(kind, n + (kind == "nn_adaptive_layer_gaussian"))) for kind in ADAPTIVE for n in (2, 5)]
    cases += [("mixed20", _mixed20()), ("boundary70", BOUNDARY70), ("boundary70_nn", BOUNDARY70_NN)]
    assert len(cases[-3][1]) == 20 and len(cases[-2][1]) == 70 and len(cases[-1][1]) == 70
    assert _count_columns(BOUNDARY70) == [(62, 5)] and _count_columns(BOUNDARY70_NN) == [(62, 5)]
    return cases


@pytest.mark.gpu
def test_device_transform_is_the_host_function(engine):
    """pchip_prior_transform (the kernels' pc_table_theta) against polychord_hip_table_prior: each adaptive type alone at n = 2 and 5, a
    20-entry table of the five types among some of the old ten, two 70-entry tables with a block across index 63 / 64; identity and
    permuted order; 10 000 seeded points plus every bin edge of every count with its neighbours, 1 - 2^-53, and coordinates within 1e-12
    of 0 and 1.  Same finiteness pattern and 1e-9 relative to max(1, |theta|) (test_device_priors' bound for device against host): a
    wrong nfunc at any point misses it by orders of magnitude."""
    api = engine
    rng = np.random.default_rng(2025)
    worst = {}
    for name, entries in _transform_cases():
        D = len(entries)
        cubes = rng.random((10000, D))
        edge = rng.random((2000, D)) < 0.15
        cubes[1000:3000][edge] = rng.random(int(edge.sum())) * 1e-12
        edge = rng.random((2000, D)) < 0.15
        cubes[3000:5000][edge] = 1.0 - rng.random(int(edge.sum())) * 1e-12
        for order in ("identity", "permuted"):
            hyper = None if order == "identity" else rng.permutation(D).astype(np.int32)
            for col, n1 in _count_columns(entries):
                ev = _edge_values(n1)
                cubes[:len(ev), col if hyper is None else hyper[col]] = ev
            for i, n, t in _adaptive_blocks(entries):
                if t == 15:                                 # the layer boundary
                    cubes[20:23, i if hyper is None else hyper[i]] = [0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)]
            dev = api.prior_transform(entries, cubes, hyper)
            api.set_table_prior(entries, hyper)
            host = np.array([api.table_prior(c) for c in cubes])
            fin = np.isfinite(host)
            assert np.array_equal(fin, np.isfinite(dev)), (name, order)
            assert np.array_equal(host[~fin], dev[~fin]), (name, order)
            rel = np.abs(dev[fin] - host[fin]) / np.maximum(1.0, np.abs(host[fin]))
            print(f"device transform {name:36s} {order:9s}: max deviation {rel.max():.3e} relative to max(1, |theta|)")
            worst[name] = max(worst.get(name, 0.0), float(rel.max()))
            if not rel.max() < 1e-9:
                full = np.where(fin, np.abs(dev - host) / np.maximum(1.0, np.abs(host)), 0.0)
                i, j = np.unravel_index(np.argmax(full), full.shape)
                print(f"worst: point {i}, parameter {j} {entries[j]}: host {host[i, j]!r}, device {dev[i, j]!r}, cube row {cubes[i].tolist()}")
            assert rel.max() < 1e-9, (name, order, rel.max())
    print("largest deviation per case:", {k: f"{v:.2e}" for k, v in worst.items()})


U01 = (0.0, 1.0)
SIX = [("adaptive_sorted_uniform", 1, U01)] * 5 + [("uniform", 2, U01)]
ORACLE_CASES = {
    "gaussian6_adaptive_sorted_uniform_block_of_five": dict(kind="gaussian", entries=SIX, nlive=100, num_repeats=12, batch=16),
    "twin_gaussian4_clustering_smallest_block": dict(kind="twin_gaussian", entries=[("uniform", 1, (-1.0, 1.0))] * 2 + [("adaptive_sorted_gaussian", 2, (0.0, 0.5))] * 2,
                                                     nDer=1, nlive=200, num_repeats=8, batch=40, do_clustering=1),
    "gaussian6_nn_adaptive_layer": dict(kind="gaussian", entries=[("nn_adaptive_layer_gaussian", 1, (0.5, 0.5))] * 6, nDer=1, nlive=100, num_repeats=12, batch=16),
    "source_likelihood_adaptive_sorted_exponential": dict(kind="gaussian", entries=[("adaptive_sorted_exponential", 1, (2.0,))] * 4, source=GAUSS_SRC,
                                                          nDer=1, nlive=100, num_repeats=8, batch=16),
    # the count (and a uniform, listed last) in the slow grade, the members in the fast one: cube = [count, uniform, members]
    "two_grades_count_slow_members_fast": dict(kind="gaussian", entries=[("adaptive_sorted_uniform", 1, U01)] * 4 + [("uniform", 2, U01)],
                                               hyper=[0, 2, 3, 4, 1], grades=([2, 3], [2, 4]), nDer=1, nlive=100, num_repeats=6, batch=20),
    "gaussian70_block_across_the_lane_boundary": dict(kind="gaussian", entries=BOUNDARY70, nlive=100, num_repeats=20, batch=16, max_ndead=300),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_adaptive_table_walks_the_oracle(engine, tmp_path, case):
    """production mode against the oracle whose callback prior is polychord_hip_table_prior: counters equal, log Z to 1e-8, dead rows to 1e-7"""
    _table_vs_oracle(engine, tmp_path, **ORACLE_CASES[case])


@pytest.mark.gpu
def test_reproduces_the_reference_binary(engine, golden):
    """sequential_rng = 1 against the reference BINARY run through its own ini door under the RNG shim (tests/golden/ref_adaptive_priors.json,
    tools/dev/gen_ref_adaptive_priors.py): the five types over four runs, one with clustering, one with the count in the slow grade and the
    members in the fast one; the criteria of tests/test_device_priors.py::test_reproduces_the_reference_binary"""
    api = engine
    fx = golden["ref_adaptive_priors"]
    assert len(fx["door_proof"]) >= 1 and len(fx["cases"]) >= 4
    assert {p["type"] for c in fx["cases"] for p in c["params"]} >= set(ADAPTIVE)
    assert sum(c["clustering"] for c in fx["cases"]) >= 1 and any(len({p["speed"] for p in c["params"]}) > 1 for c in fx["cases"])
    for c in fx["cases"]:
        D = c["nDims"]
        entries = [(p["type"], p["block"], p["par"]) for p in c["params"]]
        speeds = [p["speed"] for p in c["params"]]
        grades = sorted(set(speeds))
        hyper, h = [0] * D, 0
        for g_ in grades:
            for i in range(D):
                if speeds[i] == g_:
                    hyper[i] = h; h += 1
        s = _settings(api, D, c["nDerived"], nlive=c["nlive"], num_repeats=max(c["num_repeats"], 1), seed=c["seed"],
                      do_clustering=c["clustering"], sequential_rng=1)
        keep = None
        if len(grades) > 1:
            keep = api.set_grades(s, [speeds.count(g_) for g_ in grades], [int(v) for v in c["grade_frac"].split()])
        L, P, k2 = api.make_problem(c["like"], D, c["nDerived"], prior_table=entries, hyper=hyper)
        g = api.run(s, L, P)
        assert g["path"]["device_prior"] > 0, c["name"]
        print(c["name"], g["ndead"], c["ndead"], g["nlike"], c["nlike"], g["logZ"], c["logZ"])
        assert (g["ndead"], g["nlike"]) == (c["ndead"], c["nlike"]), (c["name"], g["ndead"], c["ndead"], g["nlike"], c["nlike"])
        if len(grades) > 1:
            assert g["nlike_grade"][:len(grades)] == c["nlike_grades"], (c["name"], g["nlike_grade"], c["nlike_grades"])
        assert abs(g["logZ"] - c["logZ"]) < 1e-8 and abs(g["logZerr"] - c["logZerr"]) < 1e-8, (c["name"], g["logZ"], c["logZ"], g["logZerr"], c["logZerr"])
        assert g["ncluster_dead"] == c["ncluster_dead"], (c["name"], g["ncluster_dead"], c["ncluster_dead"])


@pytest.mark.gpu
def test_analytic_evidence_adaptive_sorted_uniform(engine):
    """log Z = log(0.5 erf(4 / (0.1 sqrt 2)) / 4) + 4 log erf(0.5 / (0.1 sqrt 2)) = -2.07944 (LOGZ_BLOCK5 above): the transform is
    measure-preserving in every nfunc bin, or the eight seeds' mean misses it"""
    assert abs(LOGZ_BLOCK5 - (-2.07944)) < 1e-5
    _evidence_check(engine, [("adaptive_sorted_uniform", 1, U01)] * 5, 5, LOGZ_BLOCK5, 10)


@pytest.mark.gpu
def test_runs_in_step_are_the_solo_runs(engine):
    api = engine
    from polychordlite_amd import repeats
    kw = dict(nlive=100, num_repeats=12)
    L, P, keep = api.make_problem("gaussian", 6, 0, prior_table=SIX)
    seeds = [3, 4]
    merged, runs = repeats.run_in_step(_settings(api, 6, 0, **kw), L, P, seeds, max_in_flight=2)
    assert len(runs) == 2
    for seed, r in zip(seeds, runs):
        solo = api.run(_settings(api, 6, 0, seed=seed, **kw), L, P)
        assert solo["path"]["device_prior"] > 0 and r["path"]["slice_step"] > 0, r["path"]
        for k in ("ndead", "nlike", "niter"):
            assert r[k] == solo[k], (seed, k, r[k], solo[k])
        assert r["ndead"] > 0 and r["logZ"] == solo["logZ"] and np.array_equal(np.asarray(r["dead"]), solo["dead"]), seed


@pytest.mark.gpu
def test_the_device_maximiser_under_an_adaptive_table(engine):
    """maximise_device on the 6-D case: a point at least as likely as the best live point, whose theta is the table's transform of its cube
    -- the cube recovered by the inverse, which a (0, 1) uniform base has: x_1 = (theta_1 - 0.5) / 4, the sorted members
    x_s = (y_s / y_(s+1))^s and x_nfunc = y_nfunc^nfunc, every other coordinate theta itself"""
    api = engine
    s = _settings(api, 6, 0, nlive=100, num_repeats=12, seed=7)
    L, P, keep = api.make_problem("gaussian", 6, 0, prior_table=SIX)
    g = api.run(s, L, P)
    m = api.maximise_device(s, L, P, g)
    assert m["max_point"] is not None and m["niter"][0] > 0, m
    best = float(np.max(np.asarray(g["live"])[:, g["nTotal"] - 1]))
    print("device maximiser:", m["max_logl"], "best live point:", best, "theta:", m["max_point"])
    assert m["max_logl"] >= best
    th = np.asarray(m["max_point"][:6])
    assert 0.5 < th[0] < 4.5 and np.all((th[1:] > 0.0) & (th[1:] < 1.0))
    nf = int(th[0] + 0.5)
    cube = th.copy()
    cube[0] = (th[0] - 0.5) / 4.0
    for k in range(1, nf):
        cube[k] = (th[k] / th[k + 1]) ** k
    cube[nf] = th[nf] ** nf
    api.set_table_prior(SIX)
    back = api.table_prior(cube)
    assert np.allclose(back, th, rtol=1e-12, atol=0.0), (th, cube, back)


# The doors run configs/gaussian_adaptive_sorted_uniform.ini's problem: the block of five of LOGZ_BLOCK5 and one more parameter, uniform on
# (-0.5, 1.5).  The likelihood is a product over the parameters, so the extra one multiplies Z by the integral of its Gaussian factor over its
# prior: (1 / 2) * erf(1 / (0.1 sqrt 2)) -- the prior density 1 / 2 of a box of width 2 times all but 1.5e-23 of the Gaussian's mass.
LOGZ_DOORS = LOGZ_BLOCK5 - math.log(2.0) + math.log(math.erf(1.0 / (0.1 * math.sqrt(2.0))))
DOOR_TABLE = [("adaptive_sorted_uniform", 1, U01)] * 5 + [("uniform", 2, (-0.5, 1.5))]


@pytest.mark.gpu
def test_cli_runs_the_adaptive_ini_on_the_device(engine, tmp_path):
    cli = os.path.join(ROOT, "tools", "polychord_hip_cli")
    ini = tmp_path / "a.ini"
    text = open(os.path.join(ROOT, "configs", "gaussian_adaptive_sorted_uniform.ini")).read()
    assert len(re.findall(r"\| adaptive_sorted_uniform \|", text)) == 5 and len(re.findall(r"\| uniform \|", text)) == 1
    ini.write_text(text.replace("nlive = 500", "nlive = 200"))
    r = subprocess.run([cli, str(ini), "gaussian"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "prior table evaluated on the device" in r.stdout, r.stdout
    z, e = _stats_logz(tmp_path / "chains" / "gaussian_adaptive_sorted_uniform.stats")
    print("cli: log Z", z, "+/-", e, "truth", LOGZ_DOORS)
    assert abs(z - LOGZ_DOORS) < 5.0 * e, (z, e, LOGZ_DOORS)


@pytest.mark.gpu
def test_pchip_run_and_pypolychord_run_with_the_adaptive_table(engine, tmp_path):
    api = engine
    s = _settings(api, 6, 0, nlive=200, num_repeats=12, seed=3)
    L, P, keep = api.make_problem("gaussian", 6, 0, prior_table=DOOR_TABLE)
    g = api.run(s, L, P)
    assert g["path"]["device_prior"] > 0, g["path"]
    assert abs(g["logZ"] - LOGZ_DOORS) < 5.0 * g["logZerr"], (g["logZ"], g["logZerr"], LOGZ_DOORS)
    from polychordlite_amd import pypolychord
    from polychordlite_amd.pypolychord.device_likelihoods import Gaussian, TablePrior
    from polychordlite_amd.pypolychord.output import PolyChordOutput
    pypolychord.run(Gaussian(0.5, 0.1), 6, prior=TablePrior(DOOR_TABLE), nlive=200, num_repeats=12, seed=3,
                    base_dir=str(tmp_path / "chains"), file_root="ap", feedback=0, do_clustering=False, write_resume=False, read_resume=False,
                    posteriors=False, equals=False, cluster_posteriors=False, write_live=False, write_prior=False)
    out = PolyChordOutput(str(tmp_path / "chains"), "ap")
    print("pypolychord: log Z", out.logZ, "+/-", out.logZerr, "truth", LOGZ_DOORS)
    assert abs(out.logZ - LOGZ_DOORS) < 5.0 * out.logZerr, (out.logZ, out.logZerr, LOGZ_DOORS)
