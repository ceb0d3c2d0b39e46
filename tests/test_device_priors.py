"""The reference's prior types as a table evaluated inside the sampling kernels (pchip_prior.kind = 2, pc_table_theta in pc_sample.hip):
the host function against the reference's priors_module, the new kernel variants' run-time compilation, the ABI, validation; on the GPU
the device transform against the host function, engine against oracle, a box written as a table, analytic evidences and the doors."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import oracle_api as orc
from tests.test_device_source import GAUSS_SRC, _host_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# prior type -> the three parameters' prior parameters of tests/golden/ref_priors.json (oracle/ref_priors.f90)
REF_PARAMS = {
    "uniform": [(-1, 2), (0, 5), (3, 4)], "log_uniform": [(1e-3, 1), (2, 50), (0.1, 0.2)], "gaussian": [(0, 1), (2, 0.5), (-3, 2)],
    "half_gaussian": [(0, 1), (2, 0.5), (-3, 2)], "exponential": [(1,), (0.5,), (4,)], "power_uniform": [(1, 4, 2), (2, 9, -1.5), (0.5, 3, 3)],
    "sorted_uniform": [(0, 10)] * 3, "sorted_gaussian": [(0, 1)] * 3, "sorted_half_gaussian": [(0, 2)] * 3, "sorted_exponential": [(2,)] * 3,
}


def _lib():
    from polychordlite_amd import _ctypes_api as api
    return api, api.load()


def _settings(api, D, nDer, **kw):
    lib = api.load()
    s = api.Settings(); lib.pchip_settings_default(C.byref(s), D, nDer)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_table_prior_matches_the_reference(golden):
    """polychord_hip_table_prior, set up through polychord_hip_set_table_prior, against the reference's priors_module on the golden
    hypercube point: all ten types at the rtol of test_ini_priors_match_the_reference, and that test's speed-ordered case"""
    api, lib = _lib()
    g = golden["ref_priors"]
    cube = np.array(g["cube"])
    assert set(REF_PARAMS) == set(api.PRIOR_TYPES) and sorted(api.PRIOR_TYPES.values()) == list(range(1, 11))
    for kind, pp in REF_PARAMS.items():
        api.set_table_prior([(kind, 1, pp[i]) for i in range(3)])
        theta = api.table_prior(cube)
        assert np.allclose(theta, g[kind], rtol=1e-13, atol=1e-15), (kind, theta, g[kind])
    # the hypercube is ordered by speed (priors.f90:708-737): the fast parameter listed first takes the last coordinate
    api.set_table_prior([("uniform", 1, (0, 1)), ("uniform", 2, (10, 20)), ("uniform", 2, (100, 200))], hyper=[2, 0, 1])
    assert np.allclose(api.table_prior(cube), [cube[2], 10 + 10 * cube[0], 100 + 100 * cube[1]])


def _table_variants():
    names = ["k_generate_live<1, 1>", "k_generate_live<2, 1>", "k_generate_live<4, 1>"]
    for dpl, nrows in ((1, 1), (1, 2), (1, 4), (2, 4), (4, 4)):
        names += [f"k_slice<{dpl}, {nrows}, false, 1, 0, 0, 1>", f"k_slice<{dpl}, {nrows}, true, 1, 0, 0, 1>"]
    for nrows, fw in ((1, 8), (1, 16), (2, 24)):
        names += [f"k_slice<1, {nrows}, false, 1, {fw}, 0, 1>"]
    return names


@pytest.mark.parametrize("with_source", [False, True])
def test_every_table_variant_compiles_for_gfx950(with_source):
    """the kernels the launchers of pc_sample.hip can choose for a run with a prior table (pc_launch_generate_live, pc_launch_slice,
    pc_launch_slice_fused), at every nDims class, through the run-time compiler: the built-ins alone and with a user's source"""
    api, lib = _lib()
    src = open(os.path.join(ROOT, "polychordlite_amd", "csrc", "pc_sample.hip")).read()
    for n in _table_variants():      # (the list is the launchers': every name is a variant their text spells out or their macros expand to)
        assert n.startswith("k_generate_live") or re.search(r"k_slice<DPL, NROWS, GR, 1, 0, 0, 1>|k_slice<1, NROWS, false, 1, FW, 0, 1>", src)
    h = api.source_create(GAUSS_SRC) if with_source else 0
    log = C.create_string_buffer(1 << 16)
    rc = lib.pchip_rtc_compile_check(h, b"gfx950", ";".join(_table_variants()).encode(), log, len(log), None)
    assert rc == 0, log.value.decode(errors="replace")
    if h:
        lib.pchip_source_destroy(h)


BAD_TABLES = [  # (entries, hyper, what the message must name)
    ([("uniform", (0, 1)), (11, (0, 1))], None, ("parameter 2", "unknown prior type")),
    ([("uniform", (0, 1)), ("power_uniform", (1, 2))], None, ("parameter 2", "needs 3")),
    ([("gaussian", (0.5,))], None, ("parameter 1", "needs 2")),
    ([("log_uniform", (0.0, 1.0))], None, ("parameter 1", "positive")),
    ([("uniform", (0, 1)), ("log_uniform", (1.0, -2.0))], None, ("parameter 2", "positive")),
    ([("power_uniform", (-1.0, 2.0, 2.0))], None, ("parameter 1", "positive")),
    ([("gaussian", (0.0, 0.0))], None, ("parameter 1", "sigma")),
    ([("uniform", (0, 1)), ("half_gaussian", (0.0, -1.0))], None, ("parameter 2", "sigma")),
    ([("sorted_gaussian", 1, (0.0, -1.0))], None, ("parameter 1", "sigma")),
    ([("exponential", (0.0,))], None, ("parameter 1", "rate")),
    ([("sorted_exponential", 1, (-2.0,))], None, ("parameter 1", "rate")),
    ([("sorted_uniform", 1, (0, 1)), ("uniform", 1, (0, 1)), ("sorted_uniform", 1, (0, 1))], None, ("parameter 3", "consecutive")),
    ([("uniform", (0, 1))] * 3, [0, 1, 1], ("parameter 3", "permutation")),
    ([("uniform", (0, 1))] * 3, [0, 1, 3], ("parameter 3", "permutation")),
]


def test_abi_and_validation():
    api, lib = _lib()
    assert lib.pchip_sizeof(b"prior") == C.sizeof(api.Prior) == 48
    assert C.sizeof(api.PriorEntry) == 40
    assert api.PATH_NAMES[20] == "device_prior" and api.PRIOR_TABLE == 2
    assert lib.pchip_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    assert "PCHIP_PRIOR_TABLE = 2" in hdr and "PCHIP_PATH_DEVICE_PRIOR = 20" in hdr
    for name, num in api.PRIOR_TYPES.items():
        assert re.search(r"PCHIP_PT_%s = %d\b" % (name.upper(), num), hdr), name
    for sym in ("polychord_hip_table_prior", "polychord_hip_set_table_prior", "pchip_prior_transform"):
        assert hasattr(lib, sym), sym
    # every validation error is caught by polychord_hip_set_table_prior already (no device needed), with a message naming the parameter
    for entries, hyper, words in BAD_TABLES:
        with pytest.raises(ValueError) as e:
            api.set_table_prior(entries, hyper)
        for w in words:
            assert w in str(e.value), (entries, str(e.value))
    # a good table clears the message; two sorted blocks of one type are told apart by their block number
    api.set_table_prior([("sorted_uniform", 1, (0, 1))] * 2 + [("sorted_uniform", 2, (0, 1))] * 2)
    assert lib.polychord_hip_last_error() is None
    th = api.table_prior([0.25, 0.5, 0.25, 0.5])
    assert np.allclose(th[:2], th[2:]) and th[0] < th[1]


def test_table_prior_object_is_the_host_function():
    from polychordlite_amd.pypolychord.device_likelihoods import TablePrior
    p = TablePrior([("gaussian", [0.5, 1.0]), ("exponential", [2.0]), ("uniform", [1.0, 3.0])])
    assert p.symbol == "polychord_hip_table_prior"
    th = p([0.5, 0.5, 0.5])
    assert np.allclose(th, [0.5, math.log(2.0) / 2.0, 2.0], rtol=1e-14)
    with pytest.raises(ValueError):
        TablePrior([("gaussian", [0.5, -1.0])])([0.5])


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _mixed20(b):
    """twenty entries that use all ten types; b tells the sorted blocks of one repetition from the next one's"""
    return ([("uniform", 1, (-1.0, 2.0)), ("log_uniform", 1, (1e-3, 5.0))] + [("sorted_uniform", 10 + b, (0.0, 10.0))] * 3 +
            [("power_uniform", 1, (1.0, 4.0, 2.0)), ("gaussian", 1, (0.3, 2.0))] + [("sorted_gaussian", 20 + b, (0.0, 1.0))] * 4 +
            [("half_gaussian", 1, (-1.0, 0.5)), ("exponential", 1, (0.7,))] + [("sorted_half_gaussian", 30 + b, (0.0, 2.0))] * 3 +
            [("power_uniform", 1, (2.0, 9.0, -1.5))] + [("sorted_exponential", 40 + b, (2.0,))] * 2 + [("gaussian", 1, (-3.0, 0.1))])


def _transform_cases():
    cases = []
    for kind, pp in REF_PARAMS.items():                    # nDims 3: every type on its own, the golden parameters
        cases.append((kind, [(kind, 1, pp[i]) for i in range(3)]))
    cases.append(("mixed20", _mixed20(0)))
    # nDims 70: members 60 .. 67 of one sorted block are lanes 60-63 of a lane's first coordinate and lanes 0-3 of its second
    cases.append(("mixed70", _mixed20(0) + _mixed20(1) + _mixed20(2) + [("sorted_gaussian", 99, (0.5, 1.5))] * 8 +
                  [("half_gaussian", 1, (0.0, 1.0)), ("exponential", 1, (3.0,))]))
    assert len(cases[-2][1]) == 20 and len(cases[-1][1]) == 70
    return cases


@pytest.mark.gpu
def test_device_transform_is_the_host_function(engine, golden):
    """pchip_prior_transform (the kernels' pc_table_theta) against polychord_hip_table_prior: the ten types, the golden cube point plus
    10 000 seeded points with coordinates within 1e-12 of 0 and 1, nDims 3 / 20 / 70 (a sorted block across index 63 / 64), identity and
    permuted order.  Bound 1e-9 relative to max(1, |theta|): the project's bound for device against host fp64 with transcendentals; the
    deviation seen is printed per case (it is rounding: orders below the bound)."""
    api = engine
    rng = np.random.default_rng(2024)
    worst = {}
    for name, entries in _transform_cases():
        D = len(entries)
        cubes = rng.random((10001, D))
        cubes[0, :] = np.resize(np.array(golden["ref_priors"]["cube"]), D)
        edge = rng.random((2000, D)) < 0.15                   # coordinates at the edges of the cube
        cubes[1:2001][edge] = rng.random(int(edge.sum())) * 1e-12
        edge = rng.random((2000, D)) < 0.15
        cubes[2001:4001][edge] = 1.0 - rng.random(int(edge.sum())) * 1e-12
        for order in ("identity", "permuted"):
            hyper = None if order == "identity" else rng.permutation(D).astype(np.int32)
            dev = api.prior_transform(entries, cubes, hyper)
            api.set_table_prior(entries, hyper)
            host = np.array([api.table_prior(c) for c in cubes])
            fin = np.isfinite(host)
            assert np.array_equal(fin, np.isfinite(dev)), (name, order)
            assert np.array_equal(host[~fin], dev[~fin]), (name, order)      # (+-huge of AS241 at p = 0 / 1 is the same constant on both sides)
            rel = np.abs(dev[fin] - host[fin]) / np.maximum(1.0, np.abs(host[fin]))
            print(f"device transform {name:22s} {order:9s}: max deviation {rel.max():.3e} relative to max(1, |theta|)")
            worst[name] = max(worst.get(name, 0.0), float(rel.max()))
            if not rel.max() < 1e-9:                         # (which point, which parameter: what the two sides made of it)
                full = np.where(fin, np.abs(dev - host) / np.maximum(1.0, np.abs(host)), 0.0)
                i, j = np.unravel_index(np.argmax(full), full.shape)
                print(f"worst: point {i}, parameter {j} {entries[j]}: host {host[i, j]!r}, device {dev[i, j]!r}, cube row {cubes[i].tolist()}")
            assert rel.max() < 1e-9, (name, order, rel.max())
    print("largest deviation per case:", {k: f"{v:.2e}" for k, v in worst.items()})


def _tramp(tmp_path):
    """oracle prior callback (cube, theta, n, ctx) -> the host function whose address is ctx"""
    so = tmp_path / "libtramp.so"
    if not so.exists():
        cpp = tmp_path / "tramp.cpp"
        cpp.write_text('extern "C" void tramp(double *c, double *t, int n, void *ctx) { ((void (*)(double *, double *, int))ctx)(c, t, n); }\n')
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", str(cpp), "-o", str(so)])
    return C.CDLL(str(so))


def _table_vs_oracle(api, tmp_path, kind, entries, nDer=0, hyper=None, grades=None, source=None, like_kw=None, **kw):
    """engine with the table on the device against pc_oracle_run with a callback prior that is polychord_hip_table_prior"""
    lib = api.load()
    D = len(entries)
    like_kw = like_kw or {}
    s = _settings(api, D, nDer, seed=5, **kw)
    keep = []
    if grades:
        keep.append(api.set_grades(s, *grades))
    h = api.source_create(source) if source else 0
    L, P, k1 = api.make_problem("source" if source else kind, D, nDer, source=h, prior_table=entries, hyper=hyper, **like_kw)
    g = api.run(s, L, P)
    assert g["path"]["device_prior"] > 0 and g["path"]["slice_wave"] > 0, g["path"]
    api.set_table_prior(entries, hyper)
    so = orc.settings(D, nDer, seed=5, **kw)
    if grades:
        keep.append(orc.set_grades(so, grades[0], grades[1]))
    Lo, Po, k2 = orc.make_problem("gaussian" if source else kind, D, **like_kw)
    if source:
        hl = _host_like(tmp_path, source, f"tp{D}_{nDer}")
        d = np.zeros(1)
        ctx = (C.c_void_p * 2)(d.ctypes.data, 0)
        Lo.kind = 0
        Lo.fn = C.cast(hl.host_logl, C.c_void_p)
        Lo.ctx = C.cast(ctx, C.c_void_p)
    tr = _tramp(tmp_path)
    Po.kind = 0
    Po.fn = C.cast(tr.tramp, C.c_void_p)
    Po.ctx = C.cast(lib.polychord_hip_table_prior, C.c_void_p)
    o = orc.run(so, Lo, Po)
    for k in ("ndead", "nlike", "niter", "nbatches", "ncluster", "ncluster_dead"):
        assert g[k] == o[k], (k, g[k], o[k])
    assert abs(g["logZ"] - o["logZ"]) < 1e-8, (g["logZ"], o["logZ"])
    rel = np.abs(g["dead"] - o["dead"]) / np.maximum(1.0, np.abs(o["dead"]))
    assert rel.max() < 1e-7, rel.max()
    if h:
        lib.pchip_source_destroy(h)
    return g


G8 = [("uniform", (0.0, 1.0)), ("log_uniform", (0.1, 2.0)), ("power_uniform", (0.2, 2.0, 2.0)), ("gaussian", (0.5, 0.3)),
      ("half_gaussian", (0.3, 0.3)), ("exponential", (2.0,)), ("sorted_uniform", 1, (0.0, 1.0)), ("sorted_uniform", 1, (0.0, 1.0))]
FIT20 = [("uniform", (0.0, 1.0))] + [("sorted_uniform", 2, (0.0, 1.0))] * 9 + [("uniform", (-0.5, 1.5))] * 10
G70 = [("gaussian", (0.5, 0.2))] * 60 + [("sorted_uniform", 3, (0.0, 1.0))] * 8 + [("half_gaussian", (0.4, 0.2))] * 2

ORACLE_CASES = {
    "gaussian8_all_unsorted_types_and_a_sorted_pair": dict(kind="gaussian", entries=G8, nDer=2, nlive=100, num_repeats=16, batch=16),
    "fitting20_sorted_block_of_nine": dict(kind="gaussian", entries=FIT20, nDer=1, nlive=100, num_repeats=40, batch=25),
    "rastrigin4_clustering_gaussian_priors": dict(kind="rastrigin", entries=[("gaussian", (0.0, 2.0))] * 4, nlive=200, num_repeats=8, batch=40, do_clustering=1),
    "twin_gaussian4_clustering_sorted_priors": dict(kind="twin_gaussian", entries=[("uniform", (-1.0, 1.0))] * 2 + [("sorted_gaussian", 1, (0.0, 0.5))] * 2,
                                                    nDer=1, nlive=200, num_repeats=8, batch=40, do_clustering=1),
    "two_grades_fast_parameters_first": dict(kind="gaussian", entries=[("gaussian", (0.5, 0.5))] * 3 + [("uniform", (0.0, 1.0)), ("exponential", (1.0,)), ("log_uniform", (0.1, 2.0))],
                                             hyper=[3, 4, 5, 0, 1, 2], grades=([3, 3], [2, 4]), nDer=1, nlive=100, num_repeats=6, batch=20),
    "source_likelihood_gaussian_priors": dict(kind="gaussian", entries=[("gaussian", (0.5, 0.5))] * 4, source=GAUSS_SRC, nDer=1, nlive=100, num_repeats=8, batch=16),
    "gaussian70_capped": dict(kind="gaussian", entries=G70, nlive=100, num_repeats=20, batch=16, max_ndead=300),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_table_walks_the_oracle(engine, tmp_path, case):
    """production mode (keyed draws, batch > 1): the same counters, log Z to 1e-8, dead rows to 1e-7 relative (test_source_walks_the_oracle's)"""
    _table_vs_oracle(engine, tmp_path, **ORACLE_CASES[case])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,D,nDer,lo,hi", [("gaussian", 20, 2, 0.0, 1.0), ("rastrigin", 8, 0, -5.12, 5.12), ("gaussian", 40, 1, -0.5, 1.5)])
def test_a_box_written_as_a_table_is_the_box(engine, kind, D, nDer, lo, hi):
    api = engine
    out = []
    for table in (False, True):
        s = _settings(api, D, nDer, nlive=150, num_repeats=2 * D, seed=11)
        if table:
            L, P, keep = api.make_problem(kind, D, nDer, prior_table=[("uniform", (lo, hi))] * D)
        else:
            L, P, keep = api.make_problem(kind, D, nDer, lo, hi)
        out.append(api.run(s, L, P))
    a, b = out
    for k in ("ndead", "nlike", "niter"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["logZ"] == b["logZ"]
    assert np.array_equal(a["dead"], b["dead"])
    assert b["path"]["device_prior"] == 0 and a["path"] == b["path"]


@pytest.mark.gpu
def test_reproduces_the_reference_binary(engine, golden):
    """the engine with the table on the device and sequential_rng = 1 (the reference's draw order) against the reference BINARY run
    through its own ini door under the RNG shim (tests/golden/ref_device_priors.json, tools/dev/gen_ref_device_priors.py): all ten
    types over the cases, two of them with clustering, one with the fast parameters listed first; ndead and nlike equal, log Z and its
    error to 1e-8 (as tests/test_sub_clustering.py::test_reproduces_the_reference_binary)"""
    api = engine
    fx = golden["ref_device_priors"]
    assert len(fx["door_proof"]) >= 1 and len(fx["cases"]) >= 5
    assert {p["type"] for c in fx["cases"] for p in c["params"]} == set(api.PRIOR_TYPES)
    assert sum(c["clustering"] for c in fx["cases"]) >= 2
    for c in fx["cases"]:
        D = c["nDims"]
        entries = [(p["type"], p["block"], p["par"]) for p in c["params"]]
        speeds = [p["speed"] for p in c["params"]]
        grades = sorted(set(speeds))                       # priors.f90:708-737: the cube lists the parameters grade by grade
        hyper, h = [0] * D, 0
        for g_ in grades:
            for i in range(D):
                if speeds[i] == g_:
                    hyper[i] = h; h += 1
        s = _settings(api, D, c["nDerived"], nlive=c["nlive"], num_repeats=max(c["num_repeats"], 1), seed=c["seed"],
                      do_clustering=c["clustering"], sequential_rng=1)
        keep = None
        if len(grades) > 1:                                # grade_frac > 1: the repeats per grade (generate.F90:303-309)
            keep = api.set_grades(s, [speeds.count(g_) for g_ in grades], [int(v) for v in c["grade_frac"].split()])
        L, P, k2 = api.make_problem(c["like"], D, c["nDerived"], prior_table=entries, hyper=hyper)
        g = api.run(s, L, P)
        assert g["path"]["device_prior"] > 0, c["name"]
        assert (g["ndead"], g["nlike"]) == (c["ndead"], c["nlike"]), (c["name"], g["ndead"], c["ndead"], g["nlike"], c["nlike"])
        if len(grades) > 1:                                # .stats lists RTI%nlike per grade
            assert g["nlike_grade"][:len(grades)] == c["nlike_grades"], (c["name"], g["nlike_grade"], c["nlike_grades"])
        assert abs(g["logZ"] - c["logZ"]) < 1e-8 and abs(g["logZerr"] - c["logZerr"]) < 1e-8, (c["name"], g["logZ"], c["logZ"], g["logZerr"], c["logZerr"])
        assert g["ncluster_dead"] == c["ncluster_dead"], (c["name"], g["ncluster_dead"], c["ncluster_dead"])


def _evidence_check(api, entries, D, truth, num_repeats):
    zs, vs = [], []
    for seed in range(1, 9):
        s = _settings(api, D, 0, nlive=200, num_repeats=num_repeats, seed=seed)
        L, P, keep = api.make_problem("gaussian", D, 0, mu=0.5, sigma=0.1, prior_table=entries)
        g = api.run(s, L, P)
        assert g["path"]["device_prior"] > 0
        zs.append(g["logZ"]); vs.append(g["varlogZ"])
    mean, var = float(np.mean(zs)), max(float(np.var(zs, ddof=1)), float(np.mean(vs)))
    print(f"log Z over eight seeds: mean {mean:.4f} (truth {truth:.4f}), sample variance {np.var(zs, ddof=1):.4f}, mean reported variance {np.mean(vs):.4f}")
    assert abs(mean - truth) < 3.0 * math.sqrt(var / 8.0), (mean, truth, var)


@pytest.mark.gpu
def test_analytic_evidence_gaussian_priors(engine):
    """10-D Gaussian likelihood (0.5, 0.1) under gaussian priors N(0.5, 1): log Z = -(D / 2) log(2 pi (0.1^2 + 1^2)) = -9.2391"""
    D = 10
    _evidence_check(engine, [("gaussian", (0.5, 1.0))] * D, D, -(D / 2.0) * math.log(2.0 * math.pi * (0.01 + 1.0)), 2 * D)


@pytest.mark.gpu
def test_analytic_evidence_sorted_uniform(engine):
    """6-D, the same likelihood under one sorted_uniform (0, 1) block of six: log Z = 0 up to 1e-6 (a symmetric likelihood integrates to
    the same value over the ordered simplex, whose prior density is 6!)"""
    D = 6
    _evidence_check(engine, [("sorted_uniform", 1, (0.0, 1.0))] * D, D, 0.0, 2 * D)


def _stats_logz(path):
    m = re.search(r"log\(Z\)\s*=\s*([-+0-9.Ee]+)\s*\+/-\s*([-+0-9.Ee]+)", open(path).read())      # (the global evidence: the first line with numbers)
    return float(m.group(1)), float(m.group(2))


@pytest.mark.gpu
def test_cli_runs_a_gaussian_prior_ini_on_the_device(engine, tmp_path):
    """tools/polychord_hip_cli on configs/gaussian_gaussian_prior.ini with the built-in Gaussian: the header line, and a .stats within
    4 sigma of -(20 / 2) log(2 pi 1.01); with option device_prior = 0 the line is absent (the host prior, as before)"""
    cli = os.path.join(ROOT, "tools", "polychord_hip_cli")
    ini = (tmp_path / "g.ini")
    ini.write_text(open(os.path.join(ROOT, "configs", "gaussian_gaussian_prior.ini")).read().replace("nlive = 500", "nlive = 200"))
    truth = -10.0 * math.log(2.0 * math.pi * 1.01)
    for args, expect in (([], True), (["device_prior=0"], False)):
        r = subprocess.run([cli, str(ini), "gaussian"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
        assert ("prior table evaluated on the device" in r.stdout) == expect, r.stdout
        z, e = _stats_logz(tmp_path / "chains" / "gaussian_gaussian_prior.stats")
        assert abs(z - truth) < 4.0 * e, (z, e, truth)


@pytest.mark.gpu
def test_pypolychord_run_with_a_table_prior(engine, tmp_path):
    from polychordlite_amd import pypolychord
    from polychordlite_amd.pypolychord.device_likelihoods import Gaussian, TablePrior
    D = 6
    from polychordlite_amd.pypolychord.output import PolyChordOutput
    pypolychord.run(Gaussian(0.5, 0.1), D, prior=TablePrior([("gaussian", (0.5, 1.0))] * D), nlive=200, num_repeats=2 * D, seed=3,
                    base_dir=str(tmp_path / "chains"), file_root="tp", feedback=0, do_clustering=False, write_resume=False, read_resume=False,
                    posteriors=False, equals=False, cluster_posteriors=False, write_live=False, write_prior=False)
    out = PolyChordOutput(str(tmp_path / "chains"), "tp")      # (the same kind of result as any run: <root>.stats)
    truth = -(D / 2.0) * math.log(2.0 * math.pi * 1.01)
    assert abs(out.logZ - truth) < 4.0 * out.logZerr, (out.logZ, out.logZerr, truth)


@pytest.mark.gpu
def test_run_repeats_with_a_table_are_the_solo_runs(engine):
    api = engine
    from polychordlite_amd import repeats
    D = 6
    entries = [("gaussian", (0.5, 1.0))] * 3 + [("sorted_uniform", 1, (0.0, 1.0))] * 3
    s = _settings(api, D, 0, nlive=100, num_repeats=12)
    L, P, keep = api.make_problem("gaussian", D, 0, prior_table=entries)
    merged, runs = repeats.run_repeats(s, L, P, [3, 4, 5])
    for seed, r in zip([3, 4, 5], runs):
        s1 = _settings(api, D, 0, nlive=100, num_repeats=12, seed=seed)
        solo = api.run(s1, L, P)
        assert solo["path"]["device_prior"] > 0
        assert r["ndead"] == solo["ndead"] and r["nlike"] == solo["nlike"] and r["logZ"] == solo["logZ"]
        assert np.array_equal(np.asarray(r["dead"]), solo["dead"])


@pytest.mark.gpu
def test_a_bad_table_fails_the_run_with_its_message(engine, capfd):
    api = engine
    lib = api.load()
    for entries, hyper, words in BAD_TABLES:
        D = len(entries)
        s = _settings(api, D, 0, nlive=50, num_repeats=4)
        L, P, keep = api.make_problem("gaussian", D, 0, prior_table=entries, hyper=hyper)
        r = api.Result()
        assert lib.pchip_run(C.byref(s), C.byref(L), C.byref(P), C.byref(r)) == 1
        err = capfd.readouterr().err
        for w in words:
            assert w in err, (entries, err)
