"""Sub-dimension clustering on the CPU side: the ini file's `*` parameter marker (ini.f90:389-393) and the list it makes,
settings%sub_clustering_dimensions = pack(hypercube_indices, sub_cluster) (priors.f90:740-741) -- hypercube indices, in
parameter order, 0-based here."""
import ctypes as C
import os
import subprocess

import pytest

from polychordlite_amd import _ctypes_api as api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "nlive = 50\nnum_repeats = 4\ndo_clustering = T\nfeedback = 0\nwrite_paramnames = T\nbase_dir = chains\nfile_root = sc\n"


def sub_list(tmp_path, params):
    ini = tmp_path / "p.ini"
    ini.write_text(HEAD + "".join(f"P : {name} | {name} | {speed} | uniform | 1 | -1 1\n" for name, speed in params))
    lib = api.load()
    buf = (C.c_int * 16)()
    n = lib.polychord_hip_ini_sub_clustering(str(ini).encode(), buf, 16)
    return n, list(buf[:min(n, 16)])


def test_trailing_marker(tmp_path):
    assert sub_list(tmp_path, [("x1*", 1), ("x2", 1), ("x3", 1)]) == (1, [0])
    assert sub_list(tmp_path, [("x1", 1), ("x2", 1), ("x3*", 1)]) == (1, [2])


def test_marker_inside_a_name_cuts_it_and_flags_it(tmp_path):
    assert sub_list(tmp_path, [("a", 1), ("b*extra", 1)]) == (1, [1])
    assert sub_list(tmp_path, [("a**", 1), ("b", 1), ("c*d*", 1)]) == (2, [0, 2])


def test_hypercube_indices_in_parameter_order(tmp_path):
    # a speed 2 marked, b speed 1, c speed 1 marked: hypercube b -> 0, c -> 1, a -> 2; the list follows the FILE order: [2, 1]
    assert sub_list(tmp_path, [("a*", 2), ("b", 1), ("c*", 1)]) == (2, [2, 1])


def test_no_marker_no_list(tmp_path):
    assert sub_list(tmp_path, [("x1", 1), ("x2", 1)]) == (0, [])


def test_count_beyond_the_capacity(tmp_path):
    ini = tmp_path / "p.ini"
    ini.write_text(HEAD + "".join(f"P : x{i}* | x | 1 | uniform | 1 | 0 1\n" for i in range(5)))
    buf = (C.c_int * 2)(-7, -7)
    assert api.load().polychord_hip_ini_sub_clustering(str(ini).encode(), buf, 2) == 5 and list(buf) == [0, 1]


def test_settings_mirror_and_path_names():
    lib = api.load()
    s = api.Settings()
    lib.pchip_settings_default(C.byref(s), 4, 0)
    assert s.n_sub_cluster == 0 and not s.sub_cluster_dims              # plain clustering by default
    keep = api.set_sub_clustering(s, [3, 1])
    assert s.n_sub_cluster == 2 and [s.sub_cluster_dims[0], s.sub_cluster_dims[1]] == [3, 1] and keep.tolist() == [3, 1]
    assert api.PATH_NAMES.index("subcluster_passes") == 17 and api.PATH_NAMES.index("subcluster_splits") == 18
    src = open(os.path.join(ROOT, "include", "polychord_hip.h")).read()
    assert "PCHIP_PATH_SUBCLUSTER_PASSES = 17" in src and "PCHIP_PATH_SUBCLUSTER_SPLITS = 18" in src and "PCHIP_PATH_COUNT = 24" in src


def test_pypolychord_keyword_and_setting():
    from polychordlite_amd import pypolychord
    assert pypolychord.PolyChordSettings(4, 0).sub_clustering_dimensions == []
    assert pypolychord.PolyChordSettings(4, 0, sub_clustering_dimensions=(0, 2)).sub_clustering_dimensions == [0, 2]


def test_cli_paramnames_without_the_marker(tmp_path):
    """the .paramnames file the ini front end writes before the run carries the names cut at the `*` (the run itself needs a GPU:
    without one the CLI stops after writing the file)"""
    cli = os.path.join(ROOT, "tools", "polychord_hip_cli")
    if not os.path.exists(cli):
        pytest.fail("tools/polychord_hip_cli is not built")
    ini = tmp_path / "m.ini"
    ini.write_text(HEAD.replace("nlive = 50", "nlive = 40") + "P : x1* | x_1 | 1 | uniform | 1 | -1 1\nP : x2 | x_2 | 1 | uniform | 1 | -1 1\n"
                   "P : y*z | y | 1 | uniform | 1 | -1 1\n")
    subprocess.run([cli, str(ini), "twin_gaussian"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    names = [l.split()[0] for l in (tmp_path / "chains" / "sc.paramnames").read_text().splitlines()]
    assert names == ["x1", "x2", "y"]
