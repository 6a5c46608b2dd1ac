"""K16 (the pile admission on the device) on a machine without a GPU: the bodies of tests/test_zz_gpu_admit.py with
nextdenovo_amd.overlap bound to the interpreted library (see test_simt_overlap.py and tests/simt), once more with the lanes of a
wavefront run highest first -- "first occurrence" must not depend on lane order."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_zz_gpu_admit as GA  # noqa: E402  (gpu-marked as a module; its functions are called from here)
from test_simt_overlap import interpreted, simt_libs  # noqa: E402,F401  (fixtures)


def test_stage_fixture_equals_the_host_routine_and_the_loop(interpreted):
    GA.test_stage_fixture_equals_the_host_routine_and_the_loop()


def test_random_record_streams_regular_and_irregular(interpreted):
    GA.test_random_record_streams_regular_and_irregular()


@pytest.mark.parametrize("descending", [0, 1], ids=["lanes-up", "lanes-down"])
@pytest.mark.parametrize("forced", [False, True], ids=["lds", "forced-table"])
def test_chunk_and_table_edges(interpreted, forced, descending, monkeypatch):
    for lib in interpreted:
        lib.simt_set_lane_order(descending)
    try:
        for case in GA._EDGES:
            GA.test_chunk_and_table_edges(case, forced, monkeypatch)
    finally:
        for lib in interpreted:
            lib.simt_set_lane_order(0)


def test_the_edges_are_the_edges(interpreted):
    GA.test_the_edges_are_the_edges()


@pytest.mark.parametrize("case", GA._DECLINE, ids=[c[0] for c in GA._DECLINE])
def test_irregular_streams_decline_to_the_host_routine(interpreted, case):
    GA.test_irregular_streams_decline_to_the_host_routine(case)


def test_sort_piles_equals_sort_then_assemble(interpreted, monkeypatch):
    GA.test_sort_piles_equals_sort_then_assemble(monkeypatch)


def test_shard_piles_with_and_without_the_device_admission(interpreted, tmp_path, monkeypatch):
    GA.test_shard_piles_with_and_without_the_device_admission(tmp_path, monkeypatch)


def test_interface_empty_input_and_the_host_flag(interpreted):
    GA.test_interface_empty_input_and_the_host_flag()


def test_the_new_entry_points_are_exported_and_nothing_else_is():
    """exports_overlap.map lets through `ndgpu_*` (and ksw_extd2_sse): ndgpu_admit_piles and ndgpu_ovl_sort_piles are exported because
    the header declares them under those names, and the admission adds no other dynamic symbol -- test_abi.py holds the exported set
    against the header's declarations; here: the two names are there, and every exported name is an ABI name."""
    from nextdenovo_amd import build
    out = subprocess.run(["nm", "-D", "--defined-only", build.OVL_LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"ndgpu_admit_piles", "ndgpu_ovl_sort_piles"} <= names
    assert all(n.startswith(("ndgpu_", "__hip_cuid_")) or n == "ksw_extd2_sse" for n in names), sorted(names)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ndgpu_overlap.h")).read()
    assert "ndgpu_admit_piles(" in header and "ndgpu_ovl_sort_piles(" in header and "ndgpu_ovl_admit_stats" in header
