"""Record sets and K18 (their stable split) on a machine without a GPU: the bodies of tests/test_zz_gpu_recset.py with
nextdenovo_amd.overlap bound to the interpreted library (see test_simt_overlap.py and tests/simt); the split cases once with the lanes
of a wavefront run lowest first and once highest first -- a record's row must not depend on the order lanes run in."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_zz_gpu_recset as GR  # noqa: E402  (gpu-marked as a module; its functions are called from here)
from test_simt_overlap import interpreted, simt_libs  # noqa: E402,F401  (fixtures)


@pytest.fixture(params=[0, 1], ids=["lanes-up", "lanes-down"])
def lanes(interpreted, request):
    for lib in interpreted:
        lib.simt_set_lane_order(request.param)
    yield request.param
    for lib in interpreted:
        lib.simt_set_lane_order(0)


def test_map_dev_equals_map_on_the_stage_fixture(interpreted):
    GR.test_map_dev_equals_map_on_the_stage_fixture()


@pytest.mark.parametrize("n_lanes", [1, 2])
def test_map_dev_in_several_batches(interpreted, n_lanes, monkeypatch):
    GR.test_map_dev_in_several_batches(n_lanes, monkeypatch)


def test_map_dev_of_an_empty_query_set(interpreted):
    GR.test_map_dev_of_an_empty_query_set()


def test_map_dev_mode3(interpreted):
    GR.check_map_dev_mode3(24)   # (the first reads of the set: the extension kernels are slow under the interpreter)


def test_map_dev_refuses_step2_options(interpreted):
    GR.test_map_dev_refuses_step2_options()


def test_split_sizes_around_the_wavefront_and_the_tile(lanes):
    for n in GR.SPLIT_N:
        for n_files in GR.SPLIT_FILES:
            GR.test_split_sizes_around_the_wavefront_and_the_tile(n, n_files)


def test_split_file_patterns(lanes):
    for case in GR._PATTERNS:
        GR.test_split_file_patterns(case)


def test_the_split_cases_are_what_they_claim():
    GR.test_the_split_cases_are_what_they_claim()


def test_split_refuses_records_that_belong_to_no_file(lanes):
    GR.test_split_refuses_records_that_belong_to_no_file()


def test_split_of_more_than_256_files_is_the_callers(interpreted):
    GR.test_split_of_more_than_256_files_is_the_callers()


@pytest.mark.parametrize("n", [0, 1, 65])
def test_upload_then_download_is_the_identity(interpreted, n):
    GR.test_upload_then_download_is_the_identity(n)


def test_concat_of_the_fixtures_sets_equals_concatenate(interpreted):
    GR.test_concat_of_the_fixtures_sets_equals_concatenate()


@pytest.mark.parametrize("hq", [False, True], ids=["plain", "H"])
def test_sorts_over_sets_arrays_and_mixed_lists(interpreted, hq, monkeypatch):
    GR.test_sorts_over_sets_arrays_and_mixed_lists(hq, monkeypatch)


def test_sorts_over_sets_in_seed_ranges(interpreted, monkeypatch):
    GR.test_sorts_over_sets_in_seed_ranges(monkeypatch)


@pytest.mark.parametrize("admit", [False, True], ids=["host-admission", "device-admission"])
def test_shard_piles_with_and_without_the_device_records(interpreted, admit, tmp_path, monkeypatch):
    GR.test_shard_piles_with_and_without_the_device_records(admit, tmp_path, monkeypatch)


def test_grouped_jobs_are_cut_on_the_device(interpreted, monkeypatch):
    GR.test_grouped_jobs_are_cut_on_the_device(monkeypatch)


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
def test_fused_stage_with_the_device_records_writes_the_golden_files(interpreted, keep, tmp_path, monkeypatch):
    GR.test_fused_stage_with_the_device_records_writes_the_golden_files(keep, tmp_path, monkeypatch)


def test_fused_stage_past_the_budget_falls_back_to_arrays(interpreted, tmp_path, monkeypatch):
    GR.test_fused_stage_past_the_budget_falls_back_to_arrays(tmp_path, monkeypatch)


def test_close_twice_and_use_after_close(interpreted):
    GR.test_close_twice_and_use_after_close()


def test_trim_leaves_a_live_set_alone(interpreted):
    GR.test_trim_leaves_a_live_set_alone()


def test_a_failed_sort_leaves_no_set_behind(interpreted, tmp_path, monkeypatch):
    GR.test_a_failed_sort_leaves_no_set_behind(tmp_path, monkeypatch)


def test_the_new_entry_points_are_exported_and_declared():
    GR.test_the_new_entry_points_are_exported_and_declared()
