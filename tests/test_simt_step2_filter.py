"""K23 (the step-2 writer on the device) on a machine without a GPU: the bodies of tests/test_zz_gpu_step2_filter.py with
nextdenovo_amd.overlap bound to the interpreted library (see test_simt_overlap.py and tests/simt); the directed streams once more
with the lanes of a wavefront run highest first -- a ballot, a prefix or a running maximum must not depend on the order lanes run
in.  Of the command-line cases the two that take seconds under the interpreter run here, all of them run on the GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_zz_gpu_step2_filter as GF  # noqa: E402  (gpu-marked as a module; its functions are called from here)
from test_simt_overlap import interpreted, simt_libs  # noqa: E402,F401  (fixtures)


@pytest.fixture(params=[0, 1], ids=["lanes-up", "lanes-down"])
def lanes(interpreted, request):
    for lib in interpreted:
        lib.simt_set_lane_order(request.param)
    yield request.param
    for lib in interpreted:
        lib.simt_set_lane_order(0)


@pytest.mark.parametrize("way", ["one", "ones", "257", "mixed"])
@pytest.mark.parametrize("p_double", GF.FRACTIONS)
@pytest.mark.parametrize("params", GF.PARAMS, ids=["r40", "r300", "r9", "r1200"])
def test_random_streams(interpreted, oracle_lib, params, p_double, way):
    """(A device call costs 27 ms under the interpreter whatever its size: in calls of 1 the 9,000-record stream alone would take four
    minutes.  The 400-record stream runs in calls of 1 throughout, the longer ones for their first 300 records and the rest in one
    call; the GPU file feeds every stream record by record to the end.)"""
    if way == "ones" and params[2] > 400:
        way = "ones-300"
    GF.check_random(oracle_lib, params, p_double, way)


def test_record_counts_against_a_carried_prev(lanes, oracle_lib):
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257):
        GF.check_record_counts(oracle_lib, n)


def test_one_read_in_k_records(lanes, oracle_lib):
    for k in (1, 2, 64, 65, 300):
        for as_target in (False, True):
            GF.check_one_read(oracle_lib, k, as_target)


def test_chains(lanes, oracle_lib, monkeypatch):
    monkeypatch.delenv("NDGPU_S2_MAX_ROUNDS", raising=False)
    GF.check_chain(oracle_lib, 1, True, monkeypatch)
    GF.check_chain(oracle_lib, 5, True, monkeypatch)
    GF.check_chain(oracle_lib, 40, False, monkeypatch)
    GF.check_chain(oracle_lib, 40, True, monkeypatch, cap=64)


def test_declined_calls_run_the_host_loop(lanes, oracle_lib, monkeypatch):
    for which in (0, 1, 5):
        GF.check_decline(oracle_lib, which, monkeypatch)


def test_state_carried_across_calls(lanes, oracle_lib):
    GF.check_across_calls(oracle_lib)


def test_interval_union(lanes, oracle_lib):
    for name in GF.UNIONS:
        GF.check_union(oracle_lib, name)


def test_encoder_fields_names_and_dropped_records(lanes, oracle_lib):
    GF.check_encoder(oracle_lib)


def test_bad_flags_write_nothing(interpreted):
    GF.check_flags()


@pytest.mark.parametrize("tag", ["ont", "hifi.self"])
def test_step2_command_with_the_device_writer(interpreted, tag, tmp_path, monkeypatch):
    argv = [c[1] for c in GF._all_cases() if c[0] == tag][0]
    GF.check_command(tag, argv, tmp_path, monkeypatch)
