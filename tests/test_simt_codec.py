"""K17 (the `.ovl` codec on the device) on a machine without a GPU: the bodies of tests/test_zz_gpu_codec.py with nextdenovo_amd.overlap
bound to the interpreted library (see test_simt_overlap.py and tests/simt); the directed streams once more with the lanes of a
wavefront run highest first -- a prefix must not depend on the order lanes run in.  The nextcorrect command line runs the consensus
and stays with the GPU suite."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_zz_gpu_codec as GC  # noqa: E402  (gpu-marked as a module; its functions are called from here)
from test_simt_overlap import interpreted, simt_libs  # noqa: E402,F401  (fixtures)


@pytest.fixture(params=[0, 1], ids=["lanes-up", "lanes-down"])
def lanes(interpreted, request):
    for lib in interpreted:
        lib.simt_set_lane_order(request.param)
    yield request.param
    for lib in interpreted:
        lib.simt_set_lane_order(0)


def test_golden_files_decode_to_the_numpy_decoder_and_encode_back(interpreted):
    GC.test_golden_files_decode_to_the_numpy_decoder_and_encode_back()


def test_golden_files_in_one_call_equal_each_alone(interpreted):
    GC.test_golden_files_in_one_call_equal_each_alone()


def test_directed_decode_streams(lanes):
    GC.test_values_of_one_to_five_bytes_in_every_field()
    for boundary in (GC.LANE, GC.ITER, GC.TILE, 2 * GC.TILE):
        for nbytes in (2, 3, 4, 5):
            GC.test_a_value_straddling_a_boundary(boundary, nbytes)
    GC.test_flags_set_and_clear_next_to_each_other()
    GC.test_empty_short_and_partial_files()
    GC.test_three_files_the_middle_one_with_a_partial_tail()
    for n in (1, 63, 64, 65, GC.BLOCK - 1, GC.BLOCK, GC.BLOCK + 1):
        GC.test_record_counts_around_the_wavefront_and_the_block(n)
    for delta in (-1, 0, 1):
        GC.test_byte_counts_around_the_tile(delta)


def test_random_byte_strings_equal_the_host_loop(interpreted):
    GC.test_random_byte_strings_equal_the_host_loop()


def test_directed_encode(lanes):
    for n in (0, 1, 63, 64, 65, 129):
        for prev in ((0, 0), (70000, 3)):
            GC.test_encode_record_counts(n, prev)
    GC.test_encode_field_edges()
    GC.test_two_encode_calls_chained_through_prev_equal_one()


@pytest.mark.parametrize("hq", [False, True], ids=["plain", "H"])
def test_sort_images_equals_decode_sort_encode(interpreted, hq, monkeypatch):
    GC.test_sort_images_equals_decode_sort_encode(hq, monkeypatch)


def test_sort_images_decides_its_form_once(interpreted, monkeypatch):
    GC.test_sort_images_decides_its_form_once(monkeypatch)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_admit_piles_image_on_the_stage_fixture(interpreted, k):
    GC.test_admit_piles_image_on_the_stage_fixture(k)


def test_admit_piles_image_on_a_stream_that_declines(interpreted):
    GC.test_admit_piles_image_on_a_stream_that_declines()


@pytest.mark.parametrize("codec", [False, True], ids=["host-codec", "device-codec"])
def test_ovl_sort_command_writes_the_golden_files(interpreted, codec, tmp_path, monkeypatch):
    GC.test_ovl_sort_command_writes_the_golden_files(codec, tmp_path, monkeypatch)


def test_the_new_entry_points_are_exported_and_declared():
    GC.test_the_new_entry_points_are_exported_and_declared()


def test_the_host_flag_gives_the_same_answers_without_device_time(interpreted):
    GC.test_the_host_flag_gives_the_same_answers_without_device_time()


def test_argument_errors_leave_the_out_pointers_null(interpreted):
    GC.test_argument_errors_leave_the_out_pointers_null()
