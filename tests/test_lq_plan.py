"""The two planners of the phases behind the main phase (csrc/nd_lqplan.h) on their own: pure arithmetic, no device and no library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_lq_and_poa_planners_under_sanitizers(tmp_path):
    """cut_lq_jobs / next_poa_slice in a stand-alone program built with -fsanitize=address,undefined (tests/csrc/lq_plan_check.cpp)
    against the loops run_lq and run_poa had inline, restated there: 2,000 seeded draws each, every field of every job and every
    slice -- rounds of 1..200 regions of 0..4,000 columns with runs of empty ones, 0..30 rows with a job, jobs of 1, 40 and 192
    columns; POA rounds of 1..80 problems of 1..2 x budget cells with rows around 65,535 -- five fixed cases have their answers
    written out, and neither sanitizer reports anything."""
    exe = str(tmp_path / "lq_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "nextdenovo_amd", "csrc"), "-o", exe, os.path.join(HERE, "csrc", "lq_plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stderr == b"" and out.stdout == b"ok\n", (out.stdout[-2000:], out.stderr[-2000:])
