"""The sub-batch planner of ndgpu_correct_piles_stream (csrc/nd_subplan.h) on its own: pure arithmetic, no device and no library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sub_batch_planner_under_sanitizers(tmp_path):
    """plan_sub_batches / round_weights in a stand-alone program built with -fsanitize=address,undefined (tests/csrc/sub_plan_check.cpp):
    2,000 seeded draws -- 1..3,000 piles of 1,000..3,000,000 columns sorted descending, 1..8 contexts, one or two rounds, caps of 384
    piles and 900,000,000 columns -- keep the cuts' properties (from 0 to n, strictly rising; no piece over the pile cap; no piece of
    several piles over the column cap; exactly contexts x rounds pieces where neither cap nor floor bites), three fixed cases have
    the cuts written out, and neither sanitizer reports anything."""
    exe = str(tmp_path / "sub_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "nextdenovo_amd", "csrc"), "-o", exe, os.path.join(HERE, "csrc", "sub_plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stderr == b"" and out.stdout == b"ok\n", (out.stdout[-2000:], out.stderr[-2000:])
