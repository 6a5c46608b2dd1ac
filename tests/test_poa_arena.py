"""The arena arithmetic of a resident POA graph (csrc/nd_lqplan.h) on its own: pure arithmetic, no device and no library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_poa_arena_layout_under_sanitizers(tmp_path):
    """poa_arena_layout / poa_arena_offsets in a stand-alone program built with -fsanitize=address,undefined
    (tests/csrc/poa_arena_check.cpp): offsets monotone, 8-byte aligned and disjoint, every part's size against the rule written out
    there, for bounds 1..299 and up to 65,535; the byte totals of bounds 1, 2 and 65,535 written out; 0 and 65,536 refused with
    nothing written; a batch's running offsets, and the 64-bit total of 10^6 problems."""
    exe = str(tmp_path / "poa_arena_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "nextdenovo_amd", "csrc"), "-o", exe, os.path.join(HERE, "csrc", "poa_arena_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stderr == b"" and out.stdout == b"ok\n", (out.stdout[-2000:], out.stderr[-2000:])
