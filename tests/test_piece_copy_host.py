"""The piece copy (strainscan_amd/csrc/ss_piece_copy.h) on the host: tests/piece_copy_check.cpp, a stand-alone program (g++) under
AddressSanitizer + UBSan, plays the sixteen lanes of gather_kernel, record_gather_kernel and the two join_kernels over host buffers
for every alignment of source and destination and compares with a byte-by-byte model.  What the kernels do with it on the device is
tests/test_select_gpu.py's, test_pairs_gpu.py's, test_bam_pairs_gpu.py's and test_bam_select_gpu.py's."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_piece_copy_sweeps_sanitized(tmp_path):
    """Both sweeps, exhaustive: the single-source copy (D mod 16 x length 0..49 + the trailing byte x every source position of a
    block of 16 and of 64 bytes x 1, 2, 13 copies; the same without the trailing byte) and the two-source join (both lengths 0..18
    x D mod 16 x blocks of 16 and 64 bytes, the line at the start, inside, at the end x the 'N' alone / the 'N' and the newline).
    Guard bytes around every span stay untouched; a load outside a source block, or an undefined shift, stops the program."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "piece_copy_check"
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(REPO, "strainscan_amd", "csrc"), os.path.join(REPO, "tests", "piece_copy_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "piece_copy_check ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"(\d+) single-source copies, (\d+) joins", r.stdout)
    # 2 block sizes x 16 offsets x 3 copy counts x the (length, position) pairs that fit; 2 forms x 19 x 19 lengths x 16 offsets x sources
    assert int(m.group(1)) > 150000 and int(m.group(2)) > 150000
