"""The chunked scan the toner, the compressor and the normaliser share (csrc/ptts_scan.h): its partition for every frame
size and its three steps against a serial run, as a stand-alone program under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_partition_and_scheme_under_host_sanitizer(tmp_path):
    """every n in 1 .. 8192 at 1024 threads: chunk, threads, the ranges' tiling and the step count; a scalar linear and a
    scalar max-plus recurrence through the host walker against the serial run at n = 1, 2, 63, 1023, 1024, 1025, 8191 and
    8192 on exact-size heap buffers.  The program itself holds the bounds"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "scan_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "scan_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    m = re.fullmatch(r"ok 8192 sizes linear (\S+) max-plus (\S+)", r.stdout.strip())
    assert m, r.stdout
    assert 0.0 <= float(m.group(1)) <= 1e-11 and 0.0 <= float(m.group(2)) <= 1e-12
