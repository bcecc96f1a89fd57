"""The counting kernel's 32-bit endpoint test (gsn_amd/csrc/count_core.h: endpoint_local, endpoint_width) on the host: the stand-alone
program tests/endpoint_check_harness.cpp, built with the address and undefined-behaviour sanitizers, runs every combination of
lo / hi in {0, 1, 37, 64} and x in {INT64_MIN, -1, 0, lo - 1, lo, hi - 1, hi, 2^31, 2^32, 2^32 + lo, INT64_MAX} against the plain 64-bit
comparison; its printed lines are checked once more here in Python integers."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_equals_the_64_bit_comparison_under_sanitizers():
    exe = os.path.join(REPO, "tests", "_build", "endpoint_check_harness")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(REPO, "tests", "endpoint_check_harness.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    seen = set()
    for line in r.stdout.split("\n"):
        if not line:
            continue
        lo, hi, x, inside, off = (int(t) for t in line.split())
        seen.add((lo, hi, x))
        assert bool(inside) == (lo <= x < hi), line
        assert off == (x - lo if inside else 0), line
    bounds = (0, 1, 37, 64)
    want = {(lo, hi, x) for lo in bounds for hi in bounds
            for x in (-2 ** 63, -1, 0, lo - 1, lo, hi - 1, hi, 2 ** 31, 2 ** 32, 2 ** 32 + lo, 2 ** 63 - 1)}
    assert seen == want and "176 combinations, 0 wrong" in r.stderr
