"""The rules of the AD-Census family (csrc/adcensus_rules.h) under AddressSanitizer and UBSan, without a GPU, HIP or
Python in the process: csrc/adcensus_selftest.hip compiled as plain C++ with tools/adcensus_selftest_main.cpp, a program
with its own main that walks every host selftest over its shape lists.  The build is -Wall -Wextra -Werror, so it is
also the proof that the rule header needs nothing but g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_selftests_hold_under_the_sanitizers(tmp_path):
    exe = tmp_path / "adcensus_selftest"
    cmd = [os.environ.get("CXX", "g++")] + FLAGS + ["-x", "c++", os.path.join(ROOT, "stereo_match_traditional_amd", "csrc", "adcensus_selftest.hip"),
                                                    os.path.join(ROOT, "tools", "adcensus_selftest_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("SMT_MAPS_TAPER", None)                            # the driver sets the forced tapers itself
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok: 0 failures" in r.stdout
