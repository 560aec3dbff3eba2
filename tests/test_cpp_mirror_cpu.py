"""The C++ host mirror (host/smt_host.hpp) against a contract stub of the C ABI, on the CPU under AddressSanitizer.

tests/cpp_mirror/smt_contract_stub.cpp implements the entries of include/smt.h the mirror calls with malloc'ed
"device" memory of exactly the byte counts asked for; it reads every input extent the header grants an entry and fills
every output extent with a pattern.  tests/cpp_mirror/mirror_contract_main.cpp calls every public function and method
of the mirror with exact-size heap buffers and asserts the logged entry and arguments, the pattern in every output
byte, untouched inputs, list semantics, and -- with each entry failing in turn -- a std::runtime_error and nothing left
allocated.  A stand-alone sanitized program: nothing is loaded into Python and no GPU is involved."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_mirror")
HPP = os.path.join(ROOT, "stereo_match_traditional_amd", "host", "smt_host.hpp")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")

FAMILIES = ["devbuf", "adcensus", "multi", "crossarm", "scanline", "post", "cblsm", "crossagg", "sad", "ncc", "asw", "filters",
            "image", "pipeline"]

# mirror functions the program's case table does not name, each with its reason
EXCLUDED = {
    "choose_arm_length_": "internal; every path runs through chooseArmLength{Left,Right,Up,Down}",
    "arm_length_": "internal; every path runs through ArmLength{L,R,Up,Down}",
    "compute_ad_": "internal; every path runs through ComputeAD / ComputeADRight",
    "compute_disp_": "internal; every path runs through ComputeDisp{Left,Right,V4}",
    "rccl_check": "SMT_HOST_WITH_RCCL block: needs rccl.h and a HIP runtime, which a host-only stub cannot stand in for",
    "AD_Census_batch_rccl": "SMT_HOST_WITH_RCCL block: needs rccl.h and a HIP runtime; run on the device by test_cpp_host_gpu.py",
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a C++ compiler is needed"
    out = tmp_path_factory.mktemp("cpp_mirror") / "mirror_contract_main"
    cmd = [cxx] + FLAGS + [os.path.join(SRC, "smt_contract_stub.cpp"), os.path.join(SRC, "mirror_contract_main.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr         # -Wall -Wextra clean
    return str(out)


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=ENV)


@pytest.mark.parametrize("family", FAMILIES)
def test_mirror_family_holds_the_contract(exe, family):
    r = _run(exe, family)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{family}: contract held" in r.stdout


def mirror_names(text):
    """every `inline` free function and every public method (constructors included, destructors and deleted members
    not) declared in smt_host.hpp, as `name` or `Class::name`"""
    names, cls, public = [], None, False
    for line in text.splitlines():
        m = re.match(r"(?:template <class T> )?(?:class|struct) (\w+) \{", line)
        if m and not line.rstrip().endswith("};"):
            cls, public = m.group(1), line.startswith("struct ")
            continue
        if cls and line.startswith("};"):
            cls = None
            continue
        if cls:
            if re.match(r"(public|private|protected):", line):
                public = line.startswith("public")
                continue
            m = re.match(r"    (?:explicit )?(?:[\w:<>]+[ \*&]+)*(~?\w+)\(", line)
            if public and m and not line.lstrip().startswith("//") and "= delete" not in line and not m.group(1).startswith("~"):
                if m.group(1) not in ("if", "for", "while", "switch", "return", "check"):
                    names.append(f"{cls}::{m.group(1)}")
            continue
        m = re.match(r"inline [\w:<>, \*&]+?[ \*&](\w+)\(", line)
        if m:
            names.append(m.group(1))
    return list(dict.fromkeys(names))          # overloads (DevBuf's two constructors) count once


def test_parser_sees_the_header():
    names = mirror_names(open(HPP).read())
    for probe in ("check", "AD_Census::Initialize", "AD_Census::GetPtrRight", "CrossAggregator::get_cost_ptr", "DevBuf::upload",
                  "Pipeline::Pipeline", "Pipeline::RunBatch", "WTASubpixel", "LeftAndRightConsistency", "NCCFlow::set_form",
                  "CBLSMFlow::runWindow", "AD_Census_batch_rccl", "imread", "ncc"):
        assert probe in names, probe
    assert not any(n.split("::")[-1] in ("fetch", "apply_subpixel", "arm_dir", "run_") for n in names), "private members leaked in"
    assert len(names) > 100


def test_every_mirror_function_has_a_case_or_a_reason(exe):
    r = _run(exe, "--list")
    assert r.returncode == 0, r.stderr
    table = {}
    for line in r.stdout.splitlines():
        family, *names = line.split()
        table[family] = names
    assert sorted(table) == sorted(FAMILIES)
    covered = {n for names in table.values() for n in names}
    declared = set(mirror_names(open(HPP).read()))
    assert not (covered & set(EXCLUDED)), "named in the case table and excluded"
    assert declared - covered - set(EXCLUDED) == set(), "mirror functions with neither a case nor a reason"
    assert (covered | set(EXCLUDED)) - declared == set(), "names that the header no longer declares"
    assert len(EXCLUDED) <= 8


@pytest.mark.parametrize("which,diagnosis", [(1, "heap-buffer-overflow"), (2, "heap-buffer-overflow"), (3, "LeakSanitizer")])
def test_every_mistake_is_rejected(exe, which, diagnosis):
    """the three wrong mini-mirrors: a DevBuf one element short, a download of n * D elements into n, a throw between
    create and destroy without cleanup"""
    r = _run(exe, "--wrong", str(which))
    assert r.returncode != 0, "the wrong mini-mirror passed"
    assert diagnosis in r.stderr, r.stderr[-2000:]
