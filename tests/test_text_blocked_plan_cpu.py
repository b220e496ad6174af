"""The blocked layout's host plan (bsdb_amd/csrc/text_plan.hpp) without a GPU:
tests/text_blocked_check.cpp is built with the system C++ compiler under
ASan + UBSan and run as a program of its own, as tests/test_text_plan_cpu.py
builds its checker.  The program holds text_place_blocked -- the sequential
statement of the placement rule the kernels are tested against -- against a
byte-level emulation of BlockedKVWriter's writeRecord / flushBlocks on every
sequence of up to 5 sizes of the table at B = 4096 and on seeded random runs,
checks that no image exceeds text_image_max_blocked and that the blocked
footprint is at least the compact one, and exits non-zero on the first
disagreement.  Asserted here: it ran clean and covered what it must."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "text_blocked_check.cpp")


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("text_blocked") / "text_blocked_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, SRC]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    probe = subprocess.run([exe, "probe"], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitized program does not start in this environment: " + probe.stderr.strip()[-300:])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


def test_rule_against_the_byte_level_emulation(result):
    assert result["exhaustive"] == sum(12 ** n for n in range(6))      # every sequence of up to 5 of the 12 sizes
    assert result["random_runs"] == 400
    assert result["runs"] == result["exhaustive"] + result["random_runs"]
    assert result["records"] > 1_000_000


def test_image_bound_and_footprint(result):
    assert result["bound_cases"] > 800
    assert 0 < result["max_image_permille_of_bound"] <= 1000           # the bound holds, and some case comes near it
    assert result["max_image_permille_of_bound"] > 500
    assert result["footprint_cases"] == 7 * 4 * 3 * 2
    assert 64 << 10 <= result["default_chunk"] <= 256 << 20
