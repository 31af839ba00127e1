"""The level scheduler of the SGD trainers (ganmf_amd/csrc/level_sched.hpp) without a device: tests/level_sched_check.cpp, a stand-alone
program with the columns of SLIM-BPR and of MF-BPR / FunkSVD, built and run under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler found")


def test_scheduler_program_sanitized(tmp_path):
    exe = str(tmp_path / "level_sched_check")
    src = os.path.join(ROOT, "tests", "level_sched_check.cpp")
    base = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    cc = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if cc.returncode != 0:
        cc = subprocess.run(base, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:] + run.stderr[-3000:])
    assert "all schedules clean" in run.stdout and "FAIL" not in run.stdout
    items, users_items = run.stdout.split("-- columns {users, pos[, neg]} over users + items")
    for name in ("empty", "independent", "repeated i", "i becomes j", "j becomes i", "two chains", "out of range"):
        assert "ok   " + name in items
    assert "ok   repeated i: 40 samples, 40 levels" in items and "ok   independent: 5 samples, 1 levels" in items
    assert items.count("ok   random items=") == 16
    for name in ("empty", "independent", "shared user", "shared positive", "j becomes i", "i becomes j", "j ignored by funk",
                 "one user in every sample", "two chains", "clean after a refusal", "out of range"):
        assert "ok   " + name in users_items
    assert "ok   one user in every sample: 40 samples, 40 levels" in users_items
    assert "ok   independent funk: 4 samples, 1 levels" in users_items
    assert users_items.count("ok   random users=") == 72


def test_the_scheduler_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "ganmf_amd", "csrc", "level_sched.hpp")).read()
    assert "hip" not in text.lower()
