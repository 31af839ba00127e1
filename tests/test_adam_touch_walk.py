"""No early touch of the Adam streams leaves a tensor (csrc/adam_touch.hpp).

The index arithmetic that maps (block, thread) to the dword of theta / m / v a fused-Adam product loads in front of its K loop is plain
C++ shared by the kernels and by tests/adam_touch_walk.cpp.  That program -- host code with its own main -- is built here with
-fsanitize=address,undefined and walks every tile and thread of the fused-Adam products (gV, gWd_ext, gWe_ext, W_0; 256, 512 and 1024 threads
per workgroup) at the shapes of tests/test_gpu_adam_touch.py, the ML-1M shape and a tile grid with empty XCD rectangles: every touched offset inside an allocation of exactly M * ld floats, every line
the row pass reads touched once, nothing else touched."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler found")


def test_adam_touch_walk_sanitized(tmp_path):
    exe = str(tmp_path / "adam_touch_walk")
    src = os.path.join(ROOT, "tests", "adam_touch_walk.cpp")
    base = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    # (the sanitizer runtimes linked statically where the compiler can: the program then starts whatever else the loader brings in first)
    cc = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if cc.returncode != 0:
        cc = subprocess.run(base, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:] + run.stderr[-3000:])
    assert "all walks clean" in run.stdout
    assert run.stdout.count("ok   ") == 7 * 11      # seven shapes x (3 products x 3 workgroup sizes + 2)
