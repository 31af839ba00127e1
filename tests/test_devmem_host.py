"""Device memory of the library (ganmf_amd/csrc/lib/devmem.inc) without a device: tests/devmem_check.cpp, a stand-alone program that
includes the file over a host-heap shim of the HIP allocator, built and run under the address and undefined-behaviour sanitizers; and
the rule that makes the owner the owner: no other file of the library calls the HIP allocator."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ganmf_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler found")


def test_devmem_program_sanitized(tmp_path):
    exe = str(tmp_path / "devmem_check")
    src = os.path.join(ROOT, "tests", "devmem_check.cpp")
    base = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    cc = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if cc.returncode != 0:
        cc = subprocess.run(base, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:] + run.stderr[-3000:])
    assert "all cases clean" in run.stdout and "FAIL" not in run.stdout
    for name in ("alloc, grow, reset, move: nothing live at the end", "a failed grow leaves null with capacity 0",
                 "the zeroed flag zeroes", "DevCsr::upload: a failure anywhere leaves an empty holder",
                 "the nnz == 0 and rows == 0 shapes"):
        assert "ok   " + name in run.stdout


def test_only_devmem_calls_the_hip_allocator():
    """With DevBuf's implicit conversion to a pointer a leftover hipFree(h->x) would still compile, and free twice."""
    calls = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(")
    found = {c: [] for c in calls}
    for folder, _, names in os.walk(CSRC):
        for name in names:
            path = os.path.join(folder, name)
            try:
                text = open(path, encoding="utf-8", errors="replace").read()
            except OSError:
                continue
            for c in calls:
                if c in text:
                    found[c].append(os.path.relpath(path, CSRC))
    for c in calls:
        assert found[c] == [os.path.join("lib", "devmem.inc")], (c, found[c])
