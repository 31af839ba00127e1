#!/usr/bin/env python3
"""Instruction counts of the split-bf16 K loops, from the gfx950 assembly (no GPU needed; the compile of tools/check_asm_prefetch.py).

For every kernel that carries one of the K loops -- gemm_bf16k_mfma, gemm_bf16w_mfma, the gemm_bf16k_body ranges inside front_kernel<4, true>
and de_dcoef_kernel<4, true>, and gemm_bf16s_body<64, 64, 32, true, true, 3> inside wgrad_pair_kernel -- the tool finds the loops of the listing
(a label and a later branch back to it) that contain MFMAs and no other such loop (widened to the enclosing one where the plane stores lie outside), and counts the instructions between label
and branch, ALL paths of the body together (the staging roles -- A / B waves, K-contiguous / K-major items -- are branches inside the body):

    mfma    v_mfma_*
    split   the VALU instructions of the exact split / the rounding: v_cvt_pk_bf16_f32, v_cvt_pk_f16_f32, v_sub_f32, v_and_b32, v_lshlrev_b32,
            v_mul_f32, v_pk_mul_f32, v_med3_f32 (v_and / v_lshlrev are counted here wherever they stand: the loops have no other use of them)
    other   every other VALU instruction -- address formation, selects, moves; the histogram is printed behind the row
    tail    VALU instructions of the basic blocks behind the scalar branch "this is the last K-tile (and it is partial)": the zero-page
            selects, which only that one tile executes (the blocks carry a marker comment; none in a tree without the guard)
    salu    s_* except branches, waits, barriers and s_nop
    branch  s_branch, s_cbranch_*
    lds     ds_*
    vmem    global_* / buffer_* / flat_*
    steps   K-tile steps the body holds: barriers of the 16-wave loops (one per K-tile step); 1 for the 4-wave staged loop

and `other / step`, the figure DESIGN.md section 4 quotes.  Behind the loops: code size in bytes, vector registers and scratch of the kernel.

    python tools/count_kloop_asm.py [--root DIR] [--md] [--asm FILE | --from-asm FILE]      DIR: another checkout of this repository (the parent commit, for the
                                                                         before-table); FILE: keeps the assembly listing
"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = """#include <hip/hip_runtime.h>
#include "%s/ganmf_amd/csrc/gemm_multi.hpp"
namespace ganmf {
template __global__ void gemm_bf16k_mfma<false, false, 3, false>(const GemmP);
template __global__ void gemm_bf16k_mfma<false, true, 3, false>(const GemmP);
template __global__ void gemm_bf16k_mfma<true, true, 3, false>(const GemmP);
template __global__ void gemm_bf16k_mfma<false, false, 1, false>(const GemmP);
template __global__ void gemm_bf16k_mfma<false, true, 1, false>(const GemmP);
template __global__ void gemm_bf16k_mfma<true, true, 1, false>(const GemmP);
template __global__ void gemm_bf16k_mfma<false, false, 1, true>(const GemmP);
template __global__ void gemm_bf16k_mfma<false, true, 1, true>(const GemmP);
template __global__ void gemm_bf16k_mfma<true, true, 1, true>(const GemmP);
template __global__ void gemm_bf16w_mfma<false>(const GemmP);
template __global__ void gemm_bf16w_mfma<true>(const GemmP);
template __global__ void gemm_bf16w_mfma<false, 1, true>(const GemmP);
template __global__ void gemm_bf16w_mfma<true, 1, true>(const GemmP);
template __global__ void gemm_bf16w_mfma<false, 1, false>(const GemmP);
template __global__ void gemm_bf16w_mfma<true, 1, false>(const GemmP);
template __global__ void front_kernel<4, true>(const GemmP, const DensP);
template __global__ void de_dcoef_kernel<4, true>(const GemmP, const DCoefP, const int);
}      // (wgrad_pair_kernel is no template: every translation unit emits it)
"""

SPLIT = ("v_cvt_pk_bf16_f32", "v_cvt_pk_f16_f32", "v_sub_f32", "v_and_b32", "v_lshlrev_b32", "v_mul_f32", "v_pk_mul_f32", "v_med3_f32")
VMEM = ("global_", "buffer_", "flat_")
SKIP_S = ("s_waitcnt", "s_barrier", "s_nop", "s_endpgm", "s_setprio", "s_sleep")
TAIL = re.compile(r"^\s*; (partial )?last K-tile")      # the marker inside the guarded zero-page selects of the last K-tile (gemm_bf16k.hpp ...)
NAMES = ("bf16k", "bf16w", "front_kernel", "de_dcoef", "wgrad_pair")


def compile_asm(root):
    if "--from-asm" in sys.argv:      # a listing kept by --asm
        return open(sys.argv[sys.argv.index("--from-asm") + 1]).read().split("\n")
    with tempfile.TemporaryDirectory() as d:
        src, asm = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        open(src, "w").write(SRC % root)
        res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-w", src, "-o", asm],
                             capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stderr[-3000:])
            sys.exit(2)
        text = open(asm).read()
        if "--asm" in sys.argv:      # keep the listing
            open(sys.argv[sys.argv.index("--asm") + 1], "w").write(text)
        return text.split("\n")


def kernels_of(text):
    out, cur, name = {}, None, None
    for line in text:
        m = re.match(r"^(_ZN5ganmf\w+):", line)
        if m:
            name, cur = m.group(1), {"lines": [], "meta": {}}
            out[name] = cur
            continue
        if cur is None:
            continue
        for key in ("codeLenInByte", "NumVgprs", "NumAgprs", "ScratchSize"):
            m = re.match(r"^;\s*%s\s*[:=]\s*(\d+)" % key, line.strip())
            if m:
                cur["meta"][key] = int(m.group(1))
        if not cur.get("done"):
            cur["lines"].append(line)
            if "s_endpgm" in line and ".LBB" not in line:
                pass
        if line.startswith(".Lfunc_end"):
            cur["done"] = True
        if "ScratchSize" in cur["meta"] and cur.get("done"):
            cur = None
    return out


def demangle(name):
    s = name
    for tool in (os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "llvm-cxxfilt"), "c++filt"):
        try:
            res = subprocess.run([tool, name], capture_output=True, text=True)
        except OSError:
            continue
        if res.returncode == 0 and res.stdout.strip():
            s = res.stdout.strip()
            break
    return s.replace("ganmf::", "").replace("void ", "").split("(")[0]


def loops_with_mfma(lines):
    ins = []      # (kind, text) with labels
    labels = {}
    for raw in lines:
        text = raw.split(";")[0].strip() if not raw.strip().startswith(";;#") else ""
        if TAIL.search(raw):
            ins.append("; tail")
            continue
        if not text or text.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", raw.strip())
            if m:
                labels[m.group(1)] = len(ins)
                ins.append("; label")
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", text)
        if m:
            labels[m.group(1)] = len(ins)
            ins.append("; label")
            continue
        ins.append(text)
    ranges = []
    for i, text in enumerate(ins):
        if text.startswith("s_branch") or text.startswith("s_cbranch"):
            tgt = text.split()[-1]
            if tgt in labels and labels[tgt] <= i:
                ranges.append((labels[tgt], i))
    ranges = [r for r in ranges if any(t.startswith("v_mfma") for t in ins[r[0]:r[1] + 1])]
    ranges = sorted(set(ranges))
    inner = [r for r in ranges if not any(o != r and r[0] <= o[0] and o[1] <= r[1] for o in ranges)]
    # a K loop stages as well as multiplies: where the block layout leaves the plane stores outside the innermost range (the 4-wave staged
    # loop), the smallest enclosing range that holds them is the loop
    loops = []
    for r in inner:
        cands = sorted((o for o in ranges if o[0] <= r[0] and r[1] <= o[1]), key=lambda o: o[1] - o[0])
        pick = next((o for o in cands if any(t.startswith("ds_write") for t in ins[o[0]:o[1] + 1])), r)
        if pick not in loops:
            loops.append(pick)
    return ins, loops


def count(body):
    c = Counter()
    other = Counter()
    # basic blocks that hold the tail marker: their VALU instructions are the guarded selects of the last K-tile, counted apart as `tail`
    tail_idx, cur, has = set(), [], False
    for i, text in enumerate(list(body) + ["; label"]):
        cur.append(i)
        has = has or text == "; tail"
        if text.startswith(("s_branch", "s_cbranch", "; label")):
            if has:
                tail_idx.update(cur)
            cur, has = [], False
    for i, text in enumerate(body):
        if text.startswith(";"):
            continue
        op = text.split()[0]
        if op.startswith("v_") and not op.startswith("v_mfma") and i in tail_idx:
            c["tail"] += 1
            continue
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            base = op[:-4] if op.endswith(("_e32", "_e64")) else op
            if base in SPLIT:
                c["split"] += 1
            else:
                c["other"] += 1
                other[base] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(VMEM):
            c["vmem"] += 1
        elif op.startswith("s_branch") or op.startswith("s_cbranch"):
            c["branch"] += 1
        elif op.startswith("s_barrier"):
            c["barrier"] += 1
        elif op.startswith("s_") and not op.startswith(SKIP_S):
            c["salu"] += 1
    return c, other


def main():
    root, md = HERE, "--md" in sys.argv
    if "--root" in sys.argv:
        root = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
    ks = kernels_of(compile_asm(root))
    cols = ("mfma", "split", "other", "tail", "salu", "branch", "lds", "vmem")
    if md:
        print("| kernel | loop | steps | " + " | ".join(cols) + " | other / step | code bytes | VGPR | scratch | other VALU |")
        print("|---|---|---|" + "---|" * len(cols) + "---|---|---|---|---|")
    total_code = 0
    for name, k in ks.items():
        if not any(n in name for n in NAMES):
            continue
        ins, loops = loops_with_mfma(k["lines"])
        meta = k["meta"]
        pretty = demangle(name)
        total_code += meta.get("codeLenInByte", 0)
        for n, (a, b) in enumerate(loops):
            c, other = count(ins[a:b + 1])
            wave16 = "bf16s" not in pretty and "wgrad_pair" not in pretty
            steps = max(c["barrier"], 1) if wave16 else 1
            hist = ", ".join("%d %s" % (v, o) for o, v in other.most_common())
            per = c["other"] / float(steps)
            if md:
                print("| `%s` | %d | %d | " % (pretty, n, steps) + " | ".join(str(c[x]) for x in cols) +
                      " | %.1f | %d | %d | %d | %s |" % (per, meta.get("codeLenInByte", 0), meta.get("NumVgprs", 0), meta.get("ScratchSize", 0), hist))
            else:
                print("%-58s loop %d steps %d  " % (pretty, n, steps) + "  ".join("%s %3d" % (x, c[x]) for x in cols) +
                      "  other/step %5.1f  code %6d B  vgpr %3d  scratch %d\n    other VALU: %s" %
                      (per, meta.get("codeLenInByte", 0), meta.get("NumVgprs", 0), meta.get("ScratchSize", 0), hist))
    print(("\n" if md else "") + "code bytes of the kernels above: %d" % total_code)
    return 0


if __name__ == "__main__":
    sys.exit(main())
