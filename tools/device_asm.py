#!/usr/bin/env python
"""The gfx950 device assembly of every source of libmmd_amd.so, in a form two trees can be compared in (needs no GPU):

    python tools/device_asm.py OUT_DIR [TREE]     # TREE: the checkout to compile, default this one
    diff -r OUT_DIR_OF_ONE_TREE OUT_DIR_OF_THE_OTHER
    python tools/device_asm.py --compare DIR_A DIR_B

Each of TREE's own __graft_entry__.SOURCES is compiled with the library build's flags plus --offload-device-only -S into OUT_DIR/<name>.s.
The compilation-unit id (__hip_cuid_<16 hex digits>) is the only text in the output that depends on the file's path and content hash; it is
replaced by a constant, so a refactor that moves no device code leaves every file identical.

--compare is for a refactor of the device code itself, where inlining order moves the scheduler and the register allocator and the files
cannot stay identical.  It reads the .s files of two earlier runs and prints, per kernel, the resources of both sides and every mnemonic
whose count differs.  Kernels are matched by symbol across files, so one that moved to another source is compared with itself (by file
and symbol where a symbol occurs twice on a side); "same text" means the kernel's body is the other side's but for the numbering of
its block labels, as a kernel that only moved should be.  Exit status 1 if side B, for any kernel, has more VGPRs, any scratch, a different LDS size or occupancy, or a
different count of a work-defining mnemonic (WORK below: matrix, LDS, memory, scalar loads, barriers, lane permutes, transcendentals).  Other
VALU / SALU counts (address arithmetic, register copies, s_nop, s_waitcnt) are printed only: time on the GPU judges those."""
import ast
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC_FLAGS  # noqa: E402


def tree_sources(tree):
    """SOURCES of the tree being compiled, read off its __graft_entry__.py without running it"""
    for node in ast.parse(open(os.path.join(tree, "__graft_entry__.py")).read()).body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "SOURCES" for t in node.targets):
            return ast.literal_eval(node.value)
    sys.exit(f"{tree}/__graft_entry__.py: no SOURCES list")


def device_asm(tree, src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in HIPCC_FLAGS if f not in ("-fPIC", "-shared")]      # (link-time flags: they do not apply to -S)
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", src, "-o", "-"], cwd=tree, check=True, capture_output=True, text=True)
    return re.sub(r"__hip_cuid_[0-9a-f]{16}", "__hip_cuid_0", r.stdout)


RESOURCES = ("NumVgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte")
WORK = re.compile(r"v_mfma_|ds_|global_|buffer_|flat_|s_load_|s_barrier$|v_permlane|v_exp_|v_log_|v_rcp_|v_rsq_")


def kernels(path):
    """{kernel: (resources, mnemonic counts, body)} of one .s file: the instructions between a function's label and its .Lfunc_end, the
    figures from the '; Kernel info:' comments behind it; body = those lines with the block labels' function number (.LBB<n>_, in comments BB<n>_) taken out
    and runs of blanks (the padding in front of a label's comment) collapsed"""
    out, name, counts = {}, None, None
    for line in open(path):
        m = re.match(r"\s+\.type\s+(\S+),@function", line)
        if m:
            name, counts = m.group(1), {}
            out[name] = ({}, counts, [])
        elif name and line.startswith(".Lfunc_end"):
            counts = None
        elif name and counts is not None:
            out[name][2].append(re.sub(r"\s+", " ", re.sub(r"BB\d+_", "BB_", line)))
            if re.match(r"\t[a-z]\w*(\s|$)", line):
                op = line.split()[0]
                counts[op] = counts.get(op, 0) + 1
        elif name and line.startswith("; "):
            m = re.match(r"; (\w+)(?::| =) (\d+)", line)
            if m and m.group(1) in RESOURCES:
                out[name][0].setdefault(m.group(1), int(m.group(2)))
    return {k: v for k, v in out.items() if "NumVgprs" in v[0]}


def side(d, files):
    """{key: (file, kernel record)} of the files of one side that are not byte-identical on both: key = the symbol, or (file, symbol)
    where the symbol occurs in more than one of them"""
    found = [(f, k, v) for f in files if os.path.exists(os.path.join(d, f)) for k, v in kernels(os.path.join(d, f)).items()]
    names = [k for _, k, _ in found]
    return {(k if names.count(k) == 1 else (f, k)): (f, v) for f, k, v in found}


def compare(dir_a, dir_b):
    bad, differ = [], []
    for f in sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b))):
        if not f.endswith(".s"):
            continue
        both = os.path.exists(os.path.join(dir_a, f)) and os.path.exists(os.path.join(dir_b, f))
        if both and open(os.path.join(dir_a, f)).read() == open(os.path.join(dir_b, f)).read():
            print(f"{f}: identical")
        else:
            differ.append(f)
            if not both and not kernels(os.path.join(dir_a if os.path.exists(os.path.join(dir_a, f)) else dir_b, f)):
                bad.append(f"{f}: on one side only")          # (with kernels: each is matched or reported by its symbol below)
    ka, kb = side(dir_a, differ), side(dir_b, differ)
    for key in sorted(set(ka) | set(kb), key=str):
        if key not in ka or key not in kb:
            f, (r, _, _) = (ka if key in ka else kb)[key]
            k = key if isinstance(key, str) else key[1]
            bad.append(f"{f} {k}: on one side only ({'A' if key in ka else 'B'})  " + "  ".join(f"{x} {r.get(x)}" for x in RESOURCES))
            continue
        (fa, (ra, ca, ta)), (fb, (rb, cb, tb)) = ka[key], kb[key]
        k = key if isinstance(key, str) else key[1]
        print(f"{fa if fa == fb else fa + ' -> ' + fb} {k}" + (": same text" if ta == tb else "") + "\n    " +
              "  ".join(f"{r} {ra.get(r)} -> {rb.get(r)}" for r in RESOURCES))
        if rb["NumVgprs"] > ra["NumVgprs"] or rb["ScratchSize"] or any(ra[r] != rb[r] for r in ("LDSByteSize", "Occupancy")):
            bad.append(f"{fb} {k}: resources")
        for op in sorted(set(ca) | set(cb)):
            if ca.get(op, 0) != cb.get(op, 0):
                work = bool(WORK.match(op))
                print(f"    {op} {ca.get(op, 0)} -> {cb.get(op, 0)}" + ("   WORK-DEFINING" if work else ""))
                if work:
                    bad.append(f"{fb} {k}: {op} {ca.get(op, 0)} -> {cb.get(op, 0)}")
    for b in bad:
        print("FAIL", b)
    return 1 if bad else 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    out, tree = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2] if len(sys.argv) == 3 else ROOT)
    os.makedirs(out, exist_ok=True)
    SOURCES = tree_sources(tree)
    with ThreadPoolExecutor(max_workers=len(SOURCES)) as pool:
        for src, text in zip(SOURCES, pool.map(lambda s: device_asm(tree, s), SOURCES)):
            name = os.path.splitext(os.path.basename(src))[0] + ".s"
            with open(os.path.join(out, name), "w") as f:
                f.write(text)
            print(f"{name}: {text.count('.amdhsa_kernel ')} kernels, {text.count(chr(10))} lines")


if __name__ == "__main__":
    main()
