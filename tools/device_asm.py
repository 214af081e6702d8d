#!/usr/bin/env python
"""The gfx950 device assembly of every source of libmmd_amd.so, in a form two trees can be compared in (needs no GPU):

    python tools/device_asm.py OUT_DIR [TREE]     # TREE: the checkout to compile, default this one
    diff -r OUT_DIR_OF_ONE_TREE OUT_DIR_OF_THE_OTHER

Each of __graft_entry__.SOURCES is compiled with the library build's flags plus --offload-device-only -S into OUT_DIR/<name>.s.  The
compilation-unit id (__hip_cuid_<16 hex digits>) is the only text in the output that depends on the file's path and content hash; it is
replaced by a constant, so a refactor that moves no device code leaves every file identical."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC_FLAGS, SOURCES  # noqa: E402


def device_asm(tree, src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in HIPCC_FLAGS if f not in ("-fPIC", "-shared")]      # (link-time flags: they do not apply to -S)
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", src, "-o", "-"], cwd=tree, check=True, capture_output=True, text=True)
    return re.sub(r"__hip_cuid_[0-9a-f]{16}", "__hip_cuid_0", r.stdout)


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    out, tree = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2] if len(sys.argv) == 3 else ROOT)
    os.makedirs(out, exist_ok=True)
    with ThreadPoolExecutor(max_workers=len(SOURCES)) as pool:
        for src, text in zip(SOURCES, pool.map(lambda s: device_asm(tree, s), SOURCES)):
            name = os.path.splitext(os.path.basename(src))[0] + ".s"
            with open(os.path.join(out, name), "w") as f:
                f.write(text)
            print(f"{name}: {text.count('.amdhsa_kernel ')} kernels, {text.count(chr(10))} lines")


if __name__ == "__main__":
    main()
