"""Device code of two builds of the band objects, compared instruction by instruction ("alpha16": mwf_band2.hip gained the 4-bit form under a macro —
with the macro unset every line must compile to what it compiled to before).

  python profiles/alpha16_device_code.py PARENT_OBJ_DIR [THIS_OBJ_DIR]

For mwf_band2.hip.o and mwf_band2_tab.hip.o of both directories (default for the second: miniwfa_amd/csrc/build): the gfx950 code object is taken out of the
.hip_fatbin section (llvm-objcopy, clang-offload-bundler) and disassembled (llvm-objdump -d); the two listings are compared from the first symbol on (the
line that names the file is dropped).  Prints one line per object — identical, or the number of differing lines and the first of them — and the SHA-256 of
each listing.  Needs no device."""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def disassemble(obj: str) -> list[str]:
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(d, "copy.o")], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co],
                       check=True, capture_output=True)
        out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    return [ln for ln in out.splitlines() if "file format" not in ln and not ln.startswith(d)]


def main() -> int:
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "miniwfa_amd", "csrc", "build")
    rc = 0
    for unit in ("mwf_band2.hip.o", "mwf_band2_tab.hip.o"):
        a, b = disassemble(os.path.join(parent, unit)), disassemble(os.path.join(this, unit))
        ha, hb = (hashlib.sha256("\n".join(x).encode()).hexdigest()[:16] for x in (a, b))
        n_insn = sum(1 for ln in a if "//" in ln)
        if a == b:
            print(f"{unit}: device code identical ({len(a)} lines, {n_insn} instructions; sha256 {ha} both)")
        else:
            diff = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
            print(f"{unit}: DIFFERS — {len(a)} against {len(b)} lines, {len(diff)} differing in the common part (sha256 {ha} / {hb})")
            if diff:
                print("  first:", a[diff[0]].strip(), "|", b[diff[0]].strip())
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
