"""Device code of two builds of the seven band objects, compared kernel by kernel: a change of the host side — which unit instantiates what, how a launch finds its
kernel — must leave every kernel as it was.

  python profiles/band_device_code.py PARENT_OBJ_DIR [THIS_OBJ_DIR]

For each object of miniwfa_amd.build.BAND2_UNITS in both directories (default for the second: miniwfa_amd/csrc/build) the gfx950 code object is taken out of the
.hip_fatbin section (llvm-objcopy, clang-offload-bundler) and compared in three ways:
  (a) the set of kernel symbols (the names of the metadata notes, llvm-readelf --notes);
  (b) per kernel symbol, the instruction stream (llvm-objdump -d) with the address column dropped — by symbol, so the order of instantiation does not matter;
  (c) per kernel, the metadata-note fields for VGPRs, SGPRs, spilled VGPRs and SGPRs, scratch and LDS.
Prints one line per object — identical, or what differs — and the SHA-256 over its kernels' listings in symbol order; exit status 1 if any object differs.
Needs no device."""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miniwfa_amd.build import BAND2_UNITS  # noqa: E402

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
NOTE_FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def code_object(obj: str) -> tuple[dict, dict]:
    """({kernel symbol: [instruction lines without addresses]}, {kernel symbol: {note field: value}}) of the object's gfx950 code object."""
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(d, "copy.o")], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co],
                       check=True, capture_output=True)
        listing = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    meta: dict = {}
    cur = None
    for ln in notes.splitlines():
        m = re.match(r"\s*(-\s+)?(\.[a-z_]+):\s*(\S.*)?$", ln)
        if not m:
            continue
        if m.group(1):  # a new entry of a list: of amdhsa.kernels (or of a kernel's .args, whose fields are none of ours)
            cur = {}
        if cur is not None and m.group(2) in NOTE_FIELDS + (".symbol",):
            cur[m.group(2)] = (m.group(3) or "").strip("'\" ")
            if m.group(2) == ".symbol":
                meta[cur[".symbol"][:-3] if cur[".symbol"].endswith(".kd") else cur[".symbol"]] = cur
    streams: dict = {}
    sym = None
    for ln in listing.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", ln)
        if m:
            sym = m.group(1)
            streams[sym] = []
        elif sym is not None and "//" in ln:
            text, _, tail = ln.partition("//")
            streams[sym].append(text.strip() + " ; " + tail.split(":", 1)[1].strip())  # mnemonic and operands ; encoding
    return {k: v for k, v in streams.items() if k in meta}, {k: {f: v.get(f) for f in NOTE_FIELDS} for k, v in meta.items()}


def main() -> int:
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "miniwfa_amd", "csrc", "build")
    rc, total = 0, 0
    for unit in BAND2_UNITS:
        (sa, ma), (sb, mb) = code_object(os.path.join(parent, unit + ".o")), code_object(os.path.join(this, unit + ".o"))
        digest = [hashlib.sha256("\n".join(f"{k}\n" + "\n".join(s[k]) for k in sorted(s)).encode()).hexdigest()[:16] for s in (sa, sb)]
        problems = []
        if set(ma) != set(mb):
            problems.append(f"kernel symbols differ: {len(set(ma) - set(mb))} only in the parent, {len(set(mb) - set(ma))} only here")
        if set(sa) != set(ma) or set(sb) != set(mb):
            problems.append("a kernel of the notes has no listing")
        for k in sorted(set(ma) & set(mb)):
            if sa.get(k) != sb.get(k):
                problems.append(f"instructions of {k} differ ({len(sa.get(k, []))} against {len(sb.get(k, []))})")
            if ma[k] != mb[k]:
                problems.append(f"notes of {k} differ: {ma[k]} against {mb[k]}")
        n_insn = sum(len(v) for v in sa.values())
        total += len(ma)
        if not problems:
            print(f"{unit}.o: {len(ma)} kernels, same symbols, instructions ({n_insn}) and register / scratch / LDS notes identical kernel by kernel (sha256 {digest[0]} both)")
        else:
            rc = 1
            print(f"{unit}.o: DIFFERS (sha256 {digest[0]} / {digest[1]})")
            for p in problems[:10]:
                print("  " + p)
    print(f"{total} kernels in {len(BAND2_UNITS)} objects: " + ("all identical" if rc == 0 else "DIFFERENCES"))
    return rc


if __name__ == "__main__":
    sys.exit(main())
