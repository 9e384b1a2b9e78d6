"""Device code of two builds of the library's HIP objects, compared kernel by kernel: a change of the host side — which unit instantiates what, how a launch finds its
kernel — or a move of device code between files must leave every kernel as it was; a restructuring of a kernel's source must say exactly which kernels it changed.

  python profiles/band_device_code.py [--all | --units A.hip,B.hip] PARENT_OBJ_DIR [THIS_OBJ_DIR]

The objects compared are those of miniwfa_amd.build.BAND2_UNITS (the default), of the units named with --units, or with --all of every .hip file of SOURCES (of
either build: a unit only one of them has is taken from that one).  For each of them in both directories (default for the second: miniwfa_amd/csrc/build) the
gfx950 code object is taken out of the .hip_fatbin section (llvm-objcopy, clang-offload-bundler) and compared in three ways:
  (a) the set of kernel symbols (the names of the metadata notes, llvm-readelf --notes);
  (b) per kernel symbol, the instruction stream (llvm-objdump -d) with the address column dropped — by symbol, so the order of instantiation does not matter;
  (c) per kernel, the metadata-note fields for VGPRs, SGPRs, spilled VGPRs and SGPRs, scratch and LDS.
A kernel is looked up by its symbol over ALL objects of the other build, so one that moved to another unit is still compared with its former self.
Prints one line per object — identical, or what differs — and the SHA-256 over its kernels' listings in symbol order.  A kernel whose instructions or notes changed
is listed with both instruction counts and the six note fields of both builds, and checked: it may not gain scratch or spilled VGPRs, and its .vgpr_count may not
cross a boundary of the allocation table that lowers the waves a SIMD holds (512 registers per lane and SIMD, granule 8: waves = min(8, 512 // alloc)).
Exit status: 0 all identical; 1 some kernel changed within those limits (or a symbol exists in one build only); 2 a changed kernel broke a limit.  Needs no device."""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miniwfa_amd.build import BAND2_UNITS, SOURCES  # noqa: E402

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


def waves_per_simd(vgprs: int) -> int:
    """Waves a SIMD can hold by registers: 512 per lane, allocated in granules of 8 (<= 64: 8 waves, 72: 7, 80: 6, 88-96: 5, 104-128: 4, 136-168: 3, 176-256: 2, above: 1)."""
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def demangle(sym: str) -> str:
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            r = subprocess.run([tool, sym], capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0 and r.stdout.strip():
            return r.stdout.strip()
    return sym


def main() -> int:
    argv = sys.argv[1:]
    units = list(BAND2_UNITS)
    if "--all" in argv:
        argv.remove("--all")
        units = None
    if "--units" in argv:
        i = argv.index("--units")
        units = argv[i + 1].split(",")
        del argv[i:i + 2]
    parent = argv[0]
    this = argv[1] if len(argv) > 1 else os.path.join(ROOT, "miniwfa_amd", "csrc", "build")
    if units is None:  # every .hip object either build has: SOURCES of this tree, and whatever else the parent's directory holds
        units = [s for s in SOURCES if s.endswith(".hip")]
        units += sorted(f[:-2] for f in os.listdir(parent) if f.endswith(".hip.o") and f[:-2] not in units)
    sides = []  # per build: {unit: (streams, notes)}
    for d in (parent, this):
        sides.append({u: code_object(os.path.join(d, u + ".o")) for u in units if os.path.exists(os.path.join(d, u + ".o"))})
    where = [{k: u for u, (s, m) in side.items() for k in m} for side in sides]  # symbol -> unit
    rc, total, changed = 0, 0, []
    for unit in units:
        if unit not in sides[1]:
            gone = sorted(sides[0][unit][1]) if unit in sides[0] else []
            print(f"{unit}.o: only in the parent ({len(gone)} kernels, {sum(k not in where[1] for k in gone)} of them in no object here)")
            rc = max(rc, 1 if any(k not in where[1] for k in gone) else 0)
            continue
        sb, mb = sides[1][unit]
        digest_b = hashlib.sha256("\n".join(f"{k}\n" + "\n".join(sb[k]) for k in sorted(sb)).encode()).hexdigest()[:16]
        problems, moved = [], {}
        if set(sb) != set(mb):
            problems.append("a kernel of the notes has no listing")
        for k in sorted(mb):
            pu = where[0].get(k)
            if pu is None:
                problems.append(f"{k}: not in the parent")
                continue
            sa, ma = sides[0][pu]
            if pu != unit:
                moved[pu] = moved.get(pu, 0) + 1
            if sa.get(k) != sb.get(k) or ma[k] != mb[k]:
                changed.append((unit, k, len(sa.get(k, [])), len(sb.get(k, [])), ma[k], mb[k]))
        if unit in sides[0]:
            lost = [k for k in sides[0][unit][1] if k not in where[1]]
            if lost:
                problems.append(f"{len(lost)} kernels of the parent's {unit}.o are in no object here: " + ", ".join(lost[:4]))
        n_changed = sum(1 for c in changed if c[0] == unit)
        n_insn = sum(len(v) for v in sb.values())
        total += len(mb)
        origin = "".join(f"; {n} of them from the parent's {pu}.o" for pu, n in sorted(moved.items()))
        if not problems and not n_changed:
            print(f"{unit}.o: {len(mb)} kernels{origin}, same symbols, instructions ({n_insn}) and register / scratch / LDS notes identical kernel by kernel (sha256 {digest_b})")
        else:
            rc = max(rc, 1)
            print(f"{unit}.o: {len(mb)} kernels{origin}, {len(mb) - n_changed} identical by symbol, instructions and notes, {n_changed} CHANGED (sha256 here {digest_b})")
            for p in problems[:10]:
                print("  " + p)
    for unit, k, na, nb, ma, mb in changed:
        print(f"changed: {demangle(k)}  [{unit}.o]")
        print(f"  instructions {na} -> {nb}")
        print("  notes parent: " + ", ".join(f"{f} {ma[f]}" for f in NOTE_FIELDS))
        print("  notes here:   " + ", ".join(f"{f} {mb[f]}" for f in NOTE_FIELDS))
        va, vb = int(ma[".vgpr_count"]), int(mb[".vgpr_count"])
        bad = []
        if int(mb[".private_segment_fixed_size"]) > int(ma[".private_segment_fixed_size"]):
            bad.append("gains scratch")
        if int(mb[".vgpr_spill_count"]) > int(ma[".vgpr_spill_count"]):
            bad.append("gains spilled VGPRs")
        if waves_per_simd(vb) < waves_per_simd(va):
            bad.append("crosses a VGPR boundary")
        print(f"  VGPRs {va} -> {vb}: {waves_per_simd(va)} -> {waves_per_simd(vb)} waves per SIMD by registers (boundaries: 64 | 72 | 80 | 96 | 128 | 168 | 256): " + (", ".join(bad).upper() if bad else "within the limits"))
        if bad:
            rc = 2
    print(f"{total} kernels in {len(sides[1])} objects: " + ("all identical" if rc == 0 else f"{len(changed)} changed" if changed else "DIFFERENCES"))
    return rc


if __name__ == "__main__":
    sys.exit(main())
