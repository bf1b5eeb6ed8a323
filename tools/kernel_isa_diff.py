#!/usr/bin/env python3
"""Per-kernel resources and ISA of the gfx950 code objects inside built objects / libraries.

    python tools/kernel_isa_diff.py NEW [--against OLD] [--filter SUBSTR ...]

NEW / OLD: an object file, libmpcekf.so or a directory of *.o.  Every bundled gfx950 code
object is extracted (clang-offload-bundler), its kernels' metadata read (llvm-readelf
--notes: VGPRs, AGPRs, SGPRs, scratch and static LDS bytes) and, with --against, each
kernel's disassembly compared with the same kernel of OLD after dropping addresses and
encodings.  Prints one line per kernel:
    name | VGPR/AGPR/SGPR/scratch/LDS/occ [| old the same | identical / differs]
occ = waves per SIMD from the unified register file (512 / allocated VGPRs + AGPRs, max 8).
"""
import argparse
import glob
import os
import re
import subprocess
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def code_objects(path, tmp):
    files = sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]
    out = []
    for i, f in enumerate(files):
        co, fb = os.path.join(tmp, f"{i}.co"), os.path.join(tmp, f"{i}.fatbin")
        try:  # the host ELF's .hip_fatbin section is the offload bundle
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", f, os.devnull],
                           check=True, capture_output=True)
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fb}",
                            f"--output={co}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True,
                           capture_output=True)
        except subprocess.CalledProcessError:
            continue
        if os.path.exists(co) and os.path.getsize(co) > 0:
            out.append(co)
    return out


def kernels(co):
    """{demangled name: (meta dict, [instruction text])}"""
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: (re.search(rf"\.{k}:\s*(\S+)", blk) or [None, None])[1]
        sym = g("symbol")
        if not sym:
            continue
        meta[sym[:-3] if sym.endswith(".kd") else sym] = {
            "vgpr": int(g("vgpr_count")), "agpr": int(g("agpr_count") or 0), "sgpr": int(g("sgpr_count")),
            "scratch": int(g("private_segment_fixed_size")), "lds": int(g("group_segment_fixed_size"))}
    dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co)
    body, cur = {}, None
    for ln in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", ln)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur and ln.strip():
            t = re.sub(r"^\s*[0-9a-f]+:\s*", "", ln)           # address column (some versions)
            t = re.sub(r"\s*//.*$", "", t).strip()              # trailing address comment
            t = re.sub(r"<(\S+?)\+0x[0-9a-f]+>", r"<\1+>", t)   # branch targets by offset
            if t:
                body[cur].append(t)
    try:
        names = run("c++filt", *meta.keys()).split("\n") if meta else []
    except (OSError, subprocess.CalledProcessError):
        names = list(meta.keys())
    return {n: (meta[s], body.get(s, [])) for s, n in zip(meta.keys(), names)}


def occ(m):
    tot = (m["vgpr"] + 7) // 8 * 8  # .vgpr_count is the unified total (AGPRs included)
    return max(1, min(8, 512 // max(tot, 1)))


def fmt(m):
    return f"{m['vgpr']}/{m['agpr']}/{m['sgpr']}/{m['scratch']}/{m['lds']}/{occ(m)}"


def load(path, tmp):
    ks = {}
    for co in code_objects(path, tmp):
        ks.update(kernels(co))
    return ks


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("new")
    ap.add_argument("--against")
    ap.add_argument("--filter", action="append", default=[])
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "n"))
        os.makedirs(os.path.join(tmp, "o"))
        new = load(a.new, os.path.join(tmp, "n"))
        old = load(a.against, os.path.join(tmp, "o")) if a.against else {}
        for n in sorted(new):
            if a.filter and not any(f in n for f in a.filter):
                continue
            m, b = new[n]
            n1 = re.sub(r"^void ", "", n).split("(")[0]
            line = f"{n1} | {fmt(m)}"
            if a.against:
                if n in old:
                    mo, bo = old[n]
                    same = "identical" if b == bo else f"differs ({len(bo)} vs {len(b)} instructions)"
                    line += f" | {fmt(mo)} | {same}"
                else:
                    line += " | - | new"
            print(line)
