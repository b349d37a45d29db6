#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of csrc/, unit by unit and kernel by kernel (no GPU).

    tools/compare_code_objects.py PARENT_OBJ_DIR BRANCH_OBJ_DIR OUT_DIR [--moved unit ...]

Each directory holds the obj/<unit>.o files of one build (make -C dnn-for-speech-enhancement_amd/csrc).  Writes
  OUT_DIR/units_code_objects.txt  sha256 of every unit's code object (llvm-objdump --offloading) in both builds
  OUT_DIR/units_kernel_text.txt   for the kernels of the --moved units: VGPRs, SGPRs, scratch, static LDS (the code object's
                                  amdhsa.kernels metadata) and the sha256 of the disassembled instruction text in both builds.
Kernels are matched by demangled name with "(anonymous namespace)::" removed, whichever unit holds them.  The instruction text of
a kernel is llvm-objdump -d of its symbol without addresses and encodings (the trailing "// ..." comment): branch offsets are
relative and stay in; the zero fill between two symbols is left out.  Exit status 1 if a unit that is in both builds outside --moved, or a matched kernel, differs."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin/"


def code_object(obj, tmp):
    d = tempfile.mkdtemp(dir=tmp)
    shutil.copy(obj, os.path.join(d, "u.o"))
    subprocess.check_call([LLVM + "llvm-objdump", "--offloading", "u.o"], cwd=d, stdout=subprocess.DEVNULL)
    co = [f for f in os.listdir(d) if "gfx950" in f]
    assert len(co) == 1, (obj, co)
    return os.path.join(d, co[0])


def demangle(names):
    out = subprocess.check_output(["c++filt"], input="\n".join(names) + "\n", universal_newlines=True).split("\n")
    return [n.replace("(anonymous namespace)::", "") for n in out[:len(names)]]


def kernels(co):
    """{demangled name: (vgpr, sgpr, scratch, lds, sha256 of the instruction text, instructions)}"""
    notes = subprocess.check_output([LLVM + "llvm-readelf", "--notes", co], universal_newlines=True)
    meta = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        meta[g("name")] = (int(g("vgpr_count")), int(g("sgpr_count")), int(g("private_segment_fixed_size")), int(g("group_segment_fixed_size")))
    dis = subprocess.check_output([LLVM + "llvm-objdump", "-d", "--no-leading-addr", co], universal_newlines=True)
    text, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            cur = m.group(1)
            text[cur] = []
        elif cur and line.strip() and line.strip() != "...":      # ("...": the zero fill up to the next symbol's alignment)
            text[cur].append(re.sub(r"\s*//.*$", "", line).strip())
    names = sorted(meta)
    out = {}
    for mangled, name in zip(names, demangle(names)):
        body = "\n".join(text[mangled])
        out[name] = meta[mangled] + (hashlib.sha256(body.encode()).hexdigest(), len(text[mangled]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent"); ap.add_argument("branch"); ap.add_argument("out")
    ap.add_argument("--moved", nargs="*", default=[])
    a = ap.parse_args()
    units = lambda d: sorted(f[:-2] for f in os.listdir(d) if f.endswith(".o") and f.count(".") == 1)
    tmp = tempfile.mkdtemp()
    bad = 0
    cos = {}
    with open(os.path.join(a.out, "units_code_objects.txt"), "w") as f:
        f.write("# sha256 of each unit's gfx950 code object (llvm-objdump --offloading on obj/<unit>.o): parent commit | this commit\n")
        for u in sorted(set(units(a.parent)) | set(units(a.branch))):
            sha = []
            for side, d in (("p", a.parent), ("b", a.branch)):
                o = os.path.join(d, u + ".o")
                if os.path.exists(o):
                    cos[side, u] = code_object(o, tmp)
                    sha.append(hashlib.sha256(open(cos[side, u], "rb").read()).hexdigest())
                else:
                    sha.append("-")
            verdict = "identical" if sha[0] == sha[1] else "new" if sha[0] == "-" else "differs"
            if verdict != "identical" and u not in a.moved:
                bad = 1
            f.write("%s %s %s %s\n" % (u, sha[0], sha[1], verdict))
    side_k = {"p": {}, "b": {}}
    for (side, u), co in sorted(cos.items()):
        if u in a.moved:
            for name, v in kernels(co).items():
                assert name not in side_k[side], name
                side_k[side][name] = (u,) + v
    with open(os.path.join(a.out, "units_kernel_text.txt"), "w") as f:
        f.write("# every kernel of %s: unit, VGPRs, SGPRs, scratch bytes, static LDS bytes, instructions, sha256 of the instruction text\n"
                "# (llvm-objdump -d without addresses and encodings): parent commit | this commit\n" % ", ".join(a.moved))
        for name in sorted(set(side_k["p"]) | set(side_k["b"])):
            p, b = side_k["p"].get(name), side_k["b"].get(name)
            same = p is not None and b is not None and p[1:] == b[1:]
            bad |= not same
            fmt = lambda v: "-" if v is None else "%s vgpr=%d sgpr=%d scratch=%d lds=%d n=%d %s" % (v[0], v[1], v[2], v[3], v[4], v[6], v[5])
            f.write("%s\n    %s\n    %s\n    %s\n" % (name, fmt(p), fmt(b), "equal" if same else "DIFFERS"))
    shutil.rmtree(tmp, ignore_errors=True)
    return bad


if __name__ == "__main__":
    sys.exit(main())
