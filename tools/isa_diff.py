#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two sets of objects (no GPU needed).

    tools/isa_diff.py --a old/lif_layers.o --b new/lif_layers.o new/wgrad.o new/train_util.o

Each object is a hipcc host object; its gfx950 code object is unbundled and disassembled per symbol.
Prints the kernels that are in one set only, in a set twice, or whose instruction text or resources
(VGPRs, AGPRs, SGPRs, LDS, scratch, kernarg size, from the .AMDGPU.metadata notes) differ.  Comments
and trailing padding are ignored.  Exit status 1 if anything differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
RES_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size",
            ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")
PADDING = re.compile(r"^(s_nop 0|s_code_end|\.\.\.)$")  # "...": the zero fill objdump elides


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, arch, tmp):
    """The arch code object of a host object: its .hip_fatbin section is an offload bundle."""
    stem = os.path.join(tmp, str(len(os.listdir(tmp))))
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + stem + ".fb", obj)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + stem + ".fb",
        "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--output=" + stem + ".co")
    return stem + ".co"


def resources(co):
    """kernel symbol -> {key: value} from the amdhsa.kernels list of the code object's metadata note
    (kernel entries start at "  - .key:", their other keys sit at four spaces, arguments deeper)."""
    res, cur, inside = {}, None, False
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        if re.match(r"^\S", line):
            inside = line.startswith("amdhsa.kernels:")
            continue
        m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", line)
        if not inside or not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip().strip("'")
        if m.group(2) == ".symbol":
            res[cur[".symbol"][:-len(".kd")]] = cur
    return {k: {r: v.get(r) for r in RES_KEYS} for k, v in res.items()}


def functions(co):
    """symbol -> list of instruction lines (comments and trailing padding removed)."""
    text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-leading-addr", "--no-show-raw-insn", co)
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        ins = re.sub(r"\s*(//|;).*$", "", line).strip()
        if ins:
            cur.append(ins)
    for body in funcs.values():
        while body and PADDING.match(body[-1]):
            body.pop()
    return funcs


def load(objs, arch, tmp):
    kernels, dups = {}, []
    for obj in objs:
        co = code_object(obj, arch, tmp)
        res, funcs = resources(co), functions(co)
        for name, r in res.items():
            if name in kernels:
                dups.append(name)
            kernels[name] = (funcs.get(name), r, os.path.basename(obj))
    return kernels, dups


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True, help="objects of the first build")
    ap.add_argument("--b", nargs="+", required=True, help="objects of the second build")
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ka, da = load(args.a, args.arch, tmp)
        kb, db = load(args.b, args.arch, tmp)
    bad = 0
    for tag, d in (("a", da), ("b", db)):
        for name in d:
            print("DUPLICATE in %s: %s" % (tag, name))
            bad += 1
    for name in sorted(set(ka) - set(kb)):
        print("ONLY in a (%s): %s" % (ka[name][2], name))
        bad += 1
    for name in sorted(set(kb) - set(ka)):
        print("ONLY in b (%s): %s" % (kb[name][2], name))
        bad += 1
    for name in sorted(set(ka) & set(kb)):
        (fa, ra, oa), (fb, rb, ob) = ka[name], kb[name]
        if fa is None or fb is None:
            print("NO CODE for %s (%s / %s)" % (name, oa, ob))
            bad += 1
            continue
        if fa != fb:
            first = next((i for i, (x, y) in enumerate(zip(fa, fb)) if x != y), min(len(fa), len(fb)))
            print("CODE differs: %s (%s: %d instructions, %s: %d; first difference at %d)"
                  % (name, oa, len(fa), ob, len(fb), first))
            bad += 1
        if ra != rb:
            print("RESOURCES differ: %s %s" % (name, {k: (ra[k], rb[k]) for k in RES_KEYS if ra[k] != rb[k]}))
            bad += 1
    per_obj = {}
    for _, _, o in kb.values():
        per_obj[o] = per_obj.get(o, 0) + 1
    print("kernels: a %d, b %d (%s); differing entries: %d"
          % (len(ka), len(kb), ", ".join("%s %d" % kv for kv in sorted(per_obj.items())), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
