#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    tools/device_code_diff.py PARENT_TREE THIS_TREE [--work DIR] [--jobs N] [--rename OLD=NEW ...]

Every `multimodalpfn_amd/csrc/*.hip` of both trees is compiled to assembly with the Makefile's flags
(`-x hip -S --cuda-device-only`).  For each kernel the instruction stream (comments and directives dropped,
`.LBB` labels renumbered in order of appearance, symbol names replaced by a placeholder) and the resource
figures of its metadata are compared.  A kernel is matched by its demangled name; `--rename OLD=NEW` maps a
parent name whose template argument list changed onto the new one (a Python regular expression on the
demangled name).  Prints one line per kernel and a summary; exit status 1 if any matched kernel differs.
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]
NO_NANS = {"attention.hip", "attention_pipe.hip", "featrow.hip"}
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def compile_tree(tree, work, jobs):
    src = os.path.join(tree, "multimodalpfn_amd", "csrc")
    os.makedirs(work, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    files = sorted(f for f in os.listdir(src) if f.endswith(".hip"))

    inc = os.path.join(tree, "include")
    headers = [os.path.join(d, h) for d in (src, inc) for h in os.listdir(d) if h.endswith(".h")]
    newest_h = max(os.path.getmtime(h) for h in headers)

    def one(f):
        out = os.path.join(work, f + ".s")
        if os.path.exists(out) and os.path.getmtime(out) > max(newest_h, os.path.getmtime(os.path.join(src, f))):
            return f, out                                            # neither it nor a header changed since
        cmd = [hipcc, *FLAGS, *(["-fno-honor-nans"] if f in NO_NANS else []),
               "-x", "hip", "-S", "--cuda-device-only", f, "-o", out]
        subprocess.run(cmd, cwd=src, check=True)
        return f, out

    with cf.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, files))


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, out.stdout.splitlines()))


def kernels_of(asm_path):
    """{mangled kernel name: (instruction lines, {resource: value})}"""
    lines = open(asm_path).read().splitlines()
    meta, cur = {}, None
    for ln in lines:                       # amdhsa.kernels metadata: one "  - .key: value" list entry per kernel
        if re.match(r"  - \.", ln):
            cur = {}
        elif not ln.startswith("    "):
            cur = None
        if cur is None:
            continue
        m = re.match(r"  [- ] (\.[a-z_]+):\s+(\S+)$", ln)
        if m and m.group(1) in RESOURCES:
            cur[m.group(1)] = m.group(2)
        elif m and m.group(1) == ".symbol":
            meta[m.group(2)[:-len(".kd")]] = cur
    syms = sorted(meta, key=len, reverse=True)
    sym_re = re.compile("|".join(re.escape(s) for s in syms)) if syms else None
    streams, name, body = {}, None, None
    for ln in lines:
        s = ln.split(";", 1)[0].rstrip()
        m = re.match(r"(\S+):\s*$", s)
        if m and m.group(1) in meta:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = s.strip()
        if t.startswith(".Lfunc_end"):
            streams[name] = body
            name = None
            continue
        if not t or (t.startswith(".") and not t.startswith(".LBB")):
            continue
        if sym_re:
            t = sym_re.sub("SYM", t)
        body.append(re.sub(r"\s+", " ", t))
    out = {}
    for k, body in streams.items():
        labels = {}
        def lab(m):
            return labels.setdefault(m.group(0), ".L%d" % len(labels))
        out[k] = ([re.sub(r"\.LBB\d+_\d+", lab, b) for b in body], meta[k])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--work", default="build/device_code_diff")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]

    trees = {}
    for tag, tree in (("parent", a.parent), ("this", a.this)):
        asm = compile_tree(tree, os.path.join(a.work, tag), a.jobs)
        ks = {}
        for f, path in asm.items():
            got = kernels_of(path)
            dm = demangle(list(got))
            for k, v in got.items():
                ks[(f, dm[k])] = v
        trees[tag] = ks

    parent, this = trees["parent"], trees["this"]
    renamed, mapped = [], {}
    for (f, n), v in parent.items():
        n2 = n
        for old, new in renames:
            n2 = re.sub(old, new, n2)
        if n2 != n and (f, n2) in this and (f, n) not in this:
            renamed.append((f, n, n2))
        else:
            n2 = n
        mapped[(f, n2)] = (n, v)

    bad = same = 0
    for key in sorted(set(mapped) | set(this)):
        f, n = key
        if key not in this:
            print(f"GONE       {f}: {n}")
            continue
        if key not in mapped:
            print(f"NEW        {f}: {n}")
            bad += 1
            continue
        (pn, (pb, pm)), (tb, tm) = mapped[key], this[key]
        tag = "IDENTICAL" if (pb == tb and pm == tm) else "DIFFERENT"
        note = f"  [was {pn}]" if pn != n else ""
        res = " ".join(f"{r[1:]}={tm.get(r, '-')}" for r in RESOURCES)
        print(f"{tag:10} {f}: {n}{note}  lines={len(tb)} {res}")
        if tag == "DIFFERENT":
            bad += 1
            if pm != tm:
                print(f"           parent resources: {pm}")
            if pb != tb:
                i = next((i for i, (x, y) in enumerate(zip(pb, tb)) if x != y), min(len(pb), len(tb)))
                print(f"           parent lines={len(pb)}; first difference at line {i}:")
                print(f"             parent: {pb[i] if i < len(pb) else '<end>'}")
                print(f"             this:   {tb[i] if i < len(tb) else '<end>'}")
        else:
            same += 1
    gone = sorted(k for k in mapped if k not in this)
    print(f"\nkernels: parent {len(parent)}, this {len(this)}; identical {same}, different or new {bad}, "
          f"gone {len(gone)}, of the identical ones {len(renamed)} under a changed symbol")
    print("kernels gone or under a changed symbol (any other difference is marked DIFFERENT / NEW above):")
    for f, n in gone:
        print(f"  no longer exists   {f}: {n}")
    for f, n, n2 in sorted(renamed):
        print(f"  symbol changed     {f}: {n}  ->  {n2}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
