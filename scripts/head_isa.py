#!/usr/bin/env python3
"""Compare the gfx950 machine code of the head-family translation units at two commits.

    python scripts/head_isa.py [--parent REV] [--units UNIT ...] [--out profiles/head_common_isa.json]

Both trees (REV from `git archive`, and the working tree) are compiled with the Makefile's CXXFLAGS plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`.  For every __global__ symbol the instruction lines (comments,
blank lines and assembler directives stripped; labels kept in the compared stream, not counted) are compared as a whole stream.
No GPU is needed."""
import argparse
import collections
import hashlib
import io
import json
import os
import re
import subprocess
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "multimodal-learning-with-alternating-unimodal-adaptation_amd"
UNITS = ["head_gs_sgd", "concat_head", "qmf_head", "feature_step", "modulation"]


def cxxflags(csrc):
    for line in open(os.path.join(csrc, "Makefile")):
        if line.startswith("CXXFLAGS"):
            return line.split("=", 1)[1].replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    raise SystemExit("no CXXFLAGS in the Makefile")


def kernels_of(csrc, unit, tmp):
    """{kernel: {"stream": [...], "n": instructions, resources...}} of one translation unit"""
    asm = os.path.join(tmp, unit + ".s")
    cmd = ["/opt/rocm/bin/hipcc"] + cxxflags(csrc) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                       unit + ".hip", "-o", asm]
    err = subprocess.run(cmd, cwd=csrc, check=True, capture_output=True, text=True).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?(Function Name|SGPRs|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[{"SGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds"}[m.group(1)]] = int(m.group(2))
    text = open(asm).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        body = text.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
        stream = []
        for line in body.splitlines():
            line = line.split(";", 1)[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue
            stream.append(re.sub(r"\s+", " ", line))
        # local labels carry the function's index in the unit: name them by their order inside the kernel instead
        labels = {l[:-1]: ".L%d" % i for i, l in enumerate(s for s in stream if s.endswith(":"))}
        stream = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.get(m.group(0), m.group(0)), s) for s in stream]
        out[name] = dict(res.get(name, {}), stream=stream, n=sum(not s.endswith(":") for s in stream))
    return out


def tree_kernels(csrc, units):
    with tempfile.TemporaryDirectory() as tmp:
        return {u: kernels_of(csrc, u, tmp) for u in units}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--units", nargs="+", default=UNITS, help="translation units (csrc/<unit>.hip); default: the head family")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_common_isa.json"))
    ap.add_argument("--digests", nargs=2, metavar=("PARENT.json", "HERE.json"),
                    help="{case: {buffer: sha256}} of the GPU outputs of the entry points whose kernels differ, at the parent's build "
                         "and at this one; one SHA-256 per case over its buffers' digests goes into the report")
    ap.add_argument("--dump", help="directory for the two streams of every kernel that differs (to diff by hand)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "archive", a.parent, PKG + "/csrc", "include"], cwd=ROOT, check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        before = tree_kernels(os.path.join(old, PKG, "csrc"), a.units)
    after = tree_kernels(os.path.join(ROOT, PKG, "csrc"), a.units)
    rev = subprocess.run(["git", "rev-parse", "--short", a.parent], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    report = {"parent": rev, "flags": "Makefile CXXFLAGS + --cuda-device-only -S -Rpass-analysis=kernel-resource-usage", "units": {}}
    bad = 0
    for u in a.units:                                 # a kernel that moved to another unit is compared there, under its new unit
        for k in [k for k in before[u] if k not in after[u]]:
            for v in a.units:
                if k in after[v] and k not in before[v]:
                    before[v][k] = dict(before[u].pop(k), moved_from=u)
    for u in a.units:
        rows = report["units"][u] = {}
        for k in sorted(set(before[u]) | set(after[u])):
            b, n = before[u].get(k), after[u].get(k)
            if b is None or n is None:
                rows[k] = {"identical": False, "only_in": "parent" if n is None else "here"}
                bad += 1
                continue
            same = b["stream"] == n["stream"]
            row = {"instructions_parent": b["n"], "instructions_here": n["n"], "identical": same,
                   "sha256_here": hashlib.sha256("\n".join(n["stream"]).encode()).hexdigest()[:16]}
            if "moved_from" in b:
                row["moved_from"] = b["moved_from"]
            for f in ("vgprs", "sgprs", "lds", "scratch"):
                row[f] = n.get(f) if b.get(f) == n.get(f) else {"parent": b.get(f), "here": n.get(f)}
            if not same:
                bad += 1
                if a.dump:
                    os.makedirs(a.dump, exist_ok=True)
                    for tag, side in (("parent", b), ("here", n)):
                        with open(os.path.join(a.dump, "%s.%s.s" % (k, tag)), "w") as f:
                            f.write("\n".join(side["stream"]) + "\n")
                ops = lambda s: collections.Counter(x.split(" ", 1)[0] for x in s if not x.endswith(":"))
                row["same_opcode_multiset"] = ops(b["stream"]) == ops(n["stream"])
            rows[k] = row
    if a.digests:
        old, new = (json.load(open(f)) for f in a.digests)
        fold = lambda d: hashlib.sha256("\n".join("%s:%s" % kv for kv in sorted(d.items())).encode()).hexdigest()
        cases = {k: {"buffers": len(v), "parent": fold(v), "here": fold(new[k])} for k, v in sorted(old.items()) if isinstance(v, dict)}
        report["gpu_outputs"] = {"buffers": sum(c["buffers"] for c in cases.values()),
                                 "all_equal": all(c["parent"] == c["here"] for c in cases.values()), "cases": cases}
    report["kernels"] = sum(len(r) for r in report["units"].values())
    report["differing"] = bad
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d kernels, %d differ -> %s" % (report["kernels"], bad, a.out))
    for u, rows in report["units"].items():
        for k, r in rows.items():
            if not r["identical"]:
                print("  DIFFERS", u, k, {x: r[x] for x in r if x != "sha256_here"})
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
