"""Per-kernel comparison of the device code of two source trees: csrc/ and
include/sgg.h of a git revision against the working tree, every .hip compiled
to gfx950 assembly with the build's flags (sgan/_srchash.py).  A kernel is
unchanged when its instruction text (comments stripped, local labels
renumbered in order of appearance) and its .amdhsa_* descriptor (registers,
LDS, scratch) are equal.  Device functions left out of line are compared like
kernels.  Exit status 1 if any kernel was changed or added.

usage: python tools/isa_diff.py <git-rev> [--files a.hip,b.hip]
"""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "group-gan-gcn-gat_amd"
sys.path.insert(0, os.path.join(ROOT, PKG))
from sgan._srchash import FILE_FLAGS, FLAGS  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assemble(src, out):
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-2000:]))
    return out


def kernels(path):
    """{symbol: (normalised instruction text, descriptor lines)} of one assembly file."""
    funcs, desc, name, body, dname = {}, {}, None, None, None
    for raw in open(path):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.type\s+([\w$.]+),@function", line)
        if m:
            name, body = m.group(1), None
        elif line.startswith(".amdhsa_kernel "):   # (the descriptor lies inside its kernel's .text range)
            dname = line.split()[1]
            desc[dname] = []
        elif line == ".end_amdhsa_kernel":
            dname = None
        elif dname:
            desc[dname].append(line)
        elif name and body is None and line == name + ":":
            body = []
        elif name and body is not None:
            if re.match(r"\.Lfunc_end\d+:", line):
                funcs[name], name, body = body, None, None
            else:
                body.append(line)
    out = {}
    for sym, lines in funcs.items():
        labels = {}
        text = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), "\n".join(lines))
        out[sym] = (text, tuple(desc.get(sym, ())))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev")
    ap.add_argument("--files", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, PKG + "/csrc", "include/sgg.h"],
                            capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=ar.stdout, check=True)
        trees = [os.path.join(tmp, PKG, "csrc"), os.path.join(ROOT, PKG, "csrc")]
        names = sorted({f for t in trees for f in os.listdir(t) if f.endswith(".hip")})
        if a.files:
            names = [f for f in names if f in a.files.split(",")]
        jobs = [(os.path.join(t, f), os.path.join(tmp, "%d_%s.s" % (i, f)))
                for f in names for i, t in enumerate(trees) if os.path.exists(os.path.join(t, f))]
        with cf.ThreadPoolExecutor(8) as ex:
            done = set(ex.map(lambda j: assemble(*j), jobs))
        bad = 0
        for f in names:
            old, new = [kernels(p) if p in done else {} for p in
                        (os.path.join(tmp, "%d_%s.s" % (i, f)) for i in (0, 1))]
            removed = sorted(set(old) - set(new))
            added = sorted(set(new) - set(old))
            changed = sorted(k for k in set(old) & set(new) if old[k] != new[k])
            print("%-18s before %3d  after %3d  removed %3d  added %3d  changed %3d" % (
                f, len(old), len(new), len(removed), len(added), len(changed)))
            dm = demangle(removed + added + changed)
            for tag, ks in (("removed", removed), ("added", added), ("changed", changed)):
                for k in ks:
                    what = ""
                    if tag == "changed":
                        what = " (descriptor)" if old[k][0] == new[k][0] else " (instructions)"
                    print("  %s%s: %s" % (tag, what, dm[k]))
            bad += len(added) + len(changed)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
