#!/usr/bin/env python3
"""Do two builds hold the same device code?  Compares the listings of `make -C target_estimation_amd/csrc listings LST=<dir>`
of two source trees, unit by unit, as text (CPU only).
    python tools/listing_diff.py A_DIR B_DIR [--pairs FILE]
Every listing is split into its functions (label to end-of-function label) and their kernel descriptors (.amdhsa_kernel blocks).
Comments go; mangled names and local labels become placeholders numbered by first appearance inside the function, so a renamed
template argument list or a shifted label number does not count, and anything else does.  A unit is `identical` when the two
multisets of (body, descriptor) are equal; otherwise the demangled names without a partner are listed.  --pairs writes, for
every function, `unit <TAB> name in A <TAB> name in B` (demangled), to check a renaming by eye or by script.
Exit status 1 if any unit differs or exists on one side only."""
import argparse
import collections
import hashlib
import os
import re
import subprocess
import sys

SYM = re.compile(r"_Z[A-Za-z0-9_$.]+|\.L[A-Za-z_]*\d+(?:_\d+)?")


def normalise(lines):
    seen = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln or ln.startswith(".section"):
            continue
        out.append(SYM.sub(lambda m: seen.setdefault(m.group(0), "@%d" % len(seen)), ln))
    return "\n".join(out)


def functions(path):
    """-> [(mangled name, digest of body + descriptor, is a kernel)]"""
    found = []
    name, body, desc, in_desc = None, [], [], False
    for ln in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            name, body, desc = m.group(1), [], []
            continue
        if name is None:
            continue
        if re.match(r"\s*\.amdhsa_kernel\s", ln):
            in_desc = True
        if in_desc:
            desc.append(ln)
            if re.match(r"\s*\.end_amdhsa_kernel", ln):
                in_desc = False
            continue
        if re.match(r"\.Lfunc_end\d+:", ln):
            text = normalise(body) + "\n--descriptor--\n" + normalise(desc)
            found.append((name, hashlib.sha256(text.encode()).hexdigest(), bool(desc)))
            name = None
            continue
        body.append(ln)
    return found


def demangle(names):
    if not names:
        return []
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"^void |\(.*", "", n) for n in out[:len(names)]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a_dir")
    ap.add_argument("b_dir")
    ap.add_argument("--pairs")
    args = ap.parse_args()
    units = lambda d: sorted(f[:-2] for f in os.listdir(d) if f.endswith(".s"))
    ua, ub = units(args.a_dir), units(args.b_dir)
    bad = 0
    pairs = open(args.pairs, "w") if args.pairs else None
    total = 0
    for u in sorted(set(ua) | set(ub)):
        if u not in ua or u not in ub:
            print("%-36s only in %s" % (u, args.a_dir if u in ua else args.b_dir))
            bad += 1
            continue
        fa, fb = functions(os.path.join(args.a_dir, u + ".s")), functions(os.path.join(args.b_dir, u + ".s"))
        ca, cb = collections.Counter(h for _, h, _ in fa), collections.Counter(h for _, h, _ in fb)
        kernels = sum(1 for _, _, k in fa if k)
        total += kernels
        if ca == cb:
            print("%-36s kernels %4d  functions %4d  identical" % (u, kernels, len(fa)))
        else:
            bad += 1
            only_a = demangle([n for n, h, _ in fa if ca[h] > cb[h]])
            only_b = demangle([n for n, h, _ in fb if cb[h] > ca[h]])
            print("%-36s kernels %4d / %4d  functions %4d / %4d  DIFFERENT" % (u, kernels, sum(1 for _, _, k in fb if k), len(fa), len(fb)))
            for n in only_a:
                print("    A only: " + n)
            for n in only_b:
                print("    B only: " + n)
        if pairs:
            by_hash = collections.defaultdict(list)
            for n, h, _ in fb:
                by_hash[h].append(n)
            na = [n for n, _, _ in fa]
            nb = [(by_hash[h].pop(0) if by_hash[h] else "") for _, h, _ in fa]
            for x, y in zip(demangle(na), demangle(nb)):
                pairs.write("%s\t%s\t%s\n" % (u, x, y))
    print("%d units, %d kernels: %s" % (len(set(ua) | set(ub)), total, "all identical" if not bad else "%d units differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
