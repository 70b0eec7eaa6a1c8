#!/usr/bin/env python3
"""Compare the device code of two builds symbol by symbol.

For a refactor that moves kernels between translation units a per-file hash of the device
assembly says nothing: the symbols change files.  This cuts the assembly of every file of a
tree per function symbol (the body from its label to its end label, and a kernel's
.amdhsa_kernel ... .end_amdhsa_kernel descriptor block), replaces the compiler's local label
numbers by a placeholder, and compares the two trees by symbol.  It only hashes and compares
text.

    # one directory of *.s per tree, made with
    #   hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only csrc/X.hip -o DIR/X.s
    python3 scripts/kernel_asm_diff.py PARENT_DIR NEW_DIR [--allow REGEX] [--renamed OLD=NEW]

Prints one line per symbol that differs (instruction counts and the descriptor's resources of
both sides), the symbols only one side has, and a summary.  Exit status 1 when a symbol
outside --allow differs or the symbol sets differ (after --renamed).
"""
import argparse
import hashlib
import pathlib
import re
import subprocess
import sys

# (the loop comments name block labels without the ".L": "Header=BB67_33")
LABEL = re.compile(r"(?:\.L)?BB\d+_\d+|\.Lfunc_(?:begin|end)\d+|\.Ltmp\d+")
TYPE_FN = re.compile(r"^\s*\.type\s+(\S+),@function")
FN_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):\s*(;.*)?$")
KD_BEGIN = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
       "private_segment_fixed_size")


def norm(lines):
    # (runs of blanks to one: the comment after a label is aligned to the label's width)
    return [re.sub(r"\s+", " ", LABEL.sub(".L#", l)).rstrip() for l in lines]


def parse(path):
    """{symbol: dict(file, body, kd)} of one assembly file."""
    out = {}
    lines = path.read_text().split("\n")
    i, n = 0, len(lines)
    pending = set()
    while i < n:
        l = lines[i]
        m = TYPE_FN.match(l)
        lab = FN_LABEL.match(l)
        if m:
            pending.add(m.group(1))
        elif lab and lab.group(1) in pending:
            # the function: its label to its end label; a kernel's descriptor block sits inside
            sym = lab.group(1)
            pending.discard(sym)
            j = i + 1
            while j < n and not re.match(r"^\.Lfunc_end\d+:", lines[j]):
                j += 1
            body, kd, inkd = [], [], False
            for t in lines[i + 1:j]:
                if KD_BEGIN.match(t):
                    inkd = True
                (kd if inkd else body).append(t)
                if ".end_amdhsa_kernel" in t:
                    inkd = False
            out[sym] = {"file": path.name, "body": norm(body), "kd": norm(kd) if kd else None}
            i = j
        i += 1
    return out


def load(d):
    syms = {}
    for p in sorted(pathlib.Path(d).glob("*.s")):
        for s, v in parse(p).items():
            if s in syms:   # an inline function emitted by several files: keep the first
                continue
            syms[s] = v
    return syms


def digest(v):
    h = hashlib.sha256()
    h.update("\n".join(v["body"]).encode())
    h.update(b"\0")
    h.update("\n".join(v["kd"] or []).encode())
    return h.hexdigest()[:16]


def ninstr(v):
    k = 0
    for l in v["body"]:
        t = l.strip()
        if t and t[0] not in ".;" and not t.endswith(":"):
            k += 1
    return k


def resources(v):
    r = {}
    for l in v["kd"] or []:
        t = l.split()
        if len(t) >= 2 and t[0].startswith(".amdhsa_") and t[0][8:] in RES:
            r[t[0][8:]] = " ".join(t[1:])
    return " ".join(f"{k}={r[k]}" for k in RES if k in r)


def demangle(names):
    for tool in ("c++filt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        try:
            o = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                               check=True).stdout.split("\n")
            return dict(zip(names, o))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--allow", default=None, help="regex (on the mangled name) of symbols that may differ")
    ap.add_argument("--renamed", action="append", default=[], help="OLD=NEW mangled symbol")
    a = ap.parse_args()
    old, new = load(a.parent), load(a.new)
    for r in a.renamed:
        o, nw = r.split("=")
        if o in old:
            old[nw] = old.pop(o)
    allow = re.compile(a.allow) if a.allow else None
    names = sorted(set(old) | set(new))
    dm = demangle(names)
    same = moved = 0
    bad = 0
    kernels = sum(1 for s in names if s in new and new[s]["kd"])
    for s in names:
        if s not in old or s not in new:
            side = "new" if s in new else "parent"
            print(f"ONLY-{side.upper()} {dm[s]}  [{(new if s in new else old)[s]['file']}]")
            bad += 1
            continue
        o, nw = old[s], new[s]
        if o["file"] != nw["file"]:
            moved += 1
        if digest(o) == digest(nw):
            same += 1
            continue
        ok = allow is not None and allow.search(s) is not None
        if not ok:
            bad += 1
        print(f"{'DIFFERS-ALLOWED' if ok else 'DIFFERS'} {dm[s]}\n"
              f"    parent [{o['file']}] {ninstr(o)} instructions  {resources(o)}\n"
              f"    new    [{nw['file']}] {ninstr(nw)} instructions  {resources(nw)}")
    print(f"{len(names)} function symbols ({kernels} kernels in the new tree): {same} identical "
          f"(body and kernel descriptor), {moved} of all in another file than before, "
          f"{bad} not acceptable")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
