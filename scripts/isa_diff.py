#!/usr/bin/env python3
"""Compare the device assembly of one translation unit between two states of
the tree: the check for a refactor that must not change the compiled kernels.

    scripts/isa_diff.py rlev2_expand.hip REV_A [REV_B] [-D MACRO[=V]]... [--by-order]
    scripts/isa_diff.py A.hip,B.hip REV_A [REV_B] [--units-b C.hip,D.hip,E.hip]

A side may be several units, and the two sides different ones (a unit that
was split): the pieces of a side's units are pooled by name. A piece that
several units hold in the same words (a per-unit warm kernel, a per-unit
table) counts once and is listed; one that differs between a side's units
keeps its unit's name and is listed as on one side only. With several units
the .amdgpu_metadata block is cut into one piece per kernel entry, and the
unit's register maximums, which follow its last function whichever that is,
into one of their own.

REV_B defaults to the working tree. For each side, orc_amd/csrc and include/
are materialised in a temporary directory and the unit is compiled with
orc_amd/build.py's flags plus `--cuda-device-only -S` (and the -D flags). The
two assembly files are cut into one piece per function (a kernel's piece
holds its code and its .amdhsa_* resource directives) and per data object
(the compiler does not keep two device globals in one order from run to run),
paired by name and
compared as text after normalising the `__hip_cuid_<hash>` symbol, which
hashes the source, and the function ordinals in local labels; a function on
one side only is listed.
--by-order also replaces every function symbol by its ordinal, for changes
that rename kernels (a template parameter dropped) without changing them.

Prints "identical" or the first differing lines per function; exits 1 on any
difference. CPU only (a cross-compile); the two compiles run side by side.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRS = ["orc_amd/csrc", "include"]


def build_settings():
    spec = importlib.util.spec_from_file_location("_orc_build", os.path.join(ROOT, "orc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, mod.ARCH, [f for f in mod.FLAGS if not f.startswith("-D")]


def materialise(rev, dst):
    if rev is None:
        for d in DIRS:
            shutil.copytree(os.path.join(ROOT, d), os.path.join(dst, d))
        return
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "--"] + DIRS, check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)


def compile_asm(rev, tus, defines, workdir):
    """The assembly of each unit of `tus` at `rev`, compiled side by side."""
    hipcc, arch, flags = build_settings()
    materialise(rev, workdir)

    def one(tu):
        out = os.path.join(workdir, tu + ".s")
        cmd = [hipcc, "-x", "hip", "--offload-arch=" + arch] + flags + ["-D" + d for d in defines]
        cmd += ["--cuda-device-only", "-S", os.path.join(workdir, "orc_amd", "csrc", tu), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit("%s %s: compile failed\n%s" % (rev or "working tree", tu, r.stdout))
        with open(out) as f:
            return f.read()

    with ThreadPoolExecutor(len(tus)) as ex:
        return list(ex.map(one, tus))


FUNC = re.compile(r"^\s*\.type\s+(\S+),@(?:function|object)")
HEAD = re.compile(r"^\s*\.(section|text|globl|protected|hidden|weak|p2align)\b")


def pieces(text, by_order):
    """[(name, [lines])]: a preamble, one piece per function or object, the metadata."""
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)
    # local labels carry their function's ordinal (.LBB12_3, .Lfunc_end12):
    # dropped, so that a function compares equal wherever it stands in the unit
    text = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|LCPI)\d+", r".\1", text)
    text = re.sub(r"\bBB\d+_", "BB_", text)  # (the loop comments' block names)
    text = re.sub(r"[ \t]+;", " ;", text)  # (comments are aligned after the label, whose length changed)
    lines = text.split("\n")
    names = [m.group(1) for m in map(FUNC.match, lines) if m]
    if by_order:
        # longest first: no symbol may be rewritten inside a longer one
        order = {n: i for i, n in enumerate(names)}
        pat = re.compile("|".join(re.escape(n) for n in sorted(names, key=len, reverse=True)))
        if names:
            lines = [pat.sub(lambda m: "fn#%d" % order[m.group(0)], ln) if "_Z" in ln else ln for ln in lines]
        names = ["fn#%d" % i for i in range(len(names))]
    out, cur, k = [], ("(preamble)", []), 0
    for ln in lines:
        if FUNC.match(ln):
            # the directives that open the function (.section, .globl, ...)
            # stand before its .type line: they name it, so they go with it
            head = []
            while cur[1] and HEAD.match(cur[1][-1]):
                head.insert(0, cur[1].pop())
            out.append(cur)
            cur = (names[k], head)
            k += 1
        elif ln.lstrip().startswith(".amdgpu_metadata"):
            out.append(cur)
            cur = ("(metadata)", [])
        cur[1].append(ln)
    out.append(cur)
    return out


def split_metadata(ps):
    """The "(metadata)" piece cut into one piece per kernel entry, named by the
    entry's .name; what stands around the entries stays "(metadata)". The
    unit's register maximums, which follow its last function whichever that
    is, become a piece too."""
    out = []
    for name, lines in ps:
        if name != "(metadata)":
            cut = next((i for i, ln in enumerate(lines) if ".AMDGPU.gpr_maximums" in ln), len(lines))
            out.append((name, lines[:cut]))
            if cut < len(lines):
                out.append(("(gpr maximums)", lines[cut:]))
            continue
        rest, entry = [], None
        for ln in lines + [""]:
            if entry is not None and not ln.startswith("    "):  # the entry's fields are indented under it
                kernel = next(x.split(":", 1)[1].strip() for x in entry if x.startswith("    .name:"))
                out.append(("(metadata) " + kernel, entry))
                entry = None
            if ln.startswith("  - ."):
                entry = []
            (rest if entry is None else entry).append(ln)
        out.append((name, rest[:-1]))
    return out


def pool(per_unit, units):
    """One list of pieces for a side compiled from several units: a piece that
    every unit holds in the same words (the preamble, a per-unit data object)
    counts once, and is listed when more than one unit holds it; a name whose
    pieces differ between the units stays as it is and cannot pair."""
    out, seen = [], {}
    for unit, ps in zip(units, per_unit):
        for name, lines in ps:
            if name not in seen:
                seen[name] = (len(out), [unit])
                out.append((name, lines))
            elif out[seen[name][0]][1] == lines:
                seen[name][1].append(unit)
            else:
                out.append(("%s [%s]" % (name, unit), lines))
    for name, (_, us) in seen.items():
        if len(us) > 1 and not name.startswith("("):
            print("%s: once in each of %s, the same words" % (name, ", ".join(us)))
    return out


def compare_sides(ta, ua, tb, ub, by_order):
    """The two sides' pieces: a side's units pooled by name. With more than one
    unit on a side the metadata goes kernel by kernel on both."""
    sides = []
    for texts, units in ((ta, ua), (tb, ub)):
        per_unit = [pieces(t, by_order) for t in texts]
        if len(ua) > 1 or len(ub) > 1:
            per_unit = [split_metadata(ps) for ps in per_unit]
        sides.append(per_unit[0] if len(units) == 1 else pool(per_unit, units))
    return sides


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tu", help="translation unit(s) under orc_amd/csrc, e.g. rlev2_tiled.hip or a,b,c")
    ap.add_argument("rev_a")
    ap.add_argument("rev_b", nargs="?", default=None, help="default: the working tree")
    ap.add_argument("--units-b", default=None, metavar="TU[,TU...]", help="REV_B's units (default: REV_A's)")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="MACRO[=V]")
    ap.add_argument("--by-order", action="store_true", help="replace function symbols by their ordinals")
    ap.add_argument("--context", type=int, default=6, help="differing lines shown per function")
    args = ap.parse_args()
    ua = args.tu.split(",")
    ub = (args.units_b or args.tu).split(",")

    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        da, db = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        os.makedirs(da)
        os.makedirs(db)
        with ThreadPoolExecutor(2) as ex:
            fa = ex.submit(compile_asm, args.rev_a, ua, args.defines, da)
            fb = ex.submit(compile_asm, args.rev_b, ub, args.defines, db)
            ta, tb = fa.result(), fb.result()
    pa, pb = compare_sides(ta, ua, tb, ub, args.by_order)
    bad = 0
    if not args.by_order:
        # pair the pieces by name (a change may reorder the functions, e.g.
        # a kernel that became a template instance); the rest are listed
        na, nb = [n for n, _ in pa], [n for n, _ in pb]
        for n in na:
            if n not in nb:
                print("%s: only in %s" % (n, args.rev_a))
                bad += 1
        for n in nb:
            if n not in na:
                print("%s: only in %s" % (n, args.rev_b or "the working tree"))
                bad += 1
        db_ = dict(pb)
        pa = [(n, l) for n, l in pa if n in db_]
        pb = [(n, db_[n]) for n, _ in pa]
    elif len(pa) != len(pb):
        print("function count differs: %d vs %d" % (len(pa) - 2, len(pb) - 2))
        bad += 1
    kernels = 0
    for (na, la), (nb, lb) in zip(pa, pb):
        kernels += any(".amdhsa_kernel" in ln for ln in la)
        if na == nb and la == lb:
            print("%s: identical (%d lines)" % (na, len(la)))
            continue
        bad += 1
        if na != nb:
            print("names differ: %s vs %s" % (na, nb))
        i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        print("%s: DIFFERS from line %d of %d / %d" % (na, i + 1, len(la), len(lb)))
        for ln in la[i:i + args.context]:
            print("  < " + ln)
        for ln in lb[i:i + args.context]:
            print("  > " + ln)
    print("%d kernels, %d pieces compared, %d differ" % (kernels, min(len(pa), len(pb)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
