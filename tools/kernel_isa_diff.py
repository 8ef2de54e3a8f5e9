"""Compare the gfx950 instruction streams of kernels between two source trees (compiler only, no GPU).

  python tools/kernel_isa_diff.py OLD_TREE NEW_TREE --old-units wgrad.hip wgrad_rg.hip \
      --new-units wgrad_f32.hip wgrad_direct.hip wgrad_direct_rg.hip reduce.hip

Every listed unit of csrc/ is compiled to device assembly with the flags of its own tree's _build.py plus
`--cuda-device-only -S`.  Kernels are matched by name over all units of a side (a kernel may move between
units).  Per kernel it prints both sides' .vgpr_count, .sgpr_count, .private_segment_fixed_size and
.group_segment_fixed_size and whether the instruction streams match.  A stream is the kernel's lines from
its label to its end without comments, directives and blank lines, with the function index of the
.LBB<n>_<m> labels dropped (it changes when kernels move between units) and every reference to a
label written as its distance to the target.  For a differing kernel it prints
the extent of the difference (first and last differing line of each side); --show prints the diff itself.
Exit status 1 if any kernel differs or exists on one side only.  --cache DIR keeps the assembly by content
hash, so an unchanged side is not compiled again.
"""
import argparse
import concurrent.futures
import difflib
import glob
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

RES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def load_build(tree):
    hits = glob.glob(os.path.join(tree, "*", "_build.py"))
    if len(hits) != 1:
        sys.exit("%s: expected one */_build.py, found %d" % (tree, len(hits)))
    spec = importlib.util.spec_from_file_location("_build_" + hashlib.sha1(tree.encode()).hexdigest()[:8], hits[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tree_key(b, unit, extra):
    h = hashlib.sha1()
    for p in sorted(glob.glob(os.path.join(b.CSRC, "*")) + [os.path.join(b.CSRC, "..", "..", "include", "dad.h")]):
        if p.endswith((".h", ".hip")):
            h.update(os.path.basename(p).encode())
            h.update(open(p, "rb").read())
    h.update(repr((unit, b.CFLAGS, list(extra))).encode())
    return h.hexdigest()[:16]


def assembly(b, unit, extra, cache):
    out = os.path.join(cache, "%s.%s.s" % (os.path.splitext(unit)[0], tree_key(b, unit, extra)))
    if not os.path.exists(out):
        cmd = [b.HIPCC] + b.CFLAGS + list(extra) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, unit), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit("hipcc failed for %s:\n%s" % (unit, r.stdout))
    return open(out).read()


def kernels(text):
    """{kernel: (resources, stream)} of one assembly file."""
    res = {}
    for doc in re.split(r"\n  - \.", text):   # one metadata entry per kernel
        m = re.search(r"^\s*\.name:\s+(\S+)\s*$", doc, re.M)
        if m and ".vgpr_count:" in doc:
            res[m.group(1)] = tuple(int(re.search(r"^\s*%s:\s+(\d+)" % re.escape(k), doc, re.M).group(1)) for k in RES)
    lines = text.split("\n")
    start = {}
    for i, ln in enumerate(lines):
        lab = ln.split(";")[0].strip()
        if lab.endswith(":") and lab[:-1] in res:
            start[lab[:-1]] = i
    out = {}
    for name, i in start.items():
        body = []
        for ln in lines[i + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = ln.split(";")[0].strip()
            lab = re.match(r"\.LBB\d+_(\d+):$", ln)
            if not ln or (ln.startswith(".") and not lab):
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        # a label becomes "L:" and a reference to it the signed distance to its target in instructions: lines
        # added or removed in one place then change no branch that does not span them
        at, n = {}, 0
        for ln in body:
            if ln.endswith(":"):
                at[ln[:-1]] = n
            else:
                n += 1
        rel, n = [], 0
        for ln in body:
            if ln.endswith(":"):
                rel.append("L:")
                continue
            rel.append(re.sub(r"\.LBB_\d+", lambda m: "L%+d" % (at[m.group(0)] - n) if m.group(0) in at else m.group(0), ln))
            n += 1
        body = rel
        out[short(name)] = (res[name], body)
    return out


def short(mangled):
    """the function name of an Itanium-mangled free function (kernels here are free functions)"""
    m = re.match(r"_Z(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled


def side(tree, units, extra, cache):
    b = load_build(tree)
    with concurrent.futures.ThreadPoolExecutor(max(1, min(len(units), int(os.environ.get("MAX_JOBS", "8"))))) as ex:
        texts = list(ex.map(lambda u: assembly(b, u, extra, cache), units))
    ks = {}
    for u, t in zip(units, texts):
        for name, v in kernels(t).items():
            if name in ks:
                sys.exit("%s: kernel %s is defined by two of the listed units" % (tree, name))
            ks[name] = v + (u,)
    return ks


def extent(a, b):
    """first / last differing line numbers (1-based) of both streams, differing lines of both, places"""
    ops = [o for o in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if o[0] != "equal"]
    return (ops[0][1] + 1, ops[-1][2], ops[0][3] + 1, ops[-1][4], sum(o[2] - o[1] for o in ops),
            sum(o[4] - o[3] for o in ops), len(ops))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--old-units", nargs="+", required=True)
    ap.add_argument("--new-units", nargs="+", required=True)
    ap.add_argument("--extra", nargs="*", default=[], help="extra compiler flags for both sides")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--show", action="store_true", help="print the unified diff of differing kernels")
    args = ap.parse_args()
    extra = list(args.extra)
    with tempfile.TemporaryDirectory() as tmp:
        cache = args.cache or tmp
        os.makedirs(cache, exist_ok=True)
        old = side(args.old, args.old_units, extra, cache)
        new = side(args.new, args.new_units, extra, cache)
    bad = 0
    print("%-34s %-22s %-22s %s" % ("kernel", "old vgpr/sgpr/priv/lds", "new vgpr/sgpr/priv/lds", "stream"))
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%-34s only in %s" % (name, "old" if name in old else "new"))
            bad += 1
            continue
        (ro, so, uo), (rn, sn, un) = old[name], new[name]
        same = so == sn
        verdict = "identical (%d lines)" % len(so) if same else "DIFFERENT (%d -> %d lines)" % (len(so), len(sn))
        if ro != rn:
            verdict += ", RESOURCES DIFFER"
        print("%-34s %-22s %-22s %s   [%s -> %s]" % (name, "/".join(map(str, ro)), "/".join(map(str, rn)), verdict, uo, un))
        if not same:
            print("    differs in old lines %d-%d, new lines %d-%d: %d old and %d new lines in %d places" % extent(so, sn))
            if args.show:
                sys.stdout.writelines("    " + d + "\n" for d in difflib.unified_diff(so, sn, "old", "new", lineterm="", n=2))
        bad += (not same) or ro != rn
    print("%d kernels, %d differ" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
