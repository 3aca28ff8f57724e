"""Is the device code of a revision and of the working tree the same?  (host Python only: cross-compiles, needs no GPU)

    python tools/device_code_diff.py REV [unit ...] [--map 'REGEX=REPL' ...]
    python tools/device_code_diff.py REV --rev-unit U [--rev-unit U ...] --tree-unit U [--tree-unit U ...]

Compiles the named units of build.units() (object names without .o: gemv_0, gemm, quantize ..; default: all) twice -- from
`git archive REV` and from the working tree -- with build.FLAGS plus -Rpass-analysis=kernel-resource-usage -save-temps=obj, and
compares per unit and per kernel: the resource-usage remark (registers, scratch, occupancy, LDS), the .amdhsa descriptor and the
instruction text of the device assembly (comments and directives dropped, local labels renumbered per kernel in order of
appearance: the kernels of a unit come out in another order when a template changes).  Kernels are paired by their demangled
name without "(anonymous namespace)::"; --map rewrites REV's names first (re.sub, repeatable, applied in order) when a change
renames what the kernels are instantiated on.  Unpaired symbols are listed; a differing kernel is shown with the difference
of its per-opcode counts (none: register naming or instruction order only).  Exit status 1 if anything differs.
--rev-unit / --tree-unit (repeatable; units of plain .hip sources, which need not exist on the other side) pool the kernels of
the units named per side and pair across the pool: for kernels that moved between units.  The report is then one section.
"""
import argparse
import collections
import concurrent.futures
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ["-Rpass-analysis=kernel-resource-usage", "-save-temps=obj"]
MAX_COMPILES = 16

_LABEL = re.compile(r"\.L[A-Za-z_$]*\d+(?:_\d+)*")
_FUNC = re.compile(r"^\s*\.type\s+([\w$.]+),@function")


def normalize(lines):
    """Instruction text of one kernel: comments, directives and blank lines dropped, white space collapsed, local labels
    (.LBB3_17, .Ltmp4 ..) renamed .L0, .L1 .. in order of first appearance."""
    out, names = [], {}
    for ln in lines:
        t = " ".join(ln.split(";", 1)[0].split())
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        out.append(_LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), t))
    return out


def opcode_counts(text):
    return collections.Counter(t.split(" ", 1)[0] for t in text if not t.endswith(":"))


def split_functions(asm_lines):
    """{symbol: (instruction text, descriptor lines or None)} of a device assembly file.  A function's text runs from its
    label to its .Lfunc_end; the descriptor is the body of its .amdhsa_kernel block."""
    funcs, desc, cur, in_desc, body = {}, {}, None, None, []
    pending = set()
    for ln in asm_lines:
        m = _FUNC.match(ln)
        if m:
            pending.add(m.group(1))
            continue
        t = ln.strip()
        if in_desc is not None:
            if t.startswith(".end_amdhsa_kernel"):
                in_desc = None
            else:
                desc[in_desc].append(" ".join(t.split(";", 1)[0].split()))
            continue
        if t.startswith(".amdhsa_kernel"):
            in_desc = t.split()[1]
            desc[in_desc] = []
            continue
        m = re.match(r"^([\w$.]+):", ln)
        if m and m.group(1) in pending:
            pending.discard(m.group(1))
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if t.startswith(".Lfunc_end"):
                funcs[cur] = normalize(body)
                cur = None
            else:
                body.append(ln)
    return {s: (text, desc.get(s)) for s, text in funcs.items()}


def parse_remarks(stderr):
    """{symbol: 'TotalSGPRs: 34; VGPRs: 110; ..'} from the compiler's kernel-resource-usage remarks (locations dropped)."""
    out, cur = {}, None
    for ln in stderr.splitlines():
        # "FILE:L:C: remark: ITEM [-R..]", or with -save-temps "remark: FILE:L:C: ITEM [-R..]"
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", ln)
        if not m:
            continue
        item = m.group(1)
        if item.startswith("Function Name:"):
            cur = item.split(":", 1)[1].strip()
            out[cur] = []
        elif cur is not None:
            out[cur].append(item)
    return {k: "; ".join(v) for k, v in out.items()}


def parse_map(spec):
    pat, sep, repl = spec.partition("=")
    if not sep or not pat:
        raise ValueError("--map wants REGEX=REPL, got %r" % spec)
    return re.compile(pat), repl


def pair_name(demangled, maps=()):
    """The name a symbol is paired by: demangled, without the anonymous namespace, rewritten by the maps in order."""
    name = demangled.replace("(anonymous namespace)::", "")
    for pat, repl in maps:
        name = pat.sub(repl, name)
    return name


def compare(old, new):
    """old, new: {pair name: (text, descriptor, remark)}.  -> dict of the lists a report prints."""
    common = sorted(set(old) & set(new))
    res = {"only_old": sorted(set(old) - set(new)), "only_new": sorted(set(new) - set(old)), "common": common,
           "remark": [], "desc": [], "text": []}
    for k in common:
        (t0, d0, r0), (t1, d1, r1) = old[k], new[k]
        if r0 != r1:
            res["remark"].append(k)
        if d0 != d1:
            res["desc"].append(k)
        if t0 != t1:
            c0, c1 = opcode_counts(t0), opcode_counts(t1)
            res["text"].append((k, {op: c1[op] - c0[op] for op in sorted(set(c0) | set(c1)) if c0[op] != c1[op]}))
    return res


def _readelf():
    from cogview_amd.csrc import build as B
    bin_dir = os.path.dirname(os.path.realpath(B._hipcc()))
    for cand in (os.path.join(bin_dir, "..", "lib", "llvm", "bin", "llvm-readelf"), os.path.join(bin_dir, "..", "llvm", "bin", "llvm-readelf"),
                 shutil.which("llvm-readelf")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("llvm-readelf not found next to hipcc: cannot demangle the kernel names")


def _demangled(elf):
    """{symbol: demangled name} of the functions of a device code object: its symbol table read twice, plain and demangled
    (the compiler's own demangler: it knows the 16-bit float types)"""
    def names(*opt):
        out = subprocess.run([_readelf(), "--dyn-syms", "-W"] + list(opt) + [elf], capture_output=True, text=True, check=True).stdout
        return [m.group(1) for m in re.finditer(r"^\s*\d+:\s+\w+\s+\d+\s+FUNC\s+\w+\s+\w+\s+\S+\s+(.*)$", out, re.M)]
    return dict(zip(names(), names("--demangle")))


def _compile_unit(job):
    """-> (functions of the device assembly, remarks, demangled names) of one unit compiled in a directory of its own"""
    from cogview_amd.csrc import build as B
    src, flags, extra, out_dir = job
    os.makedirs(out_dir)
    r = subprocess.run([B._hipcc()] + flags + extra + EXTRA + ["-c", src, "-o", os.path.join(out_dir, "unit.o")], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s %s:\n%s" % (src, " ".join(extra), r.stderr[-3000:]))
    funcs, dem = {}, {}
    for asm in glob.glob(os.path.join(out_dir, "*amdgcn*.s")):
        funcs.update(split_functions(open(asm).read().splitlines()))
        dem.update(_demangled(asm[:-2] + ".out"))
    return funcs, parse_remarks(r.stderr), dem


def _table(funcs, remarks, dem, maps):
    rem = {pair_name(dem.get(s, s), maps): v for s, v in remarks.items()}
    out = {}
    for s, (text, desc) in funcs.items():
        k = pair_name(dem.get(s, s), maps)
        out[k] = (text, desc, rem.get(k))
    return out


def _report(title, old, new, rev):
    """prints one section: the tables old / new of _table() compared.  -> True if anything differs"""
    res = compare(old, new)
    nk = [sum(1 for v in t.values() if v[1] is not None) for t in (old, new)]
    nlines = sum(len(old[k][0]) for k in res["common"])
    sha = [hashlib.sha256("\n".join(k + "\n" + "\n".join(t[k][0]) for k in res["common"]).encode()).hexdigest()[:16] for t in (old, new)]
    print("== %s" % title)
    print("   kernels: %s %d, working tree %d; functions in all: %d, %d; paired: %d" % (rev, nk[0], nk[1], len(old), len(new), len(res["common"])))
    print("   only in %s: %s" % (rev, res["only_old"]))
    print("   only in the working tree: %s" % res["only_new"])
    norem = [k for k in res["common"] if old[k][1] is not None and (old[k][2] is None or new[k][2] is None)]
    print("   kernels whose resource-usage remark differs: %d%s" % (len(res["remark"]), "; WITHOUT a remark: %s" % norem if norem else ""))
    print("   kernels whose .amdhsa descriptor differs: %d" % len(res["desc"]))
    print("   kernels whose instruction text differs (%d instruction lines compared per symbol, labels renumbered): %d" % (nlines, len(res["text"])))
    print("   sha256 of the paired per-symbol text: %s %s  working tree %s" % (rev, sha[0], sha[1]))
    for k in res["common"][:1]:
        print("   e.g. %s | %s" % (k, new[k][2]))
    for k in res["remark"]:
        print("   remark  %s\n      %s: %s\n      tree: %s" % (k, rev, old[k][2], new[k][2]))
    for k in res["desc"]:
        d0, d1 = old[k][1] or [], new[k][1] or []
        print("   descriptor  %s\n      %s" % (k, "\n      ".join("%s -> %s" % p for p in zip(d0, d1) if p[0] != p[1])))
    for k, dc in res["text"]:
        print("   text  %s\n      opcode counts (tree - %s): %s" % (k, rev, dc or "equal (register naming or order only)"))
    return bool(res["only_old"] or res["only_new"] or res["remark"] or res["desc"] or res["text"] or norem or nk[0] != nk[1])


def _pooled(built, maps):
    """one table of several units' kernels; a pair name that two units of a side define cannot be paired"""
    out = {}
    for b in built:
        t = _table(*b, maps)
        dup = sorted(set(out) & set(t))
        if dup:
            raise SystemExit("defined in two units of one side: %s" % dup)
        out.update(t)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev")
    ap.add_argument("units", nargs="*")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL", help="rewrite REV's demangled kernel names (re.sub)")
    ap.add_argument("--rev-unit", action="append", default=[], metavar="UNIT", help="pooled form: a unit of REV (repeatable)")
    ap.add_argument("--tree-unit", action="append", default=[], metavar="UNIT", help="pooled form: a unit of the working tree (repeatable)")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    from cogview_amd.csrc import build as B
    maps = [parse_map(m) for m in a.map]
    units = [(src, os.path.basename(obj)[:-2], extra) for src, obj, extra in B.units()]
    pooled = bool(a.rev_unit or a.tree_unit)
    if pooled and (a.units or not (a.rev_unit and a.tree_unit)):
        raise SystemExit("the pooled form wants --rev-unit and --tree-unit, and no positional units")
    names = a.units or [u for _, u, _ in units]
    unknown = sorted(set(a.tree_unit if pooled else names) - {u for _, u, _ in units})
    if unknown:
        raise SystemExit("no such unit: %s (units: %s)" % (" ".join(unknown), " ".join(u for _, u, _ in units)))
    rev = subprocess.run(["git", "rev-parse", "--short", a.rev], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    csrc_rel, inc_rel = os.path.relpath(B.HERE, ROOT), os.path.relpath(B.INCLUDE, ROOT)
    by_name = {u: (src, extra) for src, u, extra in units}
    with tempfile.TemporaryDirectory() as td:
        old_root = os.path.join(td, "rev")
        os.makedirs(old_root)
        tar = subprocess.run(["git", "archive", a.rev, csrc_rel, inc_rel], cwd=ROOT, capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old_root], input=tar, check=True)
        old_flags = [{"-I" + B.HERE: "-I" + os.path.join(old_root, csrc_rel), "-I" + B.INCLUDE: "-I" + os.path.join(old_root, inc_rel)}.get(f, f)
                     for f in B.FLAGS]

        def old_job(unit):
            # a unit the working tree no longer has is a plain source of REV: UNIT.hip, no extra flags
            src, extra = by_name.get(unit, (os.path.join(B.HERE, unit + ".hip"), []))
            old_src = os.path.join(old_root, os.path.relpath(src, ROOT))
            if not os.path.exists(old_src):
                raise SystemExit("%s has no %s" % (rev, os.path.relpath(src, ROOT)))
            return old_src, old_flags, extra, os.path.join(td, "old_" + unit)

        new_job = lambda unit: (by_name[unit][0], B.FLAGS, by_name[unit][1], os.path.join(td, "new_" + unit))
        if pooled:
            jobs = [old_job(u) for u in a.rev_unit] + [new_job(u) for u in a.tree_unit]
        else:
            jobs = [j for _, unit, _ in units if unit in names for j in (old_job(unit), new_job(unit))]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_COMPILES, os.cpu_count() or 1, len(jobs))) as ex:
            built = list(ex.map(_compile_unit, jobs))
    print("device code of %s against the working tree, cross-compiled for %s (%s)" % (rev, B.ARCH, " ".join(B.FLAGS[:4] + EXTRA)))
    for spec in a.map:
        print("name map (applied to %s's demangled kernel names): %s" % (rev, spec))
    differs = False
    if pooled:
        n = len(a.rev_unit)
        differs = _report("%s: %s | working tree: %s (kernels pooled per side)" % (rev, " ".join(a.rev_unit), " ".join(a.tree_unit)),
                          _pooled(built[:n], maps), _pooled(built[n:], ()), rev)
    else:
        for i, (src, unit, extra) in enumerate(u for u in units if u[1] in names):
            differs |= _report("%s (%s %s)" % (unit, os.path.basename(src), " ".join(extra)), _table(*built[2 * i], maps), _table(*built[2 * i + 1], ()), rev)
    print("RESULT: device code %s" % ("DIFFERS" if differs else "identical"))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())

