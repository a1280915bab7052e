#!/usr/bin/env python3
"""Are the kernels of two source trees the same machine code?  For a change that is meant to leave device code alone:

    python tools/kernel_identity.py OLD [NEW] [--units blend.hip binning.hip ...] [--from blend_stats.hip=blend.hip]
                                    [-o profiles/<name>.txt]

OLD and NEW are source trees or git revisions (a revision is unpacked with `git archive`); NEW defaults to the working
tree, the units to every .hip of NEW's monogs_amd/csrc that OLD has too or that --from names.  `--from U=V`: unit U of NEW was
split off unit V of OLD; its functions are looked up, by symbol, in OLD's V.  Several units may come from the same V: the functions
that V lost must be exactly those that the units split off it hold, taken together.  Each unit is compiled from both trees to gfx950
assembly with the command its Makefile would run for that file (taken from `make -n`, so per-file flags are included),
`-c` replaced by `--cuda-device-only -S`; no GPU needed.  The listing is cut into functions; comments go, and the
numbers the compiler gives out in order of appearance -- `.LBB<function>_<block>` and the like -- lose the function
part, so that a function removed earlier in the file does not show up as a difference in every later one.  A kernel is
identical when its instruction text and its `.amdhsa_*` descriptor (registers, LDS, scratch, ...) are.

Exit status 0: every function of NEW exists in OLD and is identical (functions only OLD has are listed: the removals), and
every --from accounts for what its source lost.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("monogs_amd", "csrc")


def tree_of(spec: str, tmp: str) -> str:
    if os.path.isdir(os.path.join(spec, CSRC)):
        return os.path.abspath(spec)
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--verify", spec + "^{commit}"], text=True).strip()
    out = os.path.join(tmp, rev[:12])
    os.makedirs(out)
    ar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, CSRC, "include"], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", out], stdin=ar.stdout)
    if ar.wait():
        raise SystemExit(f"git archive {spec} failed")
    return out


def compile_commands(tree: str, unit: str) -> list:
    """The commands (argument lists) that the tree's Makefile runs to compile `unit` (a dry run: per-file flags included).
    Run them in the tree's monogs_amd/csrc; `-c` and the `-o` argument are there to be replaced."""
    obj = "OBJ/" + unit[:-len(".hip")] + ".o"
    dry = subprocess.check_output(["make", "-C", os.path.join(tree, CSRC), "-n", "-B", "OUT=OBJ", obj], text=True)
    return [ln.split() for ln in dry.split("\n") if f" -c {unit} " in ln]


def listing(tree: str, unit: str, tmp: str) -> str:
    """The unit's device assembly, compiled with the tree's own Makefile command for it."""
    cmd = compile_commands(tree, unit)[0]
    asm = os.path.join(tmp, f"{len(os.listdir(tmp))}_{unit}.s")
    cmd[cmd.index("-c"):cmd.index("-c") + 1] = ["--cuda-device-only", "-S"]
    cmd[cmd.index("-o") + 1] = asm
    subprocess.check_call(cmd, cwd=os.path.join(tree, CSRC), stderr=subprocess.DEVNULL)
    return open(asm).read()


LOCAL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")        # .LBB12_7, .LJTI12_0, .Ltmp...: drop the function's number


def functions(text: str) -> dict:
    """{symbol: (is_kernel, [instruction and descriptor lines])} of one listing"""
    out, name, body = {}, None, []
    types = set(re.findall(r"^\s*\.type\s+([^,\s]+),@function", text, re.M))
    for ln in text.split("\n"):
        t = ln.split(";")[0].strip()
        if name is None:
            if t.endswith(":") and t[:-1] in types:
                name, body = t[:-1], []
            continue
        if re.match(r"\.Lfunc_end\d+:", t):
            out[name] = (any(b.startswith(".amdhsa_kernel") for b in body), body)
            name = None
        elif t and not t.startswith((".section", ".text", ".p2align")):
            body.append(LOCAL.sub(r".L\1_\2", t))
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=ROOT)
    ap.add_argument("--units", nargs="*")
    ap.add_argument("--from", dest="moved", action="append", default=[], metavar="NEW_UNIT=OLD_UNIT")
    ap.add_argument("-o", "--output")
    args = ap.parse_args()
    lines, bad = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        asm_dir = os.path.join(tmp, "asm")
        os.makedirs(asm_dir)
        old, new = tree_of(args.old, tmp), tree_of(args.new, tmp)
        source = dict(m.split("=") for m in args.moved)        # unit of NEW -> the unit of OLD it was split off
        units = args.units or sorted(u for u in os.listdir(os.path.join(new, CSRC))
                                     if u.endswith(".hip") and (u in source or os.path.exists(os.path.join(old, CSRC, u))))
        lost, found, held = {}, {}, {}                         # per unit: functions only OLD has; identical ones; all of NEW's
        lines.append(f"kernel identity, gfx950 device assembly (tools/kernel_identity.py): OLD = {args.old}, "
                     f"NEW = {'the change' if args.new == ROOT else args.new}")
        for unit in units:
            fo, fn = functions(listing(old, source.get(unit, unit), asm_dir)), functions(listing(new, unit, asm_dir))
            names = demangle(sorted(set(fo) | set(fn)))
            same = [n for n in fn if n in fo and fn[n] == fo[n]]
            differ = [n for n in fn if n in fo and fn[n] != fo[n]]
            added = [n for n in fn if n not in fo]
            gone = [n for n in fo if n not in fn] if unit not in source else []     # (what stayed behind is no removal)
            bad += len(differ) + len(added)
            lost[unit], found[unit], held[unit] = set(gone), set(same), set(fn)
            kern = lambda ns, f: sum(1 for n in ns if f[n][0])  # noqa: E731
            lines.append(f"\n{unit}{' (against ' + source[unit] + ' of OLD)' if unit in source else ''}: OLD {kern(fo, fo)} kernels, NEW {kern(fn, fn)} kernels; identical {len(same)}, "
                         f"different {len(differ)}, only in NEW {len(added)}, only in OLD {len(gone)}")
            for tag, group, f in (("DIFFERENT", differ, fn), ("ONLY IN NEW", added, fn), ("only in OLD", gone, fo),
                                  ("identical", same, fn)):
                for n in sorted(group):
                    size = sum(1 for b in f[n][1] if not b.startswith(".") and not b.endswith(":"))
                    lines.append(f"  {tag:<11} {'kernel' if f[n][0] else 'func  '} {size:6d} instr  {names[n]}")
        for src in sorted(set(source.values()) & set(lost)):
            split = sorted(u for u in source if source[u] == src and u in found)
            if split:
                took = set().union(*(found[u] for u in split)) - held[src]    # (all may hold common.h's static kernels)
                ok = took == lost[src]
                bad += not ok
                lines.append(f"\n{src}: the identical functions of {', '.join(split)} are {'exactly' if ok else 'NOT'} those only OLD's {src} has")
        lines.append(f"\nRESULT: {'every function of NEW is in OLD and identical' if not bad else f'{bad} functions of NEW differ from OLD'}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.output:
        open(args.output, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
