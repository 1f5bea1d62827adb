"""Compare the gfx950 code of every kernel of this tree with another checkout's (a refactor's parent: `git worktree add <dir> <commit>`).
    python tools/isa_diff.py <path to the other tree's csrc> [--tools] [substring of the demangled kernel name]
Both trees are compiled unit by unit with build.py's flags; per kernel symbol the instruction text up to .Lfunc_end (comments stripped) and
the .amdhsa_ descriptor lines (registers, LDS, private segment) are compared as text.  Prints the counts and, per changed kernel, the
instruction count, VGPRs and scratch operations of both sides.  Exit status 1 if any kernel differs."""
import os, re, subprocess, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_check


def kernels(asm_path):
    """{mangled kernel name: (instruction lines, descriptor lines)}"""
    s = open(asm_path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", s, re.M | re.S):
        nm = m.group(1)
        start = re.search(r"^" + re.escape(nm) + r":", s, re.M).end()
        body = [l.split(";")[0].strip() for l in s[start:min(m.start(), s.index(".Lfunc_end", start))].split("\n")]
        out[nm] = ([l for l in body if l], [l.split(";")[0].strip() for l in m.group(2).split("\n") if ".amdhsa_" in l])
    return out


def describe(k):
    ins, desc = k
    vg = [l.split()[-1] for l in desc if l.startswith(".amdhsa_next_free_vgpr")]
    return f"instr={sum(not l.endswith(':') and not l.startswith('.') for l in ins):5d} vgpr={vg[0] if vg else '?':>3s} scratch={sum(l.startswith('scratch_') for l in ins):3d}"


def diff_unit(asm_new, asm_old, pattern=""):
    """(identical, [report line per kernel that changed, appeared or vanished])"""
    new, old = kernels(asm_new), kernels(asm_old)
    same, changed = 0, []
    names = sorted(set(new) | set(old))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")      # one process for all names
    for nm, d in zip(names, plain):
        d = d.strip().replace("tsnet::", "")
        if pattern not in d:
            continue
        if new.get(nm) == old.get(nm):
            same += 1
        else:
            changed.append(f"  {d}\n      other: {describe(old[nm]) if nm in old else 'absent'}\n      this:  {describe(new[nm]) if nm in new else 'absent'}")
    return same, changed


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        sys.exit(__doc__)
    other, pattern, tools = args[0], (args[1] if len(args) > 1 else ""), "--tools" in sys.argv
    sys.path.insert(0, isa_check.ROOT)
    from wacv23_tsnet_amd import build as B
    isa_check.compile_all(list(B.UNITS), tools)
    isa_check.compile_all(list(B.UNITS), tools, other)
    same, changed = 0, []
    for u in B.UNITS:
        s, c = diff_unit(isa_check.compile_asm(tools, u), isa_check.compile_asm(tools, u, other), pattern)
        print(f"{u:24s} {s:4d} identical {len(c):4d} changed", flush=True)
        same += s; changed += c
    print("\n".join(changed))
    print(f"isa_diff{' --tools' if tools else ''}: {same} kernels identical, {len(changed)} changed")
    sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
