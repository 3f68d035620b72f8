"""Static count of a kernel's serialized global-memory round trips in its assembly listing.

Counts, for one function, the vector global loads (``global_load_*`` / ``buffer_load_*`` / ``flat_load_*``)
and the "loads followed by an ``s_waitcnt vmcnt``" groups: a group is one or more loads issued since the
last vmcnt wait, closed by the next one.  Each group is at least one exposed memory round trip of the
wave, so the group count bounds from below how often the wave stands waiting for global memory; the
counts are static (every path of the function, rare ones included).

    python scripts/vm_groups.py k.s [--func _ZN2as6k_stepILi27ELm207817167EEEvNS_8StepArgsE] [-v]
"""
import argparse
import re


def count(lines: list[str], func: str) -> tuple[int, int, list[tuple[int, int]]]:
    """(vector global loads, load-then-wait groups, [(1-based line of the closing wait, loads in the group)])."""
    start = next(i for i, l in enumerate(lines) if l.startswith(func + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    loads = groups = pending = 0
    marks = []
    for i in range(start, end):
        s = lines[i].strip()
        op = s.split(None, 1)[0] if s else ""
        if op.startswith(("global_load", "buffer_load", "flat_load")):
            loads += 1
            pending += 1
        elif op == "s_waitcnt" and "vmcnt" in s:
            if pending:
                groups += 1
                marks.append((i + 1, pending))
            pending = 0
    return loads, groups, marks


def main():
    p = argparse.ArgumentParser()
    p.add_argument("asm")
    p.add_argument("--func", default=None, help="mangled name (default: every k_step / k_obs / k_quad)")
    p.add_argument("-v", action="store_true", help="list the groups")
    a = p.parse_args()
    lines = open(a.asm).read().split("\n")
    funcs = [a.func] if a.func else [l.split(":")[0] for l in lines if re.match(r"^_ZN2as\d(k_step|k_obs|k_quad)\S*:", l)]
    for f in funcs:
        loads, groups, marks = count(lines, f)
        print(f"{f}: {loads} vector global loads in {groups} groups")
        if a.v:
            for line, k in marks:
                print(f"  wait at line {line}: {k} loads")


if __name__ == "__main__":
    main()
