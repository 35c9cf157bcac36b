"""Compare the gfx950 assembly of two builds kernel by kernel (a refactor's
"is the instruction stream the parent's" check).  Needs no GPU.

  python tools/asm_compare.py BASE_DIR NEW_DIR ["KERNEL<ARGS>"]
      with a kernel's name as the table prints it: its normalised diff first

BASE_DIR / NEW_DIR hold the .s files of the kernel sources from the tree before
and from this tree (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S, or
the .s that -save-temps leaves).  Registers and labels are normalised (v12 ->
v, s[4:5] -> s[2], .LBB3_7 -> .L).  Per kernel of BASE: found by name in NEW;
the counts of global loads, global stores, ds_read, s_waitcnt vmcnt(0) and
v_perm_b32; whether the whole text, and the text from the first s_barrier on,
is BASE's; and whether every basic block that holds a non-temporal access is
BASE's.  The last column stands for "the text from the first s_barrier to the
end of the full-column path" in kernels whose partial-column paths follow the
barrier too: only the full-column paths (ld_g / st_g) load and store
non-temporally, so a partial-column change leaves those blocks alone and a
full-column change does not.  The proxy sees no block of a column loop that
only computes (a fold between the loads and the stores that sits in blocks of
its own, as in the runtime-shaped kernels): for a kernel listed with "same"
there, read its diff.  Prints one markdown row per kernel that differs
anywhere and a summary; exit 1 if a kernel (or the .s file of one) is missing
or a count differs."""
import collections
import difflib
import glob
import os
import re
import subprocess
import sys

COUNTED = ("global_load", "global_store", "ds_read", "vmcnt(0)", "v_perm_b32")


def norm(line):
    line = line.split(";")[0].strip()
    line = re.sub(r"\b([vsa])\[(\d+):(\d+)\]", lambda m: f"{m.group(1)}[{int(m.group(3)) - int(m.group(2)) + 1}]", line)
    line = re.sub(r"\b([vsa])\d+\b", r"\1", line)
    return re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", ".L", line)


def kernels(path):
    """{mangled name: [normalised instruction lines]} of the .amdhsa kernels of one .s file."""
    out, cur, names = {}, None, set()
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            names.add(m.group(1))
        m = re.match(r"(\w+):", line)
        if m and not line.startswith(".L"):
            cur = out.setdefault(m.group(1), [])
            continue
        if re.match(r"\.Lfunc_end", line):
            cur = None
        elif cur is not None:
            t = norm(line)
            if t and not t.startswith(".") or t == ".L:":
                cur.append(t)
    return {n: v for n, v in out.items() if n in names}


def after_barrier(lines):
    for i, t in enumerate(lines):
        if t.startswith("s_barrier"):
            return lines[i:]
    return lines


def nt_blocks(lines):
    """The basic blocks that hold a non-temporal access -- only the full-column paths of the
    product kernels load and store non-temporally -- as a multiset."""
    out, cur = collections.Counter(), []
    for t in lines + [".L:"]:
        cur.append(t)
        if t == ".L:" or t.startswith(("s_cbranch", "s_branch")):
            if any(x.endswith(" nt") for x in cur):
                out[tuple(x for x in cur if x != ".L:")] += 1
            cur = []
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (s.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
                                     for s in res.stdout.splitlines())))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    base_dir, new_dir = sys.argv[1:3]
    show = sys.argv[3] if len(sys.argv) > 3 else None
    bad = total = same = same_tail = nt_bad = 0
    rows = []
    for bpath in sorted(glob.glob(os.path.join(base_dir, "*.s"))):
        npath = os.path.join(new_dir, os.path.basename(bpath))
        base, new = kernels(bpath), kernels(npath) if os.path.exists(npath) else {}
        pretty = demangle(sorted(base))
        for name in sorted(base):
            total += 1
            if name not in new:
                rows.append(f"| `{pretty[name]}` | MISSING | | | | |")
                bad = 1
                continue
            b, n = base[name], new[name]
            if show and show == pretty[name]:
                print("\n".join(difflib.unified_diff(b, n, "base", "new", lineterm="", n=2)))
            cb = [sum(c in t for t in b) for c in COUNTED]
            cn = [sum(c in t for t in n) for c in COUNTED]
            if b == n:
                same += 1
                same_tail += 1
                continue
            tb, tn = after_barrier(b), after_barrier(n)
            same_tail += tb == tn
            nt = "same" if nt_blocks(b) == nt_blocks(n) else "differ"
            nt_bad += nt == "differ"
            changed = sum(1 for d in difflib.unified_diff(b, n, lineterm="", n=0) if d[0] in "+-" and d[:3] not in ("+++", "---"))
            counts = "same" if cb == cn else "DIFFER " + " ".join(f"{c} {x}->{y}" for c, x, y in zip(COUNTED, cb, cn) if x != y)
            bad |= cb != cn
            rows.append(f"| `{pretty[name]}` | {len(b)} -> {len(n)} | {changed} | {'same' if tb == tn else 'differs'} | {nt} | {counts} |")
    if show:
        return 0
    print("| kernel | instructions | lines changed | after the first s_barrier | blocks with non-temporal accesses "
          "| counted instructions |")
    print("|---|---|---|---|---|---|")
    print("\n".join(rows))
    print(f"\n{total} kernels of the base: {same} identical, {same_tail} identical from the first s_barrier on, "
          f"{nt_bad} with a differing block of non-temporal accesses, "
          + ("COUNTS DIFFER OR KERNELS MISSING" if bad else "every count as the base's"))
    return bad


if __name__ == "__main__":
    sys.exit(main())
