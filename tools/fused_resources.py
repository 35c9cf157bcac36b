"""Resource table of the fused product + checksum kernels from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (the stderr of compiling
daos_amd/csrc/kernels/ecg_fused_kernels.hip with that flag, or of `make
report`).  Needs no GPU.

  python tools/fused_resources.py NEW.txt             # table of NEW
  python tools/fused_resources.py NEW.txt BASE.txt    # + compare the plain
      instantiations with BASE's (exit 1 on any difference or on scratch in
      a SRC instantiation; SGPRs spilled into VGPR lanes are listed, they
      use no scratch)
  python tools/fused_resources.py --verify VERIFY.txt [PRODUCT.txt]
      the ecg_verify kernels, strided and cell-table (ptr) alike (remarks of
      ecg_verify_kernels.hip), each ptr lane kernel below its strided
      counterpart and each lane kernel beside its product counterpart from
      the remarks of ecg_kernels.hip; exit 1 if one uses scratch
  python tools/fused_resources.py --repair REPAIR.txt [NEW.txt BASE.txt]...
      the ecg_repair kernels, strided and cell-table (ptr) alike (remarks of
      ecg_repair_kernels.hip); exit 1 if one uses scratch.  Each NEW BASE pair after it: the remarks of one
      other kernel file from this tree and from the tree before, every
      kernel of which must show identical figures (mm_ptr_item moved into
      ecg_mm_dev.h; exit 1 on any difference)
  python tools/fused_resources.py --recover-masks RM.txt [NEW.txt BASE.txt]...
      the ecg_recover_masks kernels, strided and cell-table (ptr) alike
      (remarks of ecg_recover_masks_kernels.hip), SGPRs spilled into VGPR
      lanes listed; exit 1 if one uses scratch.  NEW BASE pairs as for
      --repair.  With --base BASE.txt right after RM.txt (the remarks of the
      same file from the tree before): every kernel of BASE must show
      identical figures in RM.txt, kernels only RM.txt has are new (exit 1
      on any difference)
  python tools/fused_resources.py --csum-masked NEW.txt BASE.txt
      the ecg_csum_masked kernels (remarks of ecg_csum_kernels.hip from this
      tree, NEW, and from the tree before, BASE): their table, exit 1 if one
      uses scratch; every kernel of BASE must show identical figures in NEW
      (exit 1 on any difference)
  python tools/fused_resources.py --update-masks UM.txt [NEW.txt BASE.txt]...
      the ecg_update_masks kernels, strided and cell-table (ptr) alike
      (remarks of ecg_update_masks_kernels.hip), SGPRs spilled into VGPR lanes listed;
      exit 1 if one uses scratch.  NEW BASE pairs as for --repair (upd_fold
      moved into ecg_mm_dev.h)
  python tools/fused_resources.py --agg-masks UM.txt [BASE.txt]
      the ecg_agg_masks kernels, strided and cell-table (ptr) alike (remarks
      of ecg_update_masks_kernels.hip, which holds them), SGPRs spilled into
      VGPR lanes listed; exit 1 if one uses scratch.  With BASE.txt (the
      remarks of the same file from the tree before): every kernel of BASE
      -- the ecg_update_masks kernels -- must show identical figures in
      UM.txt (exit 1 on any difference)
  python tools/fused_resources.py --kept NEW.txt BASE.txt [NEW.txt BASE.txt]...
      a refactor's check over any kernel files: every kernel of each BASE
      found by name in its NEW with VGPRs, AGPRs, scratch and LDS equal or
      lower and occupancy not lower (exit 1 otherwise); kernels whose
      figures differ at all are listed

The SRC flag is the last template argument of ecg_mm_csum_kernel; a build
from before it existed mangles the plain instantiations without it, which
the comparison accounts for."""
import re
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
NAME = re.compile(r"_Z18ecg_mm_csum_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)E(?:Lb([01])E)?Ev")


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            n = NAME.match(m.group(1))
            cur = None
            if n:
                k, r, w, _, tb, src = n.groups()
                cur = (int(k), int(r), int(w), int(tb), src == "1")
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.*?): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            out[cur][m.group(1)] = int(m.group(2))
    return out


VERIFY = re.compile(r"_Z\d+(ecg_verify_(?:ptr_)?(?:byte_|summary_)?kernel)(?:ILi(\d+)ELi(\d+)EE)?")
PRODUCT = re.compile(r"_Z13ecg_mm_kernelILi(\d+)ELi(\d+)ELb0ELb0ELi16EE")


def parse_named(path, pattern):
    """{(kernel name, K, R): fields} of the kernels whose mangled name matches `pattern`."""
    out, cur = {}, None
    for line in open(path):     # "remark: <file:line:col:> Function Name: ..." with or without the location
        m = re.search(r"\sFunction Name: (\S+)", line)
        if m:
            n = pattern.match(m.group(1))
            cur = None
            if n:
                g = n.groups()
                cur = (g[0], int(g[1] or -1), int(g[2] or -1)) if len(g) == 3 else ("ecg_mm_kernel", int(g[0]), int(g[1]))
                out[cur] = {}
            continue
        if cur is None:
            continue
        for f in FIELDS:
            m = re.search(r"\s" + re.escape(f) + r": (\d+)", line)
            if m:
                out[cur][f] = int(m.group(1))
    return out


def verify_table(verify_txt, product_txt=None):
    """Table of the ecg_verify kernels (remarks of ecg_verify_kernels.hip); with the
    remarks of ecg_kernels.hip, each lane kernel's VGPRs / occupancy beside its
    product counterpart ecg_mm_kernel<K,R,0,0> (16-byte lanes).  Exit 1 on scratch."""
    ver = parse_named(verify_txt, VERIFY)
    prod = parse_named(product_txt, PRODUCT) if product_txt else {}
    bad = 0
    extra = " product VGPRs | product waves/SIMD |" if prod else ""
    print("| kernel | " + " | ".join(FIELDS) + " |" + extra)
    print("|" + "---|" * (1 + len(FIELDS) + (2 if prod else 0)))
    # each cell-table (ptr) lane kernel right below its strided counterpart
    for key in sorted(ver, key=lambda t: (t[1] < 0, t[0] if t[1] < 0 else "", t[1] == 0, t[1], t[2], "ptr" in t[0])):
        name, k, r = key
        v = ver[key]
        label = f"`{name}<{k},{r}>`" if k >= 0 else f"`{name}`"
        row = f"| {label} | " + " | ".join(str(v.get(f, "")) for f in FIELDS) + " |"
        if prod:
            pv = prod.get(("ecg_mm_kernel", k, r), {})
            row += f" {pv.get('VGPRs', '')} | {pv.get('Occupancy [waves/SIMD]', '')} |"
        print(row)
        if v.get("ScratchSize [bytes/lane]") or v.get("VGPRs Spill"):
            print(f"SCRATCH in {label}", file=sys.stderr)
            bad = 1
    print(f"\nverify kernels: {len(ver)}, " + ("SCRATCH USED" if bad else "none uses scratch"))
    return bad


REPAIR = re.compile(r"_Z\d+(ecg_repair_(?:ptr_)?(?:byte_)?kernel)(?:ILi(\d+)EE)?()")
RECOVER_MASKS = re.compile(r"_Z\d+(ecg_recover_masks_(?:ptr_)?(?:byte_)?kernel)(?:ILi(\d+)ELi(\d+)EE)?")
UPDATE_MASKS = re.compile(r"_Z\d+(ecg_update_masks_(?:ptr_)?(?:byte_)?kernel)(?:ILi(\d+)EE)?()")
AGG_MASKS = re.compile(r"_Z\d+(ecg_agg_masks_(?:ptr_)?(?:byte_)?kernel)(?:ILi(\d+)EE)?()")
ANY = re.compile(r"(\S+)()()")


def repair_table(repair_txt, *pairs, pattern=REPAIR, what="repair"):
    """Table of the ecg_repair kernels (remarks of ecg_repair_kernels.hip), or with
    pattern=RECOVER_MASKS of the ecg_recover_masks kernels, exit 1 on scratch; then every
    kernel of each (new, base) pair of remarks files compared field by field."""
    rep = parse_named(repair_txt, pattern)
    bad = 0
    print("| kernel | " + " | ".join(FIELDS) + " |")
    print("|" + "---|" * (1 + len(FIELDS)))
    for key in sorted(rep, key=lambda t: ("byte" in t[0], t[1] == 0, t[1], t[2], t[0])):
        name, k, r = key
        v = rep[key]
        label = f"`{name}<{k}>`" if k >= 0 else f"`{name}`"
        if r >= 0:
            label = f"`{name}<{k},{r}>`"
        print(f"| {label} | " + " | ".join(str(v.get(f, "")) for f in FIELDS) + " |")
        if v.get("ScratchSize [bytes/lane]") or v.get("VGPRs Spill"):
            print(f"SCRATCH in {label}", file=sys.stderr)
            bad = 1
    print(f"\n{what} kernels: {len(rep)}, " + ("SCRATCH USED" if bad else "none uses scratch"))
    for new_txt, base_txt in zip(pairs[0::2], pairs[1::2]):
        new, base = parse_named(new_txt, ANY), parse_named(base_txt, ANY)
        diff = [key[0] for key in sorted(set(new) | set(base)) if new.get(key) != base.get(key)]
        for name in diff:
            print(f"DIFF {name}: base {base.get((name, -1, -1))} new {new.get((name, -1, -1))}", file=sys.stderr)
        bad |= bool(diff)
        print(f"{new_txt}: {len(new)} kernels compared with {base_txt}, " + ("DIFFERENT" if diff else "identical"))
    return bad


def kept_identical(new_txt, base_txt):
    """Every kernel in the remarks base_txt compared field by field with its figures in new_txt."""
    new, base = parse_named(new_txt, ANY), parse_named(base_txt, ANY)
    diff = [key[0] for key in sorted(base) if new.get(key) != base[key]]
    for name in diff:
        print(f"DIFF {name}: base {base.get((name, -1, -1))} new {new.get((name, -1, -1))}", file=sys.stderr)
    print(f"{new_txt}: the {len(base)} kernels of {base_txt} compared, " + ("DIFFERENT" if diff else "identical")
          + f"; {len(set(new) - set(base))} kernels are new\n")
    return int(bool(diff))


def kept_or_lower(*pairs):
    """Every kernel of each BASE remarks file found by name in its NEW file with VGPRs, AGPRs,
    scratch and LDS equal or lower and occupancy equal or higher; the kernels whose figures
    (SGPRs included) differ at all are listed."""
    bad = total = 0
    for new_txt, base_txt in zip(pairs[0::2], pairs[1::2]):
        new, base = parse_named(new_txt, ANY), parse_named(base_txt, ANY)
        total += len(base)
        for key in sorted(base):
            b, n = base[key], new.get(key)
            if n == b:
                continue
            worse = n is None or n["Occupancy [waves/SIMD]"] < b["Occupancy [waves/SIMD]"] or any(
                n[f] > b[f] for f in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"))
            what = "MISSING" if n is None else ", ".join(f"{f} {b[f]} -> {n[f]}" for f in FIELDS if n[f] != b[f])
            print(f"| `{key[0]}` | {what} | {'WORSE' if worse else 'ok'} |")
            bad |= worse
    print(f"\n{total} kernels of the base compared: " + ("A KERNEL IS WORSE OR MISSING" if bad else
          "VGPRs, AGPRs, scratch and LDS equal or lower and occupancy not lower in every one"))
    return int(bad)


MASKED = re.compile(r"ecg_(crc|adler)_masked_kernelI(?:Li(\d+)ELb([01])E)?Lb([01])E")


def csum_masked_table(new_txt, base_txt):
    """Table of the ecg_csum_masked kernels in the remarks of ecg_csum_kernels.hip (new_txt), exit 1
    on scratch; every kernel of base_txt (the same file of the tree before) compared field by
    field with its figures in new_txt."""
    new, base = parse_named(new_txt, ANY), parse_named(base_txt, ANY)
    bad, n = 0, 0
    print("| kernel | " + " | ".join(FIELDS) + " |")
    print("|" + "---|" * (1 + len(FIELDS)))
    for key in sorted(new):
        m = MASKED.search(key[0])
        if not m:
            continue
        n += 1
        kind, w, _, aligned = m.groups()
        label = f"`ecg_{kind}_masked_kernel<{'crc' + w + ',' if w else ''}{'aligned' if aligned == '1' else 'bytes'}>`"
        v = new[key]
        print(f"| {label} | " + " | ".join(str(v.get(f, "")) for f in FIELDS) + " |")
        if v.get("ScratchSize [bytes/lane]") or v.get("VGPRs Spill"):
            print(f"SCRATCH in {label}", file=sys.stderr)
            bad = 1
    print(f"\ncsum_masked kernels: {n}, " + ("SCRATCH USED" if bad else "none uses scratch"))
    diff = [key[0] for key in sorted(base) if new.get(key) != base[key]]
    for name in diff:
        print(f"DIFF {name}: base {base.get((name, -1, -1))} new {new.get((name, -1, -1))}", file=sys.stderr)
    print(f"{new_txt}: the {len(base)} kernels of {base_txt} compared, " + ("DIFFERENT" if diff else "identical"))
    return bad | bool(diff) | (n == 0)


def main():
    if sys.argv[1] == "--kept":
        return kept_or_lower(*sys.argv[2:])
    if sys.argv[1] == "--csum-masked":
        return csum_masked_table(*sys.argv[2:4])
    if sys.argv[1] == "--verify":
        return verify_table(*sys.argv[2:4])
    if sys.argv[1] == "--repair":
        return repair_table(*sys.argv[2:])
    if sys.argv[1] == "--recover-masks":
        args, bad = sys.argv[2:], 0
        if len(args) >= 3 and args[1] == "--base":
            bad = kept_identical(args[0], args[2])
            del args[1:3]
        return repair_table(*args, pattern=RECOVER_MASKS, what="recover_masks") | bad
    if sys.argv[1] == "--update-masks":
        return repair_table(*sys.argv[2:], pattern=UPDATE_MASKS, what="update_masks")
    if sys.argv[1] == "--agg-masks":
        bad = kept_identical(sys.argv[2], sys.argv[3]) if len(sys.argv) > 3 else 0
        return repair_table(sys.argv[2], pattern=AGG_MASKS, what="agg_masks") | bad
    new = parse(sys.argv[1])
    base = parse(sys.argv[2]) if len(sys.argv) > 2 else None
    bad = 0
    print("| K | R | W | TB | SRC | " + " | ".join(FIELDS) + " |")
    print("|" + "---|" * (5 + len(FIELDS)))
    for key in sorted(new, key=lambda t: (t[4], t[0], t[1], t[2])):
        k, r, w, tb, src = key
        v = new[key]
        print(f"| {k} | {r} | {w} | {tb} | {int(src)} | " + " | ".join(str(v.get(f, "")) for f in FIELDS) + " |")
        if src and (v.get("ScratchSize [bytes/lane]") or v.get("VGPRs Spill")):
            print(f"SCRATCH in SRC instantiation {key}", file=sys.stderr)
            bad = 1
        if base is not None and not src:
            if base.get(key) != v:
                print(f"DIFF {key}: base {base.get(key)} new {v}", file=sys.stderr)
                bad = 1
    if base is not None:
        n = sum(1 for key in new if not key[4])
        print(f"\nplain instantiations compared with the base: {n}, " + ("DIFFERENT" if bad else "identical"))
    return bad


if __name__ == "__main__":
    sys.exit(main())
