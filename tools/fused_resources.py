"""Resource table of the fused product + checksum kernels from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (the stderr of compiling
daos_amd/csrc/kernels/ecg_fused_kernels.hip with that flag, or of `make
report`).  Needs no GPU.

  python tools/fused_resources.py NEW.txt             # table of NEW
  python tools/fused_resources.py NEW.txt BASE.txt    # + compare the plain
      instantiations with BASE's (exit 1 on any difference or on scratch in
      a SRC instantiation; SGPRs spilled into VGPR lanes are listed, they
      use no scratch)

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


def main():
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
