"""Per-kernel hashes and resource facts of the conv_igemm_kernel instantiations in two device-assembly files (the method of
tools/conv16w_asm_hash.py), to show that adding a math mode left the other instantiations' code as it was:
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -w -S --cuda-device-only -I include -o new.s gen6d_amd/csrc/conv_igemm.hip   (both trees)
    python tools/igemm_asm_hash.py old.s new.s
Instructions and directives only: comments, block-label numbering and the kernel's own mangled name are normalised.  Prints a markdown
table: instantiation <BM,BN,WGM,WGN,MODE,MM>, hash and line count in each file, SAME / DIFF / NEW, and for the second file the kernel's
VGPRs + AGPRs, spilled VGPRs, scratch bytes and occupancy (waves per SIMD) from the compiler's kernel-info comments and metadata."""
import hashlib
import re
import sys


def bodies(path):
    text = open(path).read()
    out = {}
    spills = {n: int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1))
              for n, b in re.findall(r"\.name:\s+(\S*conv_igemm_kernel\S*)\n(.*?)\.wavefront_size", text, re.S)}
    for m in re.finditer(r"^(_Z\w*conv_igemm_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n((?:[^\n]*\n){0,40})", text, re.S | re.M):
        name, raw, tail = m.group(1), m.group(2), m.group(3)
        body = raw.replace(name, "KERNEL")
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = "\n".join(l.split(";")[0].rstrip() for l in body.split("\n") if l.split(";")[0].strip())
        key = "<" + ",".join(re.findall(r"Li(\d+)E", name)) + ">"

        def fact(pat):
            f = re.search(pat, tail)
            return int(f.group(1)) if f else None
        res = {"vgpr": fact(r"; NumVgprs: (\d+)"), "agpr": fact(r"; NumAgprs: (\d+)"), "spill": spills.get(name),
               "scratch": fact(r"; ScratchSize: (\d+)"), "occ": fact(r"; Occupancy: (\d+)")}
        out[key] = (hashlib.sha256(body.encode()).hexdigest()[:16], body.count("\n") + 1, res)
    return out


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    print("| instantiation | old hash (lines) | new hash (lines) | code | VGPR + AGPR | VGPR spills | scratch B | waves / SIMD |")
    print("|---|---|---|---|---|---|---|---|")
    bad = 0
    for k in sorted(set(a) | set(b), key=lambda s: [int(x) for x in s[1:-1].split(",")]):
        x, y = a.get(k), b.get(k)
        same = "NEW" if x is None else "GONE" if y is None else "SAME" if x[:2] == y[:2] else "DIFF"
        bad += same in ("DIFF", "GONE")
        r = (y or x)[2]
        print(f"| `{k}` | {f'{x[0]} ({x[1]})' if x else '-'} | {f'{y[0]} ({y[1]})' if y else '-'} | {same} | {r['vgpr']} + {r['agpr']} | {r['spill']} | "
              f"{r['scratch']} | {r['occ']} |")
    print(f"\n{len(b)} instantiations, {bad} changed or removed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
