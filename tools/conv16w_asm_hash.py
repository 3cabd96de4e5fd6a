"""Per-kernel hashes of the conv16w_kernel instantiations in two device-assembly files, to show that a change left an instantiation's
code as it was:
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -w -S --cuda-device-only -I include -o new.s gen6d_amd/csrc/conv16w.hip   (both trees)
    python tools/conv16w_asm_hash.py old.s new.s [kernel-name pattern]
The optional third argument is a regular expression for the kernels' (mangled) names, default conv16w_kernel: `kernel` covers every
kernel of a translation unit, whichever file the two assembly files were built from.  The tool also serves gen6d_amd/csrc/conv16_tap.hip
(pattern conv16r?_kernel), gen6d_amd/csrc/corr16.hip (pattern corr16_kernel) and the Winograd family, gen6d_amd/csrc/wino_conv.hip,
wino16_conv.hip and wino43_conv.hip (pattern kernel, built with -fno-slp-vectorize as the Makefile builds them), and a kernel that moved
between files: old.s and new.s need not come from the same source file, and new.s may be several assembly files concatenated.
Instructions and directives only: comments, block-label numbering and the kernel's own mangled name are normalised, and a trailing
KD = 1 template argument is dropped from the name, so that an instantiation keeps its key when the template gains that parameter (a
FOURTH argument equal to 1 only: of the Winograd family this shortens wino_conv3x3_kernel<0,1,4,1> alone, to a key no other
instantiation has; the three-argument wino16_conv_kernel<MM,MODE,KD> and wino43_kernel<MODE,KD,NT> keep theirs)."""
import re, sys, hashlib
def bodies(path, pat):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w*(?:%s)\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:" % pat, text, re.S | re.M):
        name = m.group(1)
        body = m.group(2).replace(name, "KERNEL")
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = "\n".join(l.split(";")[0].rstrip() for l in body.split("\n") if l.split(";")[0].strip())
        key = re.sub(r"(ILi\dELi\dELi\d)ELi1(EEEvNS)", r"\1\2", name)
        out[key] = (hashlib.sha256(body.encode()).hexdigest()[:16], body.count("\n") + 1)
    return out
pat = sys.argv[3] if len(sys.argv) > 3 else "conv16w_kernel"
a, b = bodies(sys.argv[1], pat), bodies(sys.argv[2], pat)
for k in sorted(set(a) | set(b)):
    print(k, a.get(k), b.get(k), "SAME" if a.get(k) == b.get(k) else "DIFF")
