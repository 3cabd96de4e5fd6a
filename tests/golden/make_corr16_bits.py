"""Records tests/golden/corr16_bits.json: a SHA-256 of every output map of g6d_corr16_multi, and its largest |value|, for the two small
multi-map cases that reach every tile width of corr16_kernel (gen6d_amd/csrc/corr16.hip), in bf16, fp16 and pair mode.  Run it ON THE GPU
at the commit whose bits are to be pinned:

    python tests/golden/make_corr16_bits.py

tests/test_corr16_bits_gpu.py imports this module for the cases and replays them against the file.  The inputs come from seeded CPU
generators; the kernel has no atomics and a fixed summation order, so equal arithmetic gives equal bits."""
import hashlib
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "corr16_bits.json")
MODES = {"bf16": 1, "fp16": 2, "pairs": 3}
CASES = {
    "k7": dict(N=2, sizes=[(3, 31), (7, 15), (15, 7), (31, 3)], Cin=96, k=7),       # tile widths 32, 16, 8, 4; 3 (pairs: 6) slices
    "k15": dict(N=2, sizes=[(9, 13), (15, 7), (22, 30)], Cin=96, k=15),             # tile widths 16, 8, 16, all ragged
}


def run(case, mode):
    """One launch -> [{"sha256": ..., "amax": ...} per output map] (fp32 maps [N][1][H][W][32], pre-filled: every element must be written)."""
    from gen6d_amd import ops
    c, pairs = CASES[case], mode == "pairs"
    t16 = torch.bfloat16 if mode == "bf16" else torch.float16
    g = torch.Generator().manual_seed(1000 + c["k"])
    T = c["k"] * c["k"]
    w = (torch.rand((32, T, c["Cin"]), generator=g) * 2 - 1) * (3.0 / (T * c["Cin"])) ** 0.5
    xs = [torch.rand((c["N"], h, ww, c["Cin"]), generator=g) * 2 - 1 for h, ww in c["sizes"]]
    if pairs:
        xin = [torch.stack([x.half(), (x - x.half().float()).half()], -2).contiguous().cuda() for x in xs]
    else:
        xin = [x.to(t16).cuda() for x in xs]
    outs = [torch.full((c["N"], 1, h, ww, 32), float("nan"), device="cuda") for h, ww in c["sizes"]]
    ops.corr16_multi(xin, ops.corr16_pack(w.cuda(), MODES[mode]), outs)
    torch.cuda.synchronize()
    res = []
    for o in outs:
        a = o.cpu().contiguous()
        assert not torch.isnan(a).any(), "an output element was left unwritten"
        res.append({"sha256": hashlib.sha256(a.numpy().tobytes()).hexdigest(), "amax": float(a.abs().max())})
    return res


def main():
    d = {f"{case}.{mode}": run(case, mode) for case in CASES for mode in MODES}
    with open(PATH, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {PATH}: {len(d)} launches")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    main()
