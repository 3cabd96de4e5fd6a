"""Per-image statistics of the halo-patch kernel (conv16w_kernel) where a 128-pixel tile holds SEVERAL images: 8 x 8 maps sit two to a
tile (two bands), and with one statistics group per image the wave-private sums are flushed after every 64-pixel epilogue pass under the
pass's own group — the refiner's feature net normalises its 8 x 8 maps per image.  fp32 output plus statistics, compared with the float64
convolution of the fp32 operands (16-bit mode: of the rounded operands) and its float64 sums PER IMAGE, bars and form of the statistics
cases of test_conv16w_edges_gpu.py (2e-6 of range for pairs, 2e-5 in a 16-bit mode; sums per pixel of the group, squares twice the bar).
The output lies in a NaN-filled guarded buffer and the statistics table between two guard groups that must keep their fill."""
import pytest
import torch
import torch.nn.functional as F

from parity_log import record
from test_conv16w_edges_gpu import T16, _halo_tw, _launch, _rand, _split

pytestmark = pytest.mark.gpu

GUARD_FILL = 12345.0

CASES = [
    # rpg: pixels per statistics group; plan: what g6d_conv16_direct_plan must answer (2 = a flush per pass, 1 = one flush per tile)
    dict(id="3img-last-tile-half", seg=(3, 8, 8), Cin=32, Cout=128, rpg=64, plan=2),        # odd image count: the last tile half filled
    dict(id="5img-two-tile-blocks", seg=(5, 8, 8), Cin=64, Cout=64, rpg=64, plan=2),        # two-tile blocks (Cout = 64), three tiles
    dict(id="4img-group-per-tile", seg=(4, 8, 8), Cin=32, Cout=128, rpg=128, plan=1),       # the unchanged single-flush path
    dict(id="2img-in-image-tiles", seg=(2, 16, 16), Cin=32, Cout=64, rpg=256, plan=1),      # tiles inside one image
    dict(id="3img-fp16", seg=(3, 8, 8), Cin=64, Cout=128, rpg=64, plan=2, mode=2),          # the 16-bit wave form through the same flush
]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_band_stats(case, knob):
    from gen6d_amd import ops
    knob("conv16_halo", 1)
    c = case
    mode, Cin, Cout, rpg = c.get("mode", 3), c["Cin"], c["Cout"], c["rpg"]
    N, H, W = c["seg"]
    pair = mode == 3
    assert _halo_tw(N, H, W)[0] == (8 if H == 8 else 16), "the case no longer has the tiling it was written for"
    assert ops.conv16_direct_plan(N, H, W, Cin, Cout, mode, stats_rows=rpg) == c["plan"]
    g = torch.Generator().manual_seed(101 + N + Cin + Cout)
    w = _rand(g, Cout, 9, Cin, scale=(1.0 / (9 * Cin)) ** 0.5 * 3)
    b = _rand(g, Cout, scale=0.2)
    x = _rand(g, N, H, W, Cin)
    x = x * (1.0 + torch.arange(N).view(N, 1, 1, 1))           # every image its own scale: sums filed under a neighbour's group show
    if not pair:
        w, x = w.to(T16[mode]).float(), x.to(T16[mode]).float()
    G = N * H * W // rpg
    table = torch.zeros((G + 2, Cout, 2), dtype=torch.float64, device="cuda")
    table[0] = GUARD_FILL
    table[-1] = GUARD_FILL
    stats = table[1:G + 1]
    filt = ops.conv16_pack(w.cuda(), mode, 1)
    xin = (_split(x) if pair else x.to(T16[mode])).cuda()
    fulls, _ = _launch([xin], filt, b.cuda(), False, "f32", None, stats, rpg)
    base = 2e-6 if pair else 2e-5
    w4 = w.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w4, b.double(), padding=1).permute(0, 2, 3, 1)
    rng = float(ref.abs().max())
    got = table.cpu()
    assert bool((got[0] == GUARD_FILL).all() and (got[-1] == GUARD_FILL).all()), "statistics were added outside the table's groups"
    n = rpg
    s1, s2 = ref.reshape(G, -1, Cout).sum(1), (ref * ref).reshape(G, -1, Cout).sum(1)
    e1 = float((got[1:-1, :, 0] - s1).abs().max()) / n / rng
    e2 = float((got[1:-1, :, 1] - s2).abs().max()) / n / rng ** 2
    e = float((fulls[0].map.cpu().double() - ref).abs().max()) / rng
    print(f"{c['id']}: output error / range {e:.3e} (bar {base:.0e}), sums {e1:.3e} (bar {base:.0e}), squares {e2:.3e} (bar {2 * base:.0e})")
    record("test_conv16w_band_stats", f"banded statistics {c['id']} {c['seg']} x{Cin} -> {Cout}, {rpg} px / group (error / bar)",
           max(e, e1, e2 / 2) / base, 1.0, note="output, per-group sums and squares vs fp64")
    assert e <= base, ("output", e)                           # (NaN — a pixel never written — fails here too)
    assert fulls[0].untouched(), "the output wrote outside its map"
    assert e1 <= base, ("statistics: sum", e1)
    assert e2 <= 2 * base, ("statistics: sum of squares", e2)
