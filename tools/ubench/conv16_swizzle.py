"""LDS slot swizzle search for the halo-patch kernel (conv16w_kernel): patch rows of 64 B (4 slots of 16 B); physical slot s of patch
(row, column) holds logical slot s ^ sw(row, column), sw = ((column >> a) + row * d) & 3.  For every tile width and banded layout of
c16g::halo_tiling (csrc/conv16w_geom.h), all nine tap shifts and every ds_read_b128 lane group (4 x 16 lanes, one LDS cycle each when the 16 lanes hit 16
distinct 16-byte bank slots), prints the LDS cycles per lane group (1 = conflict-free) of the best (a, d) for the two read patterns:
  16-bit modes (32x32x16 fragments): lane l reads tile pixel 32 mt + (l & 31), logical slot 2 ks + (l >> 5);
  fp16 pairs (16x16x32 fragments):   lane l reads tile pixel 16 mt + (l & 15), logical slot l >> 4."""
import itertools

GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS += [[l + 32 for l in g] for g in GROUPS]


def layouts():
    """(tile width, rows per band) of every halo tiling: bands of segh + 2 patch rows, at most 288 patch rows of TW + 2."""
    for tw in (4, 8, 16, 32):
        th = 128 // tw
        for segh in (1, 2, 4, 8, 16, 32):
            if segh <= th and th % segh == 0 and (th // segh) * (segh + 2) * (tw + 2) <= 288:
                yield tw, segh


def reads(pattern):
    """(m-tile, k-group, lane) -> (tile pixel, logical slot) of one fragment read."""
    if pattern == "pairs":
        return [[[(16 * mt + (l & 15), l >> 4) for l in range(64)]] for mt in range(8)]
    return [[[(32 * mt + (l & 31), 2 * ks + (l >> 5)) for l in range(64)] for ks in range(2)] for mt in range(4)]


def patch_rc(p, tw, segh, ky, kx):
    py, px = p // tw, p % tw
    b, ly = py // segh, py % segh
    return b * (segh + 2) + ly + ky, px + kx


def cycles(tw, segh, sw, pattern):
    """(worst, mean) LDS cycles per lane group over m-tiles, k-groups, taps and groups."""
    worst, tot, n = 0, 0, 0
    for per_mt in reads(pattern):
        for lanes in per_mt:
            for ky, kx in itertools.product(range(3), range(3)):
                for g in GROUPS:
                    cnt = {}
                    for l in g:
                        p, s = lanes[l]
                        r, col = patch_rc(p, tw, segh, ky, kx)
                        k = (4 * (r * (tw + 2) + col) + (s ^ sw(r, col))) % 16
                        cnt[k] = cnt.get(k, 0) + 1
                    m = max(cnt.values())
                    worst, tot, n = max(worst, m), tot + m, n + 1
    return worst, tot / n


if __name__ == "__main__":
    for pattern in ("16-bit", "pairs"):
        for tw, segh in layouts():
            res = []
            for a, d in itertools.product(range(4), range(4)):
                w, avg = cycles(tw, segh, lambda r, c, a=a, d=d: ((c >> a) + r * d) & 3, pattern)
                res.append((avg, w, d, a))
            avg, w, d, a = min(res)
            print(f"{pattern:7s} TW {tw:2d} rows per band {segh:2d}: best a = {a}, d = {d}: {avg:.2f} cycles per group (worst {w})")
