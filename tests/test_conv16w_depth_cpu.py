"""Depth-folded 3x3x3 layers on the halo-patch pair kernel, without a launch: what g6d_conv16_direct_plan accepts (fake, 16-byte aligned
addresses; nothing is dereferenced) — planes at least one tile high, no pooling, statistics groups of whole volumes, pairs only — and the
folded filter order (ops.conv16_fold_depth, ops.conv16_pack layout 2) against a numpy restatement."""
import ctypes as C

import numpy as np
import torch

from gen6d_amd import lib, ops

EINVAL = -1
FAKE = 0x7F0000000000


def _plan(N=2, D=3, H=16, W=16, Cin=32, Cout=128, w_layout=2, kd=3, full=2, pool=0, mode=3, rpg=0, ld_pool=0):
    L = lib.load()
    seg = (lib.G6dConv16Seg * 1)(lib.G6dConv16Seg(in_=FAKE, out_full=FAKE + (1 << 32), out_pool=(FAKE + (2 << 32)) if pool else None, N=N, D=D, H=H, W=W,
                                                  ld_in=2 * Cin, ld_full=2 * Cout if full == 3 else Cout, ld_pool=ld_pool))
    rc = L.g6d_conv16_direct_plan(seg, 1, Cin, C.c_void_p(FAKE + (3 << 32)), w_layout, Cout, kd, full, pool, mode,
                                  C.c_void_p(FAKE + (4 << 32)) if rpg else None, rpg)
    return rc, L.g6d_last_error().decode()


def test_plan_accepts_planes_of_whole_tiles():
    for kw in (dict(), dict(Cout=64), dict(D=1), dict(H=16, W=24, Cout=64), dict(H=18, W=20), dict(H=32, W=32, D=32, Cin=256, Cout=64, N=16),
               dict(full=3), dict(rpg=3 * 16 * 16), dict(rpg=2 * 3 * 16 * 16)):
        assert _plan(**kw)[0] == 1, kw
    assert ops.conv16_direct_plan(16, 32, 32, 128, 64, 3, stats_rows=32 ** 3, D=32) == 1


def test_plan_rejects_what_the_folded_kernel_cannot_tile():
    halo_only = "depth-folded filters run on the halo-patch kernel only"
    rc, msg = _plan(H=2, W=64)                                     # every tile width: a tile higher than the plane (banded tiles span planes)
    assert rc == EINVAL and halo_only in msg, msg
    rc, msg = _plan(H=8, W=8)                                      # tw = 8 -> th = 16 > 8; tw = 16 -> th = 8 fits: accepted
    assert rc == 1, msg
    rc, msg = _plan(H=2, W=8)
    assert rc == EINVAL and halo_only in msg, msg
    rc, msg = _plan(rpg=16 * 16)                                   # a group of one plane: not whole volumes
    assert rc == EINVAL and halo_only in msg, msg
    rc, msg = _plan(rpg=3 * 16 * 16 + 128)
    assert rc == EINVAL and halo_only in msg, msg
    rc, msg = _plan(pool=3, ld_pool=256)
    assert rc == EINVAL and "pooling is 2-D only" in msg, msg
    for kw in (dict(mode=2), dict(mode=1), dict(kd=1, D=1)):       # pairs with three depth taps only
        rc, msg = _plan(**kw)
        assert rc == EINVAL and "math_mode 1 (bf16) / 2 (fp16) / 3" in msg, (kw, msg)
    assert ops.conv16_direct_plan(2, 2, 8, 32, 128, 3, D=3) is None


def test_unfolded_layouts_keep_their_answers():
    assert _plan(w_layout=1, kd=1, D=1)[0] == 1                    # the 2-D halo route
    assert _plan(w_layout=1, kd=3)[0] == 0                         # 27-tap fragment-major filters: the per-tap kernel, as before


def test_folded_filter_order():
    g = torch.Generator().manual_seed(3)
    co, ci = 128, 64
    w = torch.rand((co, 27, ci), generator=g) * 2 - 1
    f = ops.conv16_fold_depth(w).numpy()
    wn = w.numpy()
    want = np.empty((co, 9, 3 * ci), np.float32)
    for kz in range(3):
        for t in range(9):
            want[:, t, kz * ci:(kz + 1) * ci] = wn[:, kz * 9 + t, :]
    assert f.shape == want.shape and np.array_equal(f, want)
    # layout 2 = the fragment-major pack of that bank, with the layer's own shape on the handle
    a, b = ops.conv16_pack(w, 3, layout=2), ops.conv16_pack(torch.from_numpy(want), 3, layout=1)
    assert (a.layout, a.taps, a.Cin, a.Cout, a.mode) == (2, 27, ci, co, 3) and a.acc_scale == b.acc_scale
    assert torch.equal(a.data, b.data)
    # slice c of the packed bank is channel slice c % (Cin / 32) of depth tap c / (Cin / 32): [tile][slice][tap][ks][plane][j][half][l31][e]
    x = a.data.view(co // 128, 3 * ci // 32, 9, 2, 2, 4, 2, 32, 8)
    S = 1.0 / a.acc_scale
    for c in (0, 1, 2, 5):
        dz, cc = divmod(c, ci // 32)
        blk = x[0, c, 4, :, 0].permute(1, 3, 0, 2, 4).reshape(128, 32).float()          # hi plane of tap (1, 1): [co][ks, half, e]
        ref = (w[:, dz * 9 + 4, cc * 32:(cc + 1) * 32].double() * S).to(torch.float16).float()
        assert torch.equal(blk, ref), c
    # Cout = 64: one 128-channel tile whose upper half is zero, as for the 2-D layers
    h = ops.conv16_pack(w[:64], 3, layout=2)
    assert h.Cout == 64 and h.data.numel() == a.data.numel()
