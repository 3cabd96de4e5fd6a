"""Statistics groups of g6d_conv16_direct_multi_ex on tiles that hold several small images, validated without a GPU: the library checks a
table before it launches, and g6d_conv16_direct_plan runs the same validation and kernel choice with no launch at all (fake, 16-byte
aligned addresses; nothing is dereferenced).  A group must be whole 64-pixel epilogue passes of the banded tile: 16-pixel groups on 4 x 4
maps (four images per pass) and 96-pixel groups on 8 x 8 maps are refused with a message and never summed into a wrong group; one group
per 8 x 8 image — two per tile — is accepted and takes the per-pass flush."""
import ctypes as C

from gen6d_amd import lib

EINVAL = -1
BASE_IN, BASE_FULL, FAKE = 0x10000000, 0x200000000, 0x70000000
MESSAGE = "conv16_direct: statistics groups must be whole tile rows (small maps: whole 64-pixel epilogue passes)"
HALF_TILE = "conv16_direct: Cout = 64 needs a halo tiling for every segment"


def _seg(N, H, W, Cin, Cout, pairs):
    return lib.G6dConv16Seg(in_=BASE_IN, out_full=BASE_FULL, out_pool=None, N=N, D=1, H=H, W=W, ld_in=(2 if pairs else 1) * Cin, ld_full=Cout,
                            ld_pool=0)


def _plan(N, H, W, rpg, Cin=32, Cout=128, mode=3):
    L = lib.load()
    t = (lib.G6dConv16Seg * 1)(_seg(N, H, W, Cin, Cout, mode == 3))
    rc = L.g6d_conv16_direct_plan(t, 1, Cin, C.c_void_p(FAKE), 1, Cout, 1, 2, 0, mode, C.c_void_p(FAKE + 4096), rpg)
    return rc, L.g6d_last_error().decode()


def _launch_rc(N, H, W, rpg, Cin=32, Cout=128, mode=3):
    """The launching entry point on an INVALID table only: it returns before any HIP call."""
    L = lib.load()
    t = (lib.G6dConv16Seg * 1)(_seg(N, H, W, Cin, Cout, mode == 3))
    rc = L.g6d_conv16_direct_multi_ex(t, 1, Cin, C.c_void_p(FAKE), 1, 1.0, None, Cout, 1, 0, 2, 0, mode, C.c_void_p(FAKE + 4096), rpg, None, None)
    return rc, L.g6d_last_error().decode()


def test_groups_smaller_than_a_pass_are_rejected():
    # 16 images of 4 x 4: tiles of 4 columns x 32 rows = eight images, a pass = four of them
    for call in (_plan, _launch_rc):
        assert call(16, 4, 4, 16) == (EINVAL, MESSAGE)
        assert call(16, 4, 4, 16, Cin=64, mode=2) == (EINVAL, MESSAGE)
        assert call(16, 4, 4, 16, Cout=64) == (EINVAL, HALF_TILE)           # (Cout = 64 has no per-tap kernel to fall back to)


def test_groups_not_aligned_to_a_pass_are_rejected():
    # 96 pixels on 8 x 8 maps: one and a half images
    for call in (_plan, _launch_rc):
        assert call(6, 8, 8, 96) == (EINVAL, MESSAGE)
        assert call(6, 8, 8, 96, Cin=64, mode=2) == (EINVAL, MESSAGE)
        assert call(6, 8, 8, 96, Cout=64) == (EINVAL, HALF_TILE)


def test_one_group_per_8x8_image_is_accepted_up_to_the_launch():
    for N in (2, 3, 5, 112):
        for kw in (dict(), dict(Cout=64), dict(Cin=64, Cout=256), dict(Cin=64, mode=2), dict(Cin=64, mode=1)):
            assert _plan(N, 8, 8, 64, **kw)[0] == 2, (N, kw)                 # the halo-patch kernel, one flush per pass
    # groups of whole tiles and in-image tiles keep the single flush; whole passes of several images are groups too
    assert _plan(4, 8, 8, 128)[0] == 1
    assert _plan(2, 16, 16, 256, Cout=64)[0] == 1
    assert _plan(112, 32, 32, 1024)[0] == 1
    assert _plan(16, 4, 4, 64)[0] == 2
    # without statistics nothing changes: the plan of the plain launch
    L = lib.load()
    t = (lib.G6dConv16Seg * 1)(_seg(3, 8, 8, 32, 128, True))
    assert L.g6d_conv16_direct_plan(t, 1, 32, C.c_void_p(FAKE), 1, 128, 1, 2, 0, 3, None, 0) == 1
