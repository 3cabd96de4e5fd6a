"""refiner.resolve_routes — the one function that turns refiner.ROUTES into the route every layer takes in a call — with injected
admission answers (no GPU, no library): the expected route of every layer for big / small calls, with and without a range table, with
every layer admitted / one listed layer refused / one feature branch refused / crops that are no multiple of 16, and with both / only
one embed listed; and the admission questions derived from the layer table against the two hand-written lists they replace."""
import pytest

from gen6d_amd.network import refiner as R

V, F = R.VOLUME, R.FEATNET
V_SIZE, F_SIZE = (32, 32, 32), (128, 128)
EMBEDS = ["volume.mean_embed.0", "volume.mean_embed.3", "volume.var_embed.0", "volume.var_embed.3"]
V_PAIR = EMBEDS + ["volume.conv0", "volume.conv2"]
V_IGEMM = ["volume.conv1", "volume.conv3", "volume.conv5.0", "volume.conv5.3"]
F_F43 = ["featnet.conv1.0", "featnet.conv_out.0", "featnet.conv_out.3"]
BRANCHES = ["conv0", "conv1", "conv2", "conv_out"]
ALL = {k: 1 for k in R.ROUTES}


def volume(big=True, rng=True, rng_part=None, answers=ALL, routes=None):
    return R.resolve_routes(V, R.ROUTES if routes is None else routes, V_SIZE, big, rng, rng if rng_part is None else rng_part, answers)


def featnet(big=True, rng=True, answers=ALL, size=F_SIZE):
    return R.resolve_routes(F, R.ROUTES, size, big, rng, rng, answers)


def expect(keys, **routes):
    """{layer: route} from route=[layers] with every other layer of `keys` on "cores"."""
    out = {k: "cores" for k in keys}
    out.update({k: r for r, ks in routes.items() for k in ks})
    return out


V_KEYS, F_KEYS = [L.key for L in V.layers], [L.key for L in F.layers]
V_CORES_BIG = expect(V_KEYS, f43=EMBEDS + ["volume.conv0"])                   # the fp32 cores' kernels of a big call: conv2 / conv4 on F(2x2,3x3)


def test_the_table_names_layers_and_holds_todays_routes():
    assert set(R.ROUTES) <= set(V_KEYS) | set(F_KEYS)
    assert [k for k in V_KEYS + F_KEYS if "pair" in R.ROUTES.get(k, ())] == V_PAIR + F_KEYS
    assert {k: R.ROUTES[k] for k in V_IGEMM} == {k: ("igemm5",) for k in V_IGEMM}
    assert R.ROUTES["volume.conv4"] == ()
    assert [k for k in V_KEYS + F_KEYS if "f43" in R.ROUTES.get(k, ())] == EMBEDS + ["volume.conv0"] + F_F43


def test_volume_net_big_call_with_a_range_table():
    assert volume() == expect(V_KEYS, pair=V_PAIR, igemm5=V_IGEMM)            # conv4 stays on the fp32 cores (F(2x2,3x3))


def test_volume_net_small_calls_take_the_cores_and_no_f43():
    for rng in (True, False):
        assert volume(big=False, rng=rng) == expect(V_KEYS)                   # w_wino43 is passed in big calls only


def test_volume_net_without_a_range_table():
    assert volume(rng=False) == V_CORES_BIG                                   # fp32_cores, a fallback recompute, a 16-bit mode


def test_volume_pair_kernel_is_all_or_nothing():
    for refused in V_PAIR:
        for answer in (None, 0):
            got = volume(answers={**ALL, refused: answer})
            assert got == {**V_CORES_BIG, **{k: "igemm5" for k in V_IGEMM}}, refused
    for embed in EMBEDS:                                                      # both embeds must be listed: one launch writes BOTH volumes as pairs
        routes = {**R.ROUTES, embed: ("f43",)}
        assert volume(routes=routes) == {**V_CORES_BIG, **{k: "igemm5" for k in V_IGEMM}}, embed
    # conv0 / conv2 may be left out: the embeds go on, `cat` and conv2's input stay fp32
    routes = {**R.ROUTES, "volume.conv0": ("f43",), "volume.conv2": ()}
    assert volume(routes=routes) == expect(V_KEYS, pair=EMBEDS, igemm5=V_IGEMM, f43=["volume.conv0"])


def test_volumes_are_written_as_pairs_exactly_when_the_embeds_take_the_pair_kernel():
    """feature_volumes asks the plan for the route of the layer that reads mean_in: it is "pair" exactly when every listed layer's is."""
    reader = V.reader("volume.mean_in").key
    for big in (True, False):
        for rng in (True, False):
            for answers in (ALL, {**ALL, "volume.conv2": None}):
                got = volume(big=big, rng=rng, answers=answers)
                assert {got[k] == "pair" for k in V_PAIR} == {got[reader] == "pair"} == {big and rng and answers is ALL}


def test_igemm_pair_layers_follow_their_own_part():
    """Independent of the pair kernel's admission: a big call and a range table inside the layer's own part are all they need — under an
    outer 16-bit mode with lowp_keep_fp32 = ("stack", "tail") the embeds (decided where the volumes are made) stay off pairs, they run."""
    assert volume(rng=False, rng_part=True) == {**V_CORES_BIG, **{k: "igemm5" for k in V_IGEMM}}
    assert volume(rng=True, rng_part=False) == {**expect(V_KEYS, pair=V_PAIR)}               # (a 16-bit part inside an fp32 call)
    assert volume(big=False, rng=True, rng_part=True) == expect(V_KEYS)
    routes = {**R.ROUTES, **{k: ("igemm3",) for k in V_IGEMM}, "volume.conv4": ("igemm4",)}
    assert volume(routes=routes) == expect(V_KEYS, pair=V_PAIR, igemm3=V_IGEMM, igemm4=["volume.conv4"])


def test_feature_net_big_call_with_a_range_table():
    got = featnet()
    assert got == expect(F_KEYS, pair=F_KEYS)
    assert featnet(answers={k: 2 for k in R.ROUTES}) == got                   # statistics groups of whole epilogue passes: admitted too


def test_feature_net_admission_is_per_branch():
    for b in BRANCHES:
        for i in (0, 3):
            got = featnet(answers={**ALL, f"featnet.{b}.{i}": None})
            mine = [f"featnet.{b}.0", f"featnet.{b}.3"]
            want = expect(F_KEYS, pair=[k for k in F_KEYS if k not in mine], f43=[k for k in mine if k in F_F43])
            assert got == want, (b, i)
            # `cat` is a pair map exactly when conv_out runs on pairs
            assert (got[F.reader("featnet.cat").key] == "pair") == (b != "conv_out")


@pytest.mark.parametrize("size", [(120, 128), (128, 136), (8, 8)])
def test_feature_net_crops_that_are_no_multiple_of_16(size):
    assert featnet(size=size) == expect(F_KEYS, f43=F_F43)


def test_feature_net_small_calls_and_no_range_table():
    for rng in (True, False):
        assert featnet(big=False, rng=rng) == expect(F_KEYS)                  # f43=False (the cached-feature path): neither pairs nor F(4x4,3x3)
    assert featnet(rng=False) == expect(F_KEYS, f43=F_F43)


def test_admission_shapes_come_from_the_layer_table():
    got = R.admission_shapes(V, R.ROUTES, 4, V_SIZE)
    # (edge, Cin, Cout) per layer; as a set, the list volume_pair_route wrote out by hand: (sn, 256, 64), (sn, 128, 64), (sn, 64, 64),
    # conv0's (sn, 128, 64), conv2's (sn / 2, 128, 128)
    want = {"volume.mean_embed.0": (32, 256, 64), "volume.mean_embed.3": (32, 64, 64), "volume.var_embed.0": (32, 128, 64),
            "volume.var_embed.3": (32, 64, 64), "volume.conv0": (32, 128, 64), "volume.conv2": (16, 128, 128)}
    assert got == {k: (4, s, s, ci, co, s ** 3, s) for k, (s, ci, co) in want.items()}        # statistics groups of whole volumes, depth s
    assert set(want.values()) == {(32, 256, 64), (32, 128, 64), (32, 64, 64), (32, 128, 64), (16, 128, 128)}
    # the four branch tuples of _featnet_pair_branches: (divisor, Cin, Cmid, Cout)
    hand = {"conv0": (4, 256, 64, 64), "conv1": (8, 512, 256, 64), "conv2": (16, 512, 256, 64), "conv_out": (4, 192, 128, 128)}
    for b, (d, ci, cm, co) in hand.items():
        l0, l3 = F.layer(f"featnet.{b}.0"), F.layer(f"featnet.{b}.3")
        assert (l0.div, l0.cin, l0.cout, l3.cout) == (d, ci, cm, co) and (l3.div, l3.cin) == (d, cm)
    got = R.admission_shapes(F, R.ROUTES, 28, (128, 96))
    assert got == {f"featnet.{b}.{i}": (28, 128 // d, 96 // d, a, c, (128 // d) * (96 // d), None)
                   for b, (d, ci, cm, co) in hand.items() for i, a, c in ((0, ci, cm), (3, cm, co))}
    # only listed layers are asked about
    assert set(R.admission_shapes(V, {"volume.conv2": ("pair",)}, 4, V_SIZE)) == {"volume.conv2"}
