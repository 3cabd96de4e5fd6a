"""The refiner's launches, pinned: every call VolumeRefiner.run_feature_net, feature_volumes and run_volume_net make into `ops` — name,
arguments (shapes, strides, which buffer), result — with the labels the library books and the range slots, in the configurations of
tests/refiner_trace.py, equals tests/golden/refiner_trace.json.  tests/golden/make_refiner_trace.py wrote that file with the same recorder
on an MI355X at the commit before the routing moved into refiner.ROUTES, so a change to the tables or to the walk over them that moves,
adds, drops or re-arguments a launch shows here, call by call.  Values are not compared (the route tests do that)."""
import json
import os

import pytest

import refiner_trace as RT
from routes import forced_routes, igemm_layers, without, PAIR_KEYS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refiner_trace.json")
EMBEDS = tuple(k for k in PAIR_KEYS["volume"] if "embed" in k)
FORCED = {"embeds_only": lambda: without("pair", set(PAIR_KEYS["volume"]) - set(EMBEDS)),
          "igemm_variant3": lambda: {k: ("igemm3",) for k in igemm_layers()},
          "conv_out_only": lambda: without("pair", [k for k in PAIR_KEYS["featnet"] if "conv_out" not in k])}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(RT.CONFIGS))
def test_launches_equal_the_golden(golden, name):
    got = json.loads(json.dumps(RT.record(name, lambda forced: forced_routes(FORCED[forced]()))))
    want = golden[name]
    assert got["labels"] == want["labels"]
    assert got["slots"] == want["slots"]
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"{name}: call {i} differs"
    assert len(got["trace"]) == len(want["trace"])
