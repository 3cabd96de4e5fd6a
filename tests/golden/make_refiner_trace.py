"""refiner_trace.json: the launches of VolumeRefiner.run_feature_net, feature_volumes and run_volume_net in the configurations of
tests/refiner_trace.py, recorded by that file's own recorder (imported, so the same code runs when the file is written and when it is
checked) on an MI355X.  Written at the commit BEFORE the refiner's routing moved into one layer table and one route table
(refiner.ROUTES), with that commit's five route constants: this file is the record of how the golden was made and runs only against
a tree that still has those constants — `forcing` below sets them, where tests/routes.py sets entries of refiner.ROUTES today.
Rewrite the golden only from a commit whose launches are the intended ones, with a `forcing` for that commit.

    python tests/golden/make_refiner_trace.py [output file]
"""
import contextlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import refiner_trace as RT                      # noqa: E402
from gen6d_amd.network import refiner           # noqa: E402

# the forced configurations in the terms of the five constants
FORCED = {"embeds_only": ("VOLUME_PAIR_LAYERS", ("mean_embed", "var_embed")),
          "igemm_variant3": ("VOLUME_IGEMM_PAIR_LAYERS", {"conv1": 3, "conv3": 3, "conv5.0": 3, "conv5.3": 3}),
          "conv_out_only": ("FEATNET_PAIR_BRANCHES", ("conv_out",))}


@contextlib.contextmanager
def forcing(name):
    attr, value = FORCED[name]
    saved = getattr(refiner, attr)
    setattr(refiner, attr, value)
    try:
        yield
    finally:
        setattr(refiner, attr, saved)


def dump(out, path):
    """One call per line: a changed launch shows as a changed line."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (name, r) in enumerate(out.items()):
            calls = ",\n".join("   " + json.dumps(c, separators=(",", ":")) for c in r["trace"])
            f.write(f' {json.dumps(name)}: {{"labels": {json.dumps(r["labels"])},\n  "slots": {json.dumps(r["slots"])},\n  "trace": [\n{calls}]}}'
                    f'{"," if i + 1 < len(out) else ""}\n')
        f.write("}\n")


def main():
    out = {}
    for name in RT.CONFIGS:
        out[name] = RT.record(name, forcing)
        print(f"{name}: {len(out[name]['trace'])} calls, {len(out[name]['labels'])} labels, slots {out[name]['slots']}", flush=True)
    dump(out, sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "refiner_trace.json"))


if __name__ == "__main__":
    main()
