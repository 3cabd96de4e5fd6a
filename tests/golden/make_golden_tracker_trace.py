"""tracker_trace.json: the launch schedule of gen6d_amd.tracking.StreamTracker in the configurations of tests/test_tracker_trace_cpu.py,
recorded by that file's own recorder (imported, so the same code runs when the file is written and when it is checked).  Written at the
commit BEFORE the tracker's host class was restructured; rewrite it only from a commit whose schedule is the intended one.

    python tests/golden/make_golden_tracker_trace.py
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import ref_ops                          # noqa: E402
import test_tracker_trace_cpu as TT     # noqa: E402


def make_scene():
    """What the module fixture `scene` of tests/test_track_streams_cpu.py builds."""
    from gen6d_amd.synth_db import SyntheticDatabase
    from test_estimator_cpu import make_estimator
    mp = pytest.MonkeyPatch()
    ref_ops.patch_ops(mp)
    db = SyntheticDatabase(n_views=24, size=(96, 128), focal=140.0)
    est = make_estimator(refine_iter=2, damped=True)
    est.build(db, "all")
    _, que_ids = db.get_split("all")
    mp.undo()
    return est, [db.get_image(i) for i in que_ids[:4]], [db.get_K(i) for i in que_ids[:4]]


def main():
    est, frames, Ks = make_scene()
    out = {}
    for name, run in TT.CONFIGS.items():
        mp = pytest.MonkeyPatch()
        trace = TT.install(mp, est)
        run(est, frames, Ks)
        mp.undo()
        out[name] = trace
        print(f"{name}: {len(trace)} calls")
    with open(TT.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
