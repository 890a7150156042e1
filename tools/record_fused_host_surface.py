"""Record the host surface of the fused attention blocks and the feed-forward chain (tests/fused_host_surface_common.py) into
tests/golden/fused_host_surface.json.

    python tools/record_fused_host_surface.py [--out FILE] [--commit HASH]

Needs the built library and no GPU: nothing is launched.  Run it at the commit whose behaviour is to be kept (before a host-side refactor), commit the
file, and tests/test_fused_host_surface.py holds every later tree to it.  `--commit` names that commit in the file.

Whole-tile routes on a host without a GPU: the recorder patches `hip_ops._on_gpu` (and `_ff_on_gpu` where the tree has it) to True and wraps the
whole-tile predicates the models ask by name so that they see a tensor answering `is_cuda` with True (`fused_host_surface_common.Launches`) -- the same
means at the recorded commit and in any later tree."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fused_host_surface.json"))
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    import pytest
    from synfmc_amd import hip_ops
    from tests import fused_host_surface_common as S
    with pytest.MonkeyPatch.context() as mp:
        data = S.surface(hip_ops, mp)
    for ni, label, vi in data["errors"]["rows"]:
        name, (rc, msg) = data["errors"]["names"][ni], data["errors"]["values"][vi]
        assert rc != 0 and rc in S.REFUSALS and msg, f"{name} [{label}] was not refused by an argument check: rc {rc} ({msg})"
    data["recorded_at"] = args.commit
    data = json.loads(json.dumps(data))
    with open(args.out, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    counts = {k: len(data[k]["rows"]) for k in ("predicates", "errors", "routes")}
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, rows {counts}, distinct launches {len(data['routes']['launches'])}")


if __name__ == "__main__":
    main()
