"""Record the host surface of the token GEMMs and the 3x3 GEMM convolutions (tests/gemm_host_surface_common.py) into
tests/golden/gemm_host_surface.json.

    python tools/record_gemm_host_surface.py [--out FILE] [--commit HASH]

Needs the built library and a host WITHOUT a GPU: nothing is launched, and the tile-count clauses are recorded against the 256 CUs the library counts
there.  Run it at the commit whose behaviour is to be kept (before a host-side refactor), commit the file, and tests/test_gemm_host_surface.py holds
every later tree to it.  `--commit` names that commit in the file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_host_surface.json"))
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    import pytest
    from synfmc_amd import hip_ops
    from tests import gemm_host_surface_common as S
    import torch
    assert not torch.cuda.is_available(), "record on a host without a GPU (the tile-count rows are written against the 256 CUs the library counts there)"
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
