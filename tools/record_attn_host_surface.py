"""Record the host surface of the attention kernels (tests/attn_host_surface_common.py) into tests/golden/attn_host_surface.json.

    python tools/record_attn_host_surface.py [--out FILE] [--commit HASH]

Needs the built library; nothing is launched, so a host without a GPU will do.  Run it at the commit whose behaviour is to be kept (before a host-side
refactor), commit the file, and tests/test_attn_host_surface.py holds every later tree to it.  `--commit` names that commit in the file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attn_host_surface.json"))
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    import pytest
    from synfmc_amd import hip_ops
    from tests import attn_host_surface_common as S
    assert S.lds_refusal_unreachable()
    with pytest.MonkeyPatch.context() as mp:
        data = S.surface(hip_ops, mp)
    for ni, label, vi in data["errors"]["rows"]:
        name, (rc, msg) = data["errors"]["names"][ni], data["errors"]["values"][vi]
        assert rc != 0 and rc in S.ATTN_REFUSALS and msg, f"{name} [{label}] was not refused by an argument check: rc {rc} ({msg})"
    data["recorded_at"] = args.commit
    data = json.loads(json.dumps(data))
    with open(args.out, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    counts = {k: len(data[k]["rows"]) for k in ("errors", "calls")}
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, rows {counts}, distinct refusals {len(data['errors']['values'])}")


if __name__ == "__main__":
    main()
