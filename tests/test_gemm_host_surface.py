"""The host side of the token GEMMs and the 3x3 GEMM convolutions against tests/golden/gemm_host_surface.json, recorded by
tools/record_gemm_host_surface.py before the arguments, the persistent form's precondition and the launch forms were each written once: the return code
and message of every refused call of the fourteen entry points, the predicates of the tile-16 forms over a row-count axis, and what `linear()` and
`geglu_linear()` hand to the wrappers at the shipped shapes (tests/gemm_host_surface_common.py).  No GPU: nothing is launched."""
import json
import os

import pytest

from tests import gemm_host_surface_common as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_host_surface.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def K():
    from synfmc_amd import hip_ops
    return hip_ops


def test_predicates(K, golden, monkeypatch):
    S.same_table(S.predicates(K, monkeypatch), golden["predicates"], "predicates (by index in `names`; element = index into MS, or into MS_EDGES off the base configurations)", lambda data, v: S.unrle(v))


def test_refused_calls_keep_code_and_message(K, golden):
    want = golden["errors"]
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != S.CUS:
        pytest.skip("the tile-count rows are recorded against 256 CUs (an MI355X, or a host without a GPU); on another device they might launch")
    assert [[want["names"][r[0]], r[1]] for r in want["rows"]] == [list(c[:2]) for c in S.error_calls()]
    assert all(rc in S.REFUSALS for rc, _ in want["values"])                 # (recorded: every row fails before the launch)
    S.same_table(S.errors(K._lib.load()), want, "refused calls (entry point by index in `names`)", lambda data, v: v)


def test_routes(K, golden, monkeypatch):
    launches = lambda data, runs: [data["launches"][i] for i in S.unrle(runs)]
    S.same_table(S.routes(K, monkeypatch), golden["routes"], "routes (switch set by index in `switches`; element = U-Net level)", launches)
