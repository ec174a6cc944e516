"""CPU test: every size query of the C ABI returns what it returned at the commit recorded in tests/golden/ws_sizes.json
(tools/gen_golden_ws_sizes.py), for every recorded argument tuple.  The workspace cache rounds sizes to powers of two and a
workspace's address is part of the captured graph's key: a size that drifts changes allocations and graph replay."""
import json
import os

import pytest

from gradslam_amd import _native

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_sizes.json")))


def test_every_size_query_is_recorded():
    queries = [n for n in _native.SIGNATURES if n.endswith("_ws_bytes") or n.endswith("_tape_bytes")]
    assert queries and sorted(queries) == sorted(GOLDEN["sizes"])
    assert all(len(rows) >= 3 for rows in GOLDEN["sizes"].values())


@pytest.mark.parametrize("name", sorted(GOLDEN["sizes"]))
def test_size_query_unchanged(name):
    fn = getattr(_native.lib(), name)  # loads without a GPU; size queries touch no device
    got = [[args, int(fn(*args))] for args, _ in GOLDEN["sizes"][name]]
    assert got == GOLDEN["sizes"][name], "recorded at " + GOLDEN["commit"]
