"""forward() launches what it launched before it was split into a launch plan and stage methods: for every case of
tests/forward_trace.py -- each launch form, at the layer widths of three families and of tiny_cfg(), knobs on and off, fp8
caches, a tensor-parallel stub -- the same entries in the same order with the same scalars and the same buffers at the same
offsets as tests/golden/forward_launches.json, recorded from the commit before the split.  Same launches, same bits."""
import json

import pytest

import forward_trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(forward_trace.GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_the_cases(golden):
    assert list(golden) == list(forward_trace.CASES)


@pytest.mark.parametrize("name", list(forward_trace.CASES))
def test_forward_launches_what_the_parent_launched(golden, name):
    form, launches = forward_trace.trace(name)
    assert not [l for l in launches if "?" in l], "a pointer argument that lies in no named tensor"
    assert form == golden[name]["form"]
    want = golden[name]["launches"]
    for i, (got, ref) in enumerate(zip(launches, want)):
        assert got == ref, f"launch {i} of {len(want)}"
    assert len(launches) == len(want)
