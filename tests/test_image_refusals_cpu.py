"""What the image entry points refuse before a device is looked for, and in which order: tests/golden/image_refusals.json holds
the return code and the pyr_last_error() text of every call that tests/golden/make_image_refusals.py describes -- no fault, every
single fault, every pair of faults of two different groups, on device 99 -- and the built library must answer each the same. The
file records what the entries did before their host layer was restated through one staging path; a record that has to change is a
change of behaviour."""
import json
import os
import sys

import pytest

from pyrite_amd import build as gpu_build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_image_refusals as G  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    gpu_build.build()
    return G.load(gpu_build.OUT)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "image_refusals.json")) as f:
        return json.load(f)


def test_the_file_holds_every_case_of_every_entry(golden):
    assert list(golden["calls"]) == G.ENTRIES and len(G.ENTRIES) == 16
    for entry in G.ENTRIES:
        assert [r[0] for r in golden["calls"][entry]] == [" + ".join(given) for given in G.cases(entry)], entry
        assert golden["calls"][entry][0][:2] == ["", -3]  # no fault: the call ends at the device


def test_every_call_is_refused_as_recorded(lib, golden):
    wrong = []
    for entry in G.ENTRIES:
        for given, code, text in golden["calls"][entry]:
            seen = G.call(lib, entry, given.split(" + ") if given else ())
            if seen != (code, golden["messages"][text]):
                wrong.append((entry, given, seen, (code, golden["messages"][text])))
    assert not wrong, "%d calls differ, the first: %r" % (len(wrong), wrong[:5])
