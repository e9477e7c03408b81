"""The host side of libwtprune.so (csrc/host_*.hip) against tests/golden/host_plan.json, the record
tools/gen_golden_host_plan.py made from the library of the commit named in the fixture: every
workspace size, every validation error with its text and tensor index, and the bytes each layout
needs (the WTP_EWORKSPACE text).  Every call returns before the library's first HIP call: CPU only.
Exact equality, record by record."""
import importlib.util
import json
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "host_plan.json")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_golden_host_plan",
                                                  os.path.join(ROOT, "tools", "gen_golden_host_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def _same(a, b):
    """== with NaN equal to NaN (json writes and reads NaN), lists element by element."""
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def test_fixture_covers_the_generators_grid(gen, fixture):
    """The committed record is the generator's grid, call for call (a thinned or stale fixture fails)."""
    lists, calls = gen.calls()
    assert fixture["lists"] == lists
    recorded = [r[0] for r in gen.records(fixture)]
    assert len(recorded) == len(calls) > 3000
    assert all(_same(r, c) for r, c in zip(recorded, calls))
    assert len(fixture["commit"]) == 40
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_host_plan_matches_the_record(gen, fixture):
    run = gen.Runner(fixture["lists"])
    bad, n = [], 0
    for call, value, err, tensor in gen.records(fixture):
        got = run.run(call)
        n += 1
        if not _same(got, [value, err, tensor]):
            bad.append((call, got, [value, err, tensor]))
    assert not bad, "%d of %d records differ; first: %r" % (len(bad), n, bad[:5])
