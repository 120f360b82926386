"""The surface of defer_amd._hip_ops, checked without a GPU: every public
attribute's name and the first line of its pybind docstring, which carries
the argument names, their defaults and the return type.

tests/data/hip_ops_surface.json was written from a build of the commit
before the bindings were split by kernel family, and a refactor of the
bindings must leave it alone. Regenerate it only for a deliberate change to
an op's signature or for a new op: {name: first line of fn.__doc__} over the
names of dir(_hip_ops) that do not start with an underscore, as JSON with
sorted keys."""

import json
import os

import pytest

pytest.importorskip("defer_amd._hip_ops")

import defer_amd._hip_ops as hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_matches_the_recorded_one():
    with open(os.path.join(ROOT, "tests", "data",
                           "hip_ops_surface.json")) as f:
        want = json.load(f)
    assert len(want) == 56
    got = {}
    for name in dir(hip):
        if not name.startswith("_"):
            doc = (getattr(hip, name).__doc__ or "").strip()
            got[name] = doc.splitlines()[0] if doc else ""
    assert sorted(got) == sorted(want)
    differ = {n: (got[n], want[n]) for n in want if got[n] != want[n]}
    assert not differ, differ
