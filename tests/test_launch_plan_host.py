"""The engine issues the launches recorded in tests/golden/launch_plan.json (tests/launch_plan.py): the same library
calls, in the same order, with the same integer and float arguments, the same null and non-null pointers and the same
PgFusedArgs fields -- for prefill, vision and decode cases that reach every route of the engine.  The file was written
from the engine as it stood before its pinned environment knobs were folded; a refactor of the engine leaves it as it
is.  Runs on the CPU: no kernel is executed."""
import json

import pytest

import launch_plan as lp


@pytest.fixture(scope="module")
def golden_plan():
    with open(lp.GOLDEN) as f:
        yield json.load(f)
    lp._packs.clear()       # the CPU packs (a few GB) are shared by the cases and dropped with the module


def test_golden_holds_exactly_the_cases(golden_plan):
    assert sorted(golden_plan) == sorted(name for name, _, _ in lp.CASES)


@pytest.mark.parametrize("case", [name for name, _, _ in lp.CASES])
def test_launch_plan(case, golden_plan, monkeypatch):
    got = lp.lines(lp.record(monkeypatch, only=(case,)))[case]     # (record() also checks the case's witness)
    want = golden_plan[case]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"{case}: launch {i} differs\n  engine: {g}\n  golden: {w}")
            break
    else:
        if len(got) != len(want):
            n = min(len(got), len(want))
            extra = (got if len(got) > len(want) else want)[n]
            print(f"{case}: {len(got)} launches, golden {len(want)}; the first {n} agree, then: {extra}")
    assert got == want
