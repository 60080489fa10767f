"""The attention dispatch plan (``ops.attention._plan``) against the table recorded before the dispatch was
collapsed into it: ``tests/golden/attention_plan.json`` holds, for every point of a grid of dtypes, sequence
lengths, head dims, masks, scales and option sets, the shape the former ``_gpu_ok`` / ``_run_shape`` /
``_generic_shape`` / ``_sink_shape`` chain ran the call at.  Runs on the CPU with the extension's two
supported-shape predicates stubbed."""
import itertools
import json
import os
import sys
import types

import pytest
import torch

import mipipe.ops.attention  # noqa: F401  (the package attribute of that name is the function)

A = sys.modules["mipipe.ops.attention"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_plan.json")


@pytest.fixture
def stub_kernels(monkeypatch):
    stub = types.SimpleNamespace(
        attention_supported=lambda S, D: S > 0 and S % 64 == 0 and D in (64, 128, 256),
        attention_f32_supported=lambda S, D: S >= 32 and S % 32 == 0 and D in (64, 128))
    monkeypatch.setattr(A, "kernels_for", lambda t=None: stub)


def test_plan_reproduces_the_recorded_table(stub_kernels):
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["order"] == ["dtype", "causal", "S", "D", "scale", "case"]
    want = [doc["plans"][i] for i, n in doc["runs"] for _ in range(n)]
    grid = list(itertools.product(*(doc[axis] for axis in doc["order"])))
    assert len(grid) == len(want) == 3 * 2 * 15 * 13 * 3 * 5
    wrong = []
    for (dt, causal, S, D, sc, (name, generic, softcap, sinks)), w in zip(grid, want):
        scale = {"2^-9": 2.0 ** -9, "2^-8": 2.0 ** -8, "D^-0.5": D ** -0.5}[sc]
        got = A._plan(getattr(torch, dt), S, D, causal, scale, generic=generic, softcap=softcap, sinks=sinks)
        if got != (None if w is None else tuple(w)):
            wrong.append((dt, causal, S, D, sc, name, got, w))
    assert not wrong, f"{len(wrong)} rows differ, the first: {wrong[:5]}"
