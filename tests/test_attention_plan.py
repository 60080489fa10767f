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


def test_plan_differing_dims(stub_kernels):
    """The plan's row for a V head dim of its own: it asks the extension's ``attention_dims_supported`` (stubbed
    with attention_mla.hip's tiling, (192, 128) at ``S % 64 == 0``), and only for ``Dv != D``."""
    stub = A.kernels_for()
    asked = []

    def dims_supported(S, Dqk, Dv):
        asked.append((S, Dqk, Dv))
        return S > 0 and S % 64 == 0 and (Dqk, Dv) == (192, 128)

    stub.attention_dims_supported = dims_supported
    bf16, f32 = torch.bfloat16, torch.float32

    def plan(dtype, S, D, Dv, causal, generic=False, **kw):
        return A._plan(dtype, S, D, causal, D ** -0.5, generic=generic, softcap=None, sinks=False, Dv=Dv, **kw)

    for causal in (False, True):
        for S in (64, 192):
            assert plan(bf16, S, 192, 128, causal) == (S, 192, 0, False)
            assert plan(bf16, S, 192, 128, causal, rope=64) == (S, 192, 0, False)
            assert plan(bf16, S, 192, 128, causal, rope=32) is None  # the kernels read a 64-wide shared head
            assert plan(bf16, S, 192, 128, causal, generic=True) is None
            assert plan(f32, S, 192, 128, causal) is None
            assert plan(bf16, S, 96, 64, causal) is None
        assert plan(bf16, 100, 192, 128, causal, generic=True) is None
        assert plan(f32, 100, 192, 128, causal) is None
    assert plan(bf16, 100, 192, 128, True) == (128, 192, 0, False)  # causal end padding
    assert plan(bf16, 100, 192, 128, True, rope=64) == (128, 192, 0, False)
    assert plan(bf16, 100, 192, 128, False) is None
    assert plan(bf16, 100, 96, 64, True) is None
    assert asked and all(dv != d for _, d, dv in asked)

    def never(S, Dqk, Dv):
        raise AssertionError("attention_dims_supported asked for equal head dims")

    stub.attention_dims_supported = never
    for S in (64, 192):
        for causal in (False, True):
            assert plan(bf16, S, 128, 128, causal) == (S, 128, 0, False)
            assert plan(bf16, S, 128, None, causal) == (S, 128, 0, False)
    assert plan(bf16, 100, 128, 128, True) == plan(bf16, 100, 128, None, True) == (128, 128, 0, False)
    assert plan(f32, 64, 64, 64, False, generic=True) is None
