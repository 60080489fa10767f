"""The bf16 GEMM launch plan (``_C.gemm_plan``) against the table recorded before the dispatch was collapsed into it:
``tests/golden/gemm_plan.json`` holds, for every point of a grid of the three setters, operand layouts, epilogues,
option sets and shapes, what the former ``use_big`` / ``big_width`` / ``gemm_splitk_factor`` / ``launch_by_rounds``
chain and the ``gemm_*_ok`` predicates decided.  The table is dictionary coded: ``table[knobs][layout][epi][case]``
names a slab (``null``: the option set does not exist for that layout and epilogue), a slab one column per shape
(M major), a column one plan per K.  Host calls only; marked ``gpu`` because it needs the built extension."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan.json")


@pytest.mark.gpu
def test_plan_reproduces_the_recorded_table():
    from mipipe._native_loader import kernels

    k = kernels()
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["fields"] == ["big", "width", "k_splits", "rowsum_ok", "colsum_ok", "bits_ok", "by_rounds", "along_n",
                             "per", "chunks", "width_at_k_splits"]
    assert [len(doc[axis]) for axis in ("knobs", "layout", "epi", "case", "M", "N", "K")] == [7, 4, 3, 16, 13, 13, 7]
    shapes = [(M, N) for M in doc["M"] for N in doc["N"]]
    # _C.gemm_plan's arguments after epi, in its order; seg_k (true in the table) is the row's K
    names = ["act", "p", "bias", "aux", "res", "at", "trans_c", "rowsum", "colsum", "bits", "dact", "seg_k"]
    plan, rows, wrong = k.gemm_plan, 0, []
    try:
        for knobs, by_layout in zip(doc["knobs"], doc["table"]):
            k.gemm_set_width(knobs[0])
            k.gemm_set_splitk(knobs[1])
            k.gemm_set_rounds(knobs[2])
            for (a_kc, b_kc), by_epi in zip(doc["layout"], by_layout):
                for epi, by_case in zip(doc["epi"], by_epi):
                    for (name, kw), slab in zip(doc["case"], by_case):
                        if slab is None:
                            continue
                        a = [kw.get(n, 0) for n in names]
                        for (M, N), column in zip(shapes, doc["slabs"][slab]):
                            for K, i in zip(doc["K"], doc["columns"][column]):
                                rows += 1
                                a[11] = K if kw.get("seg_k") else 0
                                p = plan(M, N, K, a_kc, b_kc, epi, *a)
                                at_splits = plan(M, N, K, a_kc, b_kc, epi, *a, 0, p[1])[2] if p[1] > 1 else p[2]
                                # the fields above, in _C.gemm_plan's order; p[6]: a kernel exists
                                got = [p[0], p[2], p[1], p[11], p[12], p[13], p[7], p[8], p[9], p[10], at_splits]
                                if got != doc["plans"][i] or not p[6]:
                                    wrong.append((knobs, a_kc, b_kc, epi, name, M, N, K, got, doc["plans"][i], p[6]))
    finally:
        k.gemm_set_width(0)
        k.gemm_set_splitk(1)
        k.gemm_set_rounds(1)
    assert rows == doc["rows"] == 480298
    assert not wrong, f"{len(wrong)} of {rows} rows differ, the first: {wrong[:5]}"
