"""CPU: the cases tests/op_guard_cases.py generates from the compiled conv table reach every (tile, form) of it at the row and channel
counts its docstring names, and keep what their exact comparison rests on. The kernels run in tests/test_gpu_op_guards.py."""
import numpy as np
import pytest

import op_guard_cases as G


@pytest.fixture(scope="module")
def table(built):
    from yolact_amd import capi
    return capi.conv_forms()


def test_cases_reach_every_instance_at_every_edge(table):
    for row in table:
        R, T = row["tm"], row["tch"]
        cases = G.cases_of(row)
        ids = [c["id"] for c in cases]
        assert len(set(ids)) == len(ids), row
        assert {c["form"] for c in cases} == set(row["forms"]), row
        for form in row["forms"]:
            mine = [c for c in cases if c["form"] == form]
            assert {c["cout"] for c in mine} == ({256} if form == "TAIL" else {c for c in (8, T - 8, T, T + 8) if c > 0}), (row, form)
            if form in ("ML", "ML_SPLITK"):
                cells = sum(s * s for s in mine[0]["levels"])
                assert mine[0]["levels"][0] ** 2 < cells < R < 2 * cells, (row, "level boundaries and the end inside the first tile, two images past it")
                assert {(c["n"], c["k"]) for c in mine} == {(1, 1), (1, 3), (2, 1), (2, 3)}
            elif form == "K3":
                assert all(c["k"] == 3 and (c["n"], c["h"], c["w"]) == (2, 5, 7) for c in mine)
            else:
                rows = {c["n"] * c["h"] * c["w"] for c in mine if c["k"] == 1 and c["n"] == 1}
                assert rows == {1, R - 1, R, R + 1, 2 * R + 1}, (row, form, rows)
                assert any(c["n"] == 2 and c["k"] == 1 and c["h"] == R // 2 + 1 for c in mine), (row, form)
            if form.endswith("SPLITK"):
                assert {c["kslices"] for c in mine} == {2, 3}
            if form == "DUAL":
                assert {c["stride2"] for c in mine} == {1, 2}
        if any(f in row["forms"] for f in ("PLAIN", "SPLITK", "TAIL")):
            assert any(c["k"] == 3 and (c["n"], c["h"], c["w"]) == (2, 5, 7) for c in cases), (row, "no 3x3 case")


def test_every_sum_is_exact_and_the_reference_is_not_trivial(table, oracle):
    """sum |x| |w| + |bias| + |res| stays below 2^24 by the grids' limits alone (no data needed): every float32 partial sum of any
    order is an exact integer times the scale's power of two. One reference per (tile, form) is computed and looked at."""
    seen = set()
    for row in table:
        for c in G.cases_of(row):
            fp8 = c["kind"] in ("fp8", "levels_fp8", "tail_fp8")
            K = c["k"] * c["k"] * (c["cin"] + c.get("c2", 0))
            first = K * (4 * 3 if fp8 else 3 * 2) + 4 + 5
            assert first < 2 ** 24, c["id"]
            if c["kind"] in ("tail", "tail_fp8"):
                # the second conv sums 256 of |t| |w2| with t = f16(act(..)) bounded by the first magnitude (scales <= 1, one rounding up)
                assert 256 * (first * 1.001) * 2 + 4 < 2 ** 24, c["id"]
            if (c["tile"], c["form"]) not in seen and c["cout"] >= 32:
                seen.add((c["tile"], c["form"]))
                ref = G.reference(c, G.build(c), oracle)
                assert np.isfinite(ref).all() and np.count_nonzero(ref) > ref.size // 8, c["id"]
