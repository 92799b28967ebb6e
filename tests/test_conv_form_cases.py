"""CPU: the cases of tests/conv_form_cases.py cover exactly the table of conv kernel instances the library was compiled with - a
(tile, form) without a case does not ship - and every one of them keeps the conditions its exact comparison rests on. The kernels run
in tests/test_gpu_conv_forms.py."""
import numpy as np
import pytest

import conv_form_cases as F


@pytest.fixture(scope="module")
def table(built):
    from yolact_amd import capi
    return capi.conv_forms()


def test_cases_cover_exactly_the_compiled_table(table):
    """yh_conv_forms answers from kConvTiles itself: a row or a form bit added there without a case fails here, and so does a case
    whose (tile, form) the table no longer has."""
    compiled = {(r["tile"], f) for r in table for f in r["forms"]}
    cases = F.covered()
    assert compiled - cases == set(), f"instances without a case (a (tile, form) without a case does not ship): {sorted(compiled - cases)}"
    assert cases - compiled == set(), f"stale cases (no such instance in kConvTiles): {sorted(cases - compiled)}"
    assert len(table) == 17 and len(compiled) == 53          # (changing the table changes these two numbers on purpose)


def test_tile_ids_and_widths_are_the_tables(table):
    rows = {r["tile"]: r for r in table}
    assert sorted(F.TILES.values()) == sorted(rows)
    for name, tid in F.TILES.items():
        assert rows[tid]["tch"] == F.TILE_CH[name], name
        assert rows[tid]["fp8"] == name.endswith("FP8"), name
        assert F.PARTIAL[F.TILE_CH[name]] % F.TILE_CH[name] not in (0,) and F.PARTIAL[F.TILE_CH[name]] > F.TILE_CH[name]


def test_form_numbering_is_the_headers():
    """capi.CONV_FORMS names the forms in ConvForm's order (csrc/yh_internal.h) and YH_FORM_*'s (include/yolact_hip_debug.h; the
    library's build asserts those two equal)."""
    import os
    import re
    from yolact_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    internal = open(os.path.join(root, "tiny-object-detection_amd", "csrc", "yh_internal.h")).read()
    names = re.search(r"enum ConvForm \{(.*?)\}", internal).group(1).replace(" ", "").split(",")
    assert names == ["FORM_" + f for f in capi.CONV_FORMS] + ["CONV_FORMS"]
    debug = open(os.path.join(root, "include", "yolact_hip_debug.h")).read()
    names = re.search(r"enum \{ (YH_FORM_PLAIN.*?)\};", debug, flags=re.S).group(1).replace("\n", " ").replace(" ", "").split(",")
    assert names == ["YH_FORM_PLAIN=0"] + ["YH_FORM_" + f for f in capi.CONV_FORMS[1:]] + ["YH_CONV_FORMS", "YH_FORM_REDUCE=YH_CONV_FORMS"]


def test_every_edge_the_table_names_has_a_case():
    """Per instance: the cases reach both row counts' kind of edge where the entry point allows it, and every K depth class."""
    by = {}
    for cid, c in F.CASES.items():
        by.setdefault((c["tile"], c["form"]), []).append(cid)
    for key, ids in by.items():
        assert len(ids) >= 2, key
        assert max(F.rows_of(i) for i in ids) <= 1300, key
    for cid, c in F.CASES.items():
        tch = F.TILE_CH[c["tile"]]
        if c["kind"] not in F.GUARDED:
            assert c["cout"] % tch != 0, (cid, "every case leaves a partial last channel tile")
    # the three-stage rings run shorter than, as long as and longer than the ring
    for t in F.RING + ("128x128_S3_M16",):
        steps = {c["k"] * c["k"] * c["cin"] // 64 for c in F.CASES.values() if c["tile"] == t and c["kind"] == "conv" and c["form"] == "PLAIN"}
        assert {1, 2} <= steps and max(steps) > 3, (t, steps)
    couts = {(c["tile"], c["cout"]) for c in F.CASES.values()}
    assert ("96x128_K1", 95) in couts and ("128x256", 351) in couts and ("128x256_M16", 351) in couts


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_every_sum_is_exact(oracle, cid):
    """sum |products| (+ |bias| + |residual|) of every convolution of the case, the tail's second one included, stays below 2^24:
    every summation order is exact in float32 and the one f16 rounding is the only rounding."""
    for m in F.magnitudes(cid, oracle):
        assert 0 < m < 2.0 ** 24, (cid, m)
    ref = F.reference(cid, oracle)
    assert np.isfinite(ref).all() and np.count_nonzero(ref) > ref.size // 8, cid


@pytest.mark.parametrize("cid", [i for i in F.CASE_IDS if F.CASES[i]["kind"] == "resup"])
def test_resup_reference_does_not_hang_on_the_order_of_the_adds(oracle, cid):
    """The resized residual is the oracle's f16 bilinear (pinned bit for bit to bilinear_f16 by test_bilinear_bit_exact) and generally
    no integer, so the float32 add that takes it in may round. The reference, oracle.conv2d with that residual, adds in the kernel's
    order (acc + bias) + res; acc + (bias + res) gives the same f16 bits at EVERY element of every case (no element excluded)."""
    c, t = F.CASES[cid], F.build(cid)
    ref = F.reference(cid, oracle)
    up = oracle.bilinear(t["res_lo"], c["hi"][0], c["hi"][1], f16=True)
    assert np.array_equal(up, F.f16(up))
    assert c["lo"] == (1, 1) or np.count_nonzero(up != np.round(up)) > up.size // 4, "the resized residual is fractional"
    kernel, other = F.resup_orders(cid, oracle)
    assert np.array_equal(kernel, ref), int(np.count_nonzero(kernel != ref))
    assert np.array_equal(other, ref), int(np.count_nonzero(other != ref))


@pytest.mark.parametrize("cid", [i for i in F.CASE_IDS if F.CASES[i]["kind"] in ("fp8", "levels_fp8", "tail_fp8")])
def test_fp8_codes_carry_the_integers(oracle, cid):
    t = F.build(cid)
    table = oracle.e4m3_decode_table()
    assert np.array_equal(table[oracle.quantize_e4m3(t["x"])], t["x"]) and np.array_equal(table[oracle.quantize_e4m3(t["w"])], t["w"])
    assert np.array_equal(np.log2(t["scale"]), np.round(np.log2(t["scale"])))


def test_a_case_says_what_must_run():
    for cid in F.CASE_IDS:
        k = F.expected_kernels(cid)
        assert k[0] == (F.TILES[F.CASES[cid]["tile"]], F.CASES[cid]["form"])
        assert (len(k) == 2 and k[1] == (-1, "REDUCE")) == bool(F.CASES[cid].get("kslices"))
