"""CPU proof of tests/far_address.py: every case is admissible, lies where it claims, keeps the pitch condition, and its probe SEES a K/V byte offset
reduced modulo 2^31, 2^32 or 2^33 (the sparse address model, on the reference alone); the table names every plan of the list, and the host-only
blocks of the cases describe those plans."""
import numpy as np
import pytest
import torch

from tests import census as C
from tests import census_fp8_tree as X
from tests import census_softcap as S
from tests import far_address as F

CASES = F.cases()
ids = [c["name"] for c in CASES]


def test_every_case_is_admissible_and_fits_the_buffers():
    for c in CASES:
        assert F.admissible(c), c["name"]
        F.geometry(c)          # (asserts the view's extent and the 16-byte rule)
        assert c["geo"] != "row" or int(X.expected(c)[1].max()) <= 2048          # (bf16 at d = 64)


def test_every_case_has_k_and_v_addresses_in_each_zone_it_claims():
    """K and V views share their strides (each in its own buffer), so one address set answers for both tensors; computed from the strides passed"""
    for c in CASES:
        got = F.zones_touched(c)
        assert set(c["zones"]) <= got, "%s claims zones %s, its payload lies in %s" % (c["name"], c["zones"], sorted(got))
    # the geometries reach every zone; 8 GiB and beyond — 2^32 elements of a 2-byte cache — is reached by 2-byte cases of all three
    for geo in ("slot", "row", "deep"):
        assert any(3 in c["zones"] and not c.get("fp8") for c in CASES if c["geo"] == geo)
    # a window whose 32 / 64 keys straddle each mark (geometry `row`)
    for z in ((0, 1), (1, 2), (2, 3)):
        assert any(c["geo"] == "row" and c["zones"] == z for c in CASES)


def test_the_marks_sit_inside_tiles_of_the_far_row_geometry():
    c = next(c for c in CASES if c["geo"] == "row" and c["form"] == "dec" and c["left"] is None)
    g = F.geometry(c)
    a = F.row_address(c, g, 0, np.arange(c["lens"][0]))
    for m in F.MARKS:
        j = int(np.searchsorted(a, m))          # first row at or beyond the mark
        assert 0 < j < c["lens"][0] and j % 64 not in (0,) and j % 32 != 0, (m, j)


def test_pitch_condition():
    for c in CASES:
        assert not F.pitch_violations(c), (c["name"], F.pitch_violations(c)[:3])


def test_pitch_condition_refuses_a_pitch_of_exactly_8_mib(monkeypatch):
    c = next(c for c in CASES if c["geo"] == "row" and c["form"] == "dec" and c["left"] is None)
    monkeypatch.setattr(F, "ROW_PITCH", 8 << 20)
    bad = F.pitch_violations(c)
    starts, _ = F.payload_ranges(c)
    # the 2^32 alias of row j IS row j - 512: a payload row, 512 pitches of 8 MiB below
    hits = [(a, x) for w, a, x in bad if w == 1 << 32]
    assert hits and all(a - x == 512 * (8 << 20) and x in starts and a in starts for a, x in hits)


def _sensitivity_cases():
    """one case per (geometry, form, fp8 / tree, windowed, dtype group, D): the model depends on nothing else"""
    seen, out = set(), []
    for c in CASES:
        k = (c["geo"], c["form"], bool(c.get("fp8")), c.get("mask_kind"), c["left"], c["dt"], c["D"], tuple(c["lens"]), c["sq"], c["G"], c["causal"])
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


SENS = _sensitivity_cases()


@pytest.mark.parametrize("case", SENS, ids=[c["name"] for c in SENS])
def test_a_wrapped_offset_fails_the_comparison_and_names_a_far_entry(case):
    """for the V addresses and, apart from them, for the K addresses (separate arithmetic in every kernel)"""
    c = case

    def verdict(**kw):          # what the GPU test would see: the batched-chunk entry returns no LSE
        out, lse = F.model_output(c, **kw)
        return F.compare(torch.from_numpy(out), torch.from_numpy(lse) if c["form"] != "var" else None, c)
    for tensor in ("v", "k"):
        fails, stats = verdict(tensor=tensor)
        assert not fails and stats["max_ulp"] <= 1.0 and stats["lse_worst_times_n"] < 1e-9, "no wrap: %s" % fails[:2]
        for w in F.WRAPS:
            far = F.far_entries(c, w)
            fails, _ = verdict(wrap=w, tensor=tensor)
            what = "%s: a %s byte offset reduced modulo 2^%d" % (c["name"], tensor.upper(), w.bit_length() - 1)
            if tensor == "k" and c["form"] == "var":
                far = F.straddlers(c, w)          # (where every key of a row wraps alike only an LSE would show it — tests/far_address.py, model_output)
            if not far:
                assert not fails, "%s: no row at or beyond it, yet %s" % (what, fails[:2])
                continue
            assert fails, what + " goes unseen"
            named = {int(f.split()[1]) for f in fails if f.startswith("entry ")}
            assert (named or tensor == "k") and named <= set(far), "%s: the failures name entries %s, the far ones are %s" % (what, sorted(named), far)


def test_a_fill_key_weighs_at_least_twice_a_payload_key():
    """the K probe's margin: the smallest weight a wrapped key takes (fp8, k_scale 1/4, d = 128; softcap 50) is still >= 2"""
    assert min(F.fill_key_weight(c, hk) for c in CASES for hk in range(c["Hkv"])) >= 2.0


def test_the_table_names_every_plan_of_the_list():
    have = {F.plan_key(c) for c in CASES}
    missing = sorted(F.needed_plans() - have, key=str)
    assert not missing, missing
    for dt in ("f16", "bf16"):
        for D in (64, 128):
            sub = {F.plan_key(c)[1:] for c in CASES if c["dt"] == dt and c["D"] == D}
            want = {k[1:] for k in F.needed_plans() if D == 128 or k[3] != 7}
            assert want <= sub, (dt, D, sorted(want - sub, key=str)[:5])


# (work lists and host item plans are built from device tables: asserted on the launched block, tests/test_gpu_far_address.py)
HOST = [c for c in CASES if not c.get("pf") and not c.get("host_tiles")]


@pytest.mark.parametrize("case", HOST, ids=[c["name"] for c in HOST])
def test_host_only_block_describes_the_plan(case):
    """`describe` is pure host arithmetic: the block of the case — shapes, flags and the far view's STRIDES — through the describe entry of its call"""
    from vattention_amd import kernels as K
    c = case
    g = F.geometry(c)
    rows = g["rows"]
    if c["form"] == "tree" or c.get("fp8"):
        p = X.plan_block(c, rows)
    else:
        p = S.plan_block(dict(c, cap=c.get("cap", 0.0)), rows)
    p.k_batch_stride = p.v_batch_stride = g["bs"] // g["es"]
    p.k_row_stride = p.v_row_stride = g["rs"] // g["es"]
    p.k_head_stride = p.v_head_stride = g["hs"] // g["es"]
    if c["form"] == "tree" or c.get("fp8"):
        X.assert_plan_ext(c, X.describe_case(c, p))
    else:
        d = K.describe_softcap(p, c["cap"]) if c.get("cap") else K.describe(p)
        C.assert_plan(c, p, d, rows)
