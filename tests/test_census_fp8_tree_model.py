"""CPU proof of the FP8-cache and tree-mask probes in tests/census_fp8_tree.py, before a GPU is involved (the sibling of tests/test_census_model.py):
  * the closed-form expectation — a per-row key SET and per-head value scales — against tests/fp8kv_ref.py, tests/tree_ref.py and
    tests/fp8kv_tree_ref.py in f64 (1e-12) and f32 math (0.51 ulp), on the small twin of every case of the new tables and on seeded draws
    of (sq, Lk, mask words, cache kind): base < 0, base = 0, a word of 0, words without the self bit, garbage in bits >= sq, the sign bit;
  * admissibility of every case and sweep draw, so that a one-key error is >= 4 ulp;
  * self-tests: one flipped in-range mask bit, base shifted by one, v_scale swapped between two heads each move an element by >= 4 ulp;
  * the FP8 inputs are a fixed point of the quantiser for both dtypes (the "cache after the call, every byte" assertion depends on it);
  * every table case reaches the plan it names, through the library's describe entries on a host-only block — before it travels to a GPU;
  * the decoy constructions isolate their needle; injected errors (a flipped bit, base +- 1, swapped scales, a shifted V residue) fail
    `compare` with a message that names the row."""
import random
import re

import numpy as np
import pytest
import torch

from tests import census_fp8_tree as C
from tests.fp8kv_ref import FP8, quantize_ref

FP8_CASES, TREE_CASES = C.fp8_cases(), C.tree_cases()
TABLE = FP8_CASES + TREE_CASES
SWEEP = [C.xsweep_case(s) for s in range(200)]
NAMED = re.compile(r"entry \d+ row \d+ head \d+ \(kv head \d+, slot \d+, v_scale ")          # how `compare` names the row of a wrong element


def _cpu_inputs(c, seed=0, v_shift=0):
    """q = 0 and the census caches of case c on the CPU (an fp8 case: float8_e4m3fn tensors); v_shift: the one-hot of every value row moved
    by that many d — what a kernel reads that takes a key's bytes from a neighbouring d-group"""
    rows = max(c["lens"]) + C.XSPARE
    B, Sq, Hq = len(c["lens"]), max(C.case_qlens(c)), c["Hkv"] * c["G"]
    q = torch.zeros(B, Sq, Hq, c["D"], dtype=C.DT[c["dt"]])
    if c.get("fp8"):
        k = C.fp8_random_keys(c["n_slots"], rows, c["Hkv"], c["D"], seed).view(FP8)
        v = C.fp8_census_values(c["n_slots"], rows, c["Hkv"], c["D"]).roll(v_shift, -1).view(FP8)
    else:
        g = torch.Generator().manual_seed(seed)
        k = torch.randn(c["n_slots"], rows, c["Hkv"], c["D"], generator=g).to(C.DT[c["dt"]])
        v = C.census_values(c["n_slots"], rows, c["Hkv"], c["D"], C.DT[c["dt"]]).roll(v_shift, -1)
    return q, k, v


def _model_against_refs(c):
    q, kc, vc = _cpu_inputs(c)
    exp, n = C.expected(c)
    o64, l64 = C.xreference(c, q, kc, vc, "f64", True)
    live = torch.from_numpy(n >= 0)
    assert float((o64 - torch.from_numpy(exp)).abs().max()) < 1e-12, c["name"]
    ok, dead = torch.from_numpy(n > 0), torch.from_numpy(n == 0)
    l64 = l64.permute(0, 2, 1)
    if bool(ok.any()):
        assert float((l64[ok] - torch.log(torch.from_numpy(n)[ok].double())).abs().max()) < 1e-12, c["name"]
    assert bool(torch.isposinf(l64[dead]).all()), c["name"]
    o32 = C.xreference(c, q, kc, vc, "f32")
    fails, stats = C.compare(o32.masked_fill(~live.unsqueeze(-1), 0), None, c)
    assert not fails, "%s: %s" % (c["name"], fails)
    assert stats["max_ulp"] <= 0.51, c["name"]
    return stats["max_ulp"], int(dead.sum())


def _shape_key(t):
    return (t["form"], t["fp8"], t["dt"], t["D"], t["Hkv"], t["G"], t["sq"], tuple(t["lens"]), tuple(t["slots"]), t["causal"], tuple(t.get("qlens") or ()),
            str(t.get("masks")))


def test_model_against_the_references_on_the_small_cases_of_the_tables():
    seen, worst, dead = set(), 0.0, 0
    for c in TABLE:
        t = C.small_twin(c)
        if t is None:                      # (the one-sequence cases of 16 384 keys: the model has no branch of its own for them)
            assert len(c["lens"]) == 1, c["name"]
            continue
        if _shape_key(t) in seen:          # cases that differ only in how the library is asked to launch them are one case for the model
            continue
        seen.add(_shape_key(t))
        w, d = _model_against_refs(t)
        worst, dead = max(worst, w), dead + d
    assert len(seen) > 80 and dead > 50
    print("model == references on %d distinct call shapes (%d dead rows); f32-math reference within %.2f ulp of the closed form" % (len(seen), dead, worst))


def test_model_against_the_references_on_random_draws():
    rng = random.Random(78)
    kinds = {"neg": 0, "zero_base": 0, "word0": 0, "noself": 0, "sign": 0, "garbage": 0}
    for i in range(300):
        sq = rng.choice([2, 3, 4, 5, 7, 8])
        Lk = rng.choice([sq - 1, sq, sq + 1, 1, 31, 32, 33, 64, 93 + sq, 95 + sq, rng.randrange(1, 700)])
        G = rng.choice([1, 2, 4])
        c = C._xcase("draw%d" % i, "tree", rng.choice(["f16", "bf16"]), rng.choice([64, 128]), rng.choice([1, 2, 3]), G, sq, [Lk, rng.randrange(1, 300), sq + 40], None,
                     rng.random() < 0.5, mask=C.mask_words(rng.choice(C.MASK_KINDS + ("rand", "rand")), 3, sq, seed=i), idx=rng.random() < 0.5)
        full = (1 << sq) - 1
        kinds["neg"] += Lk < sq
        kinds["zero_base"] += Lk == sq
        for row in c["masks"]:
            kinds["word0"] += any(w & full == 0 for w in row)
            kinds["noself"] += any(w & full and not (w >> t) & 1 for t, w in enumerate(row))
            kinds["sign"] += any(w >> 31 for w in row)
            kinds["garbage"] += any(w >> sq for w in row)
        _model_against_refs(c)
    assert min(kinds.values()) >= 10, kinds


def test_chain_and_all_ones_masks_are_the_closed_form_of_the_multitoken_calls():
    n = 0
    for c in TREE_CASES:
        if c["mask_kind"] not in ("chain", "ones"):
            continue
        m = dict(c, form="mt", masks=None, causal=c["mask_kind"] == "chain")
        (e1, n1), (e2, n2) = C.expected(c), C.expected(m)
        assert np.array_equal(e1, e2) and np.array_equal(n1, n2), c["name"]
        n += 1
    assert n >= 30


@pytest.mark.parametrize("table", ["cases", "sweep"])
def test_every_case_is_admissible(table):
    for c in (TABLE if table == "cases" else SWEEP):
        assert C.admissible(c), c["name"]
        assert c["form"] not in ("mt", "tree") or (2 <= c["sq"] <= 8 and c["sq"] * c["G"] <= 64), c["name"]
        assert c["form"] != "tree" or all(0 <= w < 1 << 32 for row in c["masks"] for w in row)
        assert c["Hkv"] <= len(C.V_SCALES) and min(c["lens"]) >= 1


def _moved(a, b, dt):
    """the largest move between two expectations, in ulp of the larger of the two elements (an element that was 0 has moved by all of its ulps)"""
    top = np.maximum(a, b)
    if not (top > 0).any():
        return 0.0
    return float((np.abs(a - b) / C.ulp(np.maximum(top, 1e-30), dt))[top > 0].max())


def _row(c, b, t, hk=None):
    lo, hi, singles = C.row_keys(c, b, t)
    hk = (1 % c["Hkv"]) if hk is None else hk
    m = max(hi - lo, 0) + len(singles)
    return C.set_counts(lo, hi, singles, hk, c["slots"][b], c["D"]) / float(max(m, 1)), m


@pytest.mark.parametrize("table", ["cases", "sweep"])
def test_a_flipped_mask_bit_and_a_shifted_base_move_an_element_by_four_ulp(table):
    """for the longest entry (the least sensitive), the shortest and one between, rows 0, sq - 1 and a random one: EVERY in-range bit flipped in
    turn, and Lk + 1 / Lk - 1 under the same words"""
    rng = random.Random(5)
    flips = shifts = 0
    for c in (TREE_CASES if table == "cases" else [s for s in SWEEP if s["form"] == "tree"]):
        sq = c["sq"]
        order = sorted(range(len(c["lens"])), key=lambda b: c["lens"][b])
        for b in {order[0], order[len(order) // 2], order[-1]}:
            base = c["lens"][b] - sq
            for t in {0, sq - 1, rng.randrange(sq)}:
                a, na = _row(c, b, t)
                for s in range(sq):
                    if base + s < 0:
                        continue
                    f = dict(c, masks=[[w ^ (1 << s) if (bb, tt) == (b, t) else w for tt, w in enumerate(row)] for bb, row in enumerate(c["masks"])])
                    m = _moved(a, _row(f, b, t)[0], c["dt"])
                    assert m >= 4.0, "%s: entry %d row %d bit %d flipped moves only %.2f ulp" % (c["name"], b, t, s, m)
                    flips += 1
                for dl in (1, -1):
                    if c["lens"][b] + dl < 1:
                        continue
                    f = dict(c, lens=[x + dl if bb == b else x for bb, x in enumerate(c["lens"])])
                    z, nz = _row(f, b, t)
                    if na == 0 and nz == 0:
                        continue
                    m = _moved(a, z, c["dt"])
                    assert m >= 4.0, "%s: entry %d row %d base %+d moves only %.2f ulp" % (c["name"], b, t, dl, m)
                    shifts += 1
    assert flips > 200 and shifts > 100


@pytest.mark.parametrize("table", ["cases", "sweep"])
def test_swapped_head_scales_move_an_element_by_four_ulp(table):
    n = 0
    for c in (TABLE if table == "cases" else SWEEP):
        if not c.get("fp8") or c["Hkv"] < 2:
            continue
        _, vs = C.case_scales(c)
        assert len(set(vs)) == len(vs) and all(s >= 1 and np.log2(s) == int(np.log2(s)) for s in vs)
        ks, _ = C.case_scales(c)
        assert len(set(ks)) == len(ks) and all(0.25 <= s <= 4 and np.log2(s) == int(np.log2(s)) for s in ks)
        sw = dict(c, v_scale=[vs[1], vs[0]] + vs[2:])
        a, b = C.expected(c)[0], C.expected(sw)[0]
        for hk in (0, 1):
            m = _moved(a[:, :, hk * c["G"]], b[:, :, hk * c["G"]], c["dt"])
            assert m >= 4.0, "%s: swapped scales move kv head %d only %.2f ulp" % (c["name"], hk, m)
        n += 1
    assert n > 30


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_the_fp8_inputs_are_a_fixed_point_of_the_quantiser(dt):
    """dequantise with power-of-two scales, hand on in the I/O dtype, requantise: the same bytes — all 254 finite bytes under every scale of
    the tables, and the census inputs themselves"""
    dtype = C.DT[dt]
    every = torch.tensor(C.E4M3_FINITE, dtype=torch.uint8).view(1, 1, 254).expand(1, 4, 254).contiguous()
    for scales in (C.K_SCALES, C.V_SCALES):
        sc = torch.tensor(scales, dtype=torch.float32)
        x = C.dequantize_bytes(every, sc, dtype)
        assert bool(torch.isfinite(x).all())
        assert torch.equal(quantize_ref(x, sc).view(torch.uint8), every), scales
        want = torch.tensor([[C.e4m3_value(b) * s for b in C.E4M3_FINITE] for s in scales], dtype=torch.float64)
        assert torch.equal(x[0].double(), want)           # (the widening table of this file is torch's)
    k = C.fp8_random_keys(3, 500, 4, 128, 1)
    v = C.fp8_census_values(3, 500, 4, 128)
    assert len(torch.unique(k)) == 254 and not bool(((k & 0x7F) == 0x7F).any())
    assert sorted(torch.unique(v).tolist()) == [0, C.FP8_ONE] and bool((v.sum(-1) == C.FP8_ONE).all())
    for u8, scales in ((k, C.K_SCALES), (v, C.V_SCALES)):
        sc = torch.tensor(scales, dtype=torch.float32)
        assert torch.equal(quantize_ref(C.dequantize_bytes(u8, sc, dtype), sc).view(torch.uint8), u8)
    assert C.e4m3_value(C.FP8_ONE) == 1.0 and C.e4m3_value(0x7E) == 448.0 and np.isnan(C.e4m3_value(C.FP8_NAN)) and np.isnan(C.e4m3_value(0xFF))


def test_every_table_case_reaches_the_plan_it_names():
    """through the describe entry of the call the case makes, on a host-only parameter block: nothing is launched"""
    reached = set()
    for c in TABLE + C.xdecoy_cases() + SWEEP:
        d = C.describe_case(c, C.plan_block(c))
        C.assert_plan_ext(c, d)
        if c in TABLE:
            reached.add(C.plan_key(c, d))
    missing = [k for k in C.XNEED if k not in reached]
    assert not missing, "plans the tables no longer reach: %s" % missing


def test_the_decoy_constructions_isolate_one_key():
    seen = set()
    for c in C.xdecoy_cases():
        key = C.xinputs_key(c)
        if key in seen:
            continue
        seen.add(key)
        q, kc, vc, scales, plants = C.xdecoy_inputs(c)          # (the cell registry inside asserts that no two plants share a cell)
        assert len(plants) >= 9, c["name"]
        assert len({(s, j, hk) for _, _, _, s, hk, j in plants}) == len(plants), c["name"]
        ref = C.xdecoy_reference(c, q, kc, vc, scales, "f64")
        for b, t, h, slot, hk, j in plants:
            row = vc[slot, j, hk].double() * (scales[1][hk].double() if scales else 1.0)
            dev = float((ref[b, t, h] - row).abs().max())
            assert dev < 1e-3, "%s: row (%d, %d, %d) is not its needle's value row (key %d): %.3e" % (c["name"], b, t, h, j, dev)
        if scales is not None:
            # amax scales are no powers of two — and the stored bytes are still what the call's quantiser makes of their dequantised rows
            assert all(np.log2(float(s)) != int(np.log2(float(s))) for s in scales[0].tolist() + scales[1].tolist()), c["name"]
            for x8, sc in ((kc, scales[0]), (vc, scales[1])):
                back = quantize_ref(C.dequantize_bytes(x8.view(torch.uint8), sc, C.DT[c["dt"]]), sc)
                assert torch.equal(back.view(torch.uint8), x8.view(torch.uint8)), c["name"]
    assert len(seen) >= 20


@pytest.mark.parametrize("fp8", [False, True], ids=["2byte", "fp8"])
def test_injected_errors_fail_the_comparison_and_name_the_row(fp8):
    """What a subtly wrong kernel would return — the references' f32-math output for a case with ONE flipped mask bit, with base + 1 / - 1,
    with swapped head scales, with every value row's one-hot moved into the neighbouring 16-d group — handed to `compare` against the case."""
    c = C._xcase("inject", "tree", "f16", 128, 2, 2, 5, [5, 45, 98, 100, 64, 1025], None, fp8, mask="rand", idx=True)
    run = lambda case, **kw: C.xreference(case, *_cpu_inputs(case, **kw), "f32", True)
    out, lse = run(c)
    assert C.compare(out, lse, c)[0] == []
    b, t = 3, 2
    flipped = dict(c, masks=[[w ^ 2 if (bb, tt) == (b, t) else w for tt, w in enumerate(row)] for bb, row in enumerate(c["masks"])])
    fails = C.compare(*run(flipped), c)[0]
    assert fails and all("entry 3 row 2" in f for f in fails if f.startswith("entry")), fails
    assert any("draft key 96 = base 95 + 1: bit 1 of mask word" in f for f in fails), fails
    for dl in (1, -1):
        f = dict(c, lens=[x + dl if bb == 2 else x for bb, x in enumerate(c["lens"])])
        fails = C.compare(*run(f), c)[0]
        assert fails and any(f_.startswith("entry 2 row") for f_ in fails), (dl, fails)
        assert all(f_.startswith("entry 2 row") or f_.startswith("LSE") for f_ in fails), (dl, fails)
    fails = C.compare(*run(c, v_shift=16), c)[0]
    assert fails and all(NAMED.match(f) for f in fails), fails
    if fp8:
        _, vs = C.case_scales(c)
        fails = C.compare(*run(dict(c, v_scale=vs[::-1])), c)[0]
        assert fails and all(NAMED.match(f) for f in fails), fails


def test_injected_errors_fail_the_comparison_on_the_interval_forms():
    for form, sq, lens, kw in (("dec", 1, [700, 33, 1025], {}), ("mt", 4, [700, 33, 3, 1025], {}), ("pre", 130, [130, 300], dict(variant=2))):
        c = C._xcase("inject_" + form, form, "bf16", 64, 2, 2, sq, lens, None, True, idx=True, **kw)
        run = lambda case, **k: C.xreference(case, *_cpu_inputs(case, **k), "f32", True)
        assert C.compare(*run(c), c)[0] == []
        _, vs = C.case_scales(c)
        for wrong in (run(dict(c, v_scale=vs[::-1])), run(c, v_shift=16)):
            fails = C.compare(*wrong, c)[0]
            assert fails and all(NAMED.match(f) for f in fails), (form, fails)
        fails = C.compare(*run(dict(c, lens=[lens[0] - 1] + lens[1:])), c)[0]
        assert fails and all(f.startswith("entry 0 row") or f.startswith("LSE") for f in fails), (form, fails)
