"""CPU proof of the softcap probes in tests/census_softcap.py, before a GPU is involved (the sibling of tests/test_census_fp8_tree_model.py):
  * part 1's table holds EVERY case of tests/census.py's table that the softcap gate admits, by count, and nothing else; its closed form
    (tests/census.py `expected`, LSE ln n) against tests/softcap_ref.py in f64 (1e-12) with q = 0, random finite K and the case's cap;
  * part 2's closed form against tests/softcap_ref.py in f64 (1e-12) for every named sign entry of every third case; admissibility of every
    row of every case; the saturation facts the closed form rests on, in the fp32 emulation of the kernels' tanh expression;
  * every case of the four tables reaches the plan it names through vattn_softcap_attn_plan_describe on a host-only parameter block;
  * sensitivity: a dropped key, a key read twice, a key from the neighbouring kv head / slot, a "+" sign moved by one row, a mask edge off by
    one and the tanh taken after the mask at cap 1.0, each injected into a CPU emulation of the result, fail the comparison and name the row;
  * part 3: the fp32 emulation of one tile step is bit-identical between the twin calls, and is not once sc is built from the scale;
  * part 4: the fp32 emulation of the one-key LSE on every sample of every case stays below 2e-7 cap + ulp."""
import math

import numpy as np
import pytest
import torch

from tests import census as C
from tests import census_softcap as S

ZERO, SIGNED, TWIN, TANH = S.zero_cases(), S.signed_cases(), S.twin_cases(), S.tanh_cases()
ROWS = lambda c: max(c["lens"]) + S.SPARE


def test_the_zero_query_table_is_every_case_the_gate_admits():
    base = C.gpu_cases()
    out = [c for c in base if c.get("host_tiles") or c.get("pf") or c.get("tiling") == 7 or c.get("variant") == 14]
    assert len(ZERO) == len(base) - len(out) and len(ZERO) > 250, (len(ZERO), len(base), len(out))
    assert [c["name"] for c in ZERO] == [c["name"] for c in base if c not in out]
    for i, c in enumerate(ZERO):
        assert c["cap"] == S.ZERO_CAPS[i & 1] and max(c["lens"]) <= S.LEN_CAP and C.admissible(c), c["name"]
        assert all(a == b or (b > S.LEN_CAP and a == S.LEN_CAP - 37 * j) for j, (a, b) in enumerate(zip(c["lens"], next(x for x in base if x["name"] == c["name"])["lens"])))
        assert all(q <= n for q, n in zip(C.case_qlens(c), c["lens"])) or c["form"] in ("mt", "pre"), c["name"]
    assert sum(max(c["lens"]) > 2000 for c in ZERO) > 50
    sweep = [S.zero_sweep_case(s) for s in range(200)]
    assert all(S.gate_admits(c) and C.admissible(c) and max(c["lens"]) <= S.LEN_CAP and c["cap"] in S.SWEEP_CAPS for c in sweep)
    assert {c["cap"] for c in sweep} == set(S.SWEEP_CAPS) and {c["form"] for c in sweep} == {"dec", "mt", "pre"}


def _against_ref(c, q, kc, vc, exp, n, lse_exp):
    o64, l64 = S.capped_reference(c, q, kc, vc, c["cap"])
    live = n >= 0
    assert float(np.abs(o64.numpy() - exp)[live].max()) < 1e-12, c["name"]
    l64 = l64.permute(0, 2, 1).numpy()
    ok = n > 0
    if ok.any():
        assert float(np.abs(l64[ok] - lse_exp[ok]).max()) < 1e-12, c["name"]
    assert np.isposinf(l64[n == 0]).all(), c["name"]
    return int((n == 0).sum())


def test_zero_query_closed_form_against_the_reference():
    dead = 0
    sub = ZERO[::4]
    assert 4 * len(sub) >= len(ZERO)
    for c in sub:
        g = torch.Generator().manual_seed(len(c["name"]))
        rows = ROWS(c)
        B, Sq, Hq = len(c["lens"]), max(C.case_qlens(c)), c["Hkv"] * c["G"]
        q = torch.zeros(B, Sq, Hq, c["D"], dtype=C.DT[c["dt"]])
        k = (30 * torch.randn(c["n_slots"], rows, c["Hkv"], c["D"], generator=g)).to(C.DT[c["dt"]])
        assert bool(torch.isfinite(k).all())
        exp, n = C.expected(c)
        dead += _against_ref(c, q, k, C.census_values(c["n_slots"], rows, c["Hkv"], c["D"], C.DT[c["dt"]]), exp, n, np.log(np.maximum(n, 1)))
    assert dead > 20


def test_signed_closed_form_against_the_reference():
    dead = flips = 0
    sub = SIGNED[::3]          # (3, not 4: append and cache_batch_idx alternate with period 4 along the table)
    assert 4 * len(sub) >= len(SIGNED) and {c["append"] for c in sub} == {True, False} == {c["idx"] for c in sub}
    for c in sub:
        rows = ROWS(c)
        for mode in S.sign_modes(c):
            plus = S.plus_cells(c, mode, rows)
            q, k, v = S.signed_inputs(c, plus, rows)
            exp, n, lse = S.signed_expected(c, plus)
            dead += _against_ref(c, q, k, v, exp, n, lse)
            flips += int((lse[n > 0] > 0).sum() > 0 and (lse[n > 0] < 0).sum() > 0)
    assert dead > 20 and flips > 100      # (most calls hold rows with a "+" key AND rows without one)


def test_every_row_of_every_signed_case_is_admissible():
    modes = {m: 0 for m in S.SIGNS}
    for c in SIGNED:
        rows = ROWS(c)
        assert {"default", "lo", "hi-1", "neighbour"} <= set(S.sign_modes(c))
        for mode in S.sign_modes(c):
            plus = S.plus_cells(c, mode, rows)
            assert S.signed_admissible(c, plus), (c["name"], mode)
            modes[mode] += 1
            used = [s for s in range(c["n_slots"]) if s in c["slots"]]
            if mode != "default":          # a named entry plants "+" cells, all of them below Lk in the slots the call uses
                assert plus.any(), (c["name"], mode)
                for b, Lk in enumerate(c["lens"]):
                    assert not plus[c["slots"][b], Lk:].any()
            if mode == "neighbour":
                assert not plus[used][:, :, 0].any() and plus[[s for s in range(c["n_slots"]) if s not in c["slots"]]].any()
    assert min(modes.values()) > 100, modes
    # the issue's table: every length, group width, split count and window of it is there
    dec = [c for c in SIGNED if c["form"] == "dec"]
    assert {(c["G"], c["splits"], c["left"], c["D"], c["dt"]) for c in dec} == {(g, s, l, d, t) for g in (4, 17) for s in (0, -3, -37, 3) for l in (None, 0, 31, 32, 100)
                                                                               for d in (64, 128) for t in ("f16", "bf16")}
    assert all(c["lens"] == [max(x, 1) for x in S.DEC_LENS] for c in dec) and {c["append"] for c in dec} == {True, False} == {c["idx"] for c in dec}
    mt = [c for c in SIGNED if c["form"] == "mt" and len(c["lens"]) > 1]
    assert {(c["sq"], c["G"], c["causal"], c["left"], c["splits"]) for c in mt} == {(sq, g, ca, l, s) for sq, g in ((4, 4), (8, 4), (8, 8)) for s in (0, -400)
                                                                                   for ca, l in ((True, None), (False, None), (True, 0), (True, 32), (True, 100))}
    pre = [c for c in SIGNED if c["form"] == "pre"]
    assert {(c["sq"], c["variant"], c["splits"], c["causal"], c["left"]) for c in pre} == {(sq, v, s, ca, l) for sq in (130, 150) for v in (2, 8) for s in (1, 3) for ca, l in
                                                                                         ((True, None), (False, None), (True, 0), (True, 63), (True, 64), (True, 65), (True, 236))}
    assert {(c["tiling"], c["left"]) for c in SIGNED if c["form"] == "var"} == {(1, None), (4, None), (1, 64), (4, 64)}


def test_the_saturation_facts_in_fp32():
    """exactly +1 for x2 >= 26 and exactly -1 for x2 <= -24; the arguments of part 2; exp2(-2 * 64 * log2e) is 0 in fp32, not a denormal"""
    hi = np.concatenate([np.linspace(26, 127, 5000), [130.6, 200, np.inf]]).astype(np.float32)
    assert (S.tanh_exp2_f32(hi) == 1.0).all() and (S.tanh_exp2_f32(-np.concatenate([np.linspace(24, 127, 5000), [130.6, 200, np.inf]]).astype(np.float32)) == -1.0).all()
    assert S.tanh_exp2_f32(np.float32(0.0)) == 0.0
    for D, x2 in ((64, 92.3), (128, 130.6)):
        k2 = S.cap_k2(S.host_pre(D ** -0.5, S.SIGNED_CAP))
        s = np.float32(S.SIGNED_Q * S.SIGNED_Q * D)
        assert abs(float(s * k2) - x2) < 0.05
        assert S.tanh_exp2_f32(s * k2) == 1.0 and S.tanh_exp2_f32(-s * k2) == -1.0
    sc = np.float32(np.float32(S.SIGNED_CAP) * S.LOG2E_F32)
    assert np.exp2(np.float64(np.float32(-1.0) * sc - sc)).astype(np.float32) == 0.0
    p, lse = S.tile_step_f32(np.asarray([[256.0 * 64, -256.0 * 64, -256.0 * 64, 256.0 * 64]]), 64 ** -0.5, S.SIGNED_CAP)
    assert p.tolist() == [[1.0, 0.0, 0.0, 1.0]] and abs(float(lse[0]) - (64 + math.log(2))) < 1e-5


def test_every_case_reaches_the_plan_it_names():
    """vattn_softcap_attn_plan_describe on a host-only parameter block: nothing is launched"""
    reached = set()
    for c in ZERO + SIGNED + TWIN + TANH + [S.zero_sweep_case(s) for s in range(200)]:
        d = S.describe_host(c)
        if c in ZERO or c in SIGNED or c in TWIN:
            reached.add(S.plan_key(c, d))
    assert not S.missing_plans(reached), "plans the tables no longer reach: %s" % S.missing_plans(reached)
    for table in (SIGNED, TWIN):      # each of the two reaches every plan by itself
        assert not S.missing_plans({S.plan_key(c, S.describe_host(c)) for c in table})
    assert max(max(c["lens"]) for c in TWIN) <= 300


# ---- sensitivity: faults injected into a CPU emulation of the result ----

def _emulate(c, plus, cap, fault=None, signed=True):
    """out [B, Sq, Hq, D] / lse [B, Hq, Sq] of a kernel that walks each row's key list — with `fault(b, t, hk, keys, score)` -> (keys, score)
    applied to it.  signed: scores +-cap by `plus`; else the zero-query census (every score 0)."""
    ql = C.case_qlens(c)
    B, Sq, G = len(c["lens"]), max(ql), c["G"]
    out = torch.zeros(B, Sq, c["Hkv"] * G, c["D"], dtype=torch.float64)
    lse = torch.full((B, c["Hkv"] * G, Sq), float("inf"), dtype=torch.float64)
    for b in range(B):
        for t in range(ql[b]):
            lo, hi = C.visible_interval(ql[b], c["lens"][b], t, c["causal"], c.get("left"))
            for hk in range(c["Hkv"]):
                keys = [(c["slots"][b], j, hk) for j in range(lo, hi)]
                score = (lambda s, j, h: cap if plus[s, j, h] else -cap) if signed else (lambda s, j, h: 0.0)
                if fault is not None:
                    keys, score = fault(b, t, hk, keys, score)
                o, l = S.emulate_row(keys, c, cap, score)
                out[b, t, hk * G:(hk + 1) * G], lse[b, hk * G:(hk + 1) * G, t] = torch.from_numpy(o), l
    return out, lse


def _signed_case(mode="default"):
    c = S._xcase("inject", "mt", "f16", 64, 2, 4, 4, [3, 4, 33, 67, 127, 300], 2, left=32, idx=True)
    return c, S.plus_cells(c, mode, ROWS(c))


AT = (4, 2, 1)      # the row the faults are injected into: entry 4 (Lk = 127), row 2, kv head 1


def _only_at(change, at=AT):
    def fault(b, t, hk, keys, score):
        return change(keys, score) if (b, t, hk) == at else (keys, score)
    return fault


def _caught(c, plus, change, at=AT):
    """the clean emulation passes; with the fault the comparison fails and every element it names is in the faulted row"""
    assert S.signed_compare(*_emulate(c, plus, c["cap"]), c, plus)[0] == []
    fails = S.signed_compare(*_emulate(c, plus, c["cap"], _only_at(change, at)), c, plus)[0]
    named = [f for f in fails if f.startswith("entry")]
    assert named and all(f.startswith("entry %d row %d head" % at[:2]) and "(kv head %d," % at[2] in f for f in named), fails
    return fails


def test_a_dropped_key_fails_and_names_the_row():
    c, plus = _signed_case()
    plus_keys = lambda keys: [k for k in keys if plus[k]]
    _caught(c, plus, lambda keys, score: ([k for k in keys if k != plus_keys(keys)[3]], score))
    c, plus = _signed_case("hi-1")          # the row's ONLY "+" key dropped: the row turns into an all-minus row
    fails = _caught(c, plus, lambda keys, score: ([k for k in keys if not plus[k]], score))
    assert any(f.startswith("LSE") for f in fails)


def test_a_key_read_twice_fails_and_names_the_row():
    c, plus = _signed_case()
    _caught(c, plus, lambda keys, score: (keys + [[k for k in keys if plus[k]][5]], score))


def test_a_key_from_the_neighbouring_head_or_slot_fails_and_names_the_row():
    for mode in ("default", "neighbour"):
        c, plus = _signed_case(mode)
        other = next(s for s in range(c["n_slots"]) if s not in c["slots"])
        for swap in (lambda s, j, h: (s, j, 1 - h), lambda s, j, h: (other, j, h)):
            # the row's LAST key is read from kv head 0 / from a slot no entry uses
            _caught(c, plus, lambda keys, score, swap=swap: (keys[:-1] + [swap(*keys[-1])], score))


def test_a_sign_moved_by_one_row_fails_and_names_the_row():
    """K row j + 1 paired with V row j: the scores of the row's keys are those of their upper neighbours"""
    for mode in ("default", "lo", "hi-1", "hi", "lo-1"):
        c, plus = _signed_case(mode)
        moved = lambda keys, score: (keys, lambda s, j, h: score(s, j + 1, h))
        if mode == "lo":
            moved = lambda keys, score: (keys, lambda s, j, h: score(s, j - 1, h))
        _caught(c, plus, moved)


def test_a_mask_edge_off_by_one_fails_and_names_the_row():
    """each named sign entry is there for one edge fault — a "-" key admitted or dropped beside a "+" key weighs nothing —, and a row
    without a "+" key (kv head 0 under "neighbour") is the plain census: it sees all four"""
    grow_hi = lambda keys, score: (keys + [(keys[-1][0], keys[-1][1] + 1, keys[-1][2])], score)
    grow_lo = lambda keys, score: ([(keys[0][0], keys[0][1] - 1, keys[0][2])] + keys, score)
    shrink_hi = lambda keys, score: (keys[:-1], score)
    shrink_lo = lambda keys, score: (keys[1:], score)
    for mode, change in (("hi", grow_hi), ("hi-1", shrink_hi), ("lo-1", grow_lo), ("lo", shrink_lo)):
        c, plus = _signed_case(mode)
        fails = _caught(c, plus, change)
        assert any(f.startswith("LSE") for f in fails)          # the row changes sides: 64 + ln n+ <-> -64 + ln n
    c, plus = _signed_case("neighbour")
    for change in (grow_hi, shrink_hi, grow_lo, shrink_lo):
        _caught(c, plus, change, at=(4, 2, 0))


def test_the_tanh_taken_after_the_mask_fails_at_cap_one():
    """a cap applied AFTER the mask turns -inf into -cap: the masked keys of the walked tiles come back with weight e^-1 at cap 1.0"""
    c = S.with_cap(C._case("inject_zero", "mt", "f16", 64, 2, 4, 4, [3, 4, 33, 67, 127, 300], 2, left=32, idx=True), 1.0)
    def unmasked(keys, score, cap=1.0):
        lo, hi = keys[0][1], keys[-1][1] + 1
        walked = [(keys[0][0], j, keys[0][2]) for j in range(lo // 32 * 32, min((hi + 31) // 32 * 32, 127)) if not lo <= j < hi]
        return keys + walked, lambda s, j, h: 0.0 if lo <= j < hi else -cap
    assert C.compare(*_emulate(c, None, 1.0, signed=False), c)[0] == []
    fails = C.compare(*_emulate(c, None, 1.0, _only_at(unmasked), signed=False), c)[0]
    named = [f for f in fails if f.startswith("entry")]
    assert named and all(f.startswith("entry %d row %d head" % AT[:2]) for f in named), fails
    # ... and at cap 50 the same fault is invisible: why the caps of part 1 alternate with 1.0
    c50 = dict(c, cap=50.0)
    assert C.compare(*_emulate(c50, None, 50.0, _only_at(lambda k_, s_: unmasked(k_, s_, 50.0)), signed=False), c50)[0] == []


# ---- part 3 and part 4: the fp32 emulations ----

@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("cap", S.TWIN_CAPS)
def test_the_scale_twin_is_bit_identical_in_fp32_and_breaks_on_a_leftover_scale(D, cap):
    rng = np.random.default_rng(D + int(cap))
    sB = (rng.standard_normal((64, 96)) * 2 * D ** 0.5).astype(np.float32)
    sA = (sB * np.float32(2)).astype(np.float32)
    s = S.twin_scale(D)
    assert S.host_pre(2 * s, cap) == np.float32(2) * S.host_pre(s, cap) and S.cap_k2(S.host_pre(2 * s, cap)) == np.float32(2) * S.cap_k2(S.host_pre(s, cap))
    bits = lambda x: x.view(np.int32)
    (pA, lA), (pB, lB) = S.tile_step_f32(sA, s, cap), S.tile_step_f32(sB, 2 * s, cap)
    assert np.array_equal(bits(pA), bits(pB)) and np.array_equal(bits(lA), bits(lB))
    (pA, lA), (pB, lB) = S.tile_step_f32(sA, s, cap, sc_from_scale=True), S.tile_step_f32(sB, 2 * s, cap, sc_from_scale=True)
    assert not np.array_equal(bits(pA), bits(pB)) and not np.array_equal(bits(lA), bits(lB))
    # and the emulation is the capped softmax: against float64
    t = cap * np.tanh(sA.astype(np.float64) * s / cap)
    assert np.abs(lA * 0 + S.tile_step_f32(sA, s, cap)[1] - np.log(np.exp(t).sum(-1))).max() < 2e-5 * max(cap, 1)


def test_the_tanh_emulation_is_inside_the_bound_on_every_sample():
    """the inputs and the reference of part 4 before any kernel runs: |cap * tanh_exp2_f32(s * k2) - cap tanh64(x)| <= 2e-7 cap + ulp"""
    worst, seen = {}, set()
    for c in TANH:
        for cap in S.TANH_CAPS:
            q, k, v, smp = S.tanh_inputs(c, cap, ROWS(c))
            assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(k).all())
            got = S.capped_lse_f32(smp["s"], c["D"] ** -0.5, cap).astype(np.float64)
            want = cap * np.tanh(smp["x"])
            err = np.abs(got - want)
            assert (err <= 2e-7 * cap + S.ulp32(got)).all(), (c["name"], cap, float((err / cap).max()))
            worst[cap] = max(worst.get(cap, 0.0), float((err / cap).max()))
            # the stored arguments are near the targets: every fixed one is there (within the I/O dtype's rounding), and [-12, 12] is covered
            if c["sample"] == "all" and len(smp["x"]) >= 422:
                for x in S.TANH_FIXED:
                    assert np.abs(smp["x"] / x - 1).min() < 2.0 ** -7, (c["name"], x)
                assert np.histogram(smp["x"], bins=12, range=(-12, 12))[0].min() >= 10
                seen.add((c["form"], c["dt"], c["D"], cap))
            # each sample row's output must be ONE value row: the sample reads (b, t, h) -> (slot, j, hk) are distinct per row
            assert len({(b, t, h) for b, t, h in zip(smp["b"], smp["t"], smp["h"])}) == len(smp["x"])
    assert len(seen) >= 4 * 4 * 3 - 12      # every dtype, head size and cap on the forms with 422 cells or more
    print("fp32 emulation of the one-key LSE: worst |err| / cap per cap: %s" % {k_: "%.3e" % v_ for k_, v_ in worst.items()})
