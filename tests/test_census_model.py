"""CPU proof of the probes in tests/census.py, before a GPU is involved:
  * the closed-form census expectation against BOTH oracles — oracle/attn.py in f64 and f32 math, tests/window_ref.py for windows — on the
    small twin of every case of the shared GPU table (entries of more than 2 100 keys dropped) and on seeded random (sq, Lk, left, causal) draws;
  * admissibility of every GPU case: ceil(n / D) <= 256 (fp16) / 32 (bf16), so a one-key error is >= 4 ulp;
  * the self-test: hi or lo shifted by one in the model moves at least one element by >= 4 ulp;
  * the decoy construction isolates its needle (the oracle's row equals v[j*] within 1e-3), and no two plants share a cache cell;
  * every score-range input set is admissible: the oracle's f32 math stays within half the tolerance of its f64 math."""
import random

import numpy as np
import pytest
import torch

from tests import census as C

GPU_CASES = C.gpu_cases()
SWEEP = [C.sweep_case(s) for s in range(200)]


def _cpu_inputs(c, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = max(c["lens"]) + 8
    B, Sq, Hq = len(c["lens"]), max(C.case_qlens(c)), c["Hkv"] * c["G"]
    q = torch.zeros(B, Sq, Hq, c["D"], dtype=C.DT[c["dt"]])
    kc = torch.randn(c["n_slots"], rows, c["Hkv"], c["D"], generator=g).to(C.DT[c["dt"]])
    return q, kc, C.census_values(c["n_slots"], rows, c["Hkv"], c["D"], C.DT[c["dt"]])


def _small_twin(c):
    keep = [b for b, n in enumerate(c["lens"]) if n <= 2100]
    if not keep:
        return None
    t = dict(c)
    t["lens"] = [c["lens"][b] for b in keep]
    t["slots"] = [c["slots"][b] for b in keep]
    if c.get("qlens"):
        t["qlens"] = [c["qlens"][b] for b in keep]
    return t


def _model_against_oracles(c):
    q, kc, vc = _cpu_inputs(c)
    exp, n = C.expected(c)
    o64, l64 = C.reference(c, q, kc, vc, "f64", True)
    live = torch.from_numpy(n >= 0)
    assert float((o64 - torch.from_numpy(exp)).abs().max()) < 1e-12, c["name"]
    ok = torch.from_numpy(n > 0)
    l64 = l64.permute(0, 2, 1)
    assert float((l64[ok] - torch.log(torch.from_numpy(n)[ok].double())).abs().max()) < 1e-12 if bool(ok.any()) else True, c["name"]
    assert bool(torch.isposinf(l64[torch.from_numpy(n == 0)]).all()), c["name"]
    # the oracle's f32 math (P rounded to the I/O dtype, output rounded to it): what a correct kernel computes — must pass the GPU assertion
    o32 = C.reference(c, q, kc, vc, "f32")
    fails, stats = C.compare(o32.masked_fill(~live.unsqueeze(-1), 0), None, c)
    assert not fails, "%s: %s" % (c["name"], fails)
    assert stats["max_ulp"] <= 0.51, c["name"]
    return stats["max_ulp"]


def test_model_against_both_oracles_on_the_small_cases_of_the_table():
    seen, worst = set(), 0.0
    for c in GPU_CASES:
        t = _small_twin(c)
        if t is None:
            continue
        # cases that differ only in how the library is asked to launch them are one case for the model
        key = (t["form"], t["dt"], t["D"], t["Hkv"], t["G"], t["sq"], tuple(t["lens"]), tuple(t["slots"]), t["causal"], t["left"], tuple(t.get("qlens") or ()))
        if key in seen:
            continue
        seen.add(key)
        worst = max(worst, _model_against_oracles(t))
    assert len(seen) > 100
    print("model == oracles on %d distinct call shapes; f32-math oracle within %.2f ulp of count / n" % (len(seen), worst))


def test_model_against_both_oracles_on_random_draws():
    rng = random.Random(77)
    for i in range(300):
        sq = rng.choice([1, 1, 2, 3, 5, 8, 40, 130])
        Lk = rng.choice([1, 2, sq, max(sq - 1, 1), 31, 32, 33, 63, 64, 65, rng.randrange(1, 700)])
        left = rng.choice([None, 0, 1, 31, 32, 33, 100, 1000])
        causal = True if left is not None else rng.random() < 0.7
        c = C._case("draw%d" % i, "dec" if sq == 1 else "mt" if sq <= 8 else "pre", rng.choice(["f16", "bf16"]), rng.choice([64, 128]), rng.choice([1, 2, 3]),
                    rng.choice([1, 2, 4]), sq, [Lk, rng.randrange(1, 300)], None, causal=causal, left=left, idx=rng.random() < 0.5)
        _model_against_oracles(c)


def test_f32_math_at_the_longest_admissible_length():
    """n = 16 384, d = 128, fp16: the oracle's f32 math within 0.5 ulp of count / n"""
    c = C._case("long", "dec", "f16", 128, 1, 1, 1, [16384], None)
    assert _model_against_oracles(c) <= 0.5


@pytest.mark.parametrize("table", ["cases", "sweep"])
def test_every_gpu_case_is_admissible(table):
    for c in (GPU_CASES if table == "cases" else SWEEP):
        assert C.admissible(c), c["name"]
        assert c["form"] != "mt" or (2 <= c["sq"] <= 8 and c["sq"] * c["G"] <= 64), c["name"]


def test_a_nan_or_inf_output_fails_the_census():
    """what a read of the poisoned spare rows produces (P = 0 times V = Inf) must fail `compare` on rows where every count is positive too"""
    c = C._case("nan", "dec", "f16", 128, 1, 1, 1, [4096], None)
    exp, n = C.expected(c)
    assert (exp > 0).all()
    good = torch.from_numpy(exp).half()
    lse = torch.log(torch.from_numpy(n).double()).permute(0, 2, 1)
    assert C.compare(good, lse, c)[0] == []
    for bad_value in (float("nan"), float("inf"), -float("inf")):
        one = good.clone()
        one[0, 0, 0, 77] = bad_value
        fails, stats = C.compare(one, lse, c)
        assert fails and not np.isfinite(stats["max_ulp"]), bad_value
        assert C.compare(torch.full_like(good, bad_value), None, c)[0], bad_value
    off = good.clone()
    off[0, 0, 0, 5] += 2 * float(C.ulp(exp[0, 0, 0, 5], "f16"))
    assert C.compare(off, lse, c)[0]


def _moves(lo, hi, lo2, hi2, c):
    a = C.counts(lo, hi, 1 % c["Hkv"], 2, c["D"]) / float(hi - lo)
    b = C.counts(lo2, hi2, 1 % c["Hkv"], 2, c["D"]) / float(max(hi2 - lo2, 1))
    top = np.maximum(a, b)          # (an element that was 0 and now holds a key has moved by all of its ulps)
    return float((np.abs(a - b) / C.ulp(np.maximum(top, 1e-30), c["dt"]))[top > 0].max())


@pytest.mark.parametrize("table", ["cases", "sweep"])
def test_a_one_key_shift_moves_an_element_by_four_ulp(table):
    """the self-test: for the longest row of every case (the least sensitive one), a shortest one and a few between, hi + 1, hi - 1, lo + 1 and
    lo - 1 each move at least one element by >= 4 ulp of the output dtype"""
    rng = random.Random(3)
    for c in (GPU_CASES if table == "cases" else SWEEP):
        ql = C.case_qlens(c)
        ivs = sorted({C.visible_interval(ql[b], c["lens"][b], t, c["causal"], c["left"]) for b in range(len(ql)) for t in {0, ql[b] - 1, rng.randrange(ql[b])}},
                     key=lambda iv: iv[1] - iv[0])
        ivs = [iv for iv in ivs if iv[1] - iv[0] >= 2]
        for lo, hi in ivs[:2] + ivs[-3:]:
            shifts = [(lo, hi + 1), (lo, hi - 1), (lo + 1, hi)] + ([(lo - 1, hi)] if lo > 0 else [])
            for lo2, hi2 in shifts:
                m = _moves(lo, hi, lo2, hi2, c)
                assert m >= 4.0, "%s: keys [%d, %d) -> [%d, %d) moves only %.2f ulp" % (c["name"], lo, hi, lo2, hi2, m)


def test_the_decoy_construction_isolates_one_key():
    cases = C.decoy_cases()
    seen = set()
    for c in cases:
        key = (c["form"], c["dt"], c["D"], c["G"], c["sq"], c["left"], tuple(c["slots"]), str(c["needles"]))
        if key in seen:
            continue
        seen.add(key)
        q, kc, vc, plants = C.decoy_inputs(c)
        assert len(plants) >= 9, c["name"]
        ref = C.reference(c, q, kc, vc, "f64")
        for b, t, h, slot, hk, j in plants:
            dev = float((ref[b, t, h] - vc[slot, j, hk].double()).abs().max())
            assert dev < 1e-3, "%s: row (%d, %d, %d) is not its needle's value row (key %d): %.3e" % (c["name"], b, t, h, j, dev)


def test_every_score_range_input_set_is_admissible():
    """the oracle's own f32 math within HALF the tolerance of its f64 math, per element — else the GPU test would measure the format, not the kernel"""
    seen = set()
    for c in C.numerics_cases():
        key = (c["name"].rsplit("_s", 1)[0] if c["kind"] != "plain" else c["name"], c["dt"], c["left"], c["scale"])
        if key in seen:
            continue
        seen.add(key)
        q, kc, vc = C.numerics_inputs(c)
        r64, l64 = C.reference(c, q, kc, vc, "f64", True)
        r32 = C.reference(c, q, kc, vc, "f32").double()
        t = C.tol(c["dt"])[0]
        excess = ((r32 - r64).abs() - 0.5 * (t + t * r64.abs())).max().item()
        assert excess <= 0, "%s: f32-math oracle exceeds half the tolerance by %.3e" % (c["name"], excess)
        assert bool(torch.isfinite(r64).all())
        if c["kind"] == "v3e4":
            assert float(r64.abs().max()) > 2.5e4 and float(r32.abs().max()) < 65504
