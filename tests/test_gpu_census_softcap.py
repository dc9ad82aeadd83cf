"""The exact probes of tests/census_softcap.py on the GPU, for the 64 SOFTCAP decode builds and the 16 prefill_softcap_kernel builds that
tests/test_gpu_softcap.py holds to parity only (2e-3 / 1.6e-2 on randn data): parity cannot see one key dropped, doubled or wrongly admitted
among hundreds, a key masked before the tanh at cap 30, a K row paired with the wrong V row, or a leftover softmax_scale behind the tanh.

  part 1  zero-query census under a cap     |out - count_d / n| <= 1 ulp of the output dtype, |lse - ln n| < 0.25 / n (tests/census.py `compare`)
  part 2  signed (saturated) census         the same on the "+" keys alone; |lse - (+-64 + ln n)| <= 0.25 / n + 2 ulp_fp32(64 + ln n)
  part 3  scale twin                        (2 q, s, cap) and (q, 2 s, cap): out, LSE and the cache after an append bit for bit, equal plans;
                                            call A also against tests/softcap_ref.py in float64 with softmax_scale = s, tests/test_gpu_softcap.py's bounds
  part 4  the tanh read out                 one-key rows: out = that key's value row within 1 ulp, |lse - cap tanh64(x)| <= cap 6e-7 + ulp_fp32(|lse|)

Every call goes through the real drop-ins with softcap=cap and asserts, on the block it launched, the plan its case names
(kernels.describe_softcap); rows behind Lk hold NaN (K) and Inf (V) — a NaN score must be removed by the mask's select, never by arithmetic;
after a call with k / v the whole cache is compared bit for bit.  test_plans_reached prints the union and the worst figures."""
import os

import pytest
import torch

from tests import census as C
from tests import census_softcap as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = int(os.environ.get("VATTN_FUZZ_SCALE", "1"))
BASE = int(os.environ.get("VATTN_FUZZ_SEED_BASE", "0"))
ZERO, SIGNED, TWIN, TANH = S.zero_cases(), S.signed_cases(), S.twin_cases(), S.tanh_cases()
REACHED, SWEPT, RAN = {}, {}, {"zero": 0, "signed": 0, "twin": 0}
WORST = {"max_ulp": 0.0, "zero_lse_n": 0.0, "zero_case": "", "signed_lse_n": 0.0, "signed_case": "", "tanh": {}}
_base = {}
ids = lambda cs: [c["name"] for c in cs]


def _base_caches(dt, D, Hkv):
    """one random K and one census V per (dtype, D, kv heads), large enough for every case: the cases take clones of views"""
    key = (dt, D, Hkv)
    if key not in _base:
        g = torch.Generator(device=DEV).manual_seed(D + Hkv)
        k = 30 * torch.randn(19, S.LEN_CAP + S.SPARE, Hkv, D, device=DEV, dtype=C.DT[dt], generator=g)
        _base[key] = (k, C.census_values(19, S.LEN_CAP + S.SPARE, Hkv, D, C.DT[dt], device=DEV))
    return _base[key]


def _note(c, d, reached):
    k = S.plan_key(c, d)
    reached[k] = reached.get(k, 0) + 1


def run_zero(c, reached):
    rows = max(c["lens"]) + S.SPARE
    kb, vb = _base_caches(c["dt"], c["D"], c["Hkv"])
    k_fin, v_fin = kb[:c["n_slots"], :rows].clone(), vb[:c["n_slots"], :rows].clone()
    S.poison(c, k_fin, v_fin)
    q = torch.zeros(len(c["lens"]), max(C.case_qlens(c)), c["Hkv"] * c["G"], c["D"], dtype=C.DT[c["dt"]], device=DEV)
    out, lse, d = S.launch(c, q, k_fin, v_fin, DEV)
    _note(c, d, reached)
    fails, stats = C.compare(out.cpu(), lse.cpu(), c)
    WORST["max_ulp"] = max(WORST["max_ulp"], stats["max_ulp"])
    if stats["lse_worst_times_n"] > WORST["zero_lse_n"]:
        WORST["zero_lse_n"], WORST["zero_case"] = stats["lse_worst_times_n"], c["name"]
    assert not fails and stats["max_ulp"] <= 1.0, "%s cap %g %s\n  %s" % (c["name"], c["cap"], d, "\n  ".join(fails))


@pytest.mark.parametrize("case", ZERO, ids=ids(ZERO))
def test_zero_query_census(case):
    run_zero(case, REACHED)
    RAN["zero"] += 1


@pytest.mark.parametrize("seed", range(BASE, BASE + 10 * SCALE))
def test_zero_query_census_sweep(seed):
    """seeded draws of tests/census.py's sweep under caps 0.5 / 1.0 / 30 / 50; VATTN_FUZZ_SCALE / VATTN_FUZZ_SEED_BASE as in tests/test_gpu_fuzz.py"""
    for i in range(10):
        c = S.zero_sweep_case(10 * seed + i)
        assert C.admissible(c)
        run_zero(c, SWEPT)


@pytest.mark.parametrize("case", SIGNED, ids=ids(SIGNED))
def test_signed_census(case):
    c = case
    rows = max(c["lens"]) + S.SPARE
    for mode in S.sign_modes(c):
        plus = S.plus_cells(c, mode, rows)
        q, k_fin, v_fin = S.signed_inputs(c, plus, rows, device=DEV)
        S.poison(c, k_fin, v_fin)
        out, lse, d = S.launch(c, q, k_fin, v_fin, DEV)
        fails, stats = S.signed_compare(out.cpu(), lse.cpu(), c, plus)
        WORST["max_ulp"] = max(WORST["max_ulp"], stats["max_ulp"])
        if stats["lse_worst_times_n"] > WORST["signed_lse_n"]:
            WORST["signed_lse_n"], WORST["signed_case"] = stats["lse_worst_times_n"], "%s / %s" % (c["name"], mode)
        assert not fails and stats["max_ulp"] <= 1.0, "%s signs %r %s\n  %s" % (c["name"], mode, d, "\n  ".join(fails))
    _note(c, d, REACHED)
    RAN["signed"] += 1


@pytest.mark.parametrize("case", TWIN, ids=ids(TWIN))
def test_scale_twin(case):
    c = case
    rows = max(c["lens"]) + S.SPARE
    s = S.twin_scale(c["D"])
    qa, qb, k, v = S.twin_inputs(c, rows)
    bits = lambda x: x.view(torch.int16) if x.element_size() == 2 else x.view(torch.int32)
    for cap in S.TWIN_CAPS:
        cc = dict(c, cap=cap)
        res = []
        for q, scale in ((qa, s), (qb, 2 * s)):
            k_fin, v_fin = k.to(DEV), v.to(DEV)
            S.poison(cc, k_fin, v_fin)
            out, lse, d = S.launch(cc, q, k_fin, v_fin, DEV, scale=scale)
            res.append((out, lse, d))
        (oa, la, da), (ob, lb, db) = res
        what = "%s cap %g" % (c["name"], cap)
        assert da == db, what
        assert torch.equal(bits(oa), bits(ob)), "%s: %d output elements differ between (2 q, s) and (q, 2 s)" % (what, int((bits(oa) != bits(ob)).sum()))
        assert torch.equal(bits(la), bits(lb)), "%s: %d LSE values differ between (2 q, s) and (q, 2 s)" % (what, int((bits(la) != bits(lb)).sum()))
        # call A against float64 with the non-default scale (tests/test_gpu_softcap.py's check, restated in tests/census.py)
        ref64, lse64 = S.capped_reference(cc, qa, k, v, cap, scale=s, math="f64")
        ref32, _ = S.capped_reference(cc, qa, k, v, cap, scale=s, math="f32")
        ql = C.case_qlens(c)
        for b in range(len(ql)):          # (rows an entry of a batched call does not have hold nothing)
            C.check(oa[b:b + 1, :ql[b]], ref64[b:b + 1, :ql[b]], ref32[b:b + 1, :ql[b]], C.DT[c["dt"]], "%s entry %d" % (what, b))
            C.check_lse(la[b:b + 1, :, :ql[b]], lse64[b:b + 1, :, :ql[b]], "%s entry %d LSE" % (what, b))
    _note(c, da, REACHED)
    RAN["twin"] += 1


@pytest.mark.parametrize("cap", S.TANH_CAPS)
@pytest.mark.parametrize("case", TANH, ids=ids(TANH))
def test_tanh_read_out(case, cap):
    c = dict(case, cap=cap)
    rows = max(c["lens"]) + S.SPARE
    q, k, v, smp = S.tanh_inputs(c, cap, rows)
    k_fin, v_fin = k.to(DEV), v.to(DEV)
    S.poison(c, k_fin, v_fin)
    out, lse, d = S.launch(c, q, k_fin, v_fin, DEV)
    fails, worst = S.tanh_check(out.cpu(), lse.cpu(), c, cap, v, smp)
    if worst >= WORST["tanh"].get(cap, (0.0, ""))[0]:
        WORST["tanh"][cap] = (worst, c["name"])
    print("%s cap %g: %d one-key rows, worst |lse - cap tanh(x)| / cap = %.3e" % (c["name"], cap, len(smp["x"]), worst))
    assert not fails, "%s cap %g %s\n  %s" % (c["name"], cap, d, "\n  ".join(fails))


def test_plans_reached():
    """The union of (form, path, tiling, merge launch, windowed) parts 1-3 ran on (the sweep counted apart), and the worst figures, printed once.
    When every case of the three tables ran in this process, the union must hold every plan of tests/census_softcap.py NEED; a partial run (-k,
    a worker of a split run) says so and concludes nothing."""
    for title, reached in (("tables", REACHED), ("sweep", SWEPT)):
        print("\nsoftcap census %s: plans reached (form, path, tiling, merge_launch, windowed): cases" % title)
        for k in sorted(reached, key=str):
            print("  %s: %d" % (k, reached[k]))
    print("worst element error %.3f ulp; worst LSE error * n: part 1 %.4f (%s), part 2 %.4f (%s)"
          % (WORST["max_ulp"], WORST["zero_lse_n"], WORST["zero_case"], WORST["signed_lse_n"], WORST["signed_case"]))
    for cap in sorted(WORST["tanh"]):
        print("part 4, cap %g: worst |lse - cap tanh(x)| / cap = %.3e (%s); the bound is %.1e + ulp" % ((cap,) + WORST["tanh"][cap] + (S.TANH_BOUND,)))
    if (RAN["zero"], RAN["signed"], RAN["twin"]) != (len(ZERO), len(SIGNED), len(TWIN)):
        print("partial run: %s of %s table cases ran here, the coverage list is not checked" % (RAN, (len(ZERO), len(SIGNED), len(TWIN))))
        return
    missing = S.missing_plans(REACHED)
    print("missing plans: %s" % (missing or "none"))
    assert not missing, "plans the softcap tables no longer reach: %s" % missing
