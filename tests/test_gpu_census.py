"""The key census on the GPU (tests/census.py): q = 0 and one-hot value rows make every output element count_d / n with EXACT kernel arithmetic, so
a single key dropped, read twice, taken from the neighbouring kv head / slot or admitted at a mask edge fails by >= 4 ulp of the output dtype
where the parity tests' atol = 2e-3 cannot see it.  Asserted per element, in float64: |out - count_d / n| <= 1 ulp of the output dtype at
count_d / n (the only inexact steps are the final reciprocal, the product and the cast — and on merge paths fp32 exp2 / log2 of integers,
relative error ~1e-6, 1/500 of an fp16 half-ulp), elements with count_d = 0 exactly 0, LSE |lse - ln n| < 0.25 / n, dead rows 0 and +inf.

Every case asserts, through the plan description of the very parameter block the drop-in launches, the form, path, tiling and merge launch it
meant to reach; test_census_plans_reached prints the union.  Caches are plain torch tensors; the rows behind Lk (the rows an append will fill
included) hold NaN (K) and Inf (V), nothing is unmapped; after a call with k / v the whole cache is compared bit for bit.

Piece seams: pieces are whole 32-key (decode) / 64-key (prefill) tiles.  The one-tile pieces (host items of one tile, forced grids larger than
the tile count) put a seam at every tile edge — at the tile edge lo sits on (lens / lefts chosen so that lo is on an edge and one to either
side), in front of the tile that holds hi - 1, and inside the sq-row causal staircase whenever 1 <= Lk % 32 < sq."""
import os

import pytest
import torch

from tests import census as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = int(os.environ.get("VATTN_FUZZ_SCALE", "1"))
BASE = int(os.environ.get("VATTN_FUZZ_SEED_BASE", "0"))
SPARE = 8
CASES = C.gpu_cases()
REACHED, SWEPT, WORST = {}, {}, {"max_ulp": 0.0, "lse_worst_times_n": 0.0, "lse_case": ""}
_base = {}


def _base_caches(dt, D, Hkv):
    """one random K and one census V per (dtype, D, kv heads), large enough for every case: the cases take clones of views"""
    key = (dt, D, Hkv)
    if key not in _base:
        g = torch.Generator(device=DEV).manual_seed(D + Hkv)
        k = torch.randn(19, 16384 + SPARE, Hkv, D, device=DEV, dtype=C.DT[dt], generator=g)
        _base[key] = (k, C.census_values(19, 16384 + SPARE, Hkv, D, C.DT[dt], device=DEV))
    return _base[key]


def _bits(x):
    return x.view(torch.int16)


def run_case(c, reached=None):
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    dtype, D, Hkv, G, sq, lens, slots = C.DT[c["dt"]], c["D"], c["Hkv"], c["G"], c["sq"], c["lens"], c["slots"]
    ql = C.case_qlens(c)
    B, Sq, Hq = len(lens), max(ql), Hkv * G
    rows = max(lens) + SPARE
    kb, vb = _base_caches(c["dt"], D, Hkv)
    k_fin, v_fin = kb[:c["n_slots"], :rows].clone(), vb[:c["n_slots"], :rows].clone()      # the caches as they must be AFTER the call
    for b in range(B):
        k_fin[slots[b], lens[b]:], v_fin[slots[b], lens[b]:] = float("nan"), float("inf")
    # the rows an append will fill are poisoned like the spare rows behind Lk
    kc, vc, new, cl = C.cut_out_appended(c, k_fin, v_fin, float("nan"), float("inf"))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    idx = i32(slots) if c["idx"] else None
    win = (c["left"], 0) if c.get("left") is not None else (-1, -1)
    lse, plan = None, None
    if c["form"] == "var":
        T = sum(ql)
        starts = [sum(ql[:i]) for i in range(B)]
        if c.get("pf"):
            p = K.AttnParams()
            p.b, p.seqlen_q, p.h, p.h_k, p.d, p.is_causal = B, Sq, Hq, Hkv, D, int(c["causal"])
            p.o_row_stride, p.o_head_stride = Hq * D, D
            plan = FA.prefill_plan(p, ql, lens, torch.device(DEV), **c["pf"])
            assert plan.t is not None and (plan.n_wg > 0) == c["pf"]["persistent"] and plan.drawn == bool(c["pf"].get("drawn")), c["name"]
        flat = torch.full((T, Hq, D), 7.0, dtype=dtype, device=DEV)
        _, p = C.spy_call(FA.flash_attn_varlen_with_kvcache, torch.zeros(T, Hq, D, dtype=dtype, device=DEV), kc, vc, i32(starts), i32(ql), Sq, i32(lens), idx,
                         causal=c["causal"], out=flat, num_splits=c["splits"], _variant=c["variant"], _max_seqlen_k=max(lens), _pf_plan=plan, window_size=win)
        out = torch.zeros(B, Sq, Hq, D, dtype=dtype, device=DEV)
        for b in range(B):
            out[b, :ql[b]] = flat[starts[b]:starts[b] + ql[b]]
    else:
        host = dict(_cache_seqlens_host=cl, _plan_tiles=c["host_tiles"]) if c.get("host_tiles") else {}
        (out, lse), p = C.spy_call(FA.flash_attn_with_kvcache, torch.zeros(B, sq, Hq, D, dtype=dtype, device=DEV), kc, vc, *new, cache_seqlens=i32(cl), cache_batch_idx=idx,
                                  causal=c["causal"], window_size=win, num_splits=c["splits"], return_softmax_lse=True, _variant=c["variant"], **host)
    torch.cuda.synchronize()
    d = K.describe(p)
    what = C.assert_plan(c, p, d, rows)
    if plan is not None:
        assert d["workgroups"] == (plan.n_wg if c["pf"]["persistent"] else plan.n_items), what
    queue = ("assigned" if p.pf_wg_first else "drawn") if p.pf_num_wg else ""
    key = (c["form"], d["path"], d["tiling"], d["merge_launch"], queue, c.get("left") is not None)
    reached = REACHED if reached is None else reached
    reached[key] = reached.get(key, 0) + 1
    fails, stats = C.compare(out.cpu(), lse.cpu() if lse is not None else None, c)
    WORST["max_ulp"] = max(WORST["max_ulp"], stats["max_ulp"])
    if stats["lse_worst_times_n"] > WORST["lse_worst_times_n"]:
        WORST["lse_worst_times_n"], WORST["lse_case"] = stats["lse_worst_times_n"], c["name"]
    assert not fails, what + "\n  " + "\n  ".join(fails)
    assert stats["max_ulp"] <= 1.0, what
    if new[0] is not None:
        assert torch.equal(_bits(kc), _bits(k_fin)) and torch.equal(_bits(vc), _bits(v_fin)), what + ": the cache after the append, every row, bit for bit"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_census(case):
    run_case(case)


@pytest.mark.parametrize("seed", range(BASE, BASE + 20 * SCALE))
def test_census_sweep(seed):
    """Seeded random draws of form, sq, heads, D, dtype, lengths, left, num_splits, append and slots — windows and multi-token calls included.
    The expectation is closed-form: no oracle run.  VATTN_FUZZ_SCALE / VATTN_FUZZ_SEED_BASE as in tests/test_gpu_fuzz.py."""
    for i in range(10):
        c = C.sweep_case(10 * seed + i)
        assert C.admissible(c)
        run_case(c, SWEPT)


def test_census_plans_reached():
    """The union of (form, path, tiling, merge launch, persistent queue, windowed) the TABLE ran on (the sweep is counted apart), printed once.
    When every case of the table ran in this process, the union must hold every plan in `need`; a partial run (-k, a worker of a split run)
    says so and concludes nothing."""
    for title, reached in (("table", REACHED), ("sweep", SWEPT)):
        print("\ncensus %s: plans reached (form, path, tiling, merge_launch, queue, windowed): calls" % title)
        for k in sorted(reached, key=str):
            print("  %s: %d" % (k, reached[k]))
    print("worst element error %.3f ulp; worst LSE error * n = %.4f (%s)" % (WORST["max_ulp"], WORST["lse_worst_times_n"], WORST["lse_case"]))
    if sum(REACHED.values()) != len(CASES):
        print("partial run: %d of %d table cases ran here, the coverage list is not checked" % (sum(REACHED.values()), len(CASES)))
        return
    need = [("dec", 0, 1, 1, "", False), ("dec", 0, 2, 1, "", False), ("dec", 1, 1, 1, "", False), ("dec", 1, 2, 1, "", False), ("dec", 2, 1, 1, "", False),
            ("dec", 2, 2, 1, "", False), ("dec", 2, 1, 1, "", True), ("dec", 2, 2, 1, "", True), ("dec", 0, 1, 1, "", True), ("dec", 0, 2, 0, "", True),
            ("dec", 0, 2, 1, "", True),
            ("mt", 2, 1, 1, "", False), ("mt", 2, 2, 1, "", False), ("mt", 0, 2, 1, "", False), ("mt", 0, 1, 1, "", False), ("mt", 2, 1, 1, "", True), ("mt", 2, 2, 1, "", True),
            ("mt", 0, 2, 0, "", True), ("mt", 0, 2, 1, "", True),
            ("pre", 0, 1, 0, "", False), ("pre", 0, 4, 0, "", False), ("pre", 0, 7, 0, "", False), ("pre", 0, 1, 1, "", False), ("pre", 0, 4, 1, "", False),
            ("pre", 0, 7, 1, "", False), ("pre", 0, 1, 0, "", True), ("pre", 0, 4, 0, "", True), ("pre", 0, 7, 0, "", True), ("pre", 0, 1, 1, "", True),
            ("pre", 0, 4, 1, "", True), ("pre", 0, 7, 1, "", True),
            ("var", 0, 1, 0, "", False), ("var", 0, 4, 0, "", False), ("var", 0, 7, 0, "", False), ("var", 0, 1, 0, "", True), ("var", 0, 4, 0, "", True),
            ("var", 0, 7, 0, "", True), ("var", 1, 7, 1, "", False), ("var", 1, 7, 1, "assigned", False), ("var", 1, 7, 1, "drawn", False)]
    missing = [k for k in need if k not in REACHED]
    assert not missing, "plans the census table no longer reaches: %s" % missing
