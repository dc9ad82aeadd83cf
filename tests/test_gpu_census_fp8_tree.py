"""The key census (tests/census_fp8_tree.py beside tests/census.py; tests/test_gpu_census.py) on the builds it did not reach: FP8 (e4m3) decode — one token and multi-token —,
FP8 chunked prefill (tilings 1 and 4, batched chunks), and tree-masked multi-token decode over a 2-byte and over an FP8 cache.  q = 0 and one-hot
value rows make every output element count_d / n (x v_scale[h], a power of two) with EXACT kernel arithmetic, so one key dropped at a piece seam,
read twice, taken from the neighbouring kv head, slot or d-group of a 16-byte load, one draft key admitted against the mask, or a scale taken
from another head fails by >= 4 ulp where the parity tests' atol = 2e-3 cannot see it.  The assertions are the 2-byte census's, per element in
float64: |out - expected| <= 1 ulp of the output dtype, count-0 elements exactly 0, |lse - ln n| n < 0.25, dead rows 0 and +inf, nothing
non-finite, and the cache after an appending call equal to the given bytes, every byte (power-of-two scales make dequantise -> k / v ->
requantise the identity: tests/test_census_fp8_tree_model.py).

Every case goes through the real drop-in, over a strided [:, :rows] view, and asserts through the describe entry of ITS call, on the very
parameter block launched, the form, path, tiling and merge launch it names.  Caches are plain torch tensors with every page mapped; rows
behind Lk — the rows an append will fill included — hold the NaN byte 0x7F in K and V (2-byte caches: NaN and Inf): a wrong read is a NaN
output, never a fault.

THE BYTE TABLE (last two tests): every e4m3 byte through the widening of the decode and prefill builds, f16 and bf16 — V bytes bit for bit
through P = 1, K bytes through the LSE of a one-hot q."""
import math
import os
import time

import pytest
import torch

from tests import census_fp8_tree as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = int(os.environ.get("VATTN_FUZZ_SCALE", "1"))
BASE = int(os.environ.get("VATTN_FUZZ_SEED_BASE", "0"))
CASES = C.fp8_cases() + C.tree_cases()
REACHED, SWEPT, WORST = {}, {}, {"max_ulp": 0.0, "lse_worst_times_n": 0.0, "lse_case": "", "seconds": 0.0}
ROWS, SLOTS = 16384 + C.XSPARE, 19
_base = {}


def _base_caches(fp8, dt, D, Hkv):
    """one random K and one census V per (cache kind, dtype, D, kv heads), large enough for every case: the cases take clones of views"""
    key = ("fp8", D, Hkv) if fp8 else (dt, D, Hkv)
    if key not in _base:
        if fp8:
            _base[key] = (C.fp8_random_keys(SLOTS, ROWS, Hkv, D, D + Hkv, device=DEV), C.fp8_census_values(SLOTS, ROWS, Hkv, D, device=DEV))
        else:
            g = torch.Generator(device=DEV).manual_seed(D + Hkv)
            _base[key] = (torch.randn(SLOTS, ROWS, Hkv, D, device=DEV, dtype=C.DT[dt], generator=g), C.census_values(SLOTS, ROWS, Hkv, D, C.DT[dt], device=DEV))
    return _base[key]


def run_case(c, reached=None):
    t0 = time.time()
    fp8, lens, slots = c["fp8"], c["lens"], c["slots"]
    B, Sq, Hq = len(lens), max(C.case_qlens(c)), c["Hkv"] * c["G"]
    rows = max(lens) + C.XSPARE
    kb, vb = _base_caches(fp8, c["dt"], c["D"], c["Hkv"])
    k_fin, v_fin = kb[:c["n_slots"], :rows].clone(), vb[:c["n_slots"], :rows].clone()      # the caches as they must be AFTER the call
    pk, pv = (C.FP8_NAN, C.FP8_NAN) if fp8 else (float("nan"), float("inf"))
    for b in range(B):
        k_fin[slots[b], lens[b]:], v_fin[slots[b], lens[b]:] = pk, pv
    out, lse, d = C.launch_ext(c, torch.zeros(B, Sq, Hq, c["D"], dtype=C.DT[c["dt"]]), k_fin, v_fin, DEV, pk, pv)
    what = "%s: plan %s" % (c["name"], d)
    reached = REACHED if reached is None else reached
    key = C.plan_key(c, d)
    reached[key] = reached.get(key, 0) + 1
    fails, stats = C.compare(out.cpu(), lse.cpu() if lse is not None else None, c)
    print("%s: worst element error %.3f ulp, worst |lse - ln n| n = %.4f" % (c["name"], stats["max_ulp"], stats["lse_worst_times_n"]))
    if math.isfinite(stats["max_ulp"]):
        WORST["max_ulp"] = max(WORST["max_ulp"], stats["max_ulp"])
    if stats["lse_worst_times_n"] > WORST["lse_worst_times_n"]:
        WORST["lse_worst_times_n"], WORST["lse_case"] = stats["lse_worst_times_n"], c["name"]
    WORST["seconds"] = max(WORST["seconds"], time.time() - t0)
    assert not fails, what + "\n  " + "\n  ".join(fails)
    assert stats["max_ulp"] <= 1.0, what


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_census_fp8_tree(case):
    run_case(case)


@pytest.mark.parametrize("seed", range(BASE, BASE + 20 * SCALE))
def test_census_fp8_tree_sweep(seed):
    """Seeded random draws of form, cache kind, sq, heads, D, dtype, lengths, mask words, num_splits, append and slots; the expectation is
    closed-form: no reference run.  VATTN_FUZZ_SCALE / VATTN_FUZZ_SEED_BASE as in tests/test_gpu_census.py."""
    for i in range(10):
        c = C.xsweep_case(10 * seed + i)
        assert C.admissible(c)
        run_case(c, SWEPT)


def test_census_fp8_tree_plans_reached():
    """The union of (form, cache kind, tree mask, path, tiling, merge launch) the TABLE ran on (the sweep is counted apart), printed once.  When
    every case of the table ran in this process, the union must hold every plan in `need`; a partial run says so and concludes nothing."""
    for title, reached in (("table", REACHED), ("sweep", SWEPT)):
        print("\nfp8 / tree census %s: plans reached (form, cache, tree, path, tiling, merge_launch): calls" % title)
        for k in sorted(reached, key=str):
            print("  %s: %d" % (k, reached[k]))
    print("worst element error %.3f ulp; worst LSE error * n = %.4f (%s); slowest case %.2f s" % (WORST["max_ulp"], WORST["lse_worst_times_n"], WORST["lse_case"], WORST["seconds"]))
    if sum(REACHED.values()) != len(CASES):
        print("partial run: %d of %d table cases ran here, the coverage list is not checked" % (sum(REACHED.values()), len(CASES)))
        return
    need = [("dec", "fp8", False, 0, 1, 1), ("dec", "fp8", False, 0, 2, 1), ("dec", "fp8", False, 2, 1, 1), ("dec", "fp8", False, 2, 2, 1),
            ("mt", "fp8", False, 0, 1, 1), ("mt", "fp8", False, 0, 2, 1), ("mt", "fp8", False, 2, 1, 1), ("mt", "fp8", False, 2, 2, 1),
            ("mt", "2b", True, 0, 1, 1), ("mt", "2b", True, 0, 2, 1), ("mt", "2b", True, 2, 1, 1), ("mt", "2b", True, 2, 2, 1),
            ("mt", "fp8", True, 0, 1, 1), ("mt", "fp8", True, 0, 2, 1), ("mt", "fp8", True, 2, 1, 1), ("mt", "fp8", True, 2, 2, 1),
            ("pre", "fp8", False, 0, 1, 0), ("pre", "fp8", False, 0, 1, 1), ("pre", "fp8", False, 0, 4, 0), ("pre", "fp8", False, 0, 4, 1),
            ("var", "fp8", False, 0, 1, 0), ("var", "fp8", False, 0, 4, 0)]
    assert need == C.XNEED                                  # (the list the CPU model file checks on host-only blocks)
    missing = [k for k in need if k not in REACHED]
    assert not missing, "plans the fp8 / tree census tables no longer reach: %s" % missing


# ---------------------------------------------------------------------------------------------------------------------------------------
# the byte table
# ---------------------------------------------------------------------------------------------------------------------------------------
FORMS = ["dec", "mt", "tree", "pre_t1", "pre_t4"]


def _call(form, q, k8, v8, ks, vs, cl):
    """one call of `form` over fp8 caches in which every query row sees every key below cache_seqlens: (out, lse [B, Hq, Sq])"""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    kw = dict(cache_seqlens=cl, return_softmax_lse=True)
    if form == "tree":      # all ones: draft key base + s for every s with base + s >= 0
        r, p, mask, scl, pre = C.spy_issue(FA.flash_attn_fp8kv_tree_with_kvcache, q, k8, v8, ks, vs, torch.full(q.shape[:2], -1, dtype=torch.int32, device=DEV), **kw)
        assert K.describe_fp8kv_tree(p)["form"] == 1 and mask is not None and scl is not None
    elif form in ("dec", "mt"):
        r, p, mask, scl, pre = C.spy_issue(FA.flash_attn_fp8kv_with_kvcache, q, k8, v8, ks, vs, causal=False, **kw)
        assert K.describe_fp8kv(p)["form"] == 1 and mask is None and scl is not None and not pre
    else:
        til = int(form[-1])
        r, p, mask, scl, pre = C.spy_issue(FA.flash_attn_fp8kv_prefill_with_kvcache, q, k8, v8, ks, vs, causal=False, _variant=til << 1, **kw)
        d = K.describe_fp8kv_prefill(p)
        assert d["form"] == 0 and d["tiling"] == til and pre is True
    torch.cuda.synchronize()
    return r


def _sq(form):
    return {"dec": 1, "mt": 2, "tree": 2}.get(form, 12)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_every_value_byte_is_widened_exactly(form, dt):
    """Lk = 1, D = 128, two kv heads whose one visible value row holds the 256 bytes: P is exactly 1, so out[h, d] is value(byte) x v_scale[hk]
    rounded to the output dtype — exactly representable there, so bit for bit (the two zeros compare as zeros: +0 + 1 x -0 is +0 in the
    accumulator).  The two NaN bytes give NaN, and only their own elements."""
    dtype, D, sq = C.DT[dt], 128, _sq(form)
    g = torch.Generator().manual_seed(5)
    q = torch.randn(1, sq, 2, D, generator=g).to(dtype).to(DEV)
    v8 = torch.full((1, 4, 2, D), C.FP8_NAN, dtype=torch.uint8)
    v8[0, 0] = torch.arange(256, dtype=torch.uint8).view(2, D)
    k8 = C.fp8_random_keys(1, 4, 2, D, 3)
    k8[:, 1:] = C.FP8_NAN
    vs = [2.0, 0.5]
    out, lse = _call(form, q, k8.to(DEV).view(torch.float8_e4m3fn), v8.to(DEV).view(torch.float8_e4m3fn), torch.tensor([1.0, 0.25], device=DEV), torch.tensor(vs, device=DEV),
                     torch.ones(1, dtype=torch.int32, device=DEV))
    want = torch.tensor([[C.e4m3_value(hk * D + d) * vs[hk] for d in range(D)] for hk in range(2)], dtype=torch.float64)
    nan = torch.isnan(want)
    assert int(nan.sum()) == 2
    wd = want.to(dtype)
    assert torch.equal(wd.double()[~nan], want[~nan])          # exactly representable in the output dtype
    assert bool(torch.isfinite(lse).all())
    o = out.cpu()
    for t in range(sq):
        got = o[0, t]
        assert torch.equal(torch.isnan(got), nan), "%s %s row %d: NaN exactly where the byte is the NaN byte" % (form, dt, t)
        nz = ~nan & (want != 0)
        bad = (got.view(torch.int16) != wd.view(torch.int16)) & nz
        assert not bool(bad.any()), "%s %s row %d: bytes %s are not widened bit for bit: got %s, want %s" % (
            form, dt, t, [hex(int(h) * D + int(d)) for h, d in bad.nonzero()[:8]], got[bad][:8].tolist(), wd[bad][:8].tolist())
        assert bool((got[want == 0] == 0).all()), "%s %s row %d: the bytes 0x00 / 0x80" % (form, dt, t)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_every_key_byte_is_widened_exactly(form, dt):
    """q one-hot: entry b, head h has 1.0 at d = 8 b + h % 8, so the 16 x 16 (entry, head) pairs read 254 different finite K bytes of the byte
    row (kv head h // 8 holds bytes 128 hk + d; the NaN bytes' places hold 0x00: 0 x NaN would poison the whole row).  With the row at key 0
    and Lk = 1: lse = softmax_scale k_scale value(byte); at key 33 of Lk = 34 behind 33 keys of K byte 0: lse = ln(33 + e^x).  Against fp64
    within 1e-3 relative + 1e-6: adjacent e4m3 values differ by >= 1/16 relative (60 x the bound), the kernel's fp32 product and exp2 / log2
    round trip err by ~1e-6 relative (1000 x below it)."""
    dtype, D, B, Hq, Hkv, sq = C.DT[dt], 128, 16, 16, 2, _sq(form)
    ksc = [0.5, 0.25]
    scale = D ** -0.5
    q = torch.zeros(B, sq, Hq, D, dtype=dtype)
    byte = torch.zeros(B, Hq, dtype=torch.int64)
    for b in range(B):
        for h in range(Hq):
            d = 8 * b + h % 8
            q[b, :, h, d] = 1.0
            byte[b, h] = 128 * (h // 8) + d
    row = torch.arange(256, dtype=torch.uint8).view(Hkv, D).clone()
    row[:, D - 1] = 0
    byte[byte % 128 == D - 1] = 0
    assert len(set(byte.flatten().tolist())) == 254          # every finite byte (0x00 three times: its own place and the two NaN places)
    x = torch.tensor([[scale * ksc[h // 8] * C.e4m3_value(int(byte[b, h])) for h in range(Hq)] for b in range(B)], dtype=torch.float64)
    for pos in (0, 33):
        Lk = pos + 1
        k8 = torch.full((B, Lk + 4, Hkv, D), C.FP8_NAN, dtype=torch.uint8)
        v8 = torch.full((B, Lk + 4, Hkv, D), C.FP8_NAN, dtype=torch.uint8)
        k8[:, :pos], v8[:, :pos] = 0, 0
        k8[:, pos], v8[:, pos] = row, C.FP8_ONE
        out, lse = _call(form, q.to(DEV), k8.to(DEV).view(torch.float8_e4m3fn), v8.to(DEV).view(torch.float8_e4m3fn), torch.tensor(ksc, device=DEV),
                         torch.tensor([1.0, 2.0], device=DEV), torch.full((B,), Lk, dtype=torch.int32, device=DEV))
        ref = x if pos == 0 else torch.log(pos + torch.exp(x))
        assert bool(torch.isfinite(out).all())
        l = lse.double().cpu()
        for t in range(sq):
            err = (l[:, :, t] - ref).abs()
            bound = 1e-3 * ref.abs() + 1e-6
            bad = err > bound
            print("%s %s key %d row %d: worst |lse - ref| / bound = %.3g" % (form, dt, pos, t, float((err / bound).max())))
            assert not bool(bad.any()), "%s %s key position %d row %d: K bytes %s: lse %s, fp64 %s" % (
                form, dt, pos, t, [hex(int(v)) for v in byte[bad][:8]], l[:, :, t][bad][:8].tolist(), ref[bad][:8].tolist())
