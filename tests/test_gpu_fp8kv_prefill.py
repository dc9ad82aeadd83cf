"""GPU tests of chunked prefill over the FP8 (e4m3) KV cache (include/vattn_kernels.h, "Prefill over an fp8 cache";
flash_attn.flash_attn_fp8kv_prefill_with_kvcache / flash_attn_fp8kv_varlen_with_kvcache) against tests/fp8kv_ref.py computed FROM THE BYTES THE
GPU STORED.  Every call asserts through kernels.describe_fp8kv_prefill which tiling and split count it took.

Tolerances are the project's prefill tolerances, restated from tests/test_gpu_attention.py (`_check`: atol = rtol = 2e-3 for fp16, 1.6e-2 for
bf16 against the float64 reference, AND the kernel's error at most 2 x the reference-numerics error + 1e-5 (+ 4e-3 for bf16); LSE within 2e-3
absolute, +inf on rows without a visible key).  None is new: widening e4m3 to fp16 / bf16 is exact and the scales are two fp32 factors per
workgroup, so against the 2-byte kernels on the dequantised values the fp8 builds add no rounding step.

Shapes are small on purpose: the key tile is 64, the ring loads two tiles ahead and runs tiles in pairs, a workgroup is 256 rows (tiling 1) or
128 rows (tiling 4); d = 64 on tiling 1 is the build in which half the workgroup stages a tile.  The no-read contract is checked by POISONING
rows (the NaN byte 0x7f in K and in V); nothing is unmapped on purpose."""
import pytest
import torch

from tests.fp8kv_ref import FP8, amax_scales, fp8kv_attn_ref, quantize_ref
from vattention_amd import flash_attn as FA
from vattention_amd import kernels as K
from vattention_amd.cache_ops import cache_flat_fp8
from vattention_amd.flash_attn import flash_attn_fp8kv_prefill_with_kvcache, flash_attn_fp8kv_varlen_with_kvcache, flash_attn_fp8kv_with_kvcache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [(64, torch.float16), (64, torch.bfloat16), (128, torch.float16), (128, torch.bfloat16)]
DT_IDS = ["d64_f16", "d64_bf16", "d128_f16", "d128_bf16"]
TILINGS = (1, 4)
SPREAD = (1.0, 3.0, 0.3, 2.0)


def _tol(dtype):
    return (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)


def _check(out_gpu, ref64, ref32, dtype, what):
    atol, rtol = _tol(dtype)
    got = out_gpu.double().cpu()
    err = (got - ref64).abs()
    bound = atol + rtol * ref64.abs()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print("%s: max err %.3e (reference-numerics err %.3e)" % (what, err.max().item(), e_ref))
    assert bool((err <= bound).all()), "%s: max err %.3e (allowed %.3e)" % (what, err.max().item(), bound.max().item())
    assert err.max().item() <= 2 * e_ref + 1e-5 + (0 if dtype == torch.float16 else 4e-3), \
        "%s: kernel err %.3e vs reference-numerics err %.3e" % (what, err.max().item(), e_ref)


def _check_lse(lse, lse64, what):
    lse = lse.double().cpu()
    dead = torch.isinf(lse64)
    assert torch.equal(torch.isinf(lse) & (lse > 0), dead & (lse64 > 0)), what + ": rows without a visible key have LSE +inf"
    print("%s: max err %.3e" % (what, ((lse - lse64)[~dead]).abs().max().item()))
    assert ((lse - lse64)[~dead]).abs().max().item() < 2e-3, what


def _bytes(x8):
    return x8.view(torch.uint8)


def _spied(fn, *a, **kw):
    """fn(*a, **kw) — one of the two fp8 prefill entry points — returning also the plan description of the very parameter block the drop-in
    launched, and asserting that the call went through the fp8 PREFILL entry point (the drop-in's counter, scales and selector at the launch)"""
    seen, issue = [], FA._issue
    n0 = FA.counters["fp8kv_prefill_calls"]

    def spy(p, dev, lib, need=None, mask=None, scales=None, fp8_prefill=False):
        seen.append((p, scales, fp8_prefill))
        return issue(p, dev, lib, need, mask, scales, fp8_prefill)
    FA._issue = spy
    try:
        r = fn(*a, **kw)
    finally:
        FA._issue = issue
    assert FA.counters["fp8kv_prefill_calls"] == n0 + 1 and len(seen) == 1 and seen[0][1] is not None and seen[0][2] is True
    p = seen[0][0]
    assert not p.pf_items and not p.split_items                    # no host-side plan on this path
    d = K.describe_fp8kv_prefill(p)
    assert d["form"] == 0 and d["path"] == 0 and d["tiling"] in TILINGS, d
    return r, d


def _pf(*a, **kw):
    return _spied(flash_attn_fp8kv_prefill_with_kvcache, *a, **kw)


def _filled(lens, slots, rows, Hkv, D, dtype, seed, spread=None):
    """caches [slots, rows, Hkv, D] whose rows [0, lens[i]) of slot idx[i] were written ON THE GPU by cache_flat_fp8 from N(0,1) data in `dtype`
    (spread: per-head factors on the data, so that the per-head scales differ); every other byte is 0xA5.  Scales = amax / 448 over the rows
    written (x 1.25: headroom for rows appended later).  Returns the GPU caches, the scales (GPU), the slot permutation (CPU) and the CPU
    copies of what the GPU stored."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(slots, generator=g)[:len(lens)].to(torch.int32)
    sl = idx.tolist()
    f = torch.ones(Hkv) if spread is None else torch.tensor([spread[h % len(spread)] for h in range(Hkv)])
    src = [((torch.randn(n, Hkv, D, generator=g) * f.view(1, -1, 1)).to(dtype), (torch.randn(n, Hkv, D, generator=g) * f.flip(0).view(1, -1, 1)).to(dtype)) for n in lens]
    floor = lambda fac: (3.5 * fac).view(1, Hkv, 1).expand(1, Hkv, D)      # (so that an empty prefix has scales too)
    ks = amax_scales(torch.cat([s[0].float() for s in src] + [floor(f)])) * 1.25
    vs = amax_scales(torch.cat([s[1].float() for s in src] + [floor(f.flip(0))])) * 1.25
    k8 = torch.full((slots, rows, Hkv, D), 0xA5, dtype=torch.uint8, device=DEV).view(FP8)
    v8 = torch.full((slots, rows, Hkv, D), 0xA5, dtype=torch.uint8, device=DEV).view(FP8)
    ksg, vsg = ks.to(DEV), vs.to(DEV)
    for i, (kn, vn) in enumerate(src):
        if kn.shape[0]:
            cache_flat_fp8(kn.to(DEV), vn.to(DEV), k8[sl[i]], v8[sl[i]], ksg, vsg)
    torch.cuda.synchronize()
    return k8, v8, ksg, vsg, idx, k8.cpu(), v8.cpu(), f


def _new_rows(B, n, Hkv, D, dtype, f, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(B, n, Hkv, D, generator=g) * f.view(1, 1, -1, 1)).to(dtype), (torch.randn(B, n, Hkv, D, generator=g) * f.flip(0).view(1, 1, -1, 1)).to(dtype))


def _refs(q, k8c, v8c, ks, vs, kn, vn, cl, idx, causal):
    """(float64 out, float64 LSE, reference-numerics out, the caches after the append) from the bytes the GPU stored"""
    ka, va = k8c.clone(), v8c.clone()
    ref64, lse64 = fp8kv_attn_ref(q, ka, va, ks.cpu(), vs.cpu(), kn, vn, cache_seqlens=cl, cache_batch_idx=idx, causal=causal, return_lse=True)
    ref32 = fp8kv_attn_ref(q, k8c.clone(), v8c.clone(), ks.cpu(), vs.cpu(), kn, vn, cache_seqlens=cl, cache_batch_idx=idx, causal=causal, math="f32")
    return ref64, lse64, ref32, ka, va


# ---- 1. a chunk on a prefix ----

@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 8), (8, 1)], ids=["8_2", "8_8", "8_1"])
def test_chunk_on_a_prefix(Hq, Hkv, D, dtype):
    """b = 2 over permuted slots, prefixes (333, 70) + a 200-row chunk appended through the call: Lk = (533, 270) — 9 and 5 key tiles (odd counts,
    a partial last tile), partial query blocks for both tilings; causal and not; out and LSE."""
    pre, Sq, B, rows = [333, 70], 200, 2, 540
    k8, v8, ks, vs, idx, k8c, v8c, f = _filled(pre, 3, rows, Hkv, D, dtype, 10 * Hq + Hkv + D, spread=SPREAD)
    assert Hkv == 1 or float(ks.max() / ks.min()) > 2
    torch.manual_seed(Hq + Hkv + D)
    q = torch.randn(B, Sq, Hq, D).to(dtype)
    kn, vn = _new_rows(B, Sq, Hkv, D, dtype, f, 5)
    cl = torch.tensor(pre, dtype=torch.int32)
    for causal in (True, False):
        ref64, lse64, ref32, ka, va = _refs(q, k8c, v8c, ks, vs, kn, vn, cl, idx, causal)
        for til in TILINGS:
            what = "%d/%d d=%d %s causal=%s tiling=%d" % (Hq, Hkv, D, dtype, causal, til)
            kg, vg = k8.clone(), v8.clone()
            (out, lse), d = _pf(q.to(DEV), kg, vg, ks, vs, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=causal,
                                return_softmax_lse=True, _variant=til << 1)
            torch.cuda.synchronize()
            assert d["tiling"] == til and d["nsplit"] == 1 and d["workgroups"] == (1 if til == 1 else 2) * Hq * B, d
            assert torch.equal(_bytes(kg.cpu()), _bytes(ka)) and torch.equal(_bytes(vg.cpu()), _bytes(va)), what + ": the caches after the call"
            _check(out, ref64, ref32, dtype, what)
            _check_lse(lse, lse64, what + " lse")


# ---- 2. a whole prompt from an empty cache ----

@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("Sq", [130, 64])
def test_whole_prompt_from_an_empty_cache(Sq, D, dtype):
    """cache_seqlens = 0: three key tiles / exactly one; causal, so row 0 of an entry sees only itself (its own V row as stored)"""
    Hq, Hkv, B = 8, 2, 2
    k8, v8, ks, vs, idx, k8c, v8c, f = _filled([0, 0], 2, Sq + 6, Hkv, D, dtype, Sq + D, spread=SPREAD)
    torch.manual_seed(Sq)
    q = torch.randn(B, Sq, Hq, D).to(dtype)
    kn, vn = _new_rows(B, Sq, Hkv, D, dtype, f, 6)
    cl = torch.zeros(B, dtype=torch.int32)
    ref64, lse64, ref32, ka, va = _refs(q, k8c, v8c, ks, vs, kn, vn, cl, idx, True)
    for til in TILINGS:
        what = "whole prompt Sq=%d d=%d %s tiling=%d" % (Sq, D, dtype, til)
        kg, vg = k8.clone(), v8.clone()
        (out, lse), d = _pf(q.to(DEV), kg, vg, ks, vs, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=True,
                            return_softmax_lse=True, _variant=til << 1)
        torch.cuda.synchronize()
        assert d["tiling"] == til and d["nsplit"] == 1, d
        _check(out, ref64, ref32, dtype, what)
        _check_lse(lse, lse64, what + " lse")
        own = (quantize_ref(vn[:, 0], vs.cpu()).double() * vs.cpu().double().view(1, -1, 1)).repeat_interleave(Hq // Hkv, dim=1)      # [B, Hq, D]
        assert (out[:, 0].double().cpu() - own).abs().max().item() <= _tol(dtype)[0] * (1 + own.abs().max().item()), what + ": row 0 is its own V row"


# ---- 3. key-range shares ----

@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
def test_key_range_shares(D, dtype):
    """forced shares (fp32 partials through the workspace, merged by combine_rows_kernel): 2 and 3 over Lk = 533 (9 tiles), 3 over Lk = 100 (2 tiles:
    the third share is empty); equal to the unsplit call and to the reference"""
    Hq, Hkv, Sq = 8, 2, 40
    for Lk, shares in ((533, (2, 3)), (100, (3,))):
        k8, v8, ks, vs, idx, k8c, v8c, f = _filled([Lk, Lk - 7], 2, Lk + 3, Hkv, D, dtype, Lk + D, spread=SPREAD)
        torch.manual_seed(Lk)
        q = torch.randn(2, Sq, Hq, D).to(dtype)
        cl = torch.tensor([Lk, Lk - 7], dtype=torch.int32)
        for causal in (True, False):
            ref64, lse64, ref32, _, _ = _refs(q, k8c, v8c, ks, vs, None, None, cl, idx, causal)
            (one, _), d1 = _pf(q.to(DEV), k8, v8, ks, vs, cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=causal, return_softmax_lse=True,
                               _variant=4 << 1)
            assert d1["nsplit"] == 1 and d1["workspace_bytes"] == 0, d1
            for ns in shares:
                for til in ((0, 1) if ns == 3 else (0,)):          # (0: the planner's tiling under forced shares — the 4-wave one for so small a grid)
                    what = "Lk=%d shares=%d d=%d %s causal=%s tiling=%d" % (Lk, ns, D, dtype, causal, til)
                    (out, lse), d = _pf(q.to(DEV), k8, v8, ks, vs, cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=causal,
                                        return_softmax_lse=True, _num_splits=ns, _variant=til << 1)
                    torch.cuda.synchronize()
                    assert d["nsplit"] == ns and d["tiling"] == (til or 4) and d["merge_launch"] == 1, d
                    assert d["workspace_bytes"] == ns * 2 * Sq * Hq * (D + 1) * 4 > 0, d
                    _check(out, ref64, ref32, dtype, what)
                    _check_lse(lse, lse64, what + " lse")
                    assert (out.float() - one.float()).abs().max().item() <= _tol(dtype)[0] * (1 + one.float().abs().max().item()), what + ": equals the unsplit call"


# ---- 4. append through the call ----

@pytest.mark.parametrize("D,dtype", [(128, torch.bfloat16), (64, torch.float16)], ids=["d128_bf16", "d64_f16"])
def test_append_through_the_call(D, dtype):
    """The appended rows are the CPU quantiser's bytes (saturating values included), every other byte of both caches is what it was, and the
    result is the two-step call's (cache_flat_fp8, then attend) bit for bit."""
    Hq, Hkv, Sq, pre = 8, 2, 70, [0, 31, 130]
    B, rows = len(pre), 210
    k8, v8, ks, vs, idx, k8c, v8c, f = _filled(pre, 4, rows, Hkv, D, dtype, 40 + D, spread=SPREAD)
    torch.manual_seed(D)
    q = torch.randn(B, Sq, Hq, D).to(dtype)
    kn, vn = _new_rows(B, Sq, Hkv, D, dtype, f, 7)
    kn[1, 0, 0, 3], vn[2, Sq - 1, 1, 5] = 1e4, -1e4                # saturate
    cl = torch.tensor(pre, dtype=torch.int32)
    ref64, lse64, ref32, ka, va = _refs(q, k8c, v8c, ks, vs, kn, vn, cl, idx, True)
    for b in range(B):
        s, n0 = int(idx[b]), pre[b]
        assert torch.equal(_bytes(ka[s, n0:n0 + Sq]), _bytes(quantize_ref(kn[b], ks.cpu()))) and torch.equal(_bytes(va[s, n0:n0 + Sq]), _bytes(quantize_ref(vn[b], vs.cpu())))
    assert (_bytes(ka) == 0x7E).any() and (_bytes(va) == 0xFE).any()
    untouched = torch.ones(4, rows, dtype=torch.bool)
    for b in range(B):
        untouched[int(idx[b]), pre[b]:pre[b] + Sq] = False
    for til in TILINGS:
        kg, vg = k8.clone(), v8.clone()
        out, d = _pf(q.to(DEV), kg, vg, ks, vs, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=True, _variant=til << 1)
        torch.cuda.synchronize()
        assert d["tiling"] == til, d
        kgc, vgc = _bytes(kg.cpu()), _bytes(vg.cpu())
        assert torch.equal(kgc, _bytes(ka)) and torch.equal(vgc, _bytes(va)), "the caches after the call are the reference's, every byte"
        assert torch.equal(kgc[untouched], _bytes(k8c)[untouched]) and torch.equal(vgc[untouched], _bytes(v8c)[untouched]), "no other byte changed"
        _check(out, ref64, ref32, dtype, "append d=%d tiling=%d" % (D, til))
        k2, v2 = k8.clone(), v8.clone()
        for b in range(B):
            cache_flat_fp8(kn[b].to(DEV), vn[b].to(DEV), k2[int(idx[b]), pre[b]:], v2[int(idx[b]), pre[b]:], ks, vs)
        two, _ = _pf(q.to(DEV), k2, v2, ks, vs, cache_seqlens=(cl + Sq).to(DEV), cache_batch_idx=idx.to(DEV), causal=True, _variant=til << 1)
        torch.cuda.synchronize()
        assert torch.equal(out, two), "one call == append, then attend"


# ---- 5. the no-read contract ----

@pytest.mark.parametrize("D,dtype", [(64, torch.float16), (128, torch.bfloat16)], ids=["d64_f16", "d128_bf16"])
def test_no_read_contract(D, dtype):
    """Rows at and beyond Lk of every slot in use and ALL rows of the unused slots hold the NaN byte 0x7f in K and in V: outputs and LSE are finite
    and equal to the unpoisoned run's, bit for bit — unsplit and in key-range shares, both tilings."""
    Hq, Hkv, Sq = 8, 2, 150
    lens = [533, 150, 64, 200]
    B, slots, rows = len(lens), 6, 600
    k8, v8, ks, vs, idx, _, _, _ = _filled(lens, slots, rows, Hkv, D, dtype, 4 + D, spread=SPREAD)
    kp, vp = k8.clone(), v8.clone()
    _bytes(kp)[:] = 0x7F
    _bytes(vp)[:] = 0x7F
    for b in range(B):
        s = int(idx[b])
        _bytes(kp)[s, :lens[b]] = _bytes(k8)[s, :lens[b]]
        _bytes(vp)[s, :lens[b]] = _bytes(v8)[s, :lens[b]]
    assert bool(torch.isnan(kp.float()).any()) and int((_bytes(kp) == 0x7F).all(dim=3).all(dim=2).all(dim=1).sum()) == slots - B
    torch.manual_seed(8)
    q = torch.randn(B, Sq, Hq, D, device=DEV).to(dtype)
    cl, idg = torch.tensor(lens, dtype=torch.int32, device=DEV), idx.to(DEV)
    for causal in (True, False):
        for til, ns in ((1, 0), (4, 0), (1, 2), (4, 3)):
            (a, la), d = _pf(q, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idg, causal=causal, return_softmax_lse=True, _num_splits=ns, _variant=til << 1)
            (p, lp), _ = _pf(q, kp, vp, ks, vs, cache_seqlens=cl, cache_batch_idx=idg, causal=causal, return_softmax_lse=True, _num_splits=ns, _variant=til << 1)
            torch.cuda.synchronize()
            assert d["tiling"] == til and d["nsplit"] == (ns or 1), d
            assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "tiling=%d shares=%d causal=%s" % (til, ns, causal)
            assert torch.equal(la, lp) and not bool(torch.isnan(lp).any())


# ---- 6. batched chunks ----

@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
def test_batched_chunks(D, dtype):
    """q_lens = (37, 130, 2) on prefixes (0, 519, 64), appended beforehand with cache_flat_fp8; one launch, compared entry by entry"""
    Hq, Hkv = 8, 2
    q_lens, pre = [37, 130, 2], [0, 519, 64]
    tot = [a + b for a, b in zip(q_lens, pre)]
    k8, v8, ks, vs, idx, k8c, v8c, _ = _filled(tot, 4, 660, Hkv, D, dtype, 60 + D, spread=SPREAD)
    torch.manual_seed(D + 1)
    q = torch.randn(sum(q_lens), Hq, D).to(dtype)
    starts = [0, 37, 167]
    refs64, refs32 = [], []
    for i, (s0, n) in enumerate(zip(starts, q_lens)):
        s = int(idx[i])
        for dst, kw in ((refs64, {}), (refs32, {"math": "f32"})):
            dst.append(fp8kv_attn_ref(q[s0:s0 + n].unsqueeze(0), k8c[s:s + 1], v8c[s:s + 1], ks.cpu(), vs.cpu(), cache_seqlens=tot[i], causal=True, **kw)[0])
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    for til in TILINGS:
        out, d = _spied(flash_attn_fp8kv_varlen_with_kvcache, q.to(DEV), k8, v8, ks, vs, i32(starts), i32(q_lens), 130, i32(tot), cache_batch_idx=idx.to(DEV),
                        causal=True, _variant=til << 1)
        torch.cuda.synchronize()
        assert d["tiling"] == til and d["nsplit"] == 1 and d["workgroups"] == (1 if til == 1 else 2) * Hq * 3, d
        for i, (s0, n) in enumerate(zip(starts, q_lens)):
            _check(out[s0:s0 + n], refs64[i], refs32[i], dtype, "batched chunks entry %d d=%d %s tiling=%d" % (i, D, dtype, til))
    assert torch.equal(_bytes(k8.cpu()), _bytes(k8c)) and torch.equal(_bytes(v8.cpu()), _bytes(v8c)), "attending writes nothing"


# ---- 7. the scales are indexed by the kv head ----

@pytest.mark.parametrize("D,dtype,til", [(128, torch.float16, 1), (64, torch.bfloat16, 1), (64, torch.float16, 4)], ids=["d128_f16_t1", "d64_bf16_t1", "d64_f16_t4"])
def test_scales_are_indexed_by_the_kv_head(D, dtype, til):
    """Permuting the kv heads of the caches, the scales and (group-wise) the query heads together permutes the output heads, bit for bit; swapping
    two scales alone changes the result."""
    Hq, Hkv, Sq, Lk = 8, 4, 100, 300
    G = Hq // Hkv
    k8, v8, ks, vs, idx, k8c, v8c, _ = _filled([Lk], 1, Lk, Hkv, D, dtype, 70 + D, spread=(1.0, 10.0, 0.1, 3.0))
    r = (ks[1:] / ks[:-1]).cpu()
    assert bool(((r > 2.5) | (r < 0.4)).all())
    torch.manual_seed(D)
    q = (torch.randn(1, Sq, Hq, D) * torch.tensor([1.0, 0.1, 10.0, 0.3]).repeat_interleave(G).view(1, 1, Hq, 1)).to(dtype).to(DEV)      # scores stay O(1)
    cl = torch.tensor([Lk], dtype=torch.int32, device=DEV)
    base, d = _pf(q, k8, v8, ks, vs, cache_seqlens=cl, causal=True, _variant=til << 1)
    assert d["tiling"] == til, d
    ref64 = fp8kv_attn_ref(q.cpu(), k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=Lk, causal=True)
    ref32 = fp8kv_attn_ref(q.cpu(), k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=Lk, causal=True, math="f32")
    _check(base, ref64, ref32, dtype, "10x scales d=%d tiling=%d" % (D, til))
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    qperm = (perm.view(-1, 1) * G + torch.arange(G, device=DEV).view(1, -1)).reshape(-1)
    heads = lambda x8: _bytes(x8)[:, :, perm].contiguous().view(FP8)
    moved, _ = _pf(q[:, :, qperm].contiguous(), heads(k8), heads(v8), ks[perm].contiguous(), vs[perm].contiguous(),
                   cache_seqlens=cl, causal=True, _variant=til << 1)
    torch.cuda.synchronize()
    assert torch.equal(moved, base[:, :, qperm]), "heads, bytes and scales permuted together"
    swapped = ks.clone()
    swapped[0], swapped[1] = ks[1], ks[0]
    other, _ = _pf(q, k8, v8, swapped, vs, cache_seqlens=cl, causal=True, _variant=til << 1)
    torch.cuda.synchronize()
    assert (other[:, :, :2 * G].float() - base[:, :, :2 * G].float()).abs().max().item() > 0.05 and torch.equal(other[:, :, 2 * G:], base[:, :, 2 * G:])
    swapped = vs.clone()
    swapped[2], swapped[3] = vs[3], vs[2]
    other, _ = _pf(q, k8, v8, ks, swapped, cache_seqlens=cl, causal=True, _variant=til << 1)
    torch.cuda.synchronize()
    assert (other[:, :, 2 * G:].float() - base[:, :, 2 * G:].float()).abs().max().item() > 0.05 and torch.equal(other[:, :, :2 * G], base[:, :, :2 * G])


# ---- 8. graph capture ----

def test_graph_capture_with_append():
    """One captured chunk (append + attend in key-range shares, so also the merge launch; lengths and scales are read on the device), replayed on
    advanced cache_seqlens, equals the eager call.  A single capture stream, no parallel branches."""
    torch.manual_seed(21)
    B, Hq, Hkv, D, Sq, rows = 2, 8, 2, 128, 70, 400
    pre = [100, 31]
    k8, v8, ks, vs, idx, _, _, _ = _filled(pre, 3, rows, Hkv, D, torch.float16, 9, spread=SPREAD)
    q, kn, vn = (torch.randn(B, Sq, n, D, device=DEV).half() for n in (Hq, Hkv, Hkv))
    cl, idg = torch.tensor(pre, dtype=torch.int32, device=DEV), idx.to(DEV)
    out = torch.empty_like(q)
    kw = dict(cache_seqlens=cl, cache_batch_idx=idg, causal=True, _num_splits=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on the capture stream: creates that stream's workspace
        flash_attn_fp8kv_prefill_with_kvcache(q, k8.clone(), v8.clone(), ks, vs, kn, vn, out=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kg, vg = k8.clone(), v8.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        flash_attn_fp8kv_prefill_with_kvcache(q, kg, vg, ks, vs, kn, vn, out=out, **kw)
    for step in range(3):                               # the capture itself launched nothing: replay 0 is the first chunk
        q.copy_(torch.randn_like(q)); kn.copy_(torch.randn_like(kn)); vn.copy_(torch.randn_like(vn))
        if step:
            cl.add_(Sq)
        ke, ve = kg.clone(), vg.clone()
        g.replay()
        torch.cuda.synchronize()
        ref = flash_attn_fp8kv_prefill_with_kvcache(q, ke, ve, ks, vs, kn, vn, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), step
        assert torch.equal(_bytes(kg), _bytes(ke)) and torch.equal(_bytes(vg), _bytes(ve))
    assert cl.tolist() == [pre[0] + 2 * Sq, pre[1] + 2 * Sq]


# ---- 9. end to end through the page manager ----

def test_chunked_prefill_then_decode_through_the_page_manager():
    """init_kvcache(dtype=float8_e4m3fn): one 300-token prompt prefilled in chunks of 128, 128 and 44 with the new call, then four decode steps with
    flash_attn_fp8kv_with_kvcache; every step against the reference built from the stored bytes, the final cache = the quantiser's bytes of the
    whole sequence."""
    from vattention_amd import vattention
    torch.zeros(1, device=DEV)
    mn, _ = vattention.granularity(0)
    page = 64 << 10 if (64 << 10) % mn == 0 else 2 << 20
    L, Hkv, Hq, D, B, ctx = 1, 2, 8, 128, 4, 16384
    ts = vattention.init_kvcache(L, Hkv, D, B, ctx, 0, FP8, page, False)
    try:
        Kt, Vt = ts[0], ts[1]
        assert Kt.dtype == FP8 and Vt.dtype == FP8 and Kt.element_size() == 1
        vattention.reserve_physical_pages(64 * page)
        torch.manual_seed(9)
        total = 304
        kall, vall = torch.randn(total, Hkv, D).half() * torch.tensor([1.0, 4.0]).view(1, 2, 1).half(), torch.randn(total, Hkv, D).half()
        ks, vs = amax_scales(kall).to(DEV), amax_scales(vall).to(DEV)
        want_k, want_v = quantize_ref(kall, ks.cpu()), quantize_ref(vall, vs.cpu())
        lens = [0] * B
        s = vattention.alloc_new_batch_idx(128)
        sl = torch.tensor([s], dtype=torch.int32, device=DEV)
        cur = 0
        for step, n in enumerate((128, 128, 44, 1, 1, 1, 1)):
            lens[s] = cur + n                                      # the length INCLUDES the new rows: their pages get mapped
            vattention.step_async(lens)
            q = torch.randn(1, n, Hq, D).half()
            kn, vn = kall[cur:cur + n].unsqueeze(0), vall[cur:cur + n].unsqueeze(0)
            cl = torch.tensor([cur], dtype=torch.int32, device=DEV)
            args = (q.to(DEV), Kt[:, :cur + n], Vt[:, :cur + n], ks, vs, kn.to(DEV), vn.to(DEV))
            if n > 1:
                out, d = _pf(*args, cache_seqlens=cl, cache_batch_idx=sl, causal=True)
                assert d["tiling"] == 4 and d["nsplit"] == 1, d      # the default plan of so small a grid
            else:
                out = flash_attn_fp8kv_with_kvcache(*args, cache_seqlens=cl, cache_batch_idx=sl, causal=True)
            torch.cuda.synchronize()
            cur += n
            assert torch.equal(_bytes(Kt[s, :cur].cpu()), _bytes(want_k[:cur])) and torch.equal(_bytes(Vt[s, :cur].cpu()), _bytes(want_v[:cur])), step
            k8, v8 = want_k[:cur].unsqueeze(0), want_v[:cur].unsqueeze(0)
            ref64 = fp8kv_attn_ref(q, k8, v8, ks.cpu(), vs.cpu(), cache_seqlens=cur, causal=True)
            ref32 = fp8kv_attn_ref(q, k8, v8, ks.cpu(), vs.cpu(), cache_seqlens=cur, causal=True, math="f32")
            _check(out, ref64, ref32, torch.float16, "page manager step %d (%d rows)" % (step, n))
        assert cur == total
    finally:
        vattention.cleanup()


# ---- 10. the gate from Python ----

def test_gate():
    """Calls outside the gate raise NotImplementedError with the library's message, which names the rule; missing scales and a cache of another
    dtype raise RuntimeError; the refused calls leave nothing behind."""
    Hq, Hkv, D = 8, 2, 128
    k8, v8, ks, vs, idx, _, _, _ = _filled([300, 40], 2, 320, Hkv, D, torch.float16, 1)
    cl = torch.tensor([300, 40], dtype=torch.int32, device=DEV)
    q = torch.randn(2, 50, Hq, D, device=DEV).half()
    blocks, issue = [], FA._issue

    def spy(p, dev, lib, need=None, mask=None, scales=None, fp8_prefill=False):
        blocks.append((p, dev, lib, scales))
        return issue(p, dev, lib, need, mask, scales, fp8_prefill)
    FA._issue = spy
    try:
        good = flash_attn_fp8kv_prefill_with_kvcache(q, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idx.to(DEV), causal=True)
    finally:
        FA._issue = issue
    p, dev, lib, scales = blocks[0]

    def refused(word, **fields):
        old = {n: getattr(p, n) for n in fields}
        for n, v in fields.items():
            setattr(p, n, v)
        try:
            with pytest.raises(NotImplementedError, match=word):
                issue(p, dev, lib, None, None, scales, True)
            with pytest.raises(RuntimeError, match=word):
                K.describe_fp8kv_prefill(p)
        finally:
            for n, v in old.items():
                setattr(p, n, v)
    some = cl.data_ptr()                                   # a device address; the library refuses before anything reads it
    refused("sliding window", window_left_plus1=65)
    refused("rotary", rotary_cos_sin=some, rotary_dim=D, rotary_row_stride=D)
    refused("pf_items", pf_items=some, num_pf_items=2)
    refused("split_items", split_items=some, split_seq=some, num_split_items=2)
    with pytest.raises(NotImplementedError, match="prefill64 has no fp8 build"):
        flash_attn_fp8kv_prefill_with_kvcache(q, k8, v8, ks, vs, cache_seqlens=cl, causal=True, _variant=7 << 1)
    for qq in (torch.randn(2, 1, Hq, D, device=DEV).half(), torch.randn(2, 4, Hq, D, device=DEV).half()):      # decode-form blocks
        with pytest.raises(NotImplementedError, match="vattn_fp8kv_attn_with_kvcache"):
            flash_attn_fp8kv_prefill_with_kvcache(qq, k8, v8, ks, vs, cache_seqlens=cl, causal=True)
        flash_attn_fp8kv_with_kvcache(qq, k8, v8, ks, vs, cache_seqlens=cl, causal=True)                         # ... which that entry takes
    with pytest.raises(NotImplementedError, match="prefill form"):                                               # ... and it still refuses this one
        flash_attn_fp8kv_with_kvcache(q, k8, v8, ks, vs, cache_seqlens=cl, causal=True)
    for a, b in ((None, vs), (ks, None)):
        with pytest.raises(RuntimeError, match="k_scale and v_scale"):
            flash_attn_fp8kv_prefill_with_kvcache(q, k8, v8, a, b, cache_seqlens=cl)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    for fn, args in ((flash_attn_fp8kv_prefill_with_kvcache, ()), (flash_attn_fp8kv_varlen_with_kvcache, (i32([0, 50]), i32([50, 50]), 50))):
        qq = q if not args else q.reshape(100, Hq, D)
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            fn(qq, k8.view(torch.uint8).half(), v8.view(torch.uint8).half(), ks, vs, *args, cache_seqlens=cl)
    with pytest.raises(RuntimeError, match="same dtype"):      # the 2-byte entry points do not take an fp8 cache
        FA.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cl, causal=True)
    with pytest.raises(RuntimeError, match="same dtype"):
        FA.flash_attn_varlen_with_kvcache(q.reshape(100, Hq, D), k8, v8, i32([0, 50]), i32([50, 50]), 50, cl)
    again = flash_attn_fp8kv_prefill_with_kvcache(q, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idx.to(DEV), causal=True)
    torch.cuda.synchronize()
    assert torch.equal(good, again)                        # the refused calls left nothing behind
