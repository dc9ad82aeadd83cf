"""GPU tests of the FP8 (e4m3) KV cache (include/vattn_kernels.h, "FP8 KV cache"): the quantising append (cache_ops.cache_flat_fp8) bit for bit
against the CPU quantiser, and decode over an fp8 cache (flash_attn.flash_attn_fp8kv_with_kvcache) against tests/fp8kv_ref.py computed FROM
THE BYTES THE GPU STORED.  Every call asserts through kernels.describe_fp8kv which launch plan it took.

Tolerances are the project's, restated from tests/test_gpu_multitoken_decode.py (`_check`: 2e-3 / 2e-3 for fp16, 1.6e-2 for bf16; `_check_lse`:
2e-3 absolute).  None is new: widening e4m3 to fp16 / bf16 is exact and the scales are folded into two fp32 factors per workgroup, so against
the 2-byte kernels on the dequantised values the fp8 builds add no rounding step.  The no-read contract is checked by POISONING rows (the NaN
byte 0x7f in K and in V); nothing is unmapped on purpose."""
import pytest
import torch

from tests.fp8kv_ref import FP8, amax_scales, fp8kv_attn_ref, quantize_ref
from vattention_amd import flash_attn as FA
from vattention_amd import kernels as K
from vattention_amd.cache_ops import cache_flat_fp8
from vattention_amd.flash_attn import flash_attn_fp8kv_with_kvcache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = [(8, 2), (32, 4), (8, 8), (8, 1), (40, 1)]      # (40, 1): G > 16 (two head blocks per workgroup) and G > 32 (sibling groups)
DT = [(64, torch.float16), (64, torch.bfloat16), (128, torch.float16), (128, torch.bfloat16)]
DT_IDS = ["d64_f16", "d64_bf16", "d128_f16", "d128_bf16"]


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
    assert ((lse - lse64)[~dead]).abs().max().item() < 2e-3, what


def _bytes(x8):
    return x8.view(torch.uint8)


def _f8(*a, **kw):
    """flash_attn_fp8kv_with_kvcache, returning also the plan description of the very parameter block the drop-in launched (seen at its
    launch point) — and asserting that the call went through the fp8 entry point (the drop-in's counter, the scales at the launch)"""
    seen, issue = [], FA._issue
    n0 = FA.counters["fp8kv_decode_calls"]

    def spy(p, dev, lib, need=None, mask=None, scales=None):
        seen.append((p, scales))
        return issue(p, dev, lib, need, mask, scales)
    FA._issue = spy
    try:
        r = flash_attn_fp8kv_with_kvcache(*a, **kw)
    finally:
        FA._issue = issue
    assert FA.counters["fp8kv_decode_calls"] == n0 + 1 and len(seen) == 1 and seen[0][1] is not None
    d = K.describe_fp8kv(seen[0][0])
    assert d["form"] == 1 and d == K.describe(seen[0][0]), d
    return r, d


def _filled(lens, slots, rows, Hkv, D, dtype, seed, spread=None):
    """caches [slots, rows, Hkv, D] whose rows [0, lens[i]) of slot idx[i] were written ON THE GPU by cache_flat_fp8 from N(0,1) data in `dtype`
    (spread: per-head factors on the data, so that the per-head scales differ); every other byte is 0xA5.  Scales = amax / 448 over the rows
    written.  Returns the GPU caches, the scales (GPU), the slot permutation (CPU) and the CPU copies of what the GPU stored."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(slots, generator=g)[:len(lens)].to(torch.int32)
    sl = idx.tolist()
    f = torch.ones(Hkv) if spread is None else torch.tensor([spread[h % len(spread)] for h in range(Hkv)])
    src = [((torch.randn(n, Hkv, D, generator=g) * f.view(1, -1, 1)).to(dtype), (torch.randn(n, Hkv, D, generator=g) * f.flip(0).view(1, -1, 1)).to(dtype)) for n in lens]
    ks, vs = amax_scales(torch.cat([s[0] for s in src])), amax_scales(torch.cat([s[1] for s in src]))
    k8 = torch.full((slots, rows, Hkv, D), 0xA5, dtype=torch.uint8, device=DEV).view(FP8)
    v8 = torch.full((slots, rows, Hkv, D), 0xA5, dtype=torch.uint8, device=DEV).view(FP8)
    ksg, vsg = ks.to(DEV), vs.to(DEV)
    for i, (kn, vn) in enumerate(src):
        cache_flat_fp8(kn.to(DEV), vn.to(DEV), k8[sl[i]], v8[sl[i]], ksg, vsg)
    torch.cuda.synchronize()
    return k8, v8, ksg, vsg, idx, k8.cpu(), v8.cpu(), src


# ---- the quantising append ----

@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
def test_cache_flat_fp8_is_the_cpu_quantiser_bit_for_bit(D, dtype):
    """fp16 / bf16 sources, contiguous and strided cache views and sources, values beyond +-448 * scale, a NaN, zeros of both signs, values in
    the subnormal range of e4m3; rows outside [0, n) and bytes between the rows of a strided view keep the pattern written beforehand."""
    torch.manual_seed(D)
    Hkv, n, rows = 3, 37, 50
    key, value = torch.randn(n, Hkv, D).to(dtype), torch.randn(n, Hkv, D).to(dtype)
    ks, vs = torch.tensor([0.004, 0.04, 4.0]), torch.tensor([0.01, 0.001, 0.1])      # head 0 of K mostly saturates, head 2 reaches the subnormals (< 2^-6)
    key[3, 0, 5], key[4, 1, 0], key[5, 2, 7], value[6, 1, 9] = 500 * 0.004, -20.0, float("nan"), float("nan")
    key[7, 1, :4] = torch.tensor([0.0, -0.0, 0.04 * 2.0 ** -9, -0.04 * 2.0 ** -10]).to(dtype)
    value[8, 0, 0], value[8, 0, 1] = 1e4, -1e4
    wk, wv = _bytes(quantize_ref(key, ks)), _bytes(quantize_ref(value, vs))
    assert (wk == 0x7E).any() and (wk == 0xFE).any() and (wk == 0x7F).any() and (wv == 0x7F).any() and ((wk & 0x78) == 0).any()
    ksg, vsg = ks.to(DEV), vs.to(DEV)
    for strided in (False, True):
        W = 2 * Hkv * D if strided else Hkv * D                      # row pitch of the cache view in bytes
        kc = torch.full((rows, W), 0xA5, dtype=torch.uint8, device=DEV)
        vc = torch.full((rows, W), 0x5A, dtype=torch.uint8, device=DEV)
        kview = kc[2:, W - Hkv * D:].view(FP8).unflatten(1, (Hkv, D))      # rows 2.., the right half of every row
        vview = vc[2:, W - Hkv * D:].view(FP8).unflatten(1, (Hkv, D))
        ksrc = torch.zeros(n, 2 * Hkv, D, dtype=dtype, device=DEV)[:, :Hkv] if strided else torch.empty(n, Hkv, D, dtype=dtype, device=DEV)
        ksrc.copy_(key)
        cache_flat_fp8(ksrc, value.to(DEV), kview, vview, ksg, vsg)
        torch.cuda.synchronize()
        for got, want, fill, what in ((kc.cpu(), wk, 0xA5, "K"), (vc.cpu(), wv, 0x5A, "V")):
            body = got[2:2 + n, W - Hkv * D:]
            diff = (body != want.reshape(n, -1)).nonzero()
            assert diff.numel() == 0, "%s strided=%s: %d bytes differ, first at %s" % (what, strided, diff.shape[0], diff[0].tolist())
            keep = got.clone()
            keep[2:2 + n, W - Hkv * D:] = fill
            assert bool((keep == fill).all()), what + ": a byte outside rows [0, n) of the view was written"


def test_cache_flat_fp8_scalar_path_for_unaligned_rows():
    """head_size 24 is no whole number of 16-byte chunks: the element-wise kernel stores the same bytes"""
    torch.manual_seed(3)
    n, Hkv, D = 9, 2, 24
    key, value = torch.randn(n, Hkv, D).half() * 3, torch.randn(n, Hkv, D).half()
    ks, vs = torch.tensor([0.005, 0.02]), torch.tensor([0.01, 0.003])
    kc, vc = torch.zeros(n + 2, Hkv, D, dtype=torch.uint8, device=DEV).view(FP8), torch.zeros(n + 2, Hkv, D, dtype=torch.uint8, device=DEV).view(FP8)
    cache_flat_fp8(key.to(DEV), value.to(DEV), kc, vc, ks.to(DEV), vs.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(_bytes(kc.cpu())[:n], _bytes(quantize_ref(key, ks))) and torch.equal(_bytes(vc.cpu())[:n], _bytes(quantize_ref(value, vs)))
    assert not bool(_bytes(kc.cpu())[n:].any()) and not bool(_bytes(vc.cpu())[n:].any())


# ---- decode parity ----

LENS = ([1, 31, 32, 33, 4099], [64, 65, 257, 1000, 33])


@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("Hq,Hkv", HEADS, ids=["%d_%d" % h for h in HEADS])
def test_decode_parity(Hq, Hkv, D, dtype):
    """Ragged batches of 5 with cache_batch_idx permuted over a strided [:, :max] cache view: the default plan (the stream decomposition
    where the block takes it), a forced uniform split with its merge launch, forced stream grids; LSE; a caller-provided strided out."""
    G = Hq // Hkv
    for li, lens in enumerate(LENS):
        B, slots, rows = len(lens), 7, max(lens) + 5
        k8, v8, ks, vs, idx, k8c, v8c, _ = _filled(lens, slots, rows + 3, Hkv, D, dtype, 100 * Hq + Hkv + D + li)
        torch.manual_seed(Hq + D + li)
        q = torch.randn(B, 1, Hq, D).to(dtype)
        cl = torch.tensor(lens, dtype=torch.int32)
        ref64, lse64 = fp8kv_attn_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=cl, cache_batch_idx=idx, return_lse=True)
        ref32 = fp8kv_attn_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=cl, cache_batch_idx=idx, math="f32")
        qg, clg, idg = q.to(DEV), cl.to(DEV), idx.to(DEV)
        paths = set()
        for splits in (0, 3, -7, 1):
            what = "%d/%d d=%d %s lens=%d splits=%d" % (Hq, Hkv, D, dtype, li, splits)
            out = torch.full((B, 1, Hq + 1, D), 7.0, dtype=dtype, device=DEV)[:, :, :Hq]
            (_, d) = _f8(qg, k8[:, :rows], v8[:, :rows], ks, vs, cache_seqlens=clg, cache_batch_idx=idg, out=out, _num_splits=splits)
            torch.cuda.synchronize()
            assert d["tiling"] == (2 if G > 16 else 1), d
            stream = G <= 16 and splits <= 0                       # (two-block workgroups and explicit splits keep the grid heuristics)
            assert d["path"] == (2 if stream else 0) and (stream or d["nsplit"] == (splits if splits > 0 else d["nsplit"])), d
            assert d["merge_launch"] == (1 if stream or d["nsplit"] > 1 else 0), d
            paths.add((d["path"], d["merge_launch"]))
            _check(out, ref64, ref32, dtype, what)
            (o2, lse), _ = _f8(qg, k8[:, :rows], v8[:, :rows], ks, vs, cache_seqlens=clg, cache_batch_idx=idg, return_softmax_lse=True, _num_splits=splits)
            torch.cuda.synchronize()
            assert torch.equal(o2, out), what + ": the same plan, the same bits"
            _check_lse(lse, lse64, what + " lse")
        assert (0, 1) in paths and (0, 0) in paths and (G > 16 or (2, 1) in paths), paths
        assert torch.equal(_bytes(k8.cpu()), _bytes(k8c)) and torch.equal(_bytes(v8.cpu()), _bytes(v8c)), "attending writes nothing"


@pytest.mark.parametrize("D,dtype", [(128, torch.float16), (64, torch.bfloat16)], ids=["d128_f16", "d64_bf16"])
def test_scales_are_indexed_by_the_kv_head(D, dtype):
    """data — and so the amax scales — of neighbouring kv heads 10x apart, in opposite order for K and V"""
    lens, Hq, Hkv = [700, 33, 2049], 12, 4
    k8, v8, ks, vs, idx, k8c, v8c, _ = _filled(lens, 4, 2060, Hkv, D, dtype, 5, spread=(1.0, 10.0, 0.1, 3.0))
    r = (ks[1:] / ks[:-1]).cpu()
    assert bool(((r > 5) | (r < 0.2)).all())
    torch.manual_seed(6)
    q = torch.randn(3, 1, Hq, D).to(dtype) * torch.tensor([1.0, 0.1, 10.0, 0.3]).repeat_interleave(3).view(1, 1, Hq, 1).to(dtype)      # scores stay O(1)
    cl = torch.tensor(lens, dtype=torch.int32)
    ref64 = fp8kv_attn_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=cl, cache_batch_idx=idx)
    ref32 = fp8kv_attn_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=cl, cache_batch_idx=idx, math="f32")
    for splits in (0, 4):
        out, d = _f8(q.to(DEV), k8, v8, ks, vs, cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), _num_splits=splits)
        torch.cuda.synchronize()
        _check(out, ref64, ref32, dtype, "10x scales splits=%d" % splits)


# ---- the multi-token form ----

@pytest.mark.parametrize("Hq,Hkv,D,dtype", [(8, 2, 128, torch.float16), (32, 4, 64, torch.bfloat16), (8, 8, 128, torch.bfloat16), (16, 1, 64, torch.float16)],
                         ids=["g4_d128_f16", "g8_d64_bf16", "mha_d128_bf16", "g16_d64_f16"])
@pytest.mark.parametrize("sq", [2, 5, 8])
def test_multitoken_parity(sq, Hq, Hkv, D, dtype):
    """seqlen_q 2 / 5 / 8, causal and not, Lk straddling a tile boundary, an entry with Lk < seqlen_q (dead rows: 0 and LSE +inf)"""
    if sq * (Hq // Hkv) > 64:
        sq = 64 // (Hq // Hkv)                                   # (g16: 8 rows would be 128 columns — the widest block the form takes)
    lens = [30 + sq, 64, 65, sq - 1, 1500 + sq]
    B, slots, rows = len(lens), 6, max(lens) + 2
    k8, v8, ks, vs, idx, k8c, v8c, _ = _filled(lens, slots, rows, Hkv, D, dtype, sq * 1000 + Hq + D)
    torch.manual_seed(sq + Hq)
    q = torch.randn(B, sq, Hq, D).to(dtype)
    cl = torch.tensor(lens, dtype=torch.int32)
    for causal in (True, False):
        ref64, lse64 = fp8kv_attn_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=cl, cache_batch_idx=idx, causal=causal, return_lse=True)
        ref32 = fp8kv_attn_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), cache_seqlens=cl, cache_batch_idx=idx, causal=causal, math="f32")
        for splits in (0, -5):
            what = "sq=%d %d/%d d=%d causal=%s splits=%d" % (sq, Hq, Hkv, D, causal, splits)
            (out, lse), d = _f8(q.to(DEV), k8, v8, ks, vs, cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=causal,
                                return_softmax_lse=True, _num_splits=splits)
            torch.cuda.synchronize()
            assert d["tiling"] == (2 if sq * (Hq // Hkv) > 16 else 1), d
            _check(out, ref64, ref32, dtype, what)
            _check_lse(lse, lse64, what + " lse")
            if causal:
                assert out[3, 0].float().abs().max().item() == 0.0 and bool(torch.isinf(lse[3, :, 0]).all())      # Lk = sq - 1: row 0 sees no key


# ---- append through the call ----

@pytest.mark.parametrize("sq,dtype,D", [(1, torch.float16, 128), (1, torch.bfloat16, 64), (4, torch.float16, 64), (8, torch.bfloat16, 128)],
                         ids=["one_token_f16", "one_token_bf16_d64", "sq4_f16_d64", "sq8_bf16"])
def test_append_through_the_call(sq, dtype, D):
    """k / v given: the stored bytes are the CPU quantiser's, no other byte of the caches changes, and the result equals the two-step call
    (cache_flat_fp8's rows, then attend) bit for bit; rows that would land beyond the cache view are dropped."""
    Hq, Hkv = 8, 2
    lens = [0, 31, 500, 1030 - sq]                               # cache_seqlens BEFORE the append
    B, rows = len(lens), 1030
    k8, v8, ks, vs, idx, k8c, v8c, _ = _filled(lens, 5, rows, Hkv, D, dtype, 77 + sq)
    torch.manual_seed(sq)
    q, kn, vn = torch.randn(B, sq, Hq, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype) * 1.5, torch.randn(B, sq, Hkv, D).to(dtype) * 1.5
    kn[1, 0, 0, 3], vn[2, sq - 1, 1, 5] = 1e4, -1e4                # saturate
    cl = torch.tensor(lens, dtype=torch.int32)
    ka, va = k8c.clone(), v8c.clone()
    ref64 = fp8kv_attn_ref(q, ka, va, ks.cpu(), vs.cpu(), kn, vn, cache_seqlens=cl, cache_batch_idx=idx, causal=True)      # (appends into ka / va)
    ref32 = fp8kv_attn_ref(q, k8c.clone(), v8c.clone(), ks.cpu(), vs.cpu(), kn, vn, cache_seqlens=cl, cache_batch_idx=idx, causal=True, math="f32")
    for splits in ((0, 2) if sq == 1 else (0, -3)):          # (num_splits > 0 keeps the prefill kernels for a multi-row block: outside the gate)
        kg, vg = k8.clone(), v8.clone()
        out, _ = _f8(q.to(DEV), kg, vg, ks, vs, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=True, _num_splits=splits)
        torch.cuda.synchronize()
        assert torch.equal(_bytes(kg.cpu()), _bytes(ka)) and torch.equal(_bytes(vg.cpu()), _bytes(va)), "the caches after the call are the reference's, every byte"
        _check(out, ref64, ref32, dtype, "append sq=%d splits=%d" % (sq, splits))
        k2, v2 = k8.clone(), v8.clone()
        for b in range(B):
            cache_flat_fp8(kn[b].to(DEV), vn[b].to(DEV), k2[int(idx[b]), lens[b]:], v2[int(idx[b]), lens[b]:], ks, vs)
        two, _ = _f8(q.to(DEV), k2, v2, ks, vs, cache_seqlens=(cl + sq).to(DEV), cache_batch_idx=idx.to(DEV), causal=True, _num_splits=splits)
        torch.cuda.synchronize()
        assert torch.equal(out, two), "one call == append, then attend"
    # a view one row short of the last entry's append: that row is dropped, nothing is written behind the view
    kg, vg = k8.clone(), v8.clone()
    _f8(q.to(DEV), kg[:, :rows - 1], vg[:, :rows - 1], ks, vs, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=True)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(kg.cpu())[:, rows - 1], _bytes(k8c)[:, rows - 1]) and torch.equal(_bytes(kg.cpu())[:, :rows - 1], _bytes(ka)[:, :rows - 1])


# ---- the no-read contract ----

@pytest.mark.parametrize("sq,Hq,Hkv", [(1, 8, 2), (1, 40, 1), (4, 8, 2)], ids=["one_token", "one_token_g40", "sq4"])
def test_no_read_contract(sq, Hq, Hkv):
    """Rows at and beyond Lk hold the NaN byte 0x7f in K and in V: the outputs are finite and equal to the unpoisoned run's."""
    D, dtype = 128, torch.float16
    lens = [3000, 400, 1777, sq, 95, 1]
    lens[-1] = max(lens[-1], sq)
    B, rows = len(lens), 3100
    k8, v8, ks, vs, idx, _, _, _ = _filled(lens, B, rows, Hkv, D, dtype, 4 + sq)
    kp, vp = k8.clone(), v8.clone()
    for b in range(B):
        _bytes(kp)[int(idx[b]), lens[b]:] = 0x7F
        _bytes(vp)[int(idx[b]), lens[b]:] = 0x7F
    assert bool(torch.isnan(kp.float()).any())
    torch.manual_seed(8)
    q = torch.randn(B, sq, Hq, D, device=DEV).to(dtype)
    cl, idg = torch.tensor(lens, dtype=torch.int32, device=DEV), idx.to(DEV)
    for splits in ((0, 3, -5, -64) if sq == 1 else (0, -5, -64)):
        a, _ = _f8(q, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idg, causal=True, _num_splits=splits)
        p, _ = _f8(q, kp, vp, ks, vs, cache_seqlens=cl, cache_batch_idx=idg, causal=True, _num_splits=splits)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "splits=%d" % splits


# ---- graph capture, the page manager, the gate ----

def test_graph_capture_with_append():
    """One captured decode step (append + attend; the scales are read on the device) replayed with other data equals the eager call."""
    torch.manual_seed(21)
    B, Hq, Hkv, D, ctx = 4, 8, 2, 128, 3000
    lens = [100, 2500, 31, 1999]
    k8, v8, ks, vs, idx, _, _, _ = _filled(lens, 6, ctx, Hkv, D, torch.float16, 9)
    q, kn, vn = (torch.randn(B, 1, n, D, device=DEV).half() for n in (Hq, Hkv, Hkv))
    cl, idg = torch.tensor(lens, dtype=torch.int32, device=DEV), idx.to(DEV)
    out = torch.empty_like(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on the capture stream: creates that stream's workspace
        flash_attn_fp8kv_with_kvcache(q, k8.clone(), v8.clone(), ks, vs, kn, vn, cache_seqlens=cl, cache_batch_idx=idg, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kg, vg = k8.clone(), v8.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        flash_attn_fp8kv_with_kvcache(q, kg, vg, ks, vs, kn, vn, cache_seqlens=cl, cache_batch_idx=idg, out=out)
    for step in range(3):
        q.copy_(torch.randn_like(q)); kn.copy_(torch.randn_like(kn)); vn.copy_(torch.randn_like(vn))
        if step:
            cl.add_(1)
            ks.mul_(1.5)                                # (the scales live on the device: a replay reads their current values)
        ke, ve = kg.clone(), vg.clone()
        g.replay()
        torch.cuda.synchronize()
        ref = flash_attn_fp8kv_with_kvcache(q, ke, ve, ks, vs, kn, vn, cache_seqlens=cl, cache_batch_idx=idg)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), step
        assert torch.equal(_bytes(kg), _bytes(ke)) and torch.equal(_bytes(vg), _bytes(ve))


def test_decode_steps_through_the_page_manager():
    """init_kvcache(dtype=float8_e4m3fn) on the HIP VMM backend: fp8 tensors with the itemsize-1 layout (twice the tokens per page); a
    sequence grows across a page boundary; append and decode of one layer against the reference, every step."""
    from vattention_amd import vattention
    torch.zeros(1, device=DEV)
    mn, _ = vattention.granularity(0)
    page = 64 << 10 if (64 << 10) % mn == 0 else 2 << 20
    L, Hkv, Hq, D, B, ctx = 1, 2, 8, 128, 4, 16384
    tok_per_page = page // (Hkv * D)                                # one byte per element
    ts = vattention.init_kvcache(L, Hkv, D, B, ctx, 0, FP8, page, False)
    try:
        Kt, Vt = ts[0], ts[1]
        assert Kt.dtype == FP8 and Vt.dtype == FP8 and tuple(Kt.shape) == (B, ctx, Hkv, D) and Kt.element_size() == 1
        assert Kt.stride(1) == Hkv * D and vattention._pm.layout.tokens_per_page == tok_per_page
        vattention.reserve_physical_pages(64 * page)
        torch.manual_seed(9)
        starts = [tok_per_page - 2, 700]                              # slot 0 crosses into its second page at the third decode step
        lens, slots = [0] * B, []
        for n in starts:
            s = vattention.alloc_new_batch_idx(n)
            lens[s] = n
            slots.append(s)
        vattention.step_async(lens)
        kp, vp = [torch.randn(n, Hkv, D).half() for n in starts], [torch.randn(n, Hkv, D).half() for n in starts]
        ks, vs = (amax_scales(torch.cat(kp)) * 1.5).to(DEV), (amax_scales(torch.cat(vp)) * 1.5).to(DEV)      # (headroom for the decode rows)
        host = {}
        for s, k, v in zip(slots, kp, vp):
            cache_flat_fp8(k.to(DEV), v.to(DEV), Kt[s], Vt[s], ks, vs)
            host[s] = [quantize_ref(k, ks.cpu()), quantize_ref(v, vs.cpu())]
        cur = dict(zip(slots, starts))
        sl = torch.tensor(slots, dtype=torch.int32, device=DEV)
        for step in range(4):
            for s in slots:
                lens[s] = cur[s] + 1                                 # the length INCLUDES the new row: its page gets mapped
            vattention.step_async(lens)
            q, kn, vn = torch.randn(len(slots), 1, Hq, D).half(), torch.randn(len(slots), 1, Hkv, D).half(), torch.randn(len(slots), 1, Hkv, D).half()
            cl = torch.tensor([cur[s] for s in slots], dtype=torch.int32)
            mx = int(cl.max()) + 1
            out, _ = _f8(q.to(DEV), Kt[:, :mx], Vt[:, :mx], ks, vs, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=sl)
            torch.cuda.synchronize()
            for i, s in enumerate(slots):
                k8 = torch.cat([host[s][0], quantize_ref(kn[i], ks.cpu())]).unsqueeze(0)
                v8 = torch.cat([host[s][1], quantize_ref(vn[i], vs.cpu())]).unsqueeze(0)
                n = cur[s] + 1
                assert torch.equal(_bytes(Kt[s, :n].cpu()), _bytes(k8[0])) and torch.equal(_bytes(Vt[s, :n].cpu()), _bytes(v8[0])), (step, s)
                ref64 = fp8kv_attn_ref(q[i:i + 1], k8, v8, ks.cpu(), vs.cpu(), cache_seqlens=n)
                ref32 = fp8kv_attn_ref(q[i:i + 1], k8, v8, ks.cpu(), vs.cpu(), cache_seqlens=n, math="f32")
                _check(out[i:i + 1], ref64, ref32, torch.float16, "page manager step %d slot %d" % (step, s))
                host[s] = [k8[0], v8[0]]
                cur[s] = n
        assert vattention.state()["mapped"][slots[0]] >= 2           # the sequence did grow into a second page
    finally:
        vattention.cleanup()


def test_gate():
    """Calls outside the gate raise NotImplementedError with the library's message, which names the rule; NULL scales raise RuntimeError."""
    Hq, Hkv, D = 8, 2, 128
    k8, v8, ks, vs, idx, _, _, _ = _filled([300, 40], 2, 320, Hkv, D, torch.float16, 1)
    cl = torch.tensor([300, 40], dtype=torch.int32, device=DEV)
    q = torch.randn(2, 1, Hq, D, device=DEV).half()
    blocks, issue = [], FA._issue

    def spy(p, dev, lib, need=None, mask=None, scales=None):
        blocks.append((p, dev, lib, scales))
        return issue(p, dev, lib, need, mask, scales)
    FA._issue = spy
    try:
        good = flash_attn_fp8kv_with_kvcache(q, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idx.to(DEV))
    finally:
        FA._issue = issue
    p, dev, lib, scales = blocks[0]

    def refused(word, **fields):
        old = {n: getattr(p, n) for n in fields}
        for n, v in fields.items():
            setattr(p, n, v)
        try:
            with pytest.raises(NotImplementedError, match=word):
                issue(p, dev, lib, None, None, scales)
            with pytest.raises(RuntimeError, match=word):
                K.describe_fp8kv(p)
        finally:
            for n, v in old.items():
                setattr(p, n, v)
    some = cl.data_ptr()                                   # a device address; the library refuses before anything reads it
    refused("sliding window", window_left_plus1=65)
    refused("rotary", rotary_cos_sin=some, rotary_dim=D, rotary_row_stride=D)
    refused("split_items", split_items=some, split_seq=some, num_split_items=2)
    refused("q_lens", q_lens=some, q_start=some, seqlen_q=300)
    refused("pf_items", pf_items=some, num_pf_items=2, seqlen_q=300)
    for qq in (torch.randn(2, 9, Hq, D, device=DEV).half(), torch.randn(2, 300, Hq, D, device=DEV).half()):
        with pytest.raises(NotImplementedError, match="prefill form"):
            flash_attn_fp8kv_with_kvcache(qq, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idx.to(DEV), causal=True)
    with pytest.raises(NotImplementedError, match="prefill form"):      # an explicit split count keeps the prefill kernels for a multi-row block
        flash_attn_fp8kv_with_kvcache(torch.randn(2, 4, Hq, D, device=DEV).half(), k8, v8, ks, vs, cache_seqlens=cl, causal=True, _num_splits=2)
    for a, b in ((None, vs), (ks, None)):
        with pytest.raises(RuntimeError, match="k_scale and v_scale"):
            flash_attn_fp8kv_with_kvcache(q, k8, v8, a, b, cache_seqlens=cl)
    # the 2-byte entry points do not take an fp8 cache, and the fp8 entry no 2-byte one
    with pytest.raises(RuntimeError, match="same dtype"):
        FA.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cl)
    with pytest.raises(RuntimeError, match="same dtype"):
        FA.flash_attn_tree_with_kvcache(torch.randn(2, 4, Hq, D, device=DEV).half(), k8, v8, torch.ones(2, 4, dtype=torch.int32, device=DEV), cache_seqlens=cl)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        flash_attn_fp8kv_with_kvcache(q, k8.view(torch.uint8).half(), v8.view(torch.uint8).half(), ks, vs, cache_seqlens=cl)
    again = flash_attn_fp8kv_with_kvcache(q, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idx.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(good, again)                        # the refused calls left nothing behind
