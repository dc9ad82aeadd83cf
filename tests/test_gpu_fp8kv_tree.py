"""GPU tests of TREE-MASKED multi-token decode over an FP8 (e4m3) KV cache (include/vattn_kernels.h, vattn_fp8kv_tree_attn_with_kvcache) and of
the compaction of the accepted path in such a cache (vattn_cache_keep_rows_fp8), through the Python drop-ins
(flash_attn.flash_attn_fp8kv_tree_with_kvcache, cache_ops.keep_rows), against tests/fp8kv_tree_ref.py computed FROM THE BYTES THE GPU STORED.
Every call asserts through kernels.describe_fp8kv_tree which launch plan it took, and through the drop-in's counter which entry it went to.

Tolerances are the project's, restated the way tests/test_gpu_fp8kv.py restates them (`_check`: 2e-3 / 2e-3 for fp16, 1.6e-2 for bf16, kernel
error <= 2 x the f32 reference's own error + 1e-5 (+ 4e-3 for bf16); `_check_lse`: 2e-3 absolute).  None is new: widening e4m3 is exact and the
mask is a select, so no rounding step is added over either parent.  The no-read contract is checked by POISONING rows (the NaN byte 0x7f in K
and in V); nothing is unmapped on purpose."""
import pytest
import torch

from tests.fp8kv_ref import FP8, amax_scales
from tests.fp8kv_tree_ref import fp8kv_tree_ref
from tests.tree_ref import chain_mask
from vattention_amd import flash_attn as FA
from vattention_amd import kernels as K
from vattention_amd.cache_ops import cache_flat_fp8, keep_rows
from vattention_amd.flash_attn import flash_attn_fp8kv_tree_with_kvcache, flash_attn_fp8kv_with_kvcache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [(64, torch.float16), (64, torch.bfloat16), (128, torch.float16), (128, torch.bfloat16)]
DT_IDS = ["d64_f16", "d64_bf16", "d128_f16", "d128_bf16"]
# (8, 2): 8 / 20 / 32 columns; (32, 4): 64 columns, the widest block: four 16-column blocks in two workgroups per kv head (sibling groups);
# (8, 8): one column per token; (24, 1): 48 columns = three 16-column blocks in two such workgroups, the second half empty
SHAPES = [(8, 2, 2), (8, 2, 5), (8, 2, 8), (32, 4, 8), (8, 8, 8), (24, 1, 2)]
TREE7 = [0b1, 0b11, 0b101, 0b1011, 0b10011, 0b100101, 0b1100101]      # tools/kbench.py: the 7-node, 3-leaf tree 0-1-{3,4}, 0-2-5-6


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


def _close(a, b, dtype, what):
    """two kernel results of the same attention, within the tolerance either is held to"""
    atol, rtol = _tol(dtype)
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs()
    print("%s: max difference %.3e" % (what, err.max().item()))
    assert bool((err <= atol + rtol * b.abs()).all()), "%s: max difference %.3e" % (what, err.max().item())


def _check_lse(lse, lse64, what):
    lse = lse.double().cpu()
    dead = torch.isinf(lse64)
    assert torch.equal(torch.isinf(lse) & (lse > 0), dead & (lse64 > 0)), what + ": rows without a visible key have LSE +inf"
    assert ((lse - lse64)[~dead]).abs().max().item() < 2e-3, what


def _bytes(x8):
    return x8.view(torch.uint8)


def _ft(*a, **kw):
    """flash_attn_fp8kv_tree_with_kvcache, returning also the plan description of the very parameter block the drop-in launched (seen at its
    launch point) — and asserting that the call went to the fp8 tree entry: the drop-in's counters, mask AND scales at the launch"""
    seen, issue = [], FA._issue
    n0 = {c: FA.counters[c] for c in ("fp8kv_tree_calls", "fp8kv_decode_calls", "tree_decode_calls", "multitoken_decode_calls")}

    def spy(p, dev, lib, need=None, mask=None, scales=None, *rest):
        seen.append((p, mask, scales))
        return issue(p, dev, lib, need, mask, scales, *rest)
    FA._issue = spy
    try:
        r = flash_attn_fp8kv_tree_with_kvcache(*a, **kw)
    finally:
        FA._issue = issue
    assert FA.counters["fp8kv_tree_calls"] == n0["fp8kv_tree_calls"] + 1 and all(FA.counters[c] == n0[c] for c in n0 if c != "fp8kv_tree_calls")
    assert len(seen) == 1 and seen[0][1] is not None and seen[0][2] is not None
    d = K.describe_fp8kv_tree(seen[0][0])
    assert d["form"] == 1 and d == K.describe_tree(seen[0][0]) == K.describe(seen[0][0]), d
    return r, d


def _filled(lens, slots, rows, Hkv, D, dtype, seed, spread=(1.0, 3.0, 0.3)):
    """tests/test_gpu_fp8kv.py's: caches [slots, rows, Hkv, D] whose rows [0, lens[i]) of slot idx[i] were written ON THE GPU by cache_flat_fp8
    from N(0,1) data in `dtype` times a per-head factor (so that the per-head scales differ); every other byte is 0xA5.  Scales = 1.5 x amax /
    448 over the rows written (headroom for rows appended later).  Returns the GPU caches, the scales (GPU), the slot permutation (CPU) and
    the CPU copies of what the GPU stored."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(slots, generator=g)[:len(lens)].to(torch.int32)
    sl = idx.tolist()
    f = torch.tensor([spread[h % len(spread)] for h in range(Hkv)])
    src = [((torch.randn(n, Hkv, D, generator=g) * f.view(1, -1, 1)).to(dtype), (torch.randn(n, Hkv, D, generator=g) * f.flip(0).view(1, -1, 1)).to(dtype)) for n in lens]
    ks, vs = amax_scales(torch.cat([s[0] for s in src])) * 1.5, amax_scales(torch.cat([s[1] for s in src])) * 1.5
    k8 = torch.full((slots, rows, Hkv, D), 0xA5, dtype=torch.uint8, device=DEV).view(FP8)
    v8 = torch.full((slots, rows, Hkv, D), 0xA5, dtype=torch.uint8, device=DEV).view(FP8)
    ksg, vsg = ks.to(DEV), vs.to(DEV)
    for i, (kn, vn) in enumerate(src):
        if lens[i]:
            cache_flat_fp8(kn.to(DEV), vn.to(DEV), k8[sl[i]], v8[sl[i]], ksg, vsg)
    torch.cuda.synchronize()
    return k8, v8, ksg, vsg, idx, k8.cpu(), v8.cpu()


def _random_masks(B, sq, gen):
    """Random words, none topologically ordered on purpose; a word of 0 (dead row where base <= 0); words without the self bit; garbage in the
    bits >= sq of most words (the kernel must AND it away).  Entry 1 (base <= 0) keeps random words: bit s still names key base + s."""
    m = torch.randint(0, 1 << sq, (B, sq), generator=gen, dtype=torch.int64)
    m[0, 0] = 0                                            # entry 0 (base 0): row 0 sees nothing
    m[2, 1] &= ~2                                          # no self bit
    m[3, sq - 1] = 1                                       # the last node sees draft key 0 only, not itself
    m[4, 0] = 0                                            # a word of 0 behind a committed context: sees exactly that
    m[1:] |= torch.randint(0, 1 << 20, (B - 1, sq), generator=gen, dtype=torch.int64) << 8
    m[5] |= 0x80000000                                     # (the sign bit of the int32 word too)
    m = torch.where(m >= 1 << 31, m - (1 << 32), m)
    return m.to(torch.int32)


def _lengths(sq):
    """visible keys per entry AFTER the append: Lk = sq (base 0); Lk < sq (base < 0; with k / v: cache_seqlens 0, Lk = sq again); the draft rows
    entirely in one tile (base 40); straddling a 32-key boundary (base = 93 = 29 mod 32: for sq > 3; base = 95 = 31 mod 32: for every sq);
    Lk = 64 (a full last tile); ~3000 keys"""
    return [sq, sq - 1, 40 + sq, 93 + sq, 64, 3007, 95 + sq]


def _plan_is(d, Hq, Hkv, sq, splits):
    """the path the call was meant to take: sixteen-column blocks, stream decomposition vs grid heuristics, a merge launch"""
    cols = sq * (Hq // Hkv)
    nb = 2 if cols > 16 else 1
    groups = ((cols + 15) // 16 + nb - 1) // nb
    assert d["tiling"] == nb, d
    stream = groups == 1 and (splits < 0 or nb == 1)      # (two-block workgroups keep the grid heuristics unless a grid is forced)
    assert d["path"] == (2 if stream else 0), d
    assert d["merge_launch"] == 1 and (stream or d["nsplit"] > 1), d      # ~3000 keys in a batch of 7: every plan cuts the sequences
    return stream


@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("Hq,Hkv,sq", SHAPES, ids=["%d_%d_sq%d" % s for s in SHAPES])
def test_parity_on_random_masks(Hq, Hkv, sq, D, dtype):
    """One ragged batch (per-entry lengths of _lengths) per case, four calls: k / v appended by the call or the draft rows pre-appended by
    cache_flat_fp8, with cache_batch_idx over a strided [:, :rows] view or identity slots, the default plan or a forced stream grid.  Output
    and LSE against the reference on the bytes the GPU stored; the caches after an appending call are the reference's, every byte."""
    gen = torch.Generator().manual_seed(sq * 1000 + Hq * 10 + Hkv + D)
    vis = _lengths(sq)
    B, slots, rows = len(vis), len(vis) + 2, 3010
    mask = _random_masks(B, sq, gen)
    q = (torch.randn(B, sq, Hq, D, generator=gen)).to(dtype)
    kn, vn = torch.randn(B, sq, Hkv, D, generator=gen).to(dtype), (torch.randn(B, sq, Hkv, D, generator=gen) * 2).to(dtype)
    kn[3, 0, 0, 3] = 1e4                                   # saturates the quantiser
    paths = set()
    for append in (True, False):
        # with k / v: Lk = cache_seqlens + sq (the Lk < sq entry becomes cache_seqlens = 0); without: Lk = sq - 1 gives a negative base
        lens = [max(n - sq, 0) for n in vis] if append else vis
        cl = torch.tensor(lens, dtype=torch.int32)
        k8, v8, ks, vs, idx, k8c, v8c = _filled(lens, slots, rows + 3, Hkv, D, dtype, 7 * sq + Hq + D + append)
        new_cpu = dict(k=kn, v=vn) if append else {}
        new_gpu = dict(k=kn.to(DEV), v=vn.to(DEV)) if append else {}
        ka, va = k8c.clone(), v8c.clone()
        ref64, lse64 = fp8kv_tree_ref(q, ka, va, ks.cpu(), vs.cpu(), mask, cache_seqlens=cl, cache_batch_idx=idx, return_lse=True, **new_cpu)      # (appends into ka / va)
        ref32 = fp8kv_tree_ref(q, k8c.clone(), v8c.clone(), ks.cpu(), vs.cpu(), mask, cache_seqlens=cl, cache_batch_idx=idx, math="f32", **new_cpu)
        for with_idx, splits in ((True, 0), (False, -5)) if append else ((False, 0), (True, -5)):
            what = "%d/%d sq=%d d=%d %s append=%s idx=%s splits=%d" % (Hq, Hkv, sq, D, dtype, append, with_idx, splits)
            if with_idx:
                kg, vg, sel = k8.clone(), v8.clone(), dict(cache_batch_idx=idx.to(DEV))
                kview, vview = kg[:, :rows], vg[:, :rows]  # a strided view: the batch stride is not rows * row stride
            else:                                          # the entries' slots gathered into slots 0 .. B-1 of a cache of their own
                kg, vg, sel = _bytes(k8)[idx.long().to(DEV)].contiguous().view(FP8), _bytes(v8)[idx.long().to(DEV)].contiguous().view(FP8), {}
                kview, vview = kg, vg
            (out, lse), d = _ft(q.to(DEV), kview, vview, ks, vs, mask.to(DEV), cache_seqlens=cl.to(DEV), return_softmax_lse=True, _num_splits=splits,
                                **sel, **new_gpu)
            torch.cuda.synchronize()
            paths.add(_plan_is(d, Hq, Hkv, sq, splits))
            _check(out, ref64, ref32, dtype, what)
            _check_lse(lse, lse64, what + " lse")
            wk, wv = (_bytes(ka), _bytes(va)) if with_idx else (_bytes(ka)[idx.long()], _bytes(va)[idx.long()])
            assert torch.equal(_bytes(kg.cpu()), wk) and torch.equal(_bytes(vg.cpu()), wv), what + ": the caches after the call are the reference's, every byte"
            assert out[0, 0].float().abs().max().item() == 0.0 and bool(torch.isinf(lse[0, :, 0]).all()), what + ": base 0 and a word of 0"
    cols = sq * (Hq // Hkv)      # one block: the stream decomposition always; two blocks in one group: it only when forced; sibling groups: never
    assert paths == ({True} if cols <= 16 else {True, False} if cols <= 32 else {False}), paths


@pytest.mark.parametrize("D,dtype", DT, ids=DT_IDS)
def test_single_sequence(D, dtype):
    """B = 1 has nothing to balance: the grid heuristics with one 16-column block per workgroup (the only way to those builds of decode_kernel)
    and STRIPED pieces — a long sequence whose draft rows straddle a tile boundary (split and merged), and one of a single tile (unsplit)."""
    Hq, Hkv, sq = 8, 2, 3
    gen = torch.Generator().manual_seed(D + sq)
    mask = torch.tensor([[0b100, 0b011, 0b101]], dtype=torch.int32)      # node 0 sees node 2 only, node 1 the chain, node 2 skips node 1
    q = torch.randn(1, sq, Hq, D, generator=gen).to(dtype)
    kn, vn = torch.randn(1, sq, Hkv, D, generator=gen).to(dtype), torch.randn(1, sq, Hkv, D, generator=gen).to(dtype)
    for ctx, nsplit_gt1 in ((3006, True), (20, False)):      # (3006 = 30 mod 32: the three draft rows are keys 30, 31 | 32 of two tiles)
        k8, v8, ks, vs, idx, k8c, v8c = _filled([ctx], 2, ctx + sq, Hkv, D, dtype, ctx + D)
        cl = torch.tensor([ctx], dtype=torch.int32)
        ref64, lse64 = fp8kv_tree_ref(q, k8c.clone(), v8c.clone(), ks.cpu(), vs.cpu(), mask, kn, vn, cache_seqlens=cl, cache_batch_idx=idx, return_lse=True)
        ref32 = fp8kv_tree_ref(q, k8c.clone(), v8c.clone(), ks.cpu(), vs.cpu(), mask, kn, vn, cache_seqlens=cl, cache_batch_idx=idx, math="f32")
        (out, lse), d = _ft(q.to(DEV), k8, v8, ks, vs, mask.to(DEV), kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), return_softmax_lse=True)
        torch.cuda.synchronize()
        assert d["path"] == 0 and d["tiling"] == 1 and (d["nsplit"] > 1) == nsplit_gt1 and d["merge_launch"] == int(nsplit_gt1), d
        _check(out, ref64, ref32, dtype, "B=1 ctx=%d d=%d %s" % (ctx, D, dtype))
        _check_lse(lse, lse64, "B=1 ctx=%d lse" % ctx)


@pytest.mark.parametrize("D,dtype", [(128, torch.float16), (64, torch.bfloat16)], ids=["d128_f16", "d64_bf16"])
def test_three_leaf_tree_and_bool_masks(D, dtype):
    """kbench's 7-node, 3-leaf tree as words, and the same tree as a bool [sq, sq] tensor (packed on the device, broadcast over the batch)"""
    Hq, Hkv, sq = 8, 2, 7
    lens = [sq, 29 + sq, 1000, 3]
    B = len(lens)
    k8, v8, ks, vs, idx, k8c, v8c = _filled(lens, 5, 1003, Hkv, D, dtype, 70 + D)
    torch.manual_seed(D)
    q = torch.randn(B, sq, Hq, D).to(dtype)
    cl = torch.tensor(lens, dtype=torch.int32)
    words = torch.tensor(TREE7, dtype=torch.int32).expand(B, sq).contiguous()
    ref64, lse64 = fp8kv_tree_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), words, cache_seqlens=cl, cache_batch_idx=idx, return_lse=True)
    ref32 = fp8kv_tree_ref(q, k8c, v8c, ks.cpu(), vs.cpu(), words, cache_seqlens=cl, cache_batch_idx=idx, math="f32")
    (out, lse), d = _ft(q.to(DEV), k8, v8, ks, vs, words.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), return_softmax_lse=True)
    torch.cuda.synchronize()
    assert d["tiling"] == 2, d
    _check(out, ref64, ref32, dtype, "3-leaf tree")
    _check_lse(lse, lse64, "3-leaf tree lse")
    vis = ((words[0].view(sq, 1) >> torch.arange(sq)) & 1).bool()
    ob, _ = _ft(q.to(DEV), k8, v8, ks, vs, vis.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(ob, out), "the bool form packs to the same words: the same bits"


@pytest.mark.parametrize("Hq,Hkv,sq,D,dtype", [(8, 2, 5, 128, torch.float16), (32, 4, 8, 64, torch.bfloat16), (8, 8, 2, 64, torch.float16)],
                         ids=["g4_sq5_d128_f16", "g8_sq8_d64_bf16", "mha_sq2_d64_f16"])
def test_chain_and_all_ones_masks_are_the_fp8_multitoken_calls(Hq, Hkv, sq, D, dtype):
    """A chain mask against flash_attn_fp8kv_with_kvcache(causal=True), all ones against causal=False, on the device: the calls differ only in
    the order of the fp32 sums — the tolerance either is held to."""
    lens = [sq, sq - 1, 40 + sq, 93 + sq, 3007]
    B = len(lens)
    k8, v8, ks, vs, idx, _, _ = _filled(lens, B + 1, 3008, Hkv, D, dtype, 11 + sq)
    torch.manual_seed(sq + D)
    q = torch.randn(B, sq, Hq, D, device=DEV).to(dtype)
    cl, idg = torch.tensor(lens, dtype=torch.int32, device=DEV), idx.to(DEV)
    for causal, mask in ((True, chain_mask(sq).expand(B, sq).contiguous()), (False, torch.full((B, sq), -1, dtype=torch.int32))):
        for splits in (0, -5):
            (out, lse), _ = _ft(q, k8, v8, ks, vs, mask.to(DEV), cache_seqlens=cl, cache_batch_idx=idg, return_softmax_lse=True, _num_splits=splits)
            ref, rl = flash_attn_fp8kv_with_kvcache(q, k8, v8, ks, vs, cache_seqlens=cl, cache_batch_idx=idg, causal=causal, return_softmax_lse=True, _num_splits=splits)
            torch.cuda.synchronize()
            _close(out, ref, dtype, "sq=%d causal=%s splits=%d" % (sq, causal, splits))
            _check_lse(lse, rl.double().cpu(), "sq=%d causal=%s splits=%d lse" % (sq, causal, splits))


@pytest.mark.parametrize("Hq,Hkv,sq", [(8, 2, 4), (32, 4, 8)], ids=["g4_sq4", "g8_sq8"])
def test_no_read_contract(Hq, Hkv, sq):
    """Rows at and beyond Lk hold the NaN byte 0x7f in K and in V: the outputs stay finite, within tolerance of the reference and equal to the
    unpoisoned run's.  A draft row that NO column may see (its bit is set in no word) holds the largest finite byte (0x7e = 448) in K and V: it
    is loaded and masked, as the header says — a leak would be off by orders of magnitude."""
    D, dtype = 128, torch.float16
    lens = [3000, 93 + sq, sq, 40 + sq, 1777, 64]
    B, rows = len(lens), 3100
    k8, v8, ks, vs, idx, _, _ = _filled(lens, B, rows, Hkv, D, dtype, 4 + sq)
    hidden = 1                                             # draft key 1: no word has bit 1
    gen = torch.Generator().manual_seed(sq)
    mask = (torch.randint(0, 1 << sq, (B, sq), generator=gen, dtype=torch.int64) & ~(1 << hidden) | 1).to(torch.int32)
    for b in range(B):
        _bytes(k8)[int(idx[b]), lens[b] - sq + hidden] = 0x7E
        _bytes(v8)[int(idx[b]), lens[b] - sq + hidden] = 0x7E
    kp, vp = k8.clone(), v8.clone()
    for b in range(B):
        _bytes(kp)[int(idx[b]), lens[b]:] = 0x7F
        _bytes(vp)[int(idx[b]), lens[b]:] = 0x7F
    assert bool(torch.isnan(kp.float()).any()) and float(k8.float().max()) == 448.0
    torch.manual_seed(8)
    q = torch.randn(B, sq, Hq, D).to(dtype)
    cl = torch.tensor(lens, dtype=torch.int32)
    ref64 = fp8kv_tree_ref(q, k8.cpu(), v8.cpu(), ks.cpu(), vs.cpu(), mask, cache_seqlens=cl, cache_batch_idx=idx)
    ref32 = fp8kv_tree_ref(q, k8.cpu(), v8.cpu(), ks.cpu(), vs.cpu(), mask, cache_seqlens=cl, cache_batch_idx=idx, math="f32")
    for splits in (0, -5, -64):
        a, _ = _ft(q.to(DEV), k8, v8, ks, vs, mask.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), _num_splits=splits)
        p, _ = _ft(q.to(DEV), kp, vp, ks, vs, mask.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), _num_splits=splits)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "splits=%d" % splits
        _check(p, ref64, ref32, dtype, "poisoned, splits=%d" % splits)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n_draft", [8, 3, 1])
def test_keep_rows_on_fp8_caches(n_draft, D):
    """Random ascending keep_idx, keep_cnt 0 .. n_draft, cache_batch_idx, a strided cache view: the WHOLE allocation — the 0xA5 fill between and
    after the rows included — equals the torch-indexed expectation byte for byte."""
    torch.manual_seed(n_draft * 10 + D)
    B, slots, Hkv, rows = 6, 8, 3, 120
    # (row and head offsets keep the view's base 16-byte aligned: every stride is a multiple of 16 bytes)
    fullk = torch.full((slots, rows + 9, Hkv + 2, D), 0xA5, dtype=torch.uint8)
    fullv = torch.full((slots, rows + 9, Hkv + 2, D), 0xA5, dtype=torch.uint8)
    view = lambda t: t[:, 5:5 + rows, 1:1 + Hkv]                 # strided: row offset, head offset, wider row and batch strides
    view(fullk)[:, :rows - 7] = torch.randint(0, 256, (slots, rows - 7, Hkv, D), dtype=torch.uint8)      # (the last 7 rows of the view keep the fill)
    view(fullv)[:, :rows - 7] = torch.randint(0, 256, (slots, rows - 7, Hkv, D), dtype=torch.uint8)
    idx = torch.randperm(slots)[:B].to(torch.int32)
    row0 = torch.tensor([0, 17, rows - 7 - n_draft, 31, 64, 3], dtype=torch.int32)
    cnt = torch.tensor([0, 1, n_draft, n_draft // 2, max(n_draft - 1, 0), n_draft], dtype=torch.int32)
    keep = torch.zeros(B, n_draft, dtype=torch.int32)
    for b in range(B):
        keep[b, :cnt[b]] = torch.randperm(n_draft)[:cnt[b]].sort().values.to(torch.int32)
    keep[5] = torch.arange(n_draft, dtype=torch.int32)            # the identity: nothing moves
    keep[4, :cnt[4]] = torch.arange(1, n_draft, dtype=torch.int32)  # every kept row moves down by one
    for with_idx in (True, False):
        wantk, wantv = fullk.clone(), fullv.clone()
        for b in range(B):
            s = int(idx[b]) if with_idx else b
            for want, full in ((wantk, fullk), (wantv, fullv)):
                for i in range(int(cnt[b])):
                    view(want)[s, row0[b] + i] = view(full)[s, row0[b] + keep[b, i]]
        gk, gv = fullk.to(DEV), fullv.to(DEV)
        keep_rows(view(gk).view(FP8), view(gv).view(FP8), row0.to(DEV), keep.to(DEV), cnt.to(DEV), cache_batch_idx=idx.to(DEV) if with_idx else None)
        torch.cuda.synchronize()
        assert torch.equal(gk.cpu(), wantk) and torch.equal(gv.cpu(), wantv), with_idx
        assert not torch.equal(wantk, fullk) or n_draft == 1           # (something did move)


def test_verify_compact_decode_end_to_end():
    """Tree verify with append -> keep_rows of one accepted path per entry -> a one-token flash_attn_fp8kv_with_kvcache step, against the same
    step over a cache into which ONLY the accepted path was appended with cache_flat_fp8: the cache bytes of the visible rows are equal and
    the outputs are torch.equal."""
    torch.manual_seed(12)
    sq, Hq, Hkv, D, dtype = 7, 8, 2, 128, torch.float16
    ctx = [500, 61, 0, 2047]
    accepted = [[0, 2, 5, 6], [0, 1, 3], [0], [0, 1, 4]]
    B, rows, slots = len(ctx), 2047 + sq + 4, 6
    k8, v8, ks, vs, idx, _, _ = _filled(ctx, slots, rows, Hkv, D, dtype, 33)
    q, kn, vn = torch.randn(B, sq, Hq, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype)
    q1, k1, v1 = torch.randn(B, 1, Hq, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype)
    cl = torch.tensor(ctx, dtype=torch.int32)
    cnt = torch.tensor([len(a) for a in accepted], dtype=torch.int32)
    keep = torch.zeros(B, sq, dtype=torch.int32)
    for b, a in enumerate(accepted):
        keep[b, :len(a)] = torch.tensor(a, dtype=torch.int32)
    mask = torch.tensor(TREE7, dtype=torch.int32).expand(B, sq).contiguous()
    idg = idx.to(DEV)
    # the same history with only the accepted rows appended
    k2, v2 = k8.clone(), v8.clone()
    for b, a in enumerate(accepted):
        sel = torch.tensor(a)
        cache_flat_fp8(kn[b, sel].to(DEV), vn[b, sel].to(DEV), k2[int(idx[b]), ctx[b]:], v2[int(idx[b]), ctx[b]:], ks, vs)
    kg, vg = k8.clone(), v8.clone()
    ref64 = fp8kv_tree_ref(q, k8.cpu(), v8.cpu(), ks.cpu(), vs.cpu(), mask, kn, vn, cache_seqlens=cl, cache_batch_idx=idx)
    ref32 = fp8kv_tree_ref(q, k8.cpu(), v8.cpu(), ks.cpu(), vs.cpu(), mask, kn, vn, cache_seqlens=cl, cache_batch_idx=idx, math="f32")
    out, _ = _ft(q.to(DEV), kg, vg, ks, vs, mask.to(DEV), kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idg)
    _check(out, ref64, ref32, dtype, "verify")
    keep_rows(kg, vg, cl.to(DEV), keep.to(DEV), cnt.to(DEV), cache_batch_idx=idg)
    step = lambda kc, vc: flash_attn_fp8kv_with_kvcache(q1.to(DEV), kc, vc, ks, vs, k1.to(DEV), v1.to(DEV), cache_seqlens=(cl + cnt).to(DEV), cache_batch_idx=idg)
    dec, want = step(kg, vg), step(k2, v2)
    torch.cuda.synchronize()
    for b in range(B):
        n, s = ctx[b] + len(accepted[b]) + 1, int(idx[b])
        assert torch.equal(_bytes(kg[s, :n]), _bytes(k2[s, :n])) and torch.equal(_bytes(vg[s, :n]), _bytes(v2[s, :n])), b
    assert torch.equal(dec, want)


def test_gate():
    """The refusals of the header's GATE raise NotImplementedError / RuntimeError with the rule's name; a repeat of a good call afterwards is
    bit-identical; the 2-byte tree entry still refuses an fp8 cache."""
    Hq, Hkv, D, sq = 8, 2, 128, 4
    k8, v8, ks, vs, idx, _, _ = _filled([300, 40], 2, 320, Hkv, D, torch.float16, 1)
    cl = torch.tensor([300, 40], dtype=torch.int32, device=DEV)
    torch.manual_seed(4)
    q = torch.randn(2, sq, Hq, D, device=DEV).half()
    mask = torch.tensor([[1, 3, 5, 11]] * 2, dtype=torch.int32, device=DEV)
    blocks, issue = [], FA._issue

    def spy(p, dev, lib, need=None, mask=None, scales=None, *rest):
        blocks.append((p, dev, lib, mask, scales))
        return issue(p, dev, lib, need, mask, scales, *rest)
    FA._issue = spy
    try:
        good = flash_attn_fp8kv_tree_with_kvcache(q, k8, v8, ks, vs, mask, cache_seqlens=cl, cache_batch_idx=idx.to(DEV))
    finally:
        FA._issue = issue
    p, dev, lib, m, scales = blocks[0]

    def refused(exc, word, **fields):
        old = {n: getattr(p, n) for n in fields}
        for n, v in fields.items():
            setattr(p, n, v)
        try:
            with pytest.raises(exc, match=word):
                issue(p, dev, lib, None, m, scales)
            with pytest.raises(RuntimeError, match=word):
                K.describe_fp8kv_tree(p)
        finally:
            for n, v in old.items():
                setattr(p, n, v)
    some = cl.data_ptr()                                   # a device address; the library refuses before anything reads it
    refused(RuntimeError, "sliding window", window_left_plus1=65)      # INVALID beside a mask, as in the 2-byte tree call
    refused(RuntimeError, "sliding window", window_left_plus1=65, is_causal=1)
    refused(NotImplementedError, "rotary", rotary_cos_sin=some, rotary_dim=D, rotary_row_stride=D)
    refused(NotImplementedError, "split_items", split_items=some, split_seq=some, num_split_items=2)
    refused(NotImplementedError, "q_lens", q_lens=some, q_start=some)
    refused(NotImplementedError, "num_splits", num_splits=2)
    refused(NotImplementedError, "tiling", variant=4 << 1)
    refused(NotImplementedError, "seqlen_q", seqlen_q=1)
    refused(NotImplementedError, "seqlen_q", seqlen_q=9)
    with pytest.raises(NotImplementedError, match="seqlen_q"):
        flash_attn_fp8kv_tree_with_kvcache(torch.randn(2, 9, Hq, D, device=DEV).half(), k8, v8, ks, vs, torch.ones(2, 9, dtype=torch.int32, device=DEV), cache_seqlens=cl)
    with pytest.raises(NotImplementedError, match="<= 64"):      # 9 x 8 = 72 (token, head) columns
        flash_attn_fp8kv_tree_with_kvcache(torch.randn(2, 8, 18, D, device=DEV).half(), k8, v8, ks, vs, torch.ones(2, 8, dtype=torch.int32, device=DEV), cache_seqlens=cl)
    with pytest.raises(NotImplementedError, match="num_splits"):
        flash_attn_fp8kv_tree_with_kvcache(q, k8, v8, ks, vs, mask, cache_seqlens=cl, _num_splits=2)
    for a, b in ((None, vs), (ks, None)):
        with pytest.raises(RuntimeError, match="k_scale and v_scale"):
            flash_attn_fp8kv_tree_with_kvcache(q, k8, v8, a, b, mask, cache_seqlens=cl)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):    # the fp8 tree entry takes no 2-byte cache
        flash_attn_fp8kv_tree_with_kvcache(q, k8.view(torch.uint8).half(), v8.view(torch.uint8).half(), ks, vs, mask, cache_seqlens=cl)
    with pytest.raises(RuntimeError, match="same dtype"):       # ... and the 2-byte tree entry still no fp8 cache
        FA.flash_attn_tree_with_kvcache(q, k8, v8, mask, cache_seqlens=cl)
    again = flash_attn_fp8kv_tree_with_kvcache(q, k8, v8, ks, vs, mask, cache_seqlens=cl, cache_batch_idx=idx.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(good, again)                        # the refused calls left nothing behind
