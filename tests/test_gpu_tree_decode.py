"""GPU parity of the TREE-MASKED multi-token decode form (include/vattn_kernels.h, vattn_tree_attn_with_kvcache: the 2..8 query rows of an
entry are the nodes of a draft tree and see each other through a bit mask) and of the row compaction that follows it
(vattn_cache_keep_rows), through the Python drop-ins, against tests/tree_ref.py (itself checked against the oracle by
tests/test_tree_ref.py).  Every tree call asserts through the plan description that it took form 1, and through the drop-in's counter.

Tolerances are the project's, restated from tests/test_gpu_multitoken_decode.py (`_check`, `_close`, `_check_lse`); none is new.  The no-read
contract is checked by POISONING rows (K NaN, V Inf), as tests/test_gpu_window.py does; nothing is unmapped on purpose."""
import ctypes as C

import pytest
import torch

from oracle.attn import flash_attn_with_kvcache_ref
from tests.tree_ref import chain_mask, pack_mask, tree_attn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = [(8, 2), (32, 4), (8, 8), (8, 1)]


def _tol(dtype):
    return (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)


def _check(out_gpu, ref64, ref32, dtype, what):
    atol, rtol = _tol(dtype)
    got = out_gpu.double().cpu()
    err = (got - ref64).abs()
    bound = atol + rtol * ref64.abs()
    assert bool((err <= bound).all()), "%s: max err %.3e (allowed %.3e)" % (what, err.max().item(), bound.max().item())
    e_ref = (ref32.double() - ref64).abs().max().item()
    assert err.max().item() <= 2 * e_ref + 1e-5 + (0 if dtype == torch.float16 else 4e-3), \
        "%s: kernel err %.3e vs reference-numerics err %.3e" % (what, err.max().item(), e_ref)


def _close(a, b, dtype, what):
    """two kernel results of the same call, within the tolerance either is held to"""
    atol, rtol = _tol(dtype)
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), "%s: max difference %.3e" % (what, err.max().item())


def _check_lse(lse, lse64, what):
    lse = lse.double().cpu()
    dead = torch.isinf(lse64)
    assert torch.equal(torch.isinf(lse) & (lse > 0), dead & (lse64 > 0)), what + ": rows without a visible key have LSE +inf"
    assert ((lse - lse64)[~dead]).abs().max().item() < 2e-3, what


def _tree(*a, **kw):
    """flash_attn_tree_with_kvcache, asserting that the call took form 1 on the tree entry: the plan description of the very parameter block
    the drop-in launches (seen at its launch point) and the drop-in's counter"""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    seen, launch = [], FA._launch_tree
    n0, m0 = FA.counters["tree_decode_calls"], FA.counters["multitoken_decode_calls"]

    def spy(p, mask, dev, keep=()):
        seen.append(p)
        return launch(p, mask, dev, keep)
    FA._launch_tree = spy
    try:
        r = FA.flash_attn_tree_with_kvcache(*a, **kw)
    finally:
        FA._launch_tree = launch
    assert FA.counters["tree_decode_calls"] == n0 + 1 and FA.counters["multitoken_decode_calls"] == m0
    assert len(seen) == 1
    d = K.describe_tree(seen[0])
    assert d["form"] == 1 and seen[0].seqlen_q > 1 and d == K.describe(seen[0]), d
    return r, d


def _mt(*a, **kw):
    from vattention_amd import flash_attn as FA
    n0 = FA.counters["multitoken_decode_calls"]
    r = FA.flash_attn_with_kvcache(*a, **kw)
    assert FA.counters["multitoken_decode_calls"] == n0 + 1
    return r


def _random_masks(B, sq, gen):
    """random bits with garbage above bit seqlen_q; rows without a self bit; all-zero rows"""
    m = torch.randint(0, 1 << sq, (B, sq), generator=gen, dtype=torch.int64)
    m[0, 0] = 0                                            # an all-zero row (sees the committed context only; none when base <= 0)
    m[1] = 0                                               # entry 1 (Lk < sq resp. Lk == sq): every row
    m[2, 1] &= ~2                                          # no self bit
    m[3] = (1 << sq) - 1
    m[4:] |= torch.randint(0, 1 << 20, (B - 4, sq), generator=gen, dtype=torch.int64) << 8      # bits the kernel must AND away
    return m.to(torch.int32)


def _lengths(sq):
    """tests/test_gpu_multitoken_decode.py: Lk % 32 in {0, 1, sq - 1, sq, 31}, a draft range that straddles two tiles, Lk == sq, Lk < sq"""
    return [sq, sq - 1, 64, 65, 96 + sq - 1, 128 + sq, 32 * 9 + 31, 32 * 7 + 1, 1500 + sq, 3007]


@pytest.mark.parametrize("D,dtype", [(128, torch.float16), (128, torch.bfloat16), (64, torch.float16), (64, torch.bfloat16)], ids=["d128_f16", "d128_bf16", "d64_f16", "d64_bf16"])
@pytest.mark.parametrize("Hq,Hkv", HEADS, ids=["%d_%d" % h for h in HEADS])
@pytest.mark.parametrize("sq", [2, 3, 5, 8])
def test_tree_parity_on_random_masks(sq, Hq, Hkv, D, dtype):
    """Ragged batch with cache_batch_idx, with and without k / v (the cache after the call equals the reference's bit for bit), LSE, a strided
    q view and a caller-provided out."""
    gen = torch.Generator().manual_seed(sq * 1000 + Hq * 10 + Hkv + D)
    torch.manual_seed(sq * 1000 + Hq * 10 + Hkv + D)
    vis = _lengths(sq)
    B, slots, rows = len(vis), len(vis) + 3, 3100
    kc, vc = torch.randn(slots, rows, Hkv, D).to(dtype), torch.randn(slots, rows, Hkv, D).to(dtype)
    idx = torch.randperm(slots)[:B].to(torch.int32)
    qw = torch.randn(B, sq, Hq + 2, D).to(dtype)
    q = qw[:, :, 1:Hq + 1]                                        # a strided view
    kn, vn = torch.randn(B, sq, Hkv, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype)
    qg, idg = qw.to(DEV)[:, :, 1:Hq + 1], idx.to(DEV)
    for append in (True, False):
        # with k / v: Lk = cache_seqlens + sq (the Lk < sq entry becomes cache_seqlens == 0); without: Lk = sq - 1 gives a negative base
        cl = torch.tensor([max(n - sq, 0) for n in vis] if append else vis, dtype=torch.int32)
        mask = _random_masks(B, sq, gen)
        new_cpu = dict(k=kn, v=vn) if append else {}
        new_gpu = dict(k=kn.to(DEV), v=vn.to(DEV)) if append else {}
        what = "sq=%d %d/%d d=%d append=%s" % (sq, Hq, Hkv, D, append)
        kr, vr = kc.clone(), vc.clone()
        ref64, lse64 = tree_attn_ref(q, kr, vr, mask, cache_seqlens=cl, cache_batch_idx=idx, return_lse=True, **new_cpu)
        ref32 = tree_attn_ref(q, kc.clone(), vc.clone(), mask, cache_seqlens=cl, cache_batch_idx=idx, math="f32", **new_cpu)
        kg, vg = kc.to(DEV), vc.to(DEV)
        out = torch.full((B, sq, Hq + 1, D), 7.0, dtype=dtype, device=DEV)[:, :, :Hq]      # caller-provided, strided
        (_, d) = _tree(qg, kg, vg, mask.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idg, out=out, **new_gpu)
        torch.cuda.synchronize()
        assert d["tiling"] == (2 if sq * (Hq // Hkv) > 16 else 1), d
        _check(out, ref64, ref32, dtype, what)
        assert torch.equal(kg.cpu(), kr) and torch.equal(vg.cpu(), vr), what + ": the cache after the call is the reference's, every row"
        (o2, lse), _ = _tree(qg, kg, vg, mask.to(DEV), cache_seqlens=(cl + (sq if append else 0)).to(DEV), cache_batch_idx=idg, return_softmax_lse=True)
        torch.cuda.synchronize()
        _check(o2, ref64, ref32, dtype, what + " (+lse)")
        _check_lse(lse, lse64, what + " lse")
        assert out[0, 0].float().abs().max().item() == 0.0                                              # entry 0: base == 0, an all-zero row
        assert out[1].float().abs().max().item() == 0.0 and bool(torch.isinf(lse[1]).all())              # entry 1: base <= 0 and no bit set


def test_bool_masks_are_packed_and_broadcast():
    torch.manual_seed(2)
    B, sq, Hq, Hkv, D = 3, 4, 8, 2, 128
    kg, vg = torch.randn(B, 300, Hkv, D, device=DEV).half(), torch.randn(B, 300, Hkv, D, device=DEV).half()
    q = torch.randn(B, sq, Hq, D, device=DEV).half()
    cl = torch.tensor([300, 37, 64], dtype=torch.int32, device=DEV)
    vis = torch.tensor([[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 1, 1]], dtype=torch.bool)
    words = pack_mask(vis)
    assert words.tolist() == [1, 3, 5, 13]
    a, _ = _tree(q, kg, vg, words.expand(B, sq).contiguous().to(DEV), cache_seqlens=cl)
    b, _ = _tree(q, kg, vg, vis.to(DEV), cache_seqlens=cl)
    c, _ = _tree(q, kg, vg, vis.expand(B, sq, sq).to(DEV), cache_seqlens=cl)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    from vattention_amd.flash_attn import flash_attn_tree_with_kvcache
    with pytest.raises(NotImplementedError, match="seqlen_q"):
        flash_attn_tree_with_kvcache(q[:, :1], kg, vg, words[:1].expand(B, 1).contiguous().to(DEV), cache_seqlens=cl)
    with pytest.raises(NotImplementedError, match="<= 64"):
        flash_attn_tree_with_kvcache(torch.randn(B, 8, 18, D, device=DEV).half(), kg, vg, torch.zeros(B, 8, dtype=torch.int32, device=DEV), cache_seqlens=cl)


def _ragged16():
    return [100, 20000, 257, 4096, 31, 9999, 12345, 1024, 16000, 700, 19999, 3, 5000, 2048, 8191, 64]


@pytest.mark.parametrize("case", [
    dict(name="one_20k_sequence", lens=[20000], Hq=8, Hkv=2, sq=4, D=128, dtype=torch.float16, splits=(0, -3)),
    dict(name="ragged16", lens=_ragged16(), Hq=8, Hkv=2, sq=4, D=128, dtype=torch.float16, splits=(0, -37)),
    dict(name="R32", lens=_ragged16()[:6], Hq=32, Hkv=4, sq=4, D=128, dtype=torch.float16, splits=(0,)),
    dict(name="R64_two_groups", lens=[20000, 300, 5001], Hq=16, Hkv=2, sq=8, D=128, dtype=torch.bfloat16, splits=(0,)),
    dict(name="R64_two_groups_d64", lens=[9000], Hq=8, Hkv=1, sq=8, D=64, dtype=torch.float16, splits=(0,)),
], ids=lambda c: c["name"])
def test_tree_merges(case):
    """The five paths a mask word must reach intact: the uniform split of one sequence, the stream decomposition of a ragged batch (default
    and forced grids), two-block workgroups (R = 32), sibling head-block groups (R = 64), d = 64 with R = 64."""
    lens, Hq, Hkv, sq, D, dtype = case["lens"], case["Hq"], case["Hkv"], case["sq"], case["D"], case["dtype"]
    gen = torch.Generator().manual_seed(len(lens) + Hq + sq)
    torch.manual_seed(len(lens) + Hq + sq)
    B, rows = len(lens), max(lens) + sq
    kc, vc = torch.randn(B, rows, Hkv, D).to(dtype), torch.randn(B, rows, Hkv, D).to(dtype)
    q, kn, vn = torch.randn(B, sq, Hq, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype)
    cl = torch.tensor(lens, dtype=torch.int32)
    mask = torch.randint(0, 1 << sq, (B, sq), generator=gen, dtype=torch.int64).to(torch.int32)
    kr, vr = kc.clone(), vc.clone()
    ref64, lse64 = tree_attn_ref(q, kr, vr, mask, kn, vn, cache_seqlens=cl, return_lse=True)
    ref32 = tree_attn_ref(q, kc.clone(), vc.clone(), mask, kn, vn, cache_seqlens=cl, math="f32")
    merged = False
    for splits in case["splits"]:
        kg, vg = kc.to(DEV), vc.to(DEV)
        out, d = _tree(q.to(DEV), kg, vg, mask.to(DEV), kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), _num_splits=splits)
        torch.cuda.synchronize()
        merged |= d["merge_launch"] == 1
        _check(out, ref64, ref32, dtype, "%s splits=%d %s" % (case["name"], splits, d))
        assert torch.equal(kg.cpu(), kr) and torch.equal(vg.cpu(), vr)
        (o2, lse), _ = _tree(q.to(DEV), kg, vg, mask.to(DEV), cache_seqlens=(cl + sq).to(DEV), _num_splits=splits, return_softmax_lse=True)
        torch.cuda.synchronize()
        _check_lse(lse, lse64, "%s splits=%d lse" % (case["name"], splits))
    assert merged


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("sq,Hq,Hkv,D", [(4, 8, 2, 128), (8, 32, 4, 128), (3, 28, 4, 64)], ids=["sq4_g4", "sq8_g8", "sq3_g7_d64"])
def test_tree_equivalences_on_the_device(sq, Hq, Hkv, D, dtype):
    """chain mask = the causal multi-token call, all-ones mask = the non-causal one (within `_close`: the tree build's tail range starts one
    key earlier, a wave's tile order can differ); tree_mask = NULL through the C entry IS vattn_flash_attn_with_kvcache, bit for bit."""
    from vattention_amd import kernels as K
    torch.manual_seed(17 * sq)
    vis = [3000, sq, 65, 1024 + sq - 1, 9000, sq - 1]
    B, rows = len(vis), max(vis) + 8
    kg, vg = torch.randn(B, rows, Hkv, D, device=DEV).to(dtype), torch.randn(B, rows, Hkv, D, device=DEV).to(dtype)
    q = torch.randn(B, sq, Hq, D, device=DEV).to(dtype)
    cl = torch.tensor(vis, dtype=torch.int32, device=DEV)
    chain, _ = _tree(q, kg, vg, chain_mask(sq).expand(B, sq).contiguous().to(DEV), cache_seqlens=cl)
    ones, _ = _tree(q, kg, vg, torch.full((B, sq), -1, dtype=torch.int32, device=DEV), cache_seqlens=cl)
    po = []
    causal = _mt(q, kg, vg, cache_seqlens=cl, causal=True, _params_out=po)
    _close(chain, causal, dtype, "chain mask vs the causal multi-token call")
    _close(ones, _mt(q, kg, vg, cache_seqlens=cl, causal=False), dtype, "all-ones mask vs the non-causal multi-token call")
    p, again = po[0], torch.empty_like(causal)
    p.out = again.data_ptr()
    assert K.klib().vattn_tree_attn_with_kvcache(C.byref(p), None, K.current_stream_ptr(q.device)) == 0, K.last_error()
    torch.cuda.synchronize()
    assert torch.equal(again, causal)


# 8 nodes, two branches below the root:  0 - 1 - 2 - 3  and  0 - 4 - 5 - 6 - 7
PARENT8 = [-1, 0, 1, 2, 0, 4, 5, 6]
# 7 nodes, three leaves (3, 4, 6):  0 - 1 - {3, 4},  0 - 2 - 5 - 6
PARENT7 = [-1, 0, 0, 1, 1, 2, 5]


def _ancestors(parent, t):
    out = []
    while t >= 0:
        out.append(t)
        t = parent[t]
    return sorted(out)


def _tree_vis(parent):
    vis = torch.zeros(len(parent), len(parent), dtype=torch.bool)
    for t in range(len(parent)):
        vis[t, _ancestors(parent, t)] = True
    return vis


def test_tree_decoy_draft_keys():
    """For every query row t: the draft keys t must NOT see get K = 64 q_t / |q_t| (a score far above every honest one — finite: invisible
    draft keys are loaded and masked, not skipped) and V = 1000, visible keys have |V| <= 1: every element of row t stays within 1 +
    tolerance, one leaked key would move it by hundreds.  Draft rows straddle a tile boundary (base % 32 = 28); rows at or beyond Lk hold
    K NaN / V Inf (the no-read contract)."""
    torch.manual_seed(8)
    sq, Hq, Hkv, D = 8, 4, 2, 128
    G = Hq // Hkv
    vis = _tree_vis(PARENT8)
    bases = [28, 32 * 5 + 28, 32 * 31 + 28, 12]
    B, rows = len(bases), 32 * 31 + 28 + sq + 40
    q = torch.randn(B, sq, Hq, D, device=DEV).half()
    kc = torch.randn(B, rows, Hkv, D, device=DEV).half()
    vc = (torch.rand(B, rows, Hkv, D, device=DEV) * 2 - 1).half()
    for b, base in enumerate(bases):
        kc[b, base + sq:], vc[b, base + sq:] = float("nan"), float("inf")
    cl = torch.tensor([b_ + sq for b_ in bases], dtype=torch.int32, device=DEV)
    mask = pack_mask(vis).to(DEV)
    for t in range(sq):
        kd, vd = kc.clone(), vc.clone()
        hidden = [s for s in range(sq) if not bool(vis[t, s])]
        assert hidden
        for b, base in enumerate(bases):
            for s in hidden:
                for hk in range(Hkv):
                    qr = q[b, t, hk * G].float()
                    kd[b, base + s, hk] = (64.0 * qr / qr.norm()).half()
                vd[b, base + s] = 1000.0
        for splits in (0, -3):
            out, _ = _tree(q, kd, vd, mask.expand(B, sq).contiguous(), cache_seqlens=cl, _num_splits=splits)
            torch.cuda.synchronize()
            row = out[:, t].float()
            assert bool(torch.isfinite(out).all()), (t, splits)
            assert row.abs().max().item() <= 1.0 + 2e-3, "row %d splits %d: a hidden draft key leaked (|out| max %.1f)" % (t, splits, row.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_tree_rows_equal_the_per_path_chain_calls(dtype):
    """Each root-to-leaf path of a 7-node tree, written contiguously into a scratch cache and run through the causal multi-token call (the one
    call per path a tree draft costs without this form): its rows are the tree call's rows of the same nodes."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(5)
    sq, Hq, Hkv, D = 7, 8, 2, 128
    ctx = [1000, 29, 0, 4099]
    B, rows = len(ctx), max(ctx) + sq
    kg, vg = torch.randn(B, rows, Hkv, D, device=DEV).to(dtype), torch.randn(B, rows, Hkv, D, device=DEV).to(dtype)
    q = torch.randn(B, sq, Hq, D, device=DEV).to(dtype)
    kn, vn = torch.randn(B, sq, Hkv, D, device=DEV).to(dtype), torch.randn(B, sq, Hkv, D, device=DEV).to(dtype)
    cl = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    kt, vt = kg.clone(), vg.clone()
    out, _ = _tree(q, kt, vt, _tree_vis(PARENT7).to(DEV), kn, vn, cache_seqlens=cl)
    leaves = [t for t in range(sq) if t not in PARENT7]
    assert leaves == [3, 4, 6]
    for leaf in leaves + [0]:                                     # (+ the root alone: a 1-node path is the one-token decode)
        path = _ancestors(PARENT7, leaf)
        ks, vs = kg.clone(), vg.clone()
        if len(path) > 1:
            got = _mt(q[:, path], ks, vs, kn[:, path], vn[:, path], cache_seqlens=cl, causal=True)
        else:
            got = flash_attn_with_kvcache(q[:, path], ks, vs, kn[:, path], vn[:, path], cache_seqlens=cl, causal=True)
        torch.cuda.synchronize()
        _close(out[:, path], got, dtype, "path %s" % path)


@pytest.mark.parametrize("D,dtype", [(128, torch.float16), (64, torch.bfloat16), (64, torch.float16), (128, torch.bfloat16)], ids=["d128_f16", "d64_bf16", "d64_f16", "d128_bf16"])
@pytest.mark.parametrize("n_draft", [8, 3, 1])
def test_keep_rows(n_draft, D, dtype):
    """Random ascending keep_idx, keep_cnt 0 .. n_draft, cache_batch_idx, a strided cache view: the WHOLE allocation equals the torch-indexed
    result (nothing else was written; rows at or past row0 + keep_cnt keep their contents)."""
    from vattention_amd.cache_ops import keep_rows
    torch.manual_seed(n_draft * 10 + D)
    B, slots, Hkv, rows = 6, 8, 3, 120
    fullk, fullv = torch.randn(slots, rows + 9, Hkv + 2, D).to(dtype), torch.randn(slots, rows + 9, Hkv + 2, D).to(dtype)
    view = lambda t: t[:, 5:5 + rows, 1:1 + Hkv]                 # strided: row offset, head offset, wider row and batch strides
    idx = torch.randperm(slots)[:B].to(torch.int32)
    row0 = torch.tensor([0, 17, rows - n_draft, 31, 64, 3], dtype=torch.int32)
    cnt = torch.tensor([0, 1, n_draft, n_draft // 2, max(n_draft - 1, 0), n_draft], dtype=torch.int32)
    keep = torch.zeros(B, n_draft, dtype=torch.int32)
    for b in range(B):
        keep[b, :cnt[b]] = torch.randperm(n_draft)[:cnt[b]].sort().values.to(torch.int32)
    keep[5] = torch.arange(n_draft, dtype=torch.int32)            # the identity: nothing moves
    keep[4, :cnt[4]] = torch.arange(1, n_draft, dtype=torch.int32)  # every kept row moves down by one
    wantk, wantv = fullk.clone(), fullv.clone()
    for b in range(B):
        for want, full in ((wantk, fullk), (wantv, fullv)):
            for i in range(int(cnt[b])):
                view(want)[idx[b], row0[b] + i] = view(full)[idx[b], row0[b] + keep[b, i]]
    gk, gv = fullk.to(DEV), fullv.to(DEV)
    keep_rows(view(gk), view(gv), row0.to(DEV), keep.to(DEV), cnt.to(DEV), cache_batch_idx=idx.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(gk.cpu(), wantk) and torch.equal(gv.cpu(), wantv)
    assert not torch.equal(wantk, fullk) or n_draft == 1           # (something did move)
    # identity slots (no cache_batch_idx)
    gk, gv = fullk.to(DEV), fullv.to(DEV)
    wantk, wantv = fullk.clone(), fullv.clone()
    for b in range(B):
        for want, full in ((wantk, fullk), (wantv, fullv)):
            for i in range(int(cnt[b])):
                view(want)[b, row0[b] + i] = view(full)[b, row0[b] + keep[b, i]]
    keep_rows(view(gk), view(gv), row0.to(DEV), keep.to(DEV), cnt.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(gk.cpu(), wantk) and torch.equal(gv.cpu(), wantv)


def test_verify_compact_decode_end_to_end():
    """Tree verify with append, keep_rows of one accepted path per entry, then a one-token decode step at cache_seqlens + keep_cnt: the cache
    rows [0, cache_seqlens + keep_cnt + 1) are those of a cache built by appending the accepted tokens one after the other, and the decode
    output is the oracle's on that cache."""
    from vattention_amd.cache_ops import keep_rows
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(12)
    sq, Hq, Hkv, D, dtype = 7, 8, 2, 128, torch.float16
    ctx = [500, 61, 0, 2047]
    accepted = [[0, 2, 5, 6], [0, 1, 3], [0], [0, 1, 4]]
    B, rows, slots = len(ctx), 2047 + sq + 4, 6
    kc, vc = torch.randn(slots, rows, Hkv, D).to(dtype), torch.randn(slots, rows, Hkv, D).to(dtype)
    idx = torch.tensor([4, 0, 5, 2], dtype=torch.int32)
    q, kn, vn = torch.randn(B, sq, Hq, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype)
    q1, k1, v1 = torch.randn(B, 1, Hq, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype)
    cl = torch.tensor(ctx, dtype=torch.int32)
    cnt = torch.tensor([len(a) for a in accepted], dtype=torch.int32)
    keep = torch.zeros(B, sq, dtype=torch.int32)
    for b, a in enumerate(accepted):
        keep[b, :len(a)] = torch.tensor(a, dtype=torch.int32)
    mask = pack_mask(_tree_vis(PARENT7)).expand(B, sq).contiguous()          # int32 words [B, sq]: every entry drafts the same tree
    kg, vg = kc.to(DEV), vc.to(DEV)
    out, _ = _tree(q.to(DEV), kg, vg, mask.to(DEV), kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV))
    ref64 = tree_attn_ref(q, kc.clone(), vc.clone(), mask, kn, vn, cache_seqlens=cl, cache_batch_idx=idx)
    ref32 = tree_attn_ref(q, kc.clone(), vc.clone(), mask, kn, vn, cache_seqlens=cl, cache_batch_idx=idx, math="f32")
    _check(out, ref64, ref32, dtype, "verify")
    keep_rows(kg, vg, cl.to(DEV), keep.to(DEV), cnt.to(DEV), cache_batch_idx=idx.to(DEV))
    dec = flash_attn_with_kvcache(q1.to(DEV), kg, vg, k1.to(DEV), v1.to(DEV), cache_seqlens=(cl + cnt).to(DEV), cache_batch_idx=idx.to(DEV), causal=True)
    torch.cuda.synchronize()
    # the same history, token by token
    ks, vs = kc.clone(), vc.clone()
    for b, a in enumerate(accepted):
        for i, node in enumerate(a):
            ks[idx[b], ctx[b] + i], vs[idx[b], ctx[b] + i] = kn[b, node], vn[b, node]
    d64 = flash_attn_with_kvcache_ref(q1, ks, vs, k1, v1, cache_seqlens=cl + cnt, cache_batch_idx=idx)
    d32 = flash_attn_with_kvcache_ref(q1, ks.clone(), vs.clone(), cache_seqlens=cl + cnt + 1, cache_batch_idx=idx, math="f32")
    for b in range(B):
        n = ctx[b] + len(accepted[b]) + 1
        assert torch.equal(kg[idx[b], :n].cpu(), ks[idx[b], :n]) and torch.equal(vg[idx[b], :n].cpu(), vs[idx[b], :n]), b
    _check(dec, d64, d32, dtype, "decode step after the compaction")
