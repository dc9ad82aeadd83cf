"""GPU parity of the MULTI-TOKEN decode form (include/vattn_kernels.h: q [B, 2..8, Hq, D] — the verify step of speculative decoding — on the
split-KV decode kernels with (token, head) columns) through the Python drop-in, against the CPU oracle (oracle/attn.py) and, for windows,
tests/window_ref.py.  Every call asserts through the plan description (and the drop-in's counter) that the library TOOK the new form.

Tolerances are the project's, restated from tests/test_gpu_attention.py (`_check`) and tests/test_gpu_window.py (LSE: 2e-3 absolute).
The no-read contract is checked by POISONING rows (K NaN, V Inf), as tests/test_gpu_window.py does; nothing is unmapped on purpose."""
import pytest
import torch

from oracle.attn import flash_attn_with_kvcache_ref
from tests.window_ref import first_visible_key, window_attn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = [(8, 2), (32, 4), (28, 4), (8, 1), (8, 8)]


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


def _mt(*a, **kw):
    """flash_attn_with_kvcache, asserting that the call took the multi-token form: the plan description of the very parameter block the
    drop-in launches (seen at its launch point: `_params_out` is not filled for calls that return the LSE), and the drop-in's counter"""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    seen, launch = [], FA._launch
    n0, p0 = FA.counters["multitoken_decode_calls"], FA.counters["prefill_calls"]

    def spy(p, dev, keep=()):
        seen.append(p)
        return launch(p, dev, keep)
    FA._launch = spy
    try:
        r = FA.flash_attn_with_kvcache(*a, **kw)
    finally:
        FA._launch = launch
    assert FA.counters["multitoken_decode_calls"] == n0 + 1 and FA.counters["prefill_calls"] == p0
    assert len(seen) == 1
    d = K.describe(seen[0])
    assert d["form"] == 1 and seen[0].seqlen_q > 1, d
    return r, d


def _lengths(sq):
    """visible lengths Lk: Lk % 32 in {0, 1, sq - 1, sq, 31}, a tail that spans two tiles (1 <= Lk % 32 < sq), Lk == sq, Lk < sq (dead rows),
    and a few contexts long enough for several pieces"""
    return [sq, sq - 1, 64, 65, 96 + sq - 1, 128 + sq, 32 * 9 + 31, 32 * 7 + 1, 1500 + sq, 3007]


@pytest.mark.parametrize("D,dtype", [(128, torch.float16), (128, torch.bfloat16), (64, torch.float16), (64, torch.bfloat16)], ids=["d128_f16", "d128_bf16", "d64_f16", "d64_bf16"])
@pytest.mark.parametrize("Hq,Hkv", HEADS, ids=["%d_%d" % h for h in HEADS])
@pytest.mark.parametrize("sq", [2, 3, 4, 5, 8])
def test_multitoken_parity(sq, Hq, Hkv, D, dtype):
    """Ragged batches with cache_batch_idx, causal and not, with and without k / v (append: the cache equals the oracle's bit for bit), LSE,
    a strided q view and a caller-provided out."""
    torch.manual_seed(sq * 1000 + Hq * 10 + Hkv + D)
    vis = _lengths(sq)
    B, slots, rows = len(vis), len(vis) + 3, 3100
    kc, vc = torch.randn(slots, rows, Hkv, D).to(dtype), torch.randn(slots, rows, Hkv, D).to(dtype)
    idx = torch.randperm(slots)[:B].to(torch.int32)
    qw = torch.randn(B, sq, Hq + 2, D).to(dtype)
    q = qw[:, :, 1:Hq + 1]                                        # a strided view: head stride D, row stride (Hq + 2) D
    kn, vn = torch.randn(B, sq, Hkv, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype)
    qg, idg = qw.to(DEV)[:, :, 1:Hq + 1], idx.to(DEV)
    for append in (True, False):
        # with k / v the call appends sq rows at cache_seqlens: Lk = cache_seqlens + sq (the Lk < sq entry becomes cache_seqlens == 0)
        cl = torch.tensor([max(n - sq, 0) for n in vis] if append else vis, dtype=torch.int32)
        new_cpu = dict(k=kn, v=vn) if append else {}
        new_gpu = (kn.to(DEV), vn.to(DEV)) if append else (None, None)
        for causal in (True, False):
            what = "sq=%d %d/%d d=%d append=%s causal=%s" % (sq, Hq, Hkv, D, append, causal)
            kr, vr = kc.clone(), vc.clone()
            ref64, lse64 = flash_attn_with_kvcache_ref(q, kr, vr, cache_seqlens=cl, cache_batch_idx=idx, causal=causal, return_lse=True, **new_cpu)
            ref32 = flash_attn_with_kvcache_ref(q, kc.clone(), vc.clone(), cache_seqlens=cl, cache_batch_idx=idx, causal=causal, math="f32", **new_cpu)
            kg, vg = kc.to(DEV), vc.to(DEV)
            out = torch.full((B, sq, Hq + 1, D), 7.0, dtype=dtype, device=DEV)[:, :, :Hq]      # caller-provided, strided
            (_, d) = _mt(qg, kg, vg, *new_gpu, cache_seqlens=cl.to(DEV), cache_batch_idx=idg, causal=causal, out=out)
            torch.cuda.synchronize()
            assert d["tiling"] == (2 if sq * (Hq // Hkv) > 16 else 1), d
            _check(out, ref64, ref32, dtype, what)
            assert torch.equal(kg.cpu(), kr) and torch.equal(vg.cpu(), vr), what + ": the cache after the call is the oracle's, every row"
            (o2, lse), _ = _mt(qg, kg, vg, cache_seqlens=(cl + (sq if append else 0)).to(DEV), cache_batch_idx=idg, causal=causal, return_softmax_lse=True)
            torch.cuda.synchronize()
            _check(o2, ref64, ref32, dtype, what + " (+lse)")
            _check_lse(lse, lse64, what + " lse")
            if causal and not append:
                dead = out[1, 0].float().abs().max().item()          # entry 1: Lk = sq - 1, row 0 sees no key
                assert dead == 0.0 and bool(torch.isinf(lse[1, :, 0]).all())


def _ragged16():
    return [100, 20000, 257, 4096, 31, 9999, 12345, 1024, 16000, 700, 19999, 3, 5000, 2048, 8191, 64]


@pytest.mark.parametrize("case", [
    dict(name="one_20k_sequence", lens=[20000], Hq=8, Hkv=2, sq=4, D=128, dtype=torch.float16, splits=(0, -3)),
    dict(name="one_20k_sequence_bf16_d64", lens=[20011], Hq=28, Hkv=4, sq=2, D=64, dtype=torch.bfloat16, splits=(0,)),
    dict(name="ragged16", lens=_ragged16(), Hq=8, Hkv=2, sq=4, D=128, dtype=torch.float16, splits=(0, -37, -400)),
    dict(name="ragged16_bf16", lens=_ragged16(), Hq=8, Hkv=1, sq=2, D=128, dtype=torch.bfloat16, splits=(0, -100)),
    dict(name="R32", lens=_ragged16()[:6], Hq=32, Hkv=4, sq=4, D=128, dtype=torch.float16, splits=(0, -50)),
    dict(name="R32_one_sequence", lens=[20000], Hq=32, Hkv=4, sq=4, D=128, dtype=torch.float16, splits=(0,)),
    dict(name="R64_two_groups", lens=[20000, 300, 5001], Hq=16, Hkv=2, sq=8, D=128, dtype=torch.float16, splits=(0,)),
    dict(name="R64_two_groups_d64", lens=[9000], Hq=8, Hkv=1, sq=8, D=64, dtype=torch.float16, splits=(0,)),
], ids=lambda c: c["name"])
def test_multitoken_merges(case):
    """Pieces of one sequence merged across workgroups: the uniform split of one sequence, the device-planned stream decomposition of a ragged
    batch (default and forced grids), two-block workgroups (R = 32) and sibling head-block groups (R = 64)."""
    lens, Hq, Hkv, sq, D, dtype = case["lens"], case["Hq"], case["Hkv"], case["sq"], case["D"], case["dtype"]
    torch.manual_seed(len(lens) + Hq + sq)
    B, rows = len(lens), max(lens) + sq
    kc, vc = torch.randn(B, rows, Hkv, D).to(dtype), torch.randn(B, rows, Hkv, D).to(dtype)
    q, kn, vn = torch.randn(B, sq, Hq, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype)
    cl = torch.tensor(lens, dtype=torch.int32)
    kr, vr = kc.clone(), vc.clone()
    ref64, lse64 = flash_attn_with_kvcache_ref(q, kr, vr, kn, vn, cache_seqlens=cl, causal=True, return_lse=True)
    ref32 = flash_attn_with_kvcache_ref(q, kc.clone(), vc.clone(), kn, vn, cache_seqlens=cl, causal=True, math="f32")
    merged = False
    for splits in case["splits"]:
        kg, vg = kc.to(DEV), vc.to(DEV)
        out, d = _mt(q.to(DEV), kg, vg, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), causal=True, num_splits=splits)
        torch.cuda.synchronize()
        merged |= d["merge_launch"] == 1
        _check(out, ref64, ref32, dtype, "%s splits=%d %s" % (case["name"], splits, d))
        assert torch.equal(kg.cpu(), kr) and torch.equal(vg.cpu(), vr)
        (o2, lse), _ = _mt(q.to(DEV), kg, vg, cache_seqlens=(cl + sq).to(DEV), causal=True, num_splits=splits, return_softmax_lse=True)
        torch.cuda.synchronize()
        _check_lse(lse, lse64, "%s splits=%d lse" % (case["name"], splits))
    assert merged


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("sq,Hq,Hkv,D", [(4, 8, 2, 128), (8, 32, 4, 128), (3, 28, 4, 64), (2, 8, 8, 128)], ids=["sq4_g4", "sq8_g8", "sq3_g7_d64", "sq2_mha"])
def test_multitoken_window(sq, Hq, Hkv, D, dtype):
    """left in {0, 1, 31, 32, 33, 1000} and a left larger than every sequence (but inside the view), default launch and forced grids."""
    torch.manual_seed(sq + Hq)
    vis = [777, sq, 40, 1025 + sq, 5000, 64 + sq - 1, 33, 2048]
    B, rows = len(vis), max(vis) + 40
    kc, vc = torch.randn(B + 1, rows, Hkv, D).to(dtype), torch.randn(B + 1, rows, Hkv, D).to(dtype)
    idx = torch.randperm(B + 1)[:B].to(torch.int32)
    q, kn, vn = torch.randn(B, sq, Hq, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype), torch.randn(B, sq, Hkv, D).to(dtype)
    cl = torch.tensor([n - sq for n in vis], dtype=torch.int32)
    ka, va = kc.clone(), vc.clone()          # the caches after the append
    for b in range(B):
        ka[idx[b], vis[b] - sq:vis[b]], va[idx[b], vis[b] - sq:vis[b]] = kn[b], vn[b]
    for left in (0, 1, 31, 32, 33, 1000, max(vis) + 10):
        ref64, lse64 = window_attn_ref(q, ka, va, left, cache_seqlens=vis, cache_batch_idx=idx, return_lse=True)
        ref32 = window_attn_ref(q, ka, va, left, cache_seqlens=vis, cache_batch_idx=idx, math="f32")
        for splits in (0, -7, -90):
            kg, vg = kc.to(DEV), vc.to(DEV)
            out, d = _mt(q.to(DEV), kg, vg, kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), cache_batch_idx=idx.to(DEV), causal=True,
                         window_size=(left, 0), num_splits=splits)
            torch.cuda.synchronize()
            what = "window sq=%d left=%d splits=%d" % (sq, left, splits)
            _check(out, ref64, ref32, dtype, what)
            assert torch.equal(kg.cpu(), ka) and torch.equal(vg.cpu(), va), what
            # the LSE of the same launch plan (the merge's LSE under a window too), on the cache the call above left
            (o2, lse), _ = _mt(q.to(DEV), kg, vg, cache_seqlens=torch.tensor(vis, dtype=torch.int32, device=DEV), cache_batch_idx=idx.to(DEV),
                               window_size=(left, -1), causal=True, num_splits=splits, return_softmax_lse=True)
            torch.cuda.synchronize()
            _check(o2, ref64, ref32, dtype, what + " (+lse)")
            _check_lse(lse, lse64, what + " lse")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("sq,Hq,Hkv", [(4, 8, 2), (8, 32, 4), (5, 28, 4)], ids=["sq4", "sq8_R64", "sq5_g7"])
def test_multitoken_equals_one_token_decode_rows_and_the_prefill_form(sq, Hq, Hkv, dtype):
    """Row t is the one-token decode call at length Lk - sq + t + 1; the whole call is the prefill form of the same call (_variant = 8: an
    explicit prefill tiling keeps the prefill kernels) — each within the tolerance both are held to."""
    from vattention_amd import kernels as K
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(17 * sq)
    D, vis = 128, [3000, sq, 65, 1024 + sq - 1, 9000]
    B, rows = len(vis), max(vis) + 8
    kg, vg = torch.randn(B, rows, Hkv, D, device=DEV).to(dtype), torch.randn(B, rows, Hkv, D, device=DEV).to(dtype)
    q = torch.randn(B, sq, Hq, D, device=DEV).to(dtype)
    cl = torch.tensor(vis, dtype=torch.int32, device=DEV)
    out, _ = _mt(q, kg, vg, cache_seqlens=cl, causal=True)
    for t in range(sq):
        one = flash_attn_with_kvcache(q[:, t:t + 1], kg, vg, cache_seqlens=cl - (sq - 1 - t), causal=True)
        _close(out[:, t:t + 1], one, dtype, "row %d vs the one-token call" % t)
    pout = []
    pre = flash_attn_with_kvcache(q, kg, vg, cache_seqlens=cl, causal=True, _variant=8, _params_out=pout)
    torch.cuda.synchronize()
    assert K.describe(pout[0])["form"] == 0
    _close(out, pre, dtype, "multi-token form vs prefill form")


# ---- the no-read contract (ahead of the page-manager test) ----

@pytest.mark.parametrize("sq,Hq,Hkv", [(4, 8, 2), (8, 32, 4)], ids=["R16", "R64"])
def test_multitoken_no_read_contract(sq, Hq, Hkv):
    """No K / V load at or beyond Lk; windowed: none below align_down(first key visible to the entry's FIRST query row, 32)."""
    torch.manual_seed(4)
    D = 128
    lens = [3000, 400, 1777, 6000, 0, 95]                    # cache_seqlens; Lk = lens + sq
    B, rows = len(lens), 6100
    kc, vc = torch.randn(B, rows, Hkv, D, device=DEV).half(), torch.randn(B, rows, Hkv, D, device=DEV).half()
    q, kn, vn = torch.randn(B, sq, Hq, D, device=DEV).half(), torch.randn(B, sq, Hkv, D, device=DEV).half(), torch.randn(B, sq, Hkv, D, device=DEV).half()
    clg = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for left in (None, 500, 0):
        kp, vp = kc.clone(), vc.clone()
        for b in range(B):
            kp[b, lens[b] + sq:], vp[b, lens[b] + sq:] = float("nan"), float("inf")
            if left is not None:
                dead = first_visible_key(sq, lens[b] + sq, left) // 32 * 32          # T = 32
                kp[b, :dead], vp[b, :dead] = float("nan"), float("inf")
        assert bool(torch.isnan(kp).any())
        win = dict(window_size=(left, 0)) if left is not None else {}
        for splits in (0, -5, -64):
            for new in ((kn, vn), None):
                cs = clg if new else clg + sq
                kv = new or ()
                ka, va, kb, vb = kc.clone(), vc.clone(), kp.clone(), vp.clone()
                if not new:        # the rows the other leg appends are ordinary data in both twins
                    for b in range(B):
                        for k_, v_ in ((ka, va), (kb, vb)):
                            k_[b, lens[b]:lens[b] + sq], v_[b, lens[b]:lens[b] + sq] = kn[b], vn[b]
                a, _ = _mt(q, ka, va, *kv, cache_seqlens=cs, causal=True, num_splits=splits, **win)
                p, _ = _mt(q, kb, vb, *kv, cache_seqlens=cs, causal=True, num_splits=splits, **win)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "left=%s splits=%d append=%s" % (left, splits, bool(new))


def test_multitoken_graph_capture():
    """One captured and replayed verify call equals the eager result bit for bit (no host-to-device copy, no allocation once the workspace exists)."""
    torch.manual_seed(21)
    B, sq, Hq, Hkv, D, ctx = 4, 4, 8, 2, 128, 3000
    kc, vc = torch.randn(6, ctx, Hkv, D, device=DEV).half(), torch.randn(6, ctx, Hkv, D, device=DEV).half()
    q = torch.randn(B, sq, Hq, D, device=DEV).half()
    kn, vn = torch.randn(B, sq, Hkv, D, device=DEV).half(), torch.randn(B, sq, Hkv, D, device=DEV).half()
    cl = torch.tensor([100, 2500, 31, 1999], dtype=torch.int32, device=DEV)
    idx = torch.tensor([5, 0, 3, 1], dtype=torch.int32, device=DEV)
    out = torch.empty_like(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on the capture stream: creates that stream's workspace
        _mt(q, kc.clone(), vc.clone(), kn, vn, cache_seqlens=cl, cache_batch_idx=idx, causal=True, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    kg, vg = kc.clone(), vc.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _mt(q, kg, vg, kn, vn, cache_seqlens=cl, cache_batch_idx=idx, causal=True, out=out)
    for step in range(3):
        q.copy_(torch.randn_like(q)); kn.copy_(torch.randn_like(kn)); vn.copy_(torch.randn_like(vn))
        if step:
            cl.add_(2)                                  # two of the four draft tokens were accepted
        ke, ve = kg.clone(), vg.clone()
        g.replay()
        torch.cuda.synchronize()
        ref, _ = _mt(q, ke, ve, kn, vn, cache_seqlens=cl, cache_batch_idx=idx, causal=True)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), step
        assert torch.equal(kg, ke) and torch.equal(vg, ve)


def test_multitoken_verify_steps_through_the_page_manager():
    """The `vattention` drop-in with 64 KiB pages (128 tokens per page): the slot is stepped to len + seqlen_q so that the draft rows' pages are
    mapped, a verify call appends across a page boundary, 2 of the 4 tokens are accepted (the caller advances cache_seqlens by 2; the
    rejected rows are overwritten by the next step), and the next verify call follows.  Every step against the oracle."""
    from vattention_amd import vattention
    from vattention_amd.cache_ops import cache_flat
    torch.zeros(1, device=DEV)
    mn, _ = vattention.granularity(0)
    page = 64 << 10 if (64 << 10) % mn == 0 else 2 << 20
    L, Hkv, Hq, D, B, ctx, sq = 1, 2, 8, 128, 4, 8192, 4
    tok_per_page = page // (Hkv * D * 2)
    ts = vattention.init_kvcache(L, Hkv, D, B, ctx, 0, torch.float16, page, False)
    try:
        Kt, Vt = ts[0], ts[1]
        vattention.reserve_physical_pages(256 * page)
        torch.manual_seed(9)
        starts = [tok_per_page * 3 - 2, 700]                  # the first verify call of slot 0 appends across a page boundary
        lens, slots = [0] * B, []
        for n in starts:
            s = vattention.alloc_new_batch_idx(n)
            lens[s] = n
            slots.append(s)
        vattention.step_async(lens)
        host = {}
        for s, n in zip(slots, starts):
            k, v = torch.randn(n, Hkv, D).half(), torch.randn(n, Hkv, D).half()
            host[s] = [k, v]
            cache_flat(k.to(DEV), v.to(DEV), Kt[s].reshape(-1, Hkv, D), Vt[s].reshape(-1, Hkv, D), "auto")
        cur = dict(zip(slots, starts))
        for step in range(3):
            for s in slots:
                lens[s] = cur[s] + sq                         # lengths INCLUDE the draft rows: their pages get mapped
            vattention.step_async(lens)
            q = torch.randn(len(slots), sq, Hq, D).half()
            kn, vn = torch.randn(len(slots), sq, Hkv, D).half(), torch.randn(len(slots), sq, Hkv, D).half()
            cl = torch.tensor([cur[s] for s in slots], dtype=torch.int32)
            mx = int(cl.max()) + sq
            out, _ = _mt(q.to(DEV), Kt[:, :mx], Vt[:, :mx], kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV),
                         cache_batch_idx=torch.tensor(slots, dtype=torch.int32, device=DEV), causal=True)
            torch.cuda.synchronize()
            for i, s in enumerate(slots):
                kf = torch.cat([host[s][0][:cur[s]], kn[i]], 0).unsqueeze(0)
                vf = torch.cat([host[s][1][:cur[s]], vn[i]], 0).unsqueeze(0)
                ref64 = flash_attn_with_kvcache_ref(q[i:i + 1], kf.clone(), vf.clone(), cache_seqlens=cur[s] + sq, causal=True)
                ref32 = flash_attn_with_kvcache_ref(q[i:i + 1], kf.clone(), vf.clone(), cache_seqlens=cur[s] + sq, causal=True, math="f32")
                _check(out[i:i + 1], ref64, ref32, torch.float16, "page manager step %d slot %d" % (step, s))
                assert torch.equal(Kt[s, :cur[s] + sq].cpu(), kf[0]) and torch.equal(Vt[s, :cur[s] + sq].cpu(), vf[0])
                host[s] = [kf[0], vf[0]]
                cur[s] += 2                                   # 2 of 4 accepted
    finally:
        vattention.cleanup()
