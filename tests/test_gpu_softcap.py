"""GPU parity of logit soft-capping (softcap=x: scores = x * tanh(q.k * softmax_scale / x)) through the Python drop-in — and therefore the C
ABI (vattn_softcap_attn_with_kvcache) — of the PRODUCT library, against tests/softcap_ref.py (checked against the oracle in
tests/test_softcap_ref.py).

Tolerances are the project's (tests/test_gpu_attention.py, restated in tests/test_gpu_window.py): output against float64 at atol = rtol =
2e-3 for fp16 I/O and 1.6e-2 for bf16 I/O — bf16 cannot be held to 2e-3: the reference-numerics CPU run itself (fp32 accumulate, P and the
output rounded to bf16) is up to 1.16 x that bound off float64 on these inputs — AND the kernel's max error within 2 x the error of that
reference-numerics run + 1e-5 (+ 4e-3 for bf16), as there.  LSE (fp32 on both sides): 2e-3 absolute, as there; it is what measures the
hardware exp2 / reciprocal inside the tanh.

Inputs that make the cap matter: q = 4 randn, k, v = randn, caps 1.5 and 30.  Every parity case first asserts ON THE CPU REFERENCE ALONE that
the capped and the uncapped float64 results differ by more than 10 x the fp16 bound 2e-3 + 2e-3 |ref| (for bf16 that is still more than its
own, wider bound): a kernel that ignores the cap cannot pass, nor can a test whose inputs never reach it.  (Entries with one visible key
give the same output with or without a cap; the assertion is on the case's other entries.)  No "huge cap equals the plain call" case: the
tanh expression's error grows with the cap (include/vattn_kernels.h)."""
import ctypes as C

import pytest
import torch

from tests.softcap_ref import softcap_attn_ref
from tests.window_ref import first_visible_key

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
HEAD_DIMS = pytest.mark.parametrize("D", [64, 128])
CAPS = pytest.mark.parametrize("cap", [1.5, 30.0])


def _tol(dtype):
    return (2e-3, 2e-3) if dtype == torch.float16 else (1.6e-2, 1.6e-2)


def _check(out_gpu, ref64, ref32, dtype, what):
    atol, rtol = _tol(dtype)
    got = out_gpu.double().cpu()
    err = (got - ref64).abs()
    bound = atol + rtol * ref64.abs()
    print("%s: max err %.3e, max err / bound %.3f" % (what, err.max().item(), (err / bound).max().item()))
    assert bool((err <= bound).all()), "%s: max err %.3e (allowed %.3e)" % (what, err.max().item(), bound.max().item())
    e_ref = (ref32.double() - ref64).abs().max().item()
    assert err.max().item() <= 2 * e_ref + 1e-5 + (0 if dtype == torch.float16 else 4e-3), \
        "%s: kernel err %.3e vs reference-numerics err %.3e" % (what, err.max().item(), e_ref)


def _check_lse(lse_gpu, lse64, what):
    got = lse_gpu.double().cpu()
    live = torch.isfinite(lse64)
    assert bool((torch.isinf(got) & (got > 0))[~live].all()), "%s: a row without a visible key must have LSE +inf" % what
    err = (got[live] - lse64[live]).abs().max().item() if bool(live.any()) else 0.0
    print("%s: max LSE err %.3e" % (what, err))
    assert err < 2e-3, "%s: lse err %.3e" % (what, err)


def _refs(q, kc, vc, cap, **kw):
    """(float64 output, float64 LSE, reference-numerics output) with the cap, after asserting that the cap matters on these inputs"""
    ref64, lse64 = softcap_attn_ref(q, kc, vc, cap, math="f64", return_lse=True, **kw)
    plain = softcap_attn_ref(q, kc, vc, 0.0, math="f64", **kw)
    ratio = ((ref64 - plain).abs() / (2e-3 + 2e-3 * ref64.abs())).max().item()
    assert ratio > 10, "the inputs never reach the cap: capped vs uncapped differ by %.1f x the bound" % ratio
    return ref64, lse64, softcap_attn_ref(q, kc, vc, cap, math="f32", **kw)


def _data(B, Sq, Hq, Hkv, D, rows, dtype, seed, slots=None):
    torch.manual_seed(seed)
    q = (4 * torch.randn(B, Sq, Hq, D)).to(dtype)
    kc, vc = torch.randn(slots or B, rows, Hkv, D).to(dtype), torch.randn(slots or B, rows, Hkv, D).to(dtype)
    return q, kc, vc


def _describe_softcap(p, cap):
    from vattention_amd import kernels as K
    return K.describe_softcap(p, cap)


# ---- one-token decode ----

@CAPS
@HEAD_DIMS
@DTYPES
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (32, 1)], ids=["g4", "g32_two_head_blocks"])
def test_decode_parity(Hq, Hkv, dtype, D, cap):
    """lengths [1, 33, 300] in one batch (below one 32-key tile, one key into the second, several tiles); the default launch (device-planned
    stream for G = 4, grid heuristics for the two-head-block workgroups of G = 32), a forced stream grid (num_splits = -3) and the uniform split
    with its merge launch (num_splits = 3); with and without an appended row; slots through a permutation."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    lens, rows = [1, 33, 300], 308
    q, kc, vc = _data(3, 1, Hq, Hkv, D, rows, dtype, 11)
    kn, vn = torch.randn(3, 1, Hkv, D).to(dtype), torch.randn(3, 1, Hkv, D).to(dtype)
    idx = torch.tensor([2, 0, 1], dtype=torch.int32)
    for append in (False, True):
        ck, cv = kc.clone(), vc.clone()
        before = [n - 1 for n in lens] if append else lens
        if append:
            for b in range(3):
                ck[idx[b], lens[b] - 1], cv[idx[b], lens[b] - 1] = kn[b, 0], vn[b, 0]
        ref64, lse64, ref32 = _refs(q, ck, cv, cap, cache_seqlens=lens, cache_batch_idx=idx)
        for splits, want_path in ((0, 2 if Hq // Hkv <= 16 else 0), (-3, 2), (3, 0)):
            kg, vg = kc.to(DEV), vc.to(DEV)
            new = (kn.to(DEV), vn.to(DEV)) if append else (None, None)
            clg, idg = torch.tensor(before, dtype=torch.int32, device=DEV), idx.to(DEV)
            what = "decode G%d d%d cap %g append %d splits %d" % (Hq // Hkv, D, cap, append, splits)
            pout = []
            out = flash_attn_with_kvcache(q.to(DEV), kg, vg, *new, cache_seqlens=clg, cache_batch_idx=idg, causal=True, softcap=cap, num_splits=splits, _params_out=pout)
            torch.cuda.synchronize()
            d = _describe_softcap(pout[0], cap)
            assert d["form"] == 1 and d["path"] == want_path and d["tiling"] == (2 if Hq // Hkv > 16 else 1), (what, d)
            if splits == 3:
                assert d["nsplit"] == 3 and d["merge_launch"] == 1, d
            _check(out, ref64, ref32, dtype, what)
            if append:
                assert torch.equal(kg.cpu(), ck) and torch.equal(vg.cpu(), cv), what      # in-place append, nothing else touched
            kg, vg = kc.to(DEV), vc.to(DEV)
            out, lse = flash_attn_with_kvcache(q.to(DEV), kg, vg, *new, cache_seqlens=clg, cache_batch_idx=idg, causal=True, softcap=cap, num_splits=splits,
                                               return_softmax_lse=True)
            torch.cuda.synchronize()
            _check(out, ref64, ref32, dtype, what + " +lse")
            _check_lse(lse, lse64, what)


# ---- multi-token ----

@CAPS
@HEAD_DIMS
@DTYPES
@pytest.mark.parametrize("Sq,G", [(4, 4), (8, 8)], ids=["4x4", "8x8_64_columns"])
def test_multitoken_parity(Sq, G, dtype, D, cap):
    """lengths [3, 70, 300]: the first entry has rows without a visible key under the causal rule (0 and LSE +inf); causal, not causal,
    and causal with left = 40; the rows' K/V appended by the call in half of the runs."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    Hkv, lens, rows = 2, [3, 70, 300], 304
    Hq = G * Hkv
    q, kc, vc = _data(3, Sq, Hq, Hkv, D, rows, dtype, 12)
    for causal, left, append in ((True, None, False), (False, None, True), (True, 40, True), (True, 40, False)):
        kw = dict(cache_seqlens=lens, causal=causal, left=left)
        ref64, lse64, ref32 = _refs(q, kc, vc, cap, **kw)
        if causal:
            assert not bool(ref64[0, :Sq - 3].any()) and bool(torch.isinf(lse64[0, :, :Sq - 3]).all())
        kg, vg = kc.to(DEV), vc.to(DEV)
        before, new = lens, (None, None)
        if append:      # the last min(Sq, length) rows of every entry arrive with the call; the cache holds zeros there before it
            nnew = min(Sq, min(lens))
            before = [n - nnew for n in lens]
            kn, vn = torch.stack([kc[b, n - nnew:n] for b, n in enumerate(lens)]), torch.stack([vc[b, n - nnew:n] for b, n in enumerate(lens)])
            for b, n in enumerate(lens):
                kg[b, n - nnew:n], vg[b, n - nnew:n] = 0, 0
            new = (kn.to(DEV), vn.to(DEV))
        what = "multitoken %dx%d d%d cap %g causal %d left %s append %d" % (Sq, G, D, cap, causal, left, append)
        clg = torch.tensor(before, dtype=torch.int32, device=DEV)
        win = (-1, -1) if left is None else (left, 0)
        pout = []
        out = flash_attn_with_kvcache(q.to(DEV), kg, vg, *new, cache_seqlens=clg, causal=causal, window_size=win, softcap=cap, _params_out=pout)
        torch.cuda.synchronize()
        d = _describe_softcap(pout[0], cap)
        assert d["form"] == 1 and d["tiling"] == (2 if Sq * G > 16 else 1), (what, d)
        _check(out, ref64, ref32, dtype, what)
        assert torch.equal(kg.cpu(), kc) and torch.equal(vg.cpu(), vc), what
        out, lse = flash_attn_with_kvcache(q.to(DEV), kg, vg, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=causal, window_size=win,
                                           softcap=cap, return_softmax_lse=True)
        torch.cuda.synchronize()
        _check(out, ref64, ref32, dtype, what + " +lse")
        _check_lse(lse, lse64, what)


# ---- prefill ----

@CAPS
@HEAD_DIMS
@DTYPES
@pytest.mark.parametrize("n,c", [(300, 0), (130, 200)], ids=["prompt_on_empty_cache", "chunk_behind_200_rows"])
def test_prefill_parity(n, c, dtype, D, cap):
    """a 300-row prompt and a 130-row chunk behind 200 cached rows; causal, not causal, left = 100; the plan's choice, tilings 1 and 4 through
    the _variant selectors, two key-range shares (num_splits = 2); the chunk's K/V appended by the call in one run; LSE everywhere."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    Hq, Hkv = 8, 2
    q, kc, vc = _data(1, n, Hq, Hkv, D, c + n + 5, dtype, 13, slots=2)
    cl = torch.tensor([c + n], dtype=torch.int32, device=DEV)
    for causal, left in ((True, None), (False, None), (True, 100)):
        ref64, lse64, ref32 = _refs(q, kc[1:2], vc[1:2], cap, cache_seqlens=c + n, causal=causal, left=left)
        win = (-1, -1) if left is None else (left, 0)
        for variant, splits, tiling in ((0, 0, None), (2, 0, 1), (8, 0, 4), (2, 2, 1), (8, 2, 4)):
            what = "prefill n%d c%d d%d cap %g causal %d left %s variant %d splits %d" % (n, c, D, cap, causal, left, variant, splits)
            kg, vg = kc.to(DEV), vc.to(DEV)
            pout = []
            flash_attn_with_kvcache(q.to(DEV), kg[1:2], vg[1:2], cache_seqlens=cl, causal=causal, window_size=win, softcap=cap, _variant=variant,
                                    num_splits=splits, _params_out=pout)
            d = _describe_softcap(pout[0], cap)
            assert d["form"] == 0 and d["path"] == 0 and d["tiling"] in ((tiling,) if tiling else (1, 4)) and d["nsplit"] == (splits or d["nsplit"]), (what, d)
            out, lse = flash_attn_with_kvcache(q.to(DEV), kg[1:2], vg[1:2], cache_seqlens=cl, causal=causal, window_size=win, softcap=cap, _variant=variant,
                                               num_splits=splits, return_softmax_lse=True)
            torch.cuda.synchronize()
            _check(out, ref64, ref32, dtype, what)
            _check_lse(lse, lse64, what)
        # the chunk's own K/V arrive with the call (k_new / v_new: the append launch in front of the attention launch)
        kg, vg = kc.to(DEV), vc.to(DEV)
        kg[1, c:c + n], vg[1, c:c + n] = 0, 0
        out, lse = flash_attn_with_kvcache(q.to(DEV), kg[1:2], vg[1:2], kc[1:2, c:c + n].to(DEV), vc[1:2, c:c + n].to(DEV),
                                           cache_seqlens=torch.tensor([c], dtype=torch.int32, device=DEV), causal=causal, window_size=win, softcap=cap,
                                           return_softmax_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(kg.cpu(), kc) and torch.equal(vg.cpu(), vc)
        _check(out, ref64, ref32, dtype, "prefill append n%d c%d causal %d left %s" % (n, c, causal, left))
        _check_lse(lse, lse64, "prefill append")


@CAPS
@HEAD_DIMS
@DTYPES
def test_prefill_batched_chunks(dtype, D, cap):
    """the batched form: q_lens = [1, 70, 130] behind 40 / 0 / 200 cached rows, slots through cache_batch_idx; with and without a window,
    the plan's choice and two key-range shares.  The drop-in's batched entry returns no LSE; the C ABI takes softmax_lse beside q_lens
    ([b, h, max(q_lens)], rows beyond an entry's length are not written), so the same block is issued once more through
    vattn_softcap_attn_with_kvcache with an LSE buffer: the same output, and the LSE against the float64 statement."""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    from vattention_amd.flash_attn import flash_attn_varlen_with_kvcache
    Hq, Hkv, qls, cached, idx = 8, 2, [1, 70, 130], [40, 0, 200], [3, 0, 2]
    totals, starts = [a + b for a, b in zip(qls, cached)], [0, 1, 71]
    torch.manual_seed(14)
    q = (4 * torch.randn(sum(qls), Hq, D)).to(dtype)
    kc, vc = torch.randn(4, 340, Hkv, D).to(dtype), torch.randn(4, 340, Hkv, D).to(dtype)
    qpad = torch.zeros(3, max(qls), Hq, D, dtype=dtype)
    for i in range(3):
        qpad[i, :qls[i]] = q[starts[i]:starts[i] + qls[i]]
    t = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    for left in (None, 100):
        ref64, lse64, ref32 = _refs(qpad, kc, vc, cap, cache_seqlens=totals, cache_batch_idx=torch.tensor(idx), q_lens=qls, left=left)
        for splits in (0, 2):
            qg, kg, vg = q.to(DEV), kc.to(DEV), vc.to(DEV)
            out = flash_attn_varlen_with_kvcache(qg, kg, vg, t(starts), t(qls), max(qls), t(totals), t(idx), causal=True,
                                                 window_size=(-1, -1) if left is None else (left, 0), softcap=cap, num_splits=splits)
            torch.cuda.synchronize()
            # the same block through the C ABI with an LSE buffer (pre-set to +inf: rows beyond q_lens[i] stay unwritten)
            p, keep, out2, _dev = FA._build_varlen_block(qg, kg, vg, t(starts), t(qls), max(qls), t(totals), t(idx), None)
            p.is_causal, p.window_left_plus1 = 1, (0 if left is None else left + 1)
            FA._set_scalars(p, qg, splits, None)
            lse = torch.full((3, Hq, max(qls)), float("inf"), dtype=torch.float32, device=DEV)
            p.softmax_lse = lse.data_ptr()
            ws = torch.empty(K.klib().vattn_softcap_attn_workspace_bytes(C.byref(p), cap) // 4 + 1, dtype=torch.float32, device=DEV)
            p.workspace = ws.data_ptr()
            assert K.klib().vattn_softcap_attn_with_kvcache(C.byref(p), cap, K.current_stream_ptr(qg.device)) == 0, K.last_error()
            torch.cuda.synchronize()
            assert torch.equal(out, out2)
            _check_lse(lse, lse64, "varlen d%d cap %g left %s splits %d" % (D, cap, left, splits))
            for i in range(3):
                _check(out[starts[i]:starts[i] + qls[i]].unsqueeze(0), ref64[i:i + 1, :qls[i]], ref32[i:i + 1, :qls[i]], dtype,
                       "varlen entry %d d%d cap %g left %s splits %d" % (i, D, cap, left, splits))


# ---- the window's no-read contract holds under a cap ----

def test_no_read_contract_decode_with_a_cap():
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(4)
    Hq, Hkv, D, left, cap = 8, 2, 128, 100, 30.0
    lens = [700, 90, 333]
    B, rows = len(lens), 701
    kc, vc = torch.randn(B, rows, Hkv, D, device=DEV).half(), torch.randn(B, rows, Hkv, D, device=DEV).half()
    q, kn, vn = (4 * torch.randn(B, 1, Hq, D, device=DEV)).half(), torch.randn(B, 1, Hkv, D, device=DEV).half(), torch.randn(B, 1, Hkv, D, device=DEV).half()
    clg = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kp, vp = kc.clone(), vc.clone()
    for b in range(B):
        dead = first_visible_key(1, lens[b] + 1, left) // 32 * 32          # T = 32
        kp[b, :dead], vp[b, :dead] = float("nan"), float("inf")
    assert bool(torch.isnan(kp).any())
    for splits in (0, 4, -5):
        a = flash_attn_with_kvcache(q, kc.clone(), vc.clone(), kn, vn, cache_seqlens=clg, causal=True, window_size=(left, 0), softcap=cap, num_splits=splits)
        p = flash_attn_with_kvcache(q, kp.clone(), vp.clone(), kn, vn, cache_seqlens=clg, causal=True, window_size=(left, 0), softcap=cap, num_splits=splits)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "splits=%d" % splits
    plain = flash_attn_with_kvcache(q, kc.clone(), vc.clone(), kn, vn, cache_seqlens=clg, causal=True, window_size=(left, 0))
    assert not torch.equal(plain, a)


@pytest.mark.parametrize("variant", [2, 8, 0], ids=["w8", "w4", "default"])
def test_no_read_contract_prefill_with_a_cap(variant):
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(5)
    Hq, Hkv, D, left, cap = 8, 2, 128, 100, 30.0
    for n, c in ((300, 400), (64, 700)):
        kc, vc = torch.randn(1, c + n, Hkv, D, device=DEV).half(), torch.randn(1, c + n, Hkv, D, device=DEV).half()
        q = (4 * torch.randn(1, n, Hq, D, device=DEV)).half()
        dead = first_visible_key(n, c + n, left) // 64 * 64                # T = 64
        assert dead > 0
        kp, vp = kc.clone(), vc.clone()
        kp[0, :dead], vp[0, :dead] = float("nan"), float("inf")
        for splits in (0, 2):
            a = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=c + n, causal=True, window_size=(left, 0), softcap=cap, _variant=variant, num_splits=splits)
            p = flash_attn_with_kvcache(q, kp, vp, cache_seqlens=c + n, causal=True, window_size=(left, 0), softcap=cap, _variant=variant, num_splits=splits)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "n=%d c=%d splits=%d" % (n, c, splits)


# ---- delegation, refusals ----

def test_softcap_zero_through_the_new_entry_is_the_plain_call():
    from vattention_amd import kernels as K
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(7)
    for Sq, lens in ((1, [1, 33, 300]), (4, [3, 70, 300]), (300, [300, 300, 300])):
        q = (4 * torch.randn(3, Sq, 8, 128, device=DEV)).half()
        kc, vc = torch.randn(3, 300, 2, 128, device=DEV).half(), torch.randn(3, 300, 2, 128, device=DEV).half()
        pout = []
        plain = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=True, _params_out=pout)
        p, again = pout[0], torch.full_like(plain, float("nan"))
        p.out = again.data_ptr()
        assert K.klib().vattn_softcap_attn_with_kvcache(C.byref(p), 0.0, K.current_stream_ptr(q.device)) == 0, K.last_error()
        torch.cuda.synchronize()
        assert torch.equal(plain, again), Sq
        assert torch.equal(plain, flash_attn_with_kvcache(q, kc, vc, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=True, softcap=0.0))


def test_refusals_name_their_rule_and_leave_nothing_behind():
    from vattention_amd.flash_attn import flash_attn_func, flash_attn_with_kvcache
    torch.manual_seed(8)
    q = (4 * torch.randn(2, 1, 8, 128, device=DEV)).half()
    qp = (4 * torch.randn(2, 300, 8, 128, device=DEV)).half()
    kc, vc = torch.randn(2, 400, 2, 128, device=DEV).half(), torch.randn(2, 400, 2, 128, device=DEV).half()
    cl = torch.tensor([400, 77], dtype=torch.int32, device=DEV)
    table = torch.randn(512, 128, device=DEV).half()
    before = [flash_attn_with_kvcache(x, kc, vc, cache_seqlens=cl, causal=True).clone() for x in (q, qp)]
    for x in (q, qp):
        with pytest.raises(NotImplementedError, match="rotary"):
            flash_attn_with_kvcache(x, kc, vc, cache_seqlens=cl, causal=True, softcap=30.0, _rotary_cos_sin=table)
    with pytest.raises(NotImplementedError, match="tiling 7"):
        flash_attn_with_kvcache(qp, kc, vc, cache_seqlens=cl, causal=True, softcap=30.0, _variant=14)
    q256, k256 = torch.randn(1, 1, 4, 256, device=DEV).half(), torch.randn(1, 64, 4, 256, device=DEV).half()
    with pytest.raises(NotImplementedError, match="head dimensions"):
        flash_attn_with_kvcache(q256, k256, k256, cache_seqlens=64, softcap=30.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="softcap"):
            flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cl, softcap=bad)
    with pytest.raises(NotImplementedError, match="alibi"):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cl, softcap=30.0, alibi_slopes=torch.ones(8, device=DEV))
    with pytest.raises(NotImplementedError, match="leftpad"):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cl, softcap=30.0, cache_leftpad=torch.zeros(2, dtype=torch.int32, device=DEV))
    after = [flash_attn_with_kvcache(x, kc, vc, cache_seqlens=cl, causal=True) for x in (q, qp)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    # flash_attn_func carries the cap too
    k, v = kc[:, :300].contiguous(), vc[:, :300].contiguous()
    ref64, _, ref32 = _refs(qp.cpu(), k.cpu(), v.cpu(), 30.0)
    _check(flash_attn_func(qp, k, v, causal=True, softcap=30.0), ref64, ref32, torch.float16, "flash_attn_func")


# ---- the Gemma-2 recipe: d = 128 GQA, cap 50, window 4095 ----

def test_gemma2_recipe_decode_and_chunked_prefill():
    """flash_attn_with_kvcache(..., softcap=50.0, window_size=(4095, 0)) on 32 / 16 heads of d = 128 (Gemma-2-27B's attention shape on a
    short context: the window is wider than these caches and the library drops it, as flash_api.cpp:1380 does) and with left = 255, which binds"""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    Hq, Hkv, D, cap = 32, 16, 128, 50.0
    torch.manual_seed(9)
    lens = [700, 90]
    q = (6 * torch.randn(2, 1, Hq, D)).half()
    kc, vc = torch.randn(2, 700, Hkv, D).half(), torch.randn(2, 700, Hkv, D).half()
    qp = (6 * torch.randn(1, 200, Hq, D)).half()
    for left in (4095, 255):
        eff = None if left >= 700 else left
        ref64, _, ref32 = _refs(q, kc, vc, cap, cache_seqlens=lens, left=eff)
        out = flash_attn_with_kvcache(q.to(DEV), kc.to(DEV), vc.to(DEV), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV), causal=True,
                                      softcap=cap, window_size=(left, 0))
        _check(out, ref64, ref32, torch.float16, "gemma-2 decode left %d" % left)
        ref64, _, ref32 = _refs(qp, kc[:1], vc[:1], cap, cache_seqlens=700, left=eff)
        out = flash_attn_with_kvcache(qp.to(DEV), kc[:1].to(DEV), vc[:1].to(DEV), cache_seqlens=700, causal=True, softcap=cap, window_size=(left, 0))
        _check(out, ref64, ref32, torch.float16, "gemma-2 chunk left %d" % left)


# ---- wrapper ----

def test_wrapper_set_logit_softcap_with_a_sliding_window():
    """set_logit_softcap(30.0) together with set_sliding_window(100) on the plain wrapper over a small replay (two prompts, one chunked, then
    decode steps) of a TWO-layer model — layer 1's decode call is layer 0's parameter block re-issued with other pointers (flash_attn.relaunch),
    which must carry the cap too — every layer step by step against the helper; a rotary table and a cap exclude each other in either order."""
    from vattention_amd.attention import get_attention_wrapper, set_attention_backend
    from vattention_amd.replay import ModelConfig, ParallelConfig
    from tests.wrapper_schedule import MD, Seq
    Hq, Hkv, D, ctx, left, cap = 8, 2, 128, 1024, 100, 30.0
    dev = torch.device(DEV)
    from vattention_amd import flash_attn as FA
    L = 2
    model = ModelConfig(name="tiny", num_layers=L, num_q_heads=Hq, num_kv_heads=Hkv, head_size=D, dtype=torch.float16, max_model_len=ctx)
    set_attention_backend("fa_vattn")
    w = get_attention_wrapper()
    w.init(model, ParallelConfig(1, 1), 0, dev)
    table = torch.randn(ctx, D, device=dev).half()
    relaunched, real_relaunch = [], FA.relaunch

    def counting_relaunch(p, *a, **kw):
        relaunched.append(getattr(p, "_softcap", None))
        return real_relaunch(p, *a, **kw)
    FA.relaunch = counting_relaunch
    try:
        w.set_logit_softcap(cap)
        assert w.logit_softcap == cap
        with pytest.raises(ValueError, match="softcap"):
            w.set_fused_rotary(table)
        w.set_logit_softcap(None)
        w.set_fused_rotary(table)
        with pytest.raises(ValueError, match="rotary"):
            w.set_logit_softcap(cap)
        w.set_fused_rotary(None)
        with pytest.raises(ValueError, match="softcap"):
            w.set_logit_softcap(-1.0)
        w.set_logit_softcap(cap)
        w.set_sliding_window(left)
        torch.manual_seed(6)
        caches = [(torch.zeros(4, ctx, Hkv, D, dtype=torch.float16, device=dev), torch.zeros(4, ctx, Hkv, D, dtype=torch.float16, device=dev)) for _ in range(L)]
        a, b = Seq(0, 300, 310), Seq(1, 50, 60)
        plan = [([MD(a, 170, True)], [1], []), ([MD(a, 130, True), MD(b, 50, True)], [1, 3], [])] + [([MD(a, 0, False), MD(b, 0, False)], [], [1, 3])] * 2
        for mds, sp, sd_ in plan:
            T = sum(m.seq.get_next_prompt_chunk_len(m.prompt_chunk_len) if m.is_prompt else 1 for m in mds)
            qkv = [((4 * torch.randn(T, Hq * D, device=dev)).half(), torch.randn(T, Hkv * D, device=dev).half(), torch.randn(T, Hkv * D, device=dev).half()) for _ in range(L)]
            w.begin_forward(mds)
            w.set_batch_idx(torch.tensor(sp + sd_, dtype=torch.int32, device=dev), torch.tensor(sd_, dtype=torch.int32, device=dev))
            outs = [w.forward(*qkv[l], caches[l], D ** -0.5, l) for l in range(L)]
            w.end_forward()
            torch.cuda.synchronize()
            for l in range(L):
                tok, kh, vh = 0, caches[l][0].cpu(), caches[l][1].cpu()
                for m, slot in zip(mds, sp + sd_):
                    nq = m.seq.get_next_prompt_chunk_len(m.prompt_chunk_len) if m.is_prompt else 1
                    vis = (m.seq.prompt_processed + nq) if m.is_prompt else m.seq.get_len()
                    qi = qkv[l][0][tok:tok + nq].view(1, nq, Hq, D).cpu()
                    ref64, _, ref32 = _refs(qi, kh[slot:slot + 1], vh[slot:slot + 1], cap, left=left, cache_seqlens=vis)
                    _check(outs[l][tok:tok + nq].view(1, nq, Hq, D), ref64, ref32, torch.float16,
                           "wrapper layer %d %s seq %d" % (l, "prefill" if m.is_prompt else "decode", m.seq.seq_id))
                    tok += nq
            for m in mds:
                if m.is_prompt:
                    m.seq.prompt_processed += m.seq.get_next_prompt_chunk_len(m.prompt_chunk_len)
                    if m.seq.prompt_done:
                        m.seq.output_len += 1
                else:
                    m.seq.output_len += 1
        # the two decode iterations re-issued layer 0's block for layer 1, and the block carried the cap
        assert relaunched == [cap, cap], relaunched
    finally:
        FA.relaunch = real_relaunch
        w.set_fused_rotary(None)
        w.set_logit_softcap(None)
        w.set_sliding_window(None)
