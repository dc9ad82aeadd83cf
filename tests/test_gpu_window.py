"""GPU parity of causal sliding-window attention (window_size=(left, right)) through the Python drop-in — and therefore the C ABI — of
the PRODUCT library, against tests/window_ref.py (checked against the oracle in tests/test_window_ref.py).

Tolerances are the project's (tests/test_gpu_attention.py), restated: fp16/bf16 I/O against float64 at atol = rtol = 2e-3
(fp16) / 1.6e-2 (bf16), AND the kernel's max error within 2 x the error of the reference-numerics CPU run (fp32 accumulate, P rounded to
the I/O dtype) + 1e-5 (+ 4e-3 for bf16, as there).  LSE (fp32 on both sides, values of a few units): 2e-3 absolute.

The no-read contract (include/vattn_kernels.h) is checked by POISONING values — K rows NaN, V rows Inf below align_down(first key visible to
the entry's first query, T), T = 32 decode / 64 prefill — not by unmapping anything: outputs must be finite and torch.equal to the same call
on ordinary data in those rows."""
import pytest
import torch

from tests.window_ref import first_visible_key, window_attn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def _refs(q, kc, vc, left, **kw):
    return window_attn_ref(q, kc, vc, left, math="f64", **kw), window_attn_ref(q, kc, vc, left, math="f32", **kw)


def _describe(p):
    from vattention_amd import kernels as K
    return K.describe(p)


# ---- decode ----

DECODE_SHAPES = [                         # the shape list of tests/test_gpu_attention.py::test_decode_parity
    (1, 8, 4, [777]),
    (3, 4, 2, [1, 31, 1025]),
    (2, 7, 1, [5000, 63]),
    (4, 1, 2, [300, 2, 4095, 64]),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,G,Hkv,lens", DECODE_SHAPES)
def test_decode_window_parity(B, G, Hkv, lens, dtype):
    """left in {0, 1, 31, 32, 33, 1000, max len, view rows}, with and without the fused one-row append, cache_batch_idx, the default
    (device-planned stream, or one-sequence split) launch, forced split counts (decode_kernel) and forced stream grids; LSE where returned.
    left >= the view's rows is the window-less call by the argument rules (bit-equal); left = max len covers every key through the
    windowed kernels: within tolerance always, bit-equal whenever the host sizes both launches alike."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(1234)
    Hq, D, ctx, slots = G * Hkv, 128, 6000, 7
    kc = torch.randn(slots, ctx, Hkv, D).to(dtype)
    vc = torch.randn(slots, ctx, Hkv, D).to(dtype)
    q = torch.randn(B, 1, Hq, D).to(dtype)
    kn = torch.randn(B, 1, Hkv, D).to(dtype)
    vn = torch.randn(B, 1, Hkv, D).to(dtype)
    idx = torch.tensor([5, 0, 3, 6][:B], dtype=torch.int32)
    cl = torch.tensor(lens, dtype=torch.int32)
    rows = max(lens) + 1
    kca, vca = kc.clone(), vc.clone()          # the caches after the append
    for b in range(B):
        kca[idx[b], lens[b]], vca[idx[b], lens[b]] = kn[b, 0], vn[b, 0]
    qg, kng, vng, clg, idg = q.to(DEV), kn.to(DEV), vn.to(DEV), cl.to(DEV), idx.to(DEV)
    for append in (True, False):
        vis = [n + 1 for n in lens] if append else lens
        ck, cv = (kca, vca) if append else (kc, vc)
        new = (kng, vng) if append else (None, None)
        kg, vg = kc.to(DEV), vc.to(DEV)
        full = flash_attn_with_kvcache(qg, kg.clone()[:, :rows], vg.clone()[:, :rows], *new, cache_seqlens=clg, cache_batch_idx=idg, causal=True)
        for left in (0, 1, 31, 32, 33, 1000, max(lens), rows):
            ref64, lse64 = window_attn_ref(q, ck[:, :rows], cv[:, :rows], left, cache_seqlens=vis, cache_batch_idx=idx, return_lse=True)
            ref32 = window_attn_ref(q, ck[:, :rows], cv[:, :rows], left, cache_seqlens=vis, cache_batch_idx=idx, math="f32")
            for splits in (0, 1, 3, -2, -37):
                kgi, vgi = kg.clone(), vg.clone()
                pout = []
                out = flash_attn_with_kvcache(qg, kgi[:, :rows], vgi[:, :rows], *new, cache_seqlens=clg, cache_batch_idx=idg, causal=True,
                                              window_size=(left, 0), num_splits=splits, _params_out=pout)
                torch.cuda.synchronize()
                what = "decode left=%d append=%s splits=%d" % (left, append, splits)
                _check(out, ref64, ref32, dtype, what)
                assert pout[0].window_left_plus1 == (left + 1 if left < rows else 0)
                if append:
                    assert torch.equal(kgi.cpu(), kca) and torch.equal(vgi.cpu(), vca), what      # in-place append, nothing else touched
                if splits == 0 and left >= max(vis):
                    pfull = []
                    flash_attn_with_kvcache(qg, kgi[:, :rows], vgi[:, :rows], *new, cache_seqlens=clg, cache_batch_idx=idg, causal=True, _params_out=pfull)
                    if left >= rows or _describe(pout[0]) == _describe(pfull[0]):
                        assert torch.equal(out, full), what + ": a window over the whole sequence is the window-less call"
            if not append:
                out, lse = flash_attn_with_kvcache(qg, kg[:, :rows], vg[:, :rows], cache_seqlens=clg, cache_batch_idx=idg, causal=True,
                                                   window_size=(left, -1), return_softmax_lse=True)
                torch.cuda.synchronize()
                _check(out, ref64, ref32, dtype, "decode+lse left=%d" % left)
                assert (lse[:, :, 0].double().cpu() - lse64[:, :, 0]).abs().max().item() < 2e-3, "lse left=%d" % left


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,G,Hkv,D,lens", [(2, 71, 1, 64, [2500, 300]), (4, 17, 2, 64, [1000, 1, 64, 333]), (2, 40, 1, 128, [3000, 777]), (3, 8, 2, 64, [5000, 17, 900])],
                         ids=["falcon_g71_d64", "g17_d64", "g40", "d64_ragged"])
def test_decode_window_head_dim_64_and_wide_groups(B, G, Hkv, D, lens, dtype):
    """d = 64 and the head-block-group launches (G > 16: decode_kernel, two 16-head blocks per workgroup), with the fused append."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(B * 131 + G)
    Hq, ctx, slots = G * Hkv, max(lens) + 40, B + 2
    kc, vc = torch.randn(slots, ctx, Hkv, D).to(dtype), torch.randn(slots, ctx, Hkv, D).to(dtype)
    q, kn, vn = torch.randn(B, 1, Hq, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype)
    idx = torch.randperm(slots)[:B].to(torch.int32)
    rows = max(lens) + 1
    kca, vca = kc.clone(), vc.clone()
    for b in range(B):
        kca[idx[b], lens[b]], vca[idx[b], lens[b]] = kn[b, 0], vn[b, 0]
    for left in (0, 33, 100, 1000):
        ref64, ref32 = _refs(q, kca[:, :rows], vca[:, :rows], left, cache_seqlens=[n + 1 for n in lens], cache_batch_idx=idx)
        for splits in (0, 5):
            kg, vg = kc.to(DEV), vc.to(DEV)
            out = flash_attn_with_kvcache(q.to(DEV), kg[:, :rows], vg[:, :rows], kn.to(DEV), vn.to(DEV), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV),
                                          cache_batch_idx=idx.to(DEV), causal=True, window_size=(left, 0), num_splits=splits)
            torch.cuda.synchronize()
            _check(out, ref64, ref32, dtype, "decode d=%d G=%d left=%d splits=%d" % (D, G, left, splits))
            assert torch.equal(kg.cpu(), kca) and torch.equal(vg.cpu(), vca)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_decode_window_with_fused_rope(dtype):
    """q and the appended k are rotated in the launch (positions = the tokens' own, the window does not move them); oracle = rotate first."""
    from oracle.attn import make_cos_sin_cache, rotary_embedding_ref
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(21)
    B, Hq, Hkv, D, ctx = 3, 8, 2, 128, 2048
    lens = [1500, 40, 700]
    cs = make_cos_sin_cache(D, ctx, dtype=dtype)
    kc, vc = torch.randn(B, ctx, Hkv, D).to(dtype), torch.randn(B, ctx, Hkv, D).to(dtype)
    q, kn, vn = torch.randn(B, 1, Hq, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype)
    qr, kr = q.clone().view(B, Hq * D), kn.clone().view(B, Hkv * D)
    rotary_embedding_ref(torch.tensor(lens, dtype=torch.int64), qr, kr, D, cs)
    kca, vca = kc.clone(), vc.clone()
    for b in range(B):
        kca[b, lens[b]], vca[b, lens[b]] = kr.view(B, Hkv, D)[b], vn[b, 0]
    rows = max(lens) + 1
    for left in (33, 600):
        ref64, ref32 = _refs(qr.view(B, 1, Hq, D), kca[:, :rows], vca[:, :rows], left, cache_seqlens=[n + 1 for n in lens])
        kg, vg = kc.to(DEV), vc.to(DEV)
        out = flash_attn_with_kvcache(q.to(DEV), kg[:, :rows], vg[:, :rows], kn.to(DEV), vn.to(DEV), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV),
                                      causal=True, window_size=(left, 0), _rotary_cos_sin=cs.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(kg.cpu(), kca), "the rotated appended key rows"
        _check(out, ref64, ref32, dtype, "decode rope left=%d" % left)


@pytest.mark.parametrize("Hkv", [1, 4])
def test_decode_window_ragged_batch(Hkv):
    """Some sequences shorter than the window, some 30 x longer: the device plan distributes VISIBLE tiles."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(8)
    G, D, left = 4, 128, 1023
    lens = [31000, 200, 1024, 30000, 1023, 5, 1025, 12000, 999, 31744]
    B, Hq, rows = len(lens), G * Hkv, max(lens) + 1
    kc, vc = torch.randn(B, rows, Hkv, D).half(), torch.randn(B, rows, Hkv, D).half()
    q = torch.randn(B, 1, Hq, D).half()
    ref64, ref32 = _refs(q, kc, vc, left, cache_seqlens=lens)
    kg, vg, clg = kc.to(DEV), vc.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    for splits in (0, -3, -100):
        out = flash_attn_with_kvcache(q.to(DEV), kg, vg, cache_seqlens=clg, causal=True, window_size=(left, 0), num_splits=splits)
        torch.cuda.synchronize()
        _check(out, ref64, ref32, torch.float16, "ragged decode splits=%d" % splits)


# ---- prefill ----

def _prefill_case(n, c, Hq, Hkv, D, dtype, seed=0, slots=2, slack=9):
    torch.manual_seed(seed + n + c)
    kc, vc = torch.randn(slots, c + n + slack, Hkv, D).to(dtype), torch.randn(slots, c + n + slack, Hkv, D).to(dtype)
    q = torch.randn(1, n, Hq, D).to(dtype)
    return q, kc, vc


# variant: 14 = prefill64_kernel (tiling 7), 2 = prefill_kernel 8 waves (tiling 1), 8 = prefill_kernel 4 waves (tiling 4)
@pytest.mark.parametrize("variant,tiling", [(14, 7), (2, 1), (8, 4)], ids=["prefill64", "w8", "w4"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("n,c", [(777, 0), (300, 1500), (1100, 900)], ids=["whole_prompt", "chunk_lt_left_and_gt", "chunk_vs_cache"])
def test_prefill_window_parity(n, c, dtype, variant, tiling):
    """Whole prompt and chunk against a longer cache on the explicit tilings (asserted through vattn_attn_plan_describe), left on / off
    tile and block boundaries and below / above the chunk length; every row checked.  Forced key-range shares (KV-split + merge) too."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    Hq, Hkv, D = 8, 2, 128
    q, kc, vc = _prefill_case(n, c, Hq, Hkv, D, dtype)
    kg, vg = kc.to(DEV), vc.to(DEV)
    cl = torch.tensor([c + n], dtype=torch.int32, device=DEV)
    for left in (0, 63, 64, 65, 255, 256, 257, 1000, c + n - 1):
        ref64, lse64 = window_attn_ref(q, kc[1:2], vc[1:2], left, cache_seqlens=c + n, return_lse=True)
        ref32 = window_attn_ref(q, kc[1:2], vc[1:2], left, cache_seqlens=c + n, math="f32")
        for splits in (0, 3):
            pout = []
            out = flash_attn_with_kvcache(q.to(DEV), kg[1:2], vg[1:2], cache_seqlens=cl, causal=True, window_size=(left, 0), _variant=variant,
                                          num_splits=splits, _params_out=pout)
            torch.cuda.synchronize()
            d = _describe(pout[0])
            # (left >= the view's rows — 1000 on the 777-token prompt — is "no window" by the argument rules)
            assert d["form"] == 0 and d["path"] == 0 and d["tiling"] == tiling and pout[0].window_left_plus1 == (left + 1 if left < kc.shape[1] else 0), d
            if splits:
                assert d["nsplit"] == 3 and d["merge_launch"] == 1
            _check(out, ref64, ref32, dtype, "prefill tiling %d left=%d n=%d c=%d splits=%d" % (d["tiling"], left, n, c, splits))
        out, lse = flash_attn_with_kvcache(q.to(DEV), kg[1:2], vg[1:2], cache_seqlens=cl, causal=True, window_size=(left, 0), _variant=variant,
                                           return_softmax_lse=True)
        torch.cuda.synchronize()
        assert (lse.double().cpu() - lse64).abs().max().item() < 2e-3, "lse left=%d" % left
    # a window over the whole sequence: the window-less launch, bit for bit (the same tiling through the windowed build)
    full = flash_attn_with_kvcache(q.to(DEV), kg[1:2], vg[1:2], cache_seqlens=cl, causal=True, _variant=variant)
    wide = flash_attn_with_kvcache(q.to(DEV), kg[1:2], vg[1:2], cache_seqlens=cl, causal=True, window_size=(c + n, 0), _variant=variant)
    torch.cuda.synchronize()
    assert torch.equal(full, wide)


@pytest.mark.parametrize("Hq,Hkv,n,c,left,want", [(32, 4, 4096, 0, 1500, 7), (32, 4, 2048, 0, 100, 4), (8, 2, 600, 3000, 300, None), (71, 1, 500, 100, 65, None)],
                         ids=["plan_prefill64", "plan_w4", "plan_chunk", "d64_mqa"])
def test_prefill_window_default_plan(Hq, Hkv, n, c, left, want):
    """The launches the PLAN chooses for a windowed block (not assumed: read from vattn_attn_plan_describe), d = 128 and d = 64."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    D = 64 if Hkv == 1 else 128
    q, kc, vc = _prefill_case(n, c, Hq, Hkv, D, torch.float16, seed=3)
    ref64, ref32 = _refs(q, kc[:1], vc[:1], left, cache_seqlens=c + n)
    pout = []
    out = flash_attn_with_kvcache(q.to(DEV), kc[:1].to(DEV), vc[:1].to(DEV), cache_seqlens=c + n, causal=True, window_size=(left, 0), _params_out=pout)
    torch.cuda.synchronize()
    d = _describe(pout[0])
    assert d["path"] == 0 and (want is None or d["tiling"] == want), d
    _check(out, ref64, ref32, torch.float16, "prefill default plan %s" % d)


@pytest.mark.parametrize("variant", [0, 14, 2], ids=["default", "prefill64", "w8"])
def test_prefill_window_batched_variable_length(variant):
    """flash_attn_varlen_with_kvcache: chunks of very different lengths, one launch, one window."""
    from vattention_amd.flash_attn import flash_attn_varlen_with_kvcache
    torch.manual_seed(17)
    Hq, Hkv, D, left = 8, 2, 128, 200
    qls, cls = [700, 3, 260, 1500], [100, 900, 0, 2000]
    B, ctx = len(qls), 3600
    kc, vc = torch.randn(B + 1, ctx, Hkv, D).half(), torch.randn(B + 1, ctx, Hkv, D).half()
    idx = torch.tensor([4, 0, 2, 1], dtype=torch.int32)
    q = torch.randn(sum(qls), Hq, D).half()
    starts = [sum(qls[:i]) for i in range(B)]
    totals = [a + b for a, b in zip(qls, cls)]
    for splits in (0, 2):
        out = flash_attn_varlen_with_kvcache(q.to(DEV), kc.to(DEV), vc.to(DEV), torch.tensor(starts, dtype=torch.int32, device=DEV),
                                             torch.tensor(qls, dtype=torch.int32, device=DEV), max(qls), torch.tensor(totals, dtype=torch.int32, device=DEV),
                                             idx.to(DEV), causal=True, window_size=(left, 0), _variant=variant, num_splits=splits)
        torch.cuda.synchronize()
        for i in range(B):
            qi = q[starts[i]:starts[i] + qls[i]].unsqueeze(0)
            s = int(idx[i])
            ref64, ref32 = _refs(qi, kc[s:s + 1], vc[s:s + 1], left, cache_seqlens=totals[i])
            _check(out[starts[i]:starts[i] + qls[i]].unsqueeze(0), ref64, ref32, torch.float16, "varlen entry %d variant %d splits %d" % (i, variant, splits))


# ---- the no-read contract ----

def test_no_read_contract_decode():
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(4)
    Hq, Hkv, D, left = 8, 2, 128, 500
    lens = [3000, 400, 1777, 6000]
    B, rows = len(lens), 6001
    kc, vc = torch.randn(B, rows, Hkv, D, device=DEV).half(), torch.randn(B, rows, Hkv, D, device=DEV).half()
    q, kn, vn = torch.randn(B, 1, Hq, D, device=DEV).half(), torch.randn(B, 1, Hkv, D, device=DEV).half(), torch.randn(B, 1, Hkv, D, device=DEV).half()
    clg = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kp, vp = kc.clone(), vc.clone()
    for b in range(B):
        dead = first_visible_key(1, lens[b] + 1, left) // 32 * 32          # T = 32
        kp[b, :dead], vp[b, :dead] = float("nan"), float("inf")
    assert bool(torch.isnan(kp).any())
    for splits in (0, 4, -5):
        a = flash_attn_with_kvcache(q, kc.clone(), vc.clone(), kn, vn, cache_seqlens=clg, causal=True, window_size=(left, 0), num_splits=splits)
        p = flash_attn_with_kvcache(q, kp.clone(), vp.clone(), kn, vn, cache_seqlens=clg, causal=True, window_size=(left, 0), num_splits=splits)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "splits=%d" % splits


@pytest.mark.parametrize("variant", [14, 2, 8, 0], ids=["prefill64", "w8", "w4", "default"])
def test_no_read_contract_prefill(variant):
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(5)
    Hq, Hkv, D, left = 8, 2, 128, 333
    for n, c in ((900, 2100), (2500, 0), (64, 5000)):
        kc, vc = torch.randn(1, c + n, Hkv, D, device=DEV).half(), torch.randn(1, c + n, Hkv, D, device=DEV).half()
        q = torch.randn(1, n, Hq, D, device=DEV).half()
        dead = first_visible_key(n, c + n, left) // 64 * 64                # T = 64
        kp, vp = kc.clone(), vc.clone()
        kp[0, :dead], vp[0, :dead] = float("nan"), float("inf")
        for splits in (0, 2):
            a = flash_attn_with_kvcache(q, kc, vc, cache_seqlens=c + n, causal=True, window_size=(left, 0), _variant=variant, num_splits=splits)
            p = flash_attn_with_kvcache(q, kp, vp, cache_seqlens=c + n, causal=True, window_size=(left, 0), _variant=variant, num_splits=splits)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(p).all()) and torch.equal(a, p), "n=%d c=%d splits=%d" % (n, c, splits)


# ---- full size ----

def test_full_size_decode_yi6b_b16_32k():
    """Yi-6B (32 / 4 heads), 16 sequences at 32 k, left = 4 095: every sequence against the helper."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(1)
    B, Hq, Hkv, D, L, left = 16, 32, 4, 128, 32767, 4095
    kc, vc = torch.randn(B, L + 1, Hkv, D).half(), torch.randn(B, L + 1, Hkv, D).half()
    q, kn, vn = torch.randn(B, 1, Hq, D).half(), torch.randn(B, 1, Hkv, D).half(), torch.randn(B, 1, Hkv, D).half()
    kg, vg = kc.to(DEV), vc.to(DEV)
    out = flash_attn_with_kvcache(q.to(DEV), kg, vg, kn.to(DEV), vn.to(DEV), cache_seqlens=torch.full((B,), L, dtype=torch.int32, device=DEV),
                                  causal=True, window_size=(left, 0))
    torch.cuda.synchronize()
    kc[:, L], vc[:, L] = kn[:, 0], vn[:, 0]
    ref64, ref32 = _refs(q, kc, vc, left, cache_seqlens=L + 1)
    _check(out, ref64, ref32, torch.float16, "Yi-6B B16 @ 32k left 4095")


def test_full_size_prefill_32702_tokens():
    """The 32 702-token prompt (Yi-6B heads), left = 4 095, prefill64 by the plan.  Sampled rows, ALL heads: every 16th 256-row query block
    (and the blocks that hold rows left - 1, left, left + 1 and the last row) in full — their first and last rows included — plus rows 0,
    left - 1, left, left + 1 and the last row: > 2 048 rows per head."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    torch.manual_seed(2)
    n, Hq, Hkv, D, left = 32702, 32, 4, 128, 4095
    kc, vc = torch.randn(1, n, Hkv, D).half(), torch.randn(1, n, Hkv, D).half()
    q = torch.randn(1, n, Hq, D).half()
    pout = []
    out = flash_attn_with_kvcache(q.to(DEV), kc.to(DEV), vc.to(DEV), cache_seqlens=n, causal=True, window_size=(left, 0), _params_out=pout)
    torch.cuda.synchronize()
    d = _describe(pout[0])
    assert (d["path"], d["tiling"], d["nsplit"]) == (0, 7, 1), d
    blocks = sorted(set(list(range(0, (n + 255) // 256, 16)) + [(left - 1) // 256, left // 256, (left + 1) // 256, (n - 1) // 256]))
    rows = sorted(set(r for b in blocks for r in range(b * 256, min(n, b * 256 + 256))) | {0, left - 1, left, left + 1, n - 1})
    assert len(rows) >= 2048
    rows = torch.tensor(rows)
    ref64, ref32 = _refs(q, kc, vc, left, cache_seqlens=n, rows=rows)
    _check(out[:, rows.to(DEV)], ref64, ref32, torch.float16, "32702-token prompt left 4095 (%d sampled rows)" % rows.numel())


# ---- wrapper and the product hybrid entry ----

def test_wrapper_set_sliding_window():
    """set_sliding_window(left) on the plain wrapper over a small replay (two prompts, one chunked, then decode steps) against the helper;
    None leaves the outputs torch.equal to a wrapper that never heard of it."""
    from vattention_amd.attention import get_attention_wrapper, set_attention_backend
    from vattention_amd.replay import ModelConfig, ParallelConfig
    from tests.wrapper_schedule import MD, Seq
    Hq, Hkv, D, ctx, left = 8, 2, 128, 1024, 100
    dev = torch.device(DEV)
    model = ModelConfig(name="tiny", num_layers=1, num_q_heads=Hq, num_kv_heads=Hkv, head_size=D, dtype=torch.float16, max_model_len=ctx)
    set_attention_backend("fa_vattn")
    w = get_attention_wrapper()
    w.init(model, ParallelConfig(1, 1), 0, dev)
    outs = {}
    for mode in ("never", "window", "none"):
        if mode == "window":
            w.set_sliding_window(left)
        elif mode == "none":
            w.set_sliding_window(None)
        torch.manual_seed(6)
        kc = torch.zeros(4, ctx, Hkv, D, dtype=torch.float16, device=dev)
        vc = torch.zeros_like(kc)
        a, b = Seq(0, 300, 310), Seq(1, 50, 60)
        plan = [([MD(a, 170, True)], [1], []), ([MD(a, 130, True), MD(b, 50, True)], [1, 3], [])] + [([MD(a, 0, False), MD(b, 0, False)], [], [1, 3])] * 3
        res = []
        for mds, sp, sd_ in plan:
            T = sum(m.seq.get_next_prompt_chunk_len(m.prompt_chunk_len) if m.is_prompt else 1 for m in mds)
            q = torch.randn(T, Hq * D, device=dev).half()
            k = torch.randn(T, Hkv * D, device=dev).half()
            v = torch.randn(T, Hkv * D, device=dev).half()
            w.begin_forward(mds)
            w.set_batch_idx(torch.tensor(sp + sd_, dtype=torch.int32, device=dev), torch.tensor(sd_, dtype=torch.int32, device=dev))
            out = w.forward(q, k, v, (kc, vc), D ** -0.5, 0)
            w.end_forward()
            torch.cuda.synchronize()
            res.append(out.float().cpu())
            if mode == "window":
                tok, kh, vh = 0, kc.cpu(), vc.cpu()
                for m, slot in zip(mds, sp + sd_):
                    nq = m.seq.get_next_prompt_chunk_len(m.prompt_chunk_len) if m.is_prompt else 1
                    vis = (m.seq.prompt_processed + nq) if m.is_prompt else m.seq.get_len()
                    qi = q[tok:tok + nq].view(1, nq, Hq, D).cpu()
                    ref64, ref32 = _refs(qi, kh[slot:slot + 1], vh[slot:slot + 1], left, cache_seqlens=vis)
                    _check(out[tok:tok + nq].view(1, nq, Hq, D), ref64, ref32, torch.float16, "wrapper %s seq %d" % ("prefill" if m.is_prompt else "decode", m.seq.seq_id))
                    tok += nq
            for m in mds:
                if m.is_prompt:
                    m.seq.prompt_processed += m.seq.get_next_prompt_chunk_len(m.prompt_chunk_len)
                    if m.seq.prompt_done:
                        m.seq.output_len += 1
                else:
                    m.seq.output_len += 1
        outs[mode] = res
    w.set_sliding_window(None)
    assert all(torch.equal(x, y) for x, y in zip(outs["never"], outs["none"]))
    assert any(not torch.equal(x, y) for x, y in zip(outs["never"], outs["window"]))


def test_product_hybrid_entry_with_a_windowed_decode_block():
    """vattn_hybrid_attn of the product library (the plan-chosen prefill launch, then the decode launch) with a window on both blocks."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache, hybrid_attn
    torch.manual_seed(5)
    Hq, Hkv, D, ctx, left = 8, 2, 128, 3000, 300
    kc, vc = torch.randn(6, ctx, Hkv, D).half(), torch.randn(6, ctx, Hkv, D).half()
    T, c = 700, 1500
    q = torch.randn(T + 4, Hq, D).half()
    kn, vn = torch.randn(4, 1, Hkv, D).half(), torch.randn(4, 1, Hkv, D).half()
    dlens, di = [2500, 31, 900, 1777], torch.tensor([1, 2, 4, 5], dtype=torch.int32)
    kg, vg, qg = kc.to(DEV), vc.to(DEV), q.to(DEV)
    out = torch.zeros_like(qg)
    pre = lambda: flash_attn_with_kvcache(qg[:T].unsqueeze(0), kg[0:1], vg[0:1], cache_seqlens=torch.tensor([c + T], dtype=torch.int32, device=DEV),
                                          causal=True, window_size=(left, 0), out=out[:T].unsqueeze(0))
    dec = lambda: flash_attn_with_kvcache(qg[T:].unsqueeze(1), kg[:, :2501], vg[:, :2501], kn.to(DEV), vn.to(DEV),
                                          cache_seqlens=torch.tensor(dlens, dtype=torch.int32, device=DEV), cache_batch_idx=di.to(DEV), causal=True,
                                          window_size=(left, 0), out=out[T:].unsqueeze(1))
    hybrid_attn(pre, dec, torch.device(DEV), _product=True)
    torch.cuda.synchronize()
    ref64, ref32 = _refs(q[:T].unsqueeze(0), kc[0:1], vc[0:1], left, cache_seqlens=c + T)
    _check(out[:T].unsqueeze(0), ref64, ref32, torch.float16, "hybrid prefill part")
    for b in range(4):
        kc[di[b], dlens[b]], vc[di[b], dlens[b]] = kn[b, 0], vn[b, 0]
    ref64, ref32 = _refs(q[T:].unsqueeze(1), kc[:, :2501], vc[:, :2501], left, cache_seqlens=[n + 1 for n in dlens], cache_batch_idx=di)
    _check(out[T:].unsqueeze(1), ref64, ref32, torch.float16, "hybrid decode part")
