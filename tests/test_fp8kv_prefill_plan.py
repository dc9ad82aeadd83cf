"""Chunked prefill over the FP8 (e4m3) KV cache without a GPU (include/vattn_kernels.h, "Prefill over an fp8 cache"): the C ABI's host side —
exports, the frozen parameter block, the plan (the 2-byte call's without its prefill64 branch) and the gate of
vattn_fp8kv_prefill_with_kvcache / _workspace_bytes / _plan_describe — in the style of tests/test_fp8kv_ref.py (pure host arithmetic of
libvattn_amd.so; fake aligned pointers, nothing is launched: the launching entry point is only ever called with blocks it refuses), and
the yardstick of the GPU tests (tests/fp8kv_ref.py) for the prefill form against a dense float64 softmax written here."""
import ctypes as C
import itertools
import math

import pytest
import torch

from tests.fp8kv_ref import amax_scales, dequantize_ref, fp8kv_attn_ref, quantize_ref
from vattention_amd import kernels as K

SC = C.c_void_p(8192)                                    # a non-NULL device address: the host never dereferences it


def _params(b, sq, sk, h, hk, d=128, causal=1, splits=0, variant=0, knew=0, hint=0):
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = b, sq, sk, knew, h, hk, d
    p.is_causal, p.dtype, p.num_splits, p.variant, p.max_seqlen_k_hint = causal, 0, splits, variant, hint
    return p


def _tensors(p):
    """validate() wants non-null, aligned tensor pointers; nothing is launched and nothing dereferences them (tests/test_fp8kv_ref.py)"""
    p.q = p.out = p.k_cache = p.v_cache = 4096
    p.q_row_stride = p.o_row_stride = p.h * p.d
    p.q_head_stride = p.o_head_stride = p.k_head_stride = p.v_head_stride = p.d
    p.k_row_stride = p.v_row_stride = p.h_k * p.d
    if p.seqlen_knew:
        p.k_new = p.v_new = p.cache_seqlens = 4096
        p.knew_row_stride = p.vnew_row_stride = p.h_k * p.d
        p.knew_head_stride = p.vnew_head_stride = p.d
    return p


def test_new_symbols_are_exported_and_the_block_is_frozen():
    lib = K.klib()
    for name in ("vattn_fp8kv_prefill_with_kvcache", "vattn_fp8kv_prefill_workspace_bytes", "vattn_fp8kv_prefill_plan_describe"):
        assert getattr(lib, name) is not None
    assert K.ABI_VERSION == 6 and C.sizeof(K.AttnParams) == 400
    from vattention_amd import flash_attn as FA
    assert FA.counters["fp8kv_prefill_calls"] >= 0
    assert callable(FA.flash_attn_fp8kv_prefill_with_kvcache) and callable(FA.flash_attn_fp8kv_varlen_with_kvcache) and callable(K.describe_fp8kv_prefill)


def test_plan_is_the_two_byte_call_s_without_prefill64():
    """b x seqlen_q x seqlen_k x heads x d x causal x length hint x forced shares: 2304 blocks, each asked three questions."""
    lib = K.klib()
    n = with_p64 = split = t4 = 0
    for b, sq, sk, (h, hk), d, causal, hinted, splits in itertools.product(
            (1, 2, 4), (9, 100, 256, 1000, 2048, 4096), (4096, 30000, 131072), ((8, 2), (32, 8), (8, 1), (8, 8)), (64, 128), (0, 1), (0, 1), (0, 1, 2, 3)):
        if (n + b + sq) % 3 == 0 and splits in (1, 3):         # (thin the forced counts out: they take one branch)
            n += 1
            continue
        n += 1
        p = _params(b, sq, sk, h, hk, d, causal, splits, hint=(sk * 3) // 4 if hinted else 0)
        f, two = K.describe_fp8kv_prefill(p), K.describe(p)
        assert f["form"] == 0 and f["path"] == 0 and f["tiling"] in (1, 4), (f, two)
        if two["tiling"] != 7:
            assert f == two, (f, two)
        else:
            with_p64 += 1
        ws = int(lib.vattn_fp8kv_prefill_workspace_bytes(C.byref(p)))
        assert ws == f["workspace_bytes"] and (ws == 0) == (f["nsplit"] == 1), f
        assert f["nsplit"] == 1 or ws == f["nsplit"] * b * sq * h * (d + 1) * 4
        assert f["merge_launch"] == (f["nsplit"] > 1) and f["workgroups"] == -(-sq // (128 if f["tiling"] == 4 else 256)) * h * b * f["nsplit"]
        if splits:
            assert f["nsplit"] == splits
        split += f["nsplit"] > 1
        t4 += f["tiling"] == 4
    assert with_p64 > 20 and split > 100 and t4 > 100 and n - t4 > 100, (n, with_p64, split, t4)      # the sweep saw every kind
    # explicit tilings 1 and 4 are honoured
    for til in (1, 4):
        p = _params(2, 1000, 30000, 8, 2, variant=til << 1)
        assert K.describe_fp8kv_prefill(p)["tiling"] == til and K.describe_fp8kv_prefill(p) == K.describe(p)


def test_gate_and_argument_rules_of_the_c_abi():
    lib = K.klib()
    call = lambda p, ks=SC, vs=SC: lib.vattn_fp8kv_prefill_with_kvcache(C.byref(p), ks, vs, None)

    def refused(p, word, rc=-10):
        assert call(p) == rc and word in K.last_error(), K.last_error()
        assert "fp8" in K.last_error()
        assert lib.vattn_fp8kv_prefill_plan_describe(C.byref(p), C.byref(K.PlanDesc())) == rc and word in K.last_error()
        assert lib.vattn_fp8kv_prefill_workspace_bytes(C.byref(p)) == 0

    blk = lambda **kw: _tensors(_params(2, 300, 4096, 8, 2, **kw))
    win = blk()
    win.window_left_plus1 = 101
    refused(win, "window")
    rot = blk()
    rot.rotary_cos_sin, rot.rotary_dim, rot.rotary_row_stride = 4096, 128, 128
    refused(rot, "rotary")
    lst = blk()
    lst.pf_items, lst.num_pf_items = 4096, 4
    refused(lst, "pf_items")
    wg = blk()
    wg.pf_num_wg = 4
    refused(wg, "pf_num_wg")
    items = blk()
    items.split_items = items.split_seq = 4096
    items.num_split_items = 4
    refused(items, "split_items")
    refused(blk(variant=7 << 1), "prefill64 has no fp8 build")
    refused(blk(d=96), "head dimension")
    refused(blk(d=256), "head dimension")
    # a decode-form block (one token, the multi-token form) is pointed at the decode entry — which still takes it
    for sq in (1, 4):
        dec = _tensors(_params(2, sq, 4096, 8, 2))
        refused(dec, "vattn_fp8kv_attn_with_kvcache")
        assert "decode form" in K.last_error()
        assert lib.vattn_fp8kv_attn_plan_describe(C.byref(dec), C.byref(K.PlanDesc())) == 0
    # ... and the decode entry still refuses the prefill form by name, batched chunks included
    for p in (blk(), blk(knew=300), _tensors(_params(2, 4, 4096, 8, 2, splits=3)), _tensors(_params(2, 9, 4096, 8, 2))):
        assert lib.vattn_fp8kv_attn_with_kvcache(C.byref(p), SC, SC, None) == -10 and "prefill form" in K.last_error()
        assert lib.vattn_fp8kv_prefill_plan_describe(C.byref(p), C.byref(K.PlanDesc())) == 0          # what this entry accepts
    # what keeps the prefill kernels for a few-row block is accepted here: forced shares, an explicit tiling
    for p in (_params(2, 4, 4096, 8, 2, splits=3), _params(2, 4, 4096, 8, 2, variant=4 << 1), _params(4, 8, 4096, 9, 1, d=64)):
        assert K.describe_fp8kv_prefill(p)["form"] == 0
    # batched chunks pass the gate (causal or not); with k_new they stay refused by validate()'s rule: append with cache_flat first
    chunks = blk()
    chunks.q_lens = chunks.q_start = chunks.cache_seqlens = 4096
    assert K.describe_fp8kv_prefill(chunks)["form"] == 0
    chunks_new = blk(knew=300)
    chunks_new.q_lens = chunks_new.q_start = 4096
    assert call(chunks_new) == -10 and "cache_flat" in K.last_error()
    # inside the gate: NULL scales, cache strides that are no whole 16-byte chunks of bytes, misaligned new rows, another header's block
    ok = blk()
    assert call(ok, None, SC) == -11 and "k_scale" in K.last_error()
    assert call(ok, SC, None) == -11 and "v_scale" in K.last_error()
    odd = blk()
    odd.k_row_stride = 2 * 128 + 8                       # fine for a 2-byte cache, not a whole 16-byte chunk of bytes
    assert call(odd) == -10 and "16" in K.last_error() and "fp8" in K.last_error()
    new = blk(knew=300)
    new.k_new = 4096 + 8
    assert call(new) == -10 and "k_new" in K.last_error()
    nolen = blk(knew=300)
    nolen.cache_seqlens = None
    assert call(nolen) == -11 and "seqlens_k" in K.last_error()
    bad = blk()
    bad.struct_size -= 16
    assert call(bad) == -11 and "struct_size" in K.last_error()
    assert lib.vattn_fp8kv_prefill_workspace_bytes(C.byref(bad)) == 0
    assert lib.vattn_fp8kv_prefill_plan_describe(C.byref(bad), C.byref(K.PlanDesc())) == -11


@pytest.mark.lab
def test_the_measurement_build_has_no_fp8_prefill_kernels():
    lab = K.klib_lab()
    p = _tensors(_params(2, 300, 4096, 8, 2))
    assert lab.vattn_fp8kv_prefill_with_kvcache(C.byref(p), SC, SC, None) == -10 and "measurement build" in K.last_error(lab)
    assert lab.vattn_fp8kv_prefill_workspace_bytes(C.byref(p)) == 0
    assert lab.vattn_fp8kv_prefill_plan_describe(C.byref(p), C.byref(K.PlanDesc())) == -10


def test_reference_for_the_prefill_form_is_a_dense_softmax_over_the_stored_bytes():
    """The yardstick of tests/test_gpu_fp8kv_prefill.py: a chunk of 5 rows appended to a prefix of 7, causal (bottom-right aligned), GQA 4 / 2
    with unequal per-head scales, against a dense float64 softmax written out here — also for a row that sees no key (Lk < Sq)."""
    torch.manual_seed(3)
    Hq, Hkv, D, Sq, pre, rows = 4, 2, 64, 5, 7, 16
    q = torch.randn(1, Sq, Hq, D).half()
    kp, vp = torch.randn(pre, Hkv, D).half() * torch.tensor([1.0, 6.0]).view(1, 2, 1).half(), torch.randn(pre, Hkv, D).half() * torch.tensor([4.0, 0.5]).view(1, 2, 1).half()
    kn, vn = torch.randn(1, Sq, Hkv, D).half() * torch.tensor([1.0, 6.0]).view(1, 1, 2, 1).half(), torch.randn(1, Sq, Hkv, D).half()
    ks, vs = amax_scales(torch.cat([kp, kn[0]])), amax_scales(torch.cat([vp, vn[0]]))
    assert ks[1] / ks[0] > 3 and vs[0] / vs[1] > 3
    k8 = torch.full((1, rows, Hkv, D), 0xA5, dtype=torch.uint8).view(torch.float8_e4m3fn)
    v8 = torch.full((1, rows, Hkv, D), 0xA5, dtype=torch.uint8).view(torch.float8_e4m3fn)
    k8[0, :pre], v8[0, :pre] = quantize_ref(kp, ks), quantize_ref(vp, vs)
    scale = 0.2
    got, lse = fp8kv_attn_ref(q, k8, v8, ks, vs, kn, vn, cache_seqlens=pre, causal=True, softmax_scale=scale, return_lse=True)
    assert torch.equal(k8[0, pre:pre + Sq].view(torch.uint8), quantize_ref(kn[0], ks).view(torch.uint8))      # appended as the quantiser's bytes
    assert bool((k8[0, pre + Sq:].view(torch.uint8) == 0xA5).all())
    Lk = pre + Sq
    kd, vd = dequantize_ref(k8[0, :Lk], ks), dequantize_ref(v8[0, :Lk], vs)                                   # float64 [Lk, Hkv, D]
    for h in range(Hq):
        hk = h // (Hq // Hkv)
        for i in range(Sq):
            vis = i + Lk - Sq + 1                                                                            # keys 0 .. i + Lk - Sq
            s = [scale * sum(float(q[0, i, h, e]) * float(kd[j, hk, e]) for e in range(D)) for j in range(vis)]
            m = max(s)
            w = [math.exp(x - m) for x in s]
            want = [sum(w[j] * float(vd[j, hk, e]) for j in range(vis)) / sum(w) for e in range(D)]
            assert max(abs(a - float(b)) for a, b in zip(want, got[0, i, h])) < 1e-9
            assert abs(m + math.log(sum(w)) - float(lse[0, h, i])) < 1e-9
    # Lk = 3 < Sq = 5 (no append): rows 0 and 1 see no key — zeros, LSE +inf
    short, lse_s = fp8kv_attn_ref(q, k8, v8, ks, vs, cache_seqlens=3, causal=True, return_lse=True)
    assert float(short[0, :2].abs().max()) == 0.0 and bool(torch.isinf(lse_s[0, :, :2]).all()) and bool((lse_s[0, :, :2] > 0).all())
    assert bool(torch.isfinite(lse_s[0, :, 2:]).all())
