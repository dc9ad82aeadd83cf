"""FP8 (e4m3) KV cache without a GPU: (1) the quantiser of the GPU tests (tests/fp8kv_ref.py) — saturation, round-to-nearest-even ties,
subnormals, every byte through widen and quantise — and that widening to fp16 / bf16 is exact; (2) the page manager's layout at itemsize 1;
(3) the C ABI's host side (include/vattn_kernels.h: vattn_fp8kv_attn_with_kvcache / _workspace_bytes / _plan_describe,
vattn_cache_flat_fp8): exports, the frozen parameter block, the planners' answers and the gate, in the style of tests/test_tree_ref.py
(pure host arithmetic of libvattn_amd.so; fake aligned pointers, nothing is launched)."""
import ctypes as C

import pytest
import torch

from tests.fp8kv_ref import FP8, amax_scales, dequantize_ref, fp8kv_attn_ref, quantize_ref
from vattention_amd import kernels as K
from vattention_amd.kernels import describe_fp8kv

ONE = torch.ones(1)


def _bytes(x8):
    return x8.view(torch.uint8)


def test_every_byte_round_trips_through_widen_and_quantise():
    b = torch.arange(256, dtype=torch.uint8)
    x8 = b.view(FP8)
    val = x8.float()
    nan = torch.isnan(val)
    assert nan.sum().item() == 2 and bool(nan[0x7F]) and bool(nan[0xFF])          # e4m3fn: no infinities, one NaN pattern per sign
    assert val[~nan].abs().max().item() == 448.0
    for dt in (torch.float16, torch.bfloat16):                                     # widening is exact: 3 mantissa bits, 2^-9 .. 448
        w = x8.to(dt)
        assert torch.equal(w.float()[~nan], val[~nan]) and bool(torch.isnan(w.float()[nan]).all())
        back = _bytes(quantize_ref(w.view(256, 1, 1), ONE).view(256))
        assert torch.equal(back[~nan], b[~nan])                                    # (-0 keeps its sign: byte 0x80)
        assert bool(((back[nan] & 0x7F) == 0x7F).all())                            # a NaN stores the NaN byte


def test_saturation_ties_and_subnormals():
    q = lambda vals, s=1.0: _bytes(quantize_ref(torch.tensor(vals, dtype=torch.float32).view(-1, 1, 1), torch.tensor([s]))).view(-1).tolist()
    assert q([448.0, 449.0, 1e6, float("inf"), -448.0, -1e6, float("-inf")]) == [0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0xFE, 0xFE]
    assert q([464.0, 479.9]) == [0x7E, 0x7E]                    # beyond the largest value's rounding interval: the clamp, not a NaN
    # round-to-nearest-even between neighbours 1.0 (0x38), 1.125 (0x39), 1.25 (0x3A)
    assert q([1.0625, 1.1875, 1.06251, 1.18749]) == [0x38, 0x3A, 0x39, 0x39]
    # subnormals: multiples of 2^-9 below 2^-6; ties to even; half of the smallest rounds to zero, just above it to the smallest
    s = 2.0 ** -9
    assert q([s, 2 * s, 7 * s, 8 * s, 0.5 * s, 0.51 * s, 1.5 * s, 2.5 * s, -0.5 * s]) == [1, 2, 7, 8, 0, 1, 2, 2, 0x80]
    # the scale: y = x * (1.0f / scale)
    assert q([448.0 * 3.0, 3.0, -6.0], 3.0) == [0x7E, 0x38, 0xC0]
    assert q([float("nan")])[0] & 0x7F == 0x7F


def test_quantiser_is_per_head_and_amax_scales_use_the_whole_range():
    torch.manual_seed(0)
    x = torch.randn(50, 3, 64).half() * torch.tensor([1.0, 10.0, 0.1]).view(1, 3, 1).half()
    s = amax_scales(x)
    assert s.shape == (3,) and 5 < (s[1] / s[0]).item() < 20
    x8 = quantize_ref(x, s)
    assert _bytes(x8).view(-1, 3, 64).permute(1, 0, 2).reshape(3, -1).to(torch.int32).bitwise_and(0x7F).amax(dim=1).tolist() == [0x7E] * 3
    err = (dequantize_ref(x8, s) - x.double()).abs() / s.double().view(-1, 1)
    assert err.max().item() <= 16.0 + 1e-9                      # half a step of the top binade (step 32) in units of the scale


def test_reference_attention_over_a_quantised_cache():
    """fp8kv_attn_ref IS the oracle on the dequantised values, and appending through it stores the quantiser's bytes."""
    from oracle.attn import flash_attn_with_kvcache_ref
    torch.manual_seed(1)
    B, Hq, Hkv, D, rows = 3, 8, 2, 64, 80
    q = torch.randn(B, 1, Hq, D).half()
    k, v = torch.randn(B + 1, rows, Hkv, D).half(), torch.randn(B + 1, rows, Hkv, D).half()
    ks, vs = amax_scales(k), amax_scales(v) * 10
    k8, v8 = quantize_ref(k, ks), quantize_ref(v, vs)
    cl, idx = torch.tensor([5, 33, 79], dtype=torch.int32), torch.tensor([2, 0, 3], dtype=torch.int32)
    kn, vn = torch.randn(B, 1, Hkv, D).half(), torch.randn(B, 1, Hkv, D).half()
    a8, b8 = k8.clone(), v8.clone()
    got, lse = fp8kv_attn_ref(q, a8, b8, ks, vs, kn, vn, cache_seqlens=cl, cache_batch_idx=idx, return_lse=True)
    for b in range(B):
        assert torch.equal(_bytes(a8[idx[b], cl[b]]), _bytes(quantize_ref(kn[b, 0], ks)))
        assert torch.equal(_bytes(b8[idx[b], cl[b]]), _bytes(quantize_ref(vn[b, 0], vs)))
    ref, rl = flash_attn_with_kvcache_ref(q, dequantize_ref(a8, ks), dequantize_ref(b8, vs), cache_seqlens=cl + 1, cache_batch_idx=idx, return_lse=True)
    assert torch.equal(got, ref) and torch.equal(lse, rl)
    full = flash_attn_with_kvcache_ref(q, k.clone(), v.clone(), kn, vn, cache_seqlens=cl, cache_batch_idx=idx)
    assert (got - full).abs().max().item() < 0.15               # the quantisation error itself: e4m3 keeps 3-4 bits


def test_page_manager_layout_at_itemsize_1_holds_twice_the_tokens_per_page():
    from tests.impls import ProductImpl
    cfg = dict(num_layers=2, num_kv_heads=2, head_size=128, max_batch_size=4, max_context_length=8192, page_size=64 << 10, megacache=False)
    lay = {}
    for itemsize in (2, 1):
        p = ProductImpl(dict(cfg, itemsize=itemsize), min_gran=4096)
        try:
            lay[itemsize] = (int(p.pm.layout.tokens_per_page), p.pm.shape(), p.pm.stride(), int(p.pm.layout.virt_bytes_per_req))
        finally:
            p.pm.close()
    assert lay[2][0] == (64 << 10) // (2 * 128 * 2) == 128 and lay[1][0] == 256 == 2 * lay[2][0]
    assert lay[1][1] == lay[2][1] and lay[1][2] == lay[2][2]            # same shape, same strides in ELEMENTS
    assert 2 * lay[1][3] == lay[2][3]                                    # half the virtual bytes per request


# ---- the C ABI's host side ----

def _params(b, sq, sk, h, hk, d=128, causal=1, splits=0, variant=0, knew=None):
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = b, sq, sk, sq if knew is None else knew, h, hk, d
    p.is_causal, p.dtype, p.num_splits, p.variant = causal, 0, splits, variant
    return p


def _tensors(p):
    """validate() wants non-null, aligned tensor pointers; nothing is launched and nothing dereferences them (tests/test_tree_ref.py)"""
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
    for name in ("vattn_fp8kv_attn_with_kvcache", "vattn_fp8kv_attn_workspace_bytes", "vattn_fp8kv_attn_plan_describe", "vattn_cache_flat_fp8"):
        assert getattr(lib, name) is not None
    assert K.ABI_VERSION == 6 and C.sizeof(K.AttnParams) == 400
    from vattention_amd import flash_attn as FA
    assert FA.counters["fp8kv_decode_calls"] >= 0 and callable(FA.flash_attn_fp8kv_with_kvcache)
    from vattention_amd import cache_ops
    assert callable(cache_ops.cache_flat_fp8)
    with pytest.raises(RuntimeError, match="Unsupported data type of kv cache"):      # cache_flat mirrors the reference's check, as before
        cache_ops.cache_flat(None, None, None, None, "fp8")


# one-token and multi-token blocks: both head-block counts, stream / uniform paths, forced grids, sibling groups (G = 40), d = 64
BLOCKS = [(16, 1, 32768, 32, 8), (1, 1, 131072, 32, 8), (16, 1, 32768, 32, 4), (5, 1, 4099, 8, 2), (5, 1, 4099, 40, 1), (5, 1, 4099, 8, 8, 64),
          (5, 1, 1000, 8, 1, 128, 0, 3), (5, 1, 1000, 8, 2, 128, 0, -7), (256, 1, 2048, 32, 8), (16, 4, 32768, 32, 8), (3, 8, 4096, 8, 1),
          (2, 5, 2000, 28, 4), (4, 2, 4096, 8, 2, 64, 0), (1, 4, 20000, 8, 2, 128, 0, -3)]


@pytest.mark.parametrize("args", BLOCKS, ids=lambda a: "x".join(str(x) for x in a))
@pytest.mark.parametrize("knew", [0, None], ids=["attend", "append"])
def test_plan_and_workspace_are_the_two_byte_call_s(args, knew):
    p = _params(*args, knew=knew)
    lib = K.klib()
    d, f = K.describe(p), describe_fp8kv(p)
    assert d["form"] == 1 and f == d, (d, f)
    ws = int(lib.vattn_fp8kv_attn_workspace_bytes(C.byref(p)))
    assert ws == int(lib.vattn_attn_workspace_bytes(C.byref(p))) == f["workspace_bytes"]


def test_gate_and_argument_rules_of_the_c_abi():
    lib = K.klib()
    sc = C.c_void_p(8192)                                # a non-NULL device address: the host never dereferences it
    call = lambda p, ks=sc, vs=sc: lib.vattn_fp8kv_attn_with_kvcache(C.byref(p), ks, vs, None)

    def refused(p, word, rc=-10):
        assert call(p) == rc and word in K.last_error(), K.last_error()
        assert "fp8" in K.last_error()
        assert lib.vattn_fp8kv_attn_plan_describe(C.byref(p), C.byref(K.PlanDesc())) == rc and word in K.last_error()
        assert lib.vattn_fp8kv_attn_workspace_bytes(C.byref(p)) == 0

    for sq in (1, 4):
        win = _tensors(_params(2, sq, 4096, 8, 2))
        win.window_left_plus1 = 101
        refused(win, "window")
        rot = _tensors(_params(2, sq, 4096, 8, 2))
        rot.rotary_cos_sin, rot.rotary_dim, rot.rotary_row_stride = 4096, 128, 128
        refused(rot, "rotary")
    items = _tensors(_params(2, 1, 4096, 8, 2))
    items.split_items = items.split_seq = 4096
    items.num_split_items = 4
    refused(items, "split_items")
    chunks = _tensors(_params(2, 300, 4096, 8, 2, knew=0))
    chunks.q_lens = chunks.q_start = 4096
    refused(chunks, "q_lens")
    lst = _tensors(_params(1, 4096, 4096, 8, 1, knew=0))
    lst.pf_items, lst.num_pf_items = 4096, 4
    refused(lst, "pf_items")
    for p in (_params(2, 9, 4096, 8, 2), _params(2, 300, 4096, 8, 2), _params(4, 8, 4096, 9, 1, d=64), _params(2, 4, 4096, 8, 2, splits=3),
              _params(2, 4, 4096, 8, 2, variant=4 << 1)):          # what keeps the prefill kernels for a block (multitoken_form)
        refused(_tensors(p), "prefill form")
    # inside the gate: NULL scales, misaligned cache strides, another header's block
    ok = _tensors(_params(2, 1, 4096, 8, 2))
    assert call(ok, None, sc) == -11 and "k_scale" in K.last_error()
    assert call(ok, sc, None) == -11 and "v_scale" in K.last_error()
    odd = _tensors(_params(2, 1, 4096, 8, 2))
    odd.k_row_stride = 2 * 128 + 8                       # fine for a 2-byte cache, not a whole 16-byte chunk of bytes
    assert call(odd) == -10 and "16" in K.last_error()
    bad = _tensors(_params(2, 1, 4096, 8, 2))
    bad.struct_size -= 16
    assert call(bad) == -11 and "struct_size" in K.last_error()
    assert lib.vattn_fp8kv_attn_workspace_bytes(C.byref(bad)) == 0
    assert lib.vattn_fp8kv_attn_plan_describe(C.byref(bad), C.byref(K.PlanDesc())) == -11
    # the flat append's argument rules
    flat = lambda ks=sc, vs=sc, dt=0, ptr=4096: lib.vattn_cache_flat_fp8(ptr, ptr, ptr, ptr, 5, 2, 128, 256, 256, 256, 256, dt, ks, vs, None)
    assert flat(ks=None) == -11 and "k_scale" in K.last_error()
    assert flat(dt=2) == -10 and flat(ptr=None) == -11
    assert lib.vattn_cache_flat_fp8(None, None, None, None, 0, 2, 128, 256, 256, 256, 256, 0, None, None, None) == 0      # nothing to do


@pytest.mark.lab
def test_the_measurement_build_has_no_fp8_kernels():
    lab = K.klib_lab()
    p = _tensors(_params(2, 1, 4096, 8, 2))
    assert lab.vattn_fp8kv_attn_with_kvcache(C.byref(p), C.c_void_p(8192), C.c_void_p(8192), None) == -10
    assert "measurement build" in K.last_error(lab)
