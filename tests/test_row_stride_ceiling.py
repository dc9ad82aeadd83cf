"""The row-stride ceiling of the K/V caches (include/vattn_kernels.h, ROW-STRIDE CEILING), pinned without a GPU through the describe and
workspace entries of every call and through the shared validation of the calls themselves: pure host arithmetic, nothing is launched."""
import pytest

from vattention_amd import kernels as K


def _params(b, sq, sk, h, hk, d=128, causal=1):
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d = b, sq, sk, h, hk, d
    p.is_causal, p.dtype = causal, 0
    return p


def test_row_stride_ceiling_is_pinned_on_the_host():
    """include/vattn_kernels.h, ROW-STRIDE CEILING: a K / V row stride of 2^24 - 16 BYTES is the largest every kernel's 32-bit in-tile offsets (and
    prefill64p's 24-bit multiply) carry.  Through the describe and workspace entries, without a GPU: the bound itself is accepted; the bound + 8
    elements and any negative row stride are refused with VATTN_K_ERR_UNSUPPORTED and a message that names the rule — for the plain, tree,
    softcap (strides in 2-byte elements) and the fp8, fp8-tree, fp8-prefill entries (strides in bytes, multiples of 16)."""
    import ctypes
    lib = K.klib()
    top = (1 << 24) - 16                      # bytes
    dec, mt, pre = (16, 1, 4096, 32, 4), (16, 4, 4096, 16, 4), (2, 512, 4096, 32, 4)
    entries = [  # (name, block shape, bytes per cache element, describe, workspace)
        ("plain decode", dec, 2, lambda p: K.describe(p), lambda p: lib.vattn_attn_workspace_bytes(ctypes.byref(p))),
        ("plain prefill", pre, 2, lambda p: K.describe(p), lambda p: lib.vattn_attn_workspace_bytes(ctypes.byref(p))),
        ("tree", mt, 2, lambda p: K.describe_tree(p), lambda p: lib.vattn_tree_attn_workspace_bytes(ctypes.byref(p))),
        ("softcap decode", dec, 2, lambda p: K.describe_softcap(p, 50.0), lambda p: lib.vattn_softcap_attn_workspace_bytes(ctypes.byref(p), 50.0)),
        ("softcap prefill", pre, 2, lambda p: K.describe_softcap(p, 50.0), lambda p: lib.vattn_softcap_attn_workspace_bytes(ctypes.byref(p), 50.0)),
        ("fp8 decode", dec, 1, lambda p: K.describe_fp8kv(p), lambda p: lib.vattn_fp8kv_attn_workspace_bytes(ctypes.byref(p))),
        ("fp8 tree", mt, 1, lambda p: K.describe_fp8kv_tree(p), lambda p: lib.vattn_fp8kv_tree_attn_workspace_bytes(ctypes.byref(p))),
        ("fp8 prefill", pre, 1, lambda p: K.describe_fp8kv_prefill(p), lambda p: lib.vattn_fp8kv_prefill_workspace_bytes(ctypes.byref(p))),
    ]
    for name, shape, es, describe, workspace in entries:
        def block(k_rs, v_rs):
            p = _params(*shape, causal=0 if "tree" in name else 1)
            p.k_row_stride, p.v_row_stride = k_rs, v_rs
            return p
        ok = top // es
        good = describe(block(ok, ok))
        assert workspace(block(ok, ok)) == good["workspace_bytes"] > 0, name
        assert good == describe(block(0, 0)) == describe(block(1024, 1024)), name          # (the row stride changes no plan)
        for bad in ((ok + 8, ok), (ok, ok + 8), (ok + 16, ok), (-8, ok), (ok, -16), (-ok, -ok), (1 << 40, 1 << 40)):
            with pytest.raises(RuntimeError, match="row-stride ceiling"):
                describe(block(*bad))
            assert K.last_error().startswith("row-stride ceiling: k_row_stride / v_row_stride must be >= 0 and at most 2^24 - 16 BYTES"), name
            assert workspace(block(*bad)) == 0, (name, bad)
    # the code is UNSUPPORTED (-10), not INVALID
    d = K.PlanDesc()
    p = _params(*dec)
    p.k_row_stride = top // 2 + 8
    assert lib.vattn_attn_plan_describe(ctypes.byref(p), ctypes.byref(d)) == -10
    assert lib.vattn_softcap_attn_plan_describe(ctypes.byref(p), 50.0, ctypes.byref(d)) == -10
    assert lib.vattn_fp8kv_attn_plan_describe(ctypes.byref(p), ctypes.byref(d)) == 0          # (2^23 + 8 BYTES: far below the ceiling of an fp8 cache)
    p.k_row_stride = top + 16
    assert lib.vattn_fp8kv_attn_plan_describe(ctypes.byref(p), ctypes.byref(d)) == -10
    # the calls themselves refuse it in the shared validation, before anything is launched (dummy aligned pointers: nothing is dereferenced)
    for es, call in ((2, lambda p: lib.vattn_flash_attn_with_kvcache(ctypes.byref(p), None)), (2, lambda p: lib.vattn_softcap_attn_with_kvcache(ctypes.byref(p), 50.0, None)),
                     (1, lambda p: lib.vattn_fp8kv_attn_with_kvcache(ctypes.byref(p), 4096, 4096, None))):
        for bad in (top // es + 16, -16):
            p = _params(*dec)
            p.q = p.out = p.k_cache = p.v_cache = p.cache_seqlens = 4096
            p.k_row_stride, p.v_row_stride = 1024, bad
            assert call(p) == -10 and K.last_error().startswith("row-stride ceiling"), (es, bad)
