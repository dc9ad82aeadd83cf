"""Tree-masked multi-token decode over an FP8 (e4m3) KV cache without a GPU: (1) the C ABI's host side (include/vattn_kernels.h:
vattn_fp8kv_tree_attn_with_kvcache / _workspace_bytes / _plan_describe, vattn_cache_keep_rows_fp8) — exports, the planners' answers (exactly
the 2-byte tree call's for the same block) and the argument rules, in the style of tests/test_tree_ref.py (pure host arithmetic of
libvattn_amd.so; fake aligned pointers, nothing is launched); (2) the helper of the GPU tests (tests/fp8kv_tree_ref.py) against
tests/fp8kv_ref.py — a chain mask IS the causal multi-token fp8 call, an all-ones mask the non-causal one."""
import ctypes as C

import pytest
import torch

from tests.fp8kv_ref import FP8, amax_scales, fp8kv_attn_ref, quantize_ref
from tests.fp8kv_tree_ref import fp8kv_tree_ref
from tests.tree_ref import chain_mask
from vattention_amd import kernels as K


def _params(b, sq, sk, h, hk, d=128, causal=0, splits=0, variant=0, knew=None):
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = b, sq, sk, sq if knew is None else knew, h, hk, d
    p.is_causal, p.dtype, p.num_splits, p.variant = causal, 0, splits, variant
    return p


def _tensors(p):
    """validate() and the fp8 argument rules want non-null, 16-byte aligned tensor pointers and byte strides that are multiples of 16;
    nothing is launched and nothing dereferences them (tests/test_tree_ref.py)"""
    p.q = p.out = p.k_cache = p.v_cache = 4096
    p.q_row_stride = p.o_row_stride = p.h * p.d
    p.q_head_stride = p.o_head_stride = p.k_head_stride = p.v_head_stride = p.d
    p.k_row_stride = p.v_row_stride = p.h_k * p.d
    p.k_batch_stride = p.v_batch_stride = p.seqlen_k * p.h_k * p.d
    if p.seqlen_knew:
        p.k_new = p.v_new = p.cache_seqlens = 4096
        p.knew_row_stride = p.vnew_row_stride = p.h_k * p.d
        p.knew_head_stride = p.vnew_head_stride = p.d
    return p


def test_new_symbols_are_exported_and_the_block_is_frozen():
    lib = K.klib()
    for name in ("vattn_fp8kv_tree_attn_with_kvcache", "vattn_fp8kv_tree_attn_workspace_bytes", "vattn_fp8kv_tree_attn_plan_describe",
                 "vattn_cache_keep_rows_fp8"):
        assert getattr(lib, name) is not None
    assert K.ABI_VERSION == 6 and C.sizeof(K.AttnParams) == 400      # (the size of ABI 6: nothing was added to the block)
    from vattention_amd import flash_attn as FA
    assert FA.counters["fp8kv_tree_calls"] >= 0 and callable(FA.flash_attn_fp8kv_tree_with_kvcache) and callable(K.describe_fp8kv_tree)


# B16 sq4 32/4 @ 32k, B1 sq8 8/1 @ 128k, B256 sq2 32/8 @ 2k, d 64 — and tests/test_tree_ref.py's: both head-block counts, stream / uniform
# paths, forced grids, 64 columns
BLOCKS = [(16, 4, 32768, 32, 4), (1, 8, 131072, 8, 1), (256, 2, 2048, 32, 8), (8, 3, 900, 28, 4, 64), (16, 4, 32768, 32, 8), (1, 2, 131072, 8, 1),
          (3, 8, 4096, 8, 1), (2, 5, 2000, 28, 4), (4, 8, 4096, 8, 1, 64), (16, 4, 32768, 32, 8, 128, 1, -100), (1, 4, 20000, 8, 2, 128, 0, -3)]


@pytest.mark.parametrize("args", BLOCKS, ids=lambda a: "x".join(str(x) for x in a))
def test_plan_and_workspace_are_the_tree_call_s(args):
    p = _params(*args)
    lib = K.klib()
    t, f = K.describe_tree(p), K.describe_fp8kv_tree(p)
    assert t["form"] == 1
    for name in ("form", "path", "tiling", "nsplit", "workgroups", "merge_launch", "workspace_bytes"):
        assert f[name] == t[name], (name, f, t)
    ws = int(lib.vattn_fp8kv_tree_attn_workspace_bytes(C.byref(p)))
    assert ws == int(lib.vattn_tree_attn_workspace_bytes(C.byref(p))) == f["workspace_bytes"]
    p.is_causal = 1 - p.is_causal                        # ignored by the form, and by its plan
    assert K.describe_fp8kv_tree(p) == f


def test_argument_rules_of_the_c_abi():
    lib = K.klib()
    mask, scale = C.c_void_p(8192), C.c_void_p(12288)    # non-NULL device addresses: the host never dereferences them
    call = lambda p, m=mask, ks=scale, vs=scale: lib.vattn_fp8kv_tree_attn_with_kvcache(C.byref(p), m, ks, vs, None)

    def outside(p, code, word):
        assert call(_tensors(p)) == code and word in K.last_error(), (code, word, K.last_error())
        assert lib.vattn_fp8kv_tree_attn_workspace_bytes(C.byref(p)) == 0
        assert lib.vattn_fp8kv_tree_attn_plan_describe(C.byref(p), C.byref(K.PlanDesc())) == code and word in K.last_error()

    for sq in (1, 9):
        outside(_params(2, sq, 4096, 8, 2), -10, "seqlen_q")
    outside(_params(4, 8, 4096, 9, 1, d=64), -10, "<= 64")      # 72 (token, head) columns
    outside(_params(2, 4, 4096, 8, 2, splits=3), -10, "num_splits")
    outside(_params(2, 4, 4096, 8, 2, variant=4 << 1), -10, "tiling")
    for causal in (1, 0):
        win = _params(2, 4, 4096, 8, 2, causal=causal)
        win.window_left_plus1 = 101
        outside(win, -11, "window")
    rot = _params(2, 4, 4096, 8, 2)
    rot.rotary_cos_sin, rot.rotary_dim, rot.rotary_row_stride = 4096, 128, 128
    outside(rot, -10, "rotary")
    items = _params(2, 4, 4096, 8, 2, knew=0)            # (batched chunks take no k / v: validate() would refuse that first)
    items.q_lens = items.q_start = 4096
    outside(items, -10, "q_lens")
    # a good block: NULL scales, the fp8 stride / alignment rules; the mask is only tested for NULL
    good = lambda: _tensors(_params(2, 4, 4096, 8, 2))
    assert call(good(), ks=None) == -11 and "k_scale and v_scale" in K.last_error()
    assert call(good(), vs=None) == -11 and "k_scale and v_scale" in K.last_error()
    odd = good()
    odd.k_row_stride += 8                                # a multiple of 8 passes the 2-byte rule, not the rule for bytes
    assert call(odd) == -10 and "multiples of 16" in K.last_error()
    odd = good()
    odd.v_new += 8
    assert call(odd) == -10 and "16-byte aligned" in K.last_error()
    # another header's block
    for field, value in (("struct_size", C.sizeof(K.AttnParams) - 16), ("abi_version", K.ABI_VERSION - 1)):
        bad = good()
        setattr(bad, field, value)
        assert call(bad) == -11 and "struct_size" in K.last_error()
        assert lib.vattn_fp8kv_tree_attn_workspace_bytes(C.byref(bad)) == 0
        assert lib.vattn_fp8kv_tree_attn_plan_describe(C.byref(bad), C.byref(K.PlanDesc())) == -11
    # tree_mask == NULL delegates to the fp8 decode call, whose gate refuses a window as UNSUPPORTED (the tree call: INVALID)
    win = _tensors(_params(2, 4, 4096, 8, 2, causal=1))
    win.window_left_plus1 = 101
    assert call(win, m=None) == -10 and "sliding window" in K.last_error()
    assert call(win) == -11


def test_keep_rows_fp8_argument_rules_of_the_c_abi():
    lib = K.klib()
    call = lambda n_draft=4, d=128, rs=256, hs=128, ptr=4096: lib.vattn_cache_keep_rows_fp8(ptr, ptr, 1 << 20, rs, hs, 1 << 20, rs, hs, 4096, None, 4096, 4096,
                                                                                            2, n_draft, 2, d, None)
    assert call(n_draft=9) == -10 and "8" in K.last_error()
    assert call(d=96) == -10 and call(rs=264) == -10 and call(hs=72) == -10 and call(ptr=4104) == -10
    assert call(n_draft=0) == -11 and call(ptr=None) == -11


# ---- the reference of the GPU tests ----

def _inputs(B, sq, Hq, Hkv, D, rows, seed):
    torch.manual_seed(seed)
    kf, vf = torch.randn(B + 1, rows, Hkv, D).half(), torch.randn(B + 1, rows, Hkv, D).half()
    ks, vs = amax_scales(kf) * 1.5, amax_scales(vf) * 1.5
    return (torch.randn(B, sq, Hq, D).half(), quantize_ref(kf, ks), quantize_ref(vf, vs), ks, vs,
            torch.randn(B, sq, Hkv, D).half(), torch.randn(B, sq, Hkv, D).half())


@pytest.mark.parametrize("math", ["f64", "f32"])
@pytest.mark.parametrize("sq,Hq,Hkv,D", [(2, 8, 2, 64), (5, 7, 1, 64), (8, 8, 8, 128), (3, 4, 4, 64)])
def test_chain_and_all_ones_masks_are_the_fp8_reference(sq, Hq, Hkv, D, math):
    """f64: EXACT — both references run the same float64 operations on the same dequantised values (a masked score is -inf in either, and
    exp(-inf) = 0 adds nothing to a sum).  f32: both round P and the output to fp16 (2e-3, tests/test_tree_ref.py's bound for the 2-byte pair)."""
    lens = [sq, sq - 1, 40, 0, 97]                       # visible keys AFTER the append where there is one
    B = len(lens)
    q, k8, v8, ks, vs, kn, vn = _inputs(B, sq, Hq, Hkv, D, 110, sq * 31 + Hq)
    idx = torch.tensor([3, 0, 5, 1, 2], dtype=torch.int32)
    tol = 0.0 if math == "f64" else 2e-3
    for append in (False, True):
        cl = torch.tensor([max(n - sq, 0) for n in lens] if append else lens, dtype=torch.int32)
        new = dict(k=kn, v=vn) if append else {}
        for causal, mask in ((True, chain_mask(sq)), (False, torch.full((B, sq), -1, dtype=torch.int32))):
            kr, vr, kt, vt = k8.clone(), v8.clone(), k8.clone(), v8.clone()
            ref, rl = fp8kv_attn_ref(q, kr, vr, ks, vs, cache_seqlens=cl, cache_batch_idx=idx, causal=causal, math=math, return_lse=True, **new)
            got, gl = fp8kv_tree_ref(q, kt, vt, ks, vs, mask, cache_seqlens=cl, cache_batch_idx=idx, math=math, return_lse=True, **new)
            assert (got.double() - ref.double()).abs().max().item() <= tol
            assert torch.equal(kr.view(torch.uint8), kt.view(torch.uint8)) and torch.equal(vr.view(torch.uint8), vt.view(torch.uint8))
            live = torch.isfinite(rl)                    # (an EMPTY entry's LSE is -inf in the oracle, +inf here: "no visible key")
            assert torch.equal(torch.isfinite(gl), live) and (gl[live] - rl[live]).abs().max().item() <= (0.0 if math == "f64" else 1e-5)


def test_a_row_without_a_visible_key_gives_zero_and_lse_inf():
    q, k8, v8, ks, vs, _, _ = _inputs(2, 4, 4, 2, 64, 40, 3)
    # entry 0: Lk = 4 = sq (base 0), token 1's word is 0, token 2 only names itself; entry 1: Lk = 2 < sq (base -2): draft keys 0, 1 do not exist
    mask = torch.tensor([[1, 0, 4, 15], [3, 4, 0, 8]], dtype=torch.int32)
    out, lse = fp8kv_tree_ref(q, k8, v8, ks, vs, mask, cache_seqlens=[4, 2], return_lse=True)
    dead = torch.tensor([[False, True, False, False], [True, False, True, False]])
    for b in range(2):
        for t in range(4):
            assert bool(torch.isinf(lse[b, :, t]).all() and (lse[b, :, t] > 0).all()) == bool(dead[b, t]), (b, t)
            assert (not bool(out[b, t].any())) == bool(dead[b, t]), (b, t)
    # token 2 of entry 0 sees exactly draft key 2 = cache row 2: the output is that row's dequantised value
    want = (v8[0, 2].double() * vs.double().view(-1, 1)).repeat_interleave(2, dim=0)
    assert torch.equal(out[0, 2], want)
    assert k8.dtype == FP8
