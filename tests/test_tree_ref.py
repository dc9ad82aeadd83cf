"""Tree-masked multi-token decode without a GPU: (1) the helper of the GPU tests (tests/tree_ref.py) against the oracle — a lower-triangular
mask IS the causal multi-token call, an all-ones mask the non-causal one — and on a hand-written tree; (2) the C ABI's host side
(include/vattn_kernels.h: vattn_tree_attn_with_kvcache / _workspace_bytes / _plan_describe, vattn_cache_keep_rows): exports, the frozen
parameter block, the planners' answers and the argument rules, in the style of tests/test_window_ref.py (pure host arithmetic of
libvattn_amd.so; fake aligned pointers, nothing is launched)."""
import ctypes as C

import pytest
import torch

from oracle.attn import flash_attn_with_kvcache_ref
from tests.tree_ref import chain_mask, pack_mask, tree_attn_ref
from vattention_amd import kernels as K


def _inputs(B, sq, Hq, Hkv, D, rows, seed):
    torch.manual_seed(seed)
    return (torch.randn(B, sq, Hq, D).half(), torch.randn(B + 1, rows, Hkv, D).half(), torch.randn(B + 1, rows, Hkv, D).half(),
            torch.randn(B, sq, Hkv, D).half(), torch.randn(B, sq, Hkv, D).half())


@pytest.mark.parametrize("math", ["f64", "f32"])
@pytest.mark.parametrize("sq,Hq,Hkv,D", [(2, 8, 2, 64), (5, 7, 1, 64), (8, 8, 8, 128), (3, 4, 4, 64)])
def test_chain_and_all_ones_masks_are_the_oracle(sq, Hq, Hkv, D, math):
    lens = [sq, sq - 1, 40, 0, 97]                       # visible keys AFTER the append where there is one
    B = len(lens)
    q, kc, vc, kn, vn = _inputs(B, sq, Hq, Hkv, D, 110, sq * 31 + Hq)
    idx = torch.tensor([3, 0, 5, 1, 2], dtype=torch.int32)
    tol = 1e-12 if math == "f64" else 2e-3               # f32: both round P and the output to fp16 (test_window_ref.py)
    for append in (False, True):
        cl = torch.tensor([max(n - sq, 0) for n in lens] if append else lens, dtype=torch.int32)
        new = dict(k=kn, v=vn) if append else {}
        for causal, mask in ((True, chain_mask(sq)), (False, torch.full((B, sq), -1, dtype=torch.int32))):
            kr, vr, kt, vt = kc.clone(), vc.clone(), kc.clone(), vc.clone()
            ref, rl = flash_attn_with_kvcache_ref(q, kr, vr, cache_seqlens=cl, cache_batch_idx=idx, causal=causal, math=math, return_lse=True, **new)
            got, gl = tree_attn_ref(q, kt, vt, mask, cache_seqlens=cl, cache_batch_idx=idx, math=math, return_lse=True, **new)
            assert (got.double() - ref.double()).abs().max().item() <= tol
            assert torch.equal(kr, kt) and torch.equal(vr, vt)
            live = torch.isfinite(rl)                    # (an EMPTY entry's LSE is -inf in the oracle, +inf here: "no visible key")
            assert torch.equal(torch.isfinite(gl), live) and (gl[live] - rl[live]).abs().max().item() < (1e-12 if math == "f64" else 1e-5)


def test_hand_written_five_node_tree():
    """      0            node: parent   visible draft keys
           /   \\          0: -           {0}
          1     2         1: 0           {0, 1}
          |    / \\        2: 0           {0, 2}
          3   4           3: 1           {0, 1, 3}
                          4: 2           {0, 2, 4}
    q = 0 and one-hot value rows: element j of row t is 1 / (keys t sees) iff t sees key j (tests/test_window_ref.py's read-back)."""
    sees = {0: {0}, 1: {0, 1}, 2: {0, 2}, 3: {0, 1, 3}, 4: {0, 2, 4}}
    words = torch.tensor([[0b00001, 0b00011, 0b00101, 0b01011, 0b10101]], dtype=torch.int32)
    vis = torch.zeros(5, 5, dtype=torch.bool)
    for t, ss in sees.items():
        for s_ in ss:
            vis[t, s_] = True
    assert torch.equal(pack_mask(vis), words[0])
    D = 32
    for Lk in (5, 9, 3):                                 # base 0, base 4 (four committed keys), base -2 (draft keys 0 and 1 do not exist)
        base = Lk - 5
        q = torch.zeros(1, 5, 1, D, dtype=torch.float16)
        k = torch.randn(1, max(Lk, 1), 1, D).half()
        v = torch.zeros(1, Lk, 1, D, dtype=torch.float16)
        for j in range(Lk):
            v[0, j, 0, j] = 1.0
        out, lse = tree_attn_ref(q, k, v, words, cache_seqlens=Lk, return_lse=True)
        for t in range(5):
            keys = [j for j in range(Lk) if j < base or (j - base) in sees[t]]
            for j in range(Lk):
                want = 1.0 / len(keys) if j in keys else 0.0
                assert abs(out[0, t, 0, j].item() - want) < 1e-12, (Lk, t, j)
            assert (lse[0, 0, t].item() == float("inf")) == (not keys)
    # Lk = 3: node 1 sees draft keys {0, 1} = cache rows {-2, -1}: nothing
    assert lse[0, 0, 1].item() == float("inf") and not bool(out[0, 1].any())


def test_bits_above_seqlen_q_are_ignored():
    q, kc, vc, _, _ = _inputs(2, 3, 4, 2, 64, 50, 5)
    m = torch.tensor([[1, 2, 5], [7, 0, 3]], dtype=torch.int32)
    a = tree_attn_ref(q, kc, vc, m, cache_seqlens=[20, 33])
    b = tree_attn_ref(q, kc, vc, m | (0x7FFFFF << 8) | (1 << 3), cache_seqlens=[20, 33])
    assert torch.equal(a, b)


# ---- the C ABI's host side ----

def _params(b, sq, sk, h, hk, d=128, causal=1, splits=0, variant=0, knew=None):
    """tests/test_multitoken_plan.py's block"""
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = b, sq, sk, sq if knew is None else knew, h, hk, d
    p.is_causal, p.dtype, p.num_splits, p.variant = causal, 0, splits, variant
    return p


def _tensors(p):
    """validate() wants non-null, aligned tensor pointers; nothing is launched and nothing dereferences them (tests/test_window_ref.py)"""
    p.q = p.out = p.k_cache = p.v_cache = 4096
    p.q_row_stride = p.o_row_stride = p.h * p.d
    p.q_head_stride = p.o_head_stride = p.k_head_stride = p.v_head_stride = p.d
    p.k_row_stride = p.v_row_stride = p.h_k * p.d
    if p.seqlen_knew:
        p.k_new = p.v_new = p.cache_seqlens = 4096
    return p


def test_new_symbols_are_exported_and_the_block_is_frozen():
    lib = K.klib()
    for name in ("vattn_tree_attn_with_kvcache", "vattn_tree_attn_workspace_bytes", "vattn_tree_attn_plan_describe", "vattn_cache_keep_rows"):
        assert getattr(lib, name) is not None
    assert K.ABI_VERSION == 6
    assert [n for n, _ in K.AttnParams._fields_][-2:] == ["window_left_plus1", "window_reserved"]
    assert C.sizeof(K.AttnParams) == K.AttnParams.window_left_plus1.offset + 8 == 400      # (the size of ABI 6)
    from vattention_amd import flash_attn as FA
    assert FA.counters["tree_decode_calls"] >= 0 and callable(FA.flash_attn_tree_with_kvcache)
    from vattention_amd import cache_ops
    assert callable(cache_ops.keep_rows)


# the shapes of tests/test_multitoken_plan.py: both head-block counts, stream / uniform paths, forced grids, R = 64
BLOCKS = [(16, 4, 32768, 32, 4), (16, 4, 32768, 32, 8), (1, 2, 131072, 8, 1), (3, 8, 4096, 8, 1), (2, 5, 2000, 28, 4), (4, 2, 4096, 8, 2),
          (4, 8, 4096, 8, 1), (16, 4, 32768, 32, 8, 128, 1, -100), (1, 4, 20000, 8, 2, 128, 0, -3), (8, 3, 900, 28, 4, 64)]


@pytest.mark.parametrize("args", BLOCKS, ids=lambda a: "x".join(str(x) for x in a))
def test_plan_and_workspace_are_the_multitoken_call_s(args):
    p = _params(*args)
    lib = K.klib()
    d, t = K.describe(p), K.describe_tree(p)
    assert d["form"] == 1 and t == d, (d, t)
    ws = int(lib.vattn_tree_attn_workspace_bytes(C.byref(p)))
    assert ws == int(lib.vattn_attn_workspace_bytes(C.byref(p))) == t["workspace_bytes"]
    p.is_causal = 1 - p.is_causal                        # ignored by the form, and by its plan
    assert K.describe_tree(p) == t


def test_tree_argument_rules_of_the_c_abi():
    lib = K.klib()
    mask = C.c_void_p(8192)                              # a non-NULL device address: the host never dereferences it
    call = lambda p: lib.vattn_tree_attn_with_kvcache(C.byref(p), mask, None)
    win = _tensors(_params(2, 4, 4096, 8, 2))
    win.window_left_plus1 = 101
    for causal in (1, 0):
        win.is_causal = causal
        assert call(win) == -11 and "window" in K.last_error()
        assert lib.vattn_tree_attn_plan_describe(C.byref(win), C.byref(K.PlanDesc())) == -11
        assert lib.vattn_tree_attn_workspace_bytes(C.byref(win)) == 0
    for sq in (1, 9):
        assert call(_tensors(_params(2, sq, 4096, 8, 2))) == -10 and "seqlen_q" in K.last_error()
        assert lib.vattn_tree_attn_plan_describe(C.byref(_params(2, sq, 4096, 8, 2)), C.byref(K.PlanDesc())) == -10
    assert call(_tensors(_params(4, 8, 4096, 9, 1, d=64))) == -10 and "<= 64" in K.last_error()      # 72 columns
    rot = _tensors(_params(2, 4, 4096, 8, 2))
    rot.rotary_cos_sin, rot.rotary_dim, rot.rotary_row_stride = 4096, 128, 128
    assert call(rot) == -10 and "rotary" in K.last_error()
    assert call(_tensors(_params(2, 4, 4096, 8, 2, splits=3))) == -10 and "num_splits" in K.last_error()
    assert call(_tensors(_params(2, 4, 4096, 8, 2, variant=4 << 1))) == -10 and "tiling" in K.last_error()
    items = _tensors(_params(2, 4, 4096, 8, 2, knew=0))      # (batched chunks take no k / v: validate() would refuse that first)
    items.q_lens = items.q_start = 4096
    assert call(items) == -10 and "q_lens" in K.last_error()
    bad = _tensors(_params(2, 4, 4096, 8, 2))
    bad.struct_size -= 16
    assert call(bad) == -11 and "struct_size" in K.last_error()
    assert lib.vattn_tree_attn_workspace_bytes(C.byref(bad)) == 0
    assert lib.vattn_tree_attn_plan_describe(C.byref(bad), C.byref(K.PlanDesc())) == -11
    bad = _tensors(_params(2, 4, 4096, 8, 2))
    bad.abi_version = K.ABI_VERSION - 1
    assert call(bad) == -11


def test_keep_rows_argument_rules_of_the_c_abi():
    lib = K.klib()
    call = lambda n_draft=4, d=128, dtype=0, rs=256, ptr=4096: lib.vattn_cache_keep_rows(ptr, ptr, 1 << 20, rs, d, 1 << 20, rs, d, 4096, None, 4096, 4096,
                                                                                       2, n_draft, 2, d, dtype, None)
    assert call(n_draft=9) == -10 and "8" in K.last_error()
    assert call(d=96) == -10 and call(dtype=2) == -10 and call(rs=260) == -10
    assert call(n_draft=0) == -11 and call(ptr=None) == -11
