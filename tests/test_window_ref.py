"""Sliding-window attention without a GPU: (1) the window helper of the GPU tests (tests/window_ref.py) against the oracle — a windowed
row IS an un-windowed one-row call on a key slice: row i = flash_attn_with_kvcache_ref(q[:, i:i+1], K[:, s_i:e_i+1], V[:, s_i:e_i+1],
cache_seqlens = e_i + 1 - s_i); (2) the docstring's formula (flash_attn_interface.py:1204-1206) read back from the helper's output in the
style of tests/test_docstring_pins.py; (3) the C ABI's host side with a window — planners, plan description, workspace, argument rules —
in the style of tests/test_plan_table.py (pure host arithmetic of libvattn_amd.so)."""
import ctypes as C

import pytest
import torch

from oracle.attn import flash_attn_with_kvcache_ref
from tests.window_ref import first_visible_key, window_attn_ref
from vattention_amd import kernels as K

# (Sq, Lk, left, Hq, Hkv, D): left = 0, left >= Lk, whole prompt (Sq = Lk), chunk against a longer cache (Sq < Lk), one-token query; GQA 1 / 4 / 7
CASES = [(1, 300, 64, 8, 2, 64), (70, 333, 100, 7, 1, 64), (5, 5, 2, 4, 4, 128), (33, 200, 0, 4, 1, 64), (17, 90, 500, 8, 2, 64),
         (40, 40, 7, 14, 2, 64), (40, 40, 0, 4, 4, 64), (300, 300, 63, 4, 1, 64), (9, 700, 256, 7, 1, 128), (64, 64, 64, 4, 4, 64)]


@pytest.mark.parametrize("math", ["f64", "f32"])
@pytest.mark.parametrize("Sq,Lk,left,Hq,Hkv,D", CASES)
def test_helper_is_the_oracle_row_by_row_on_key_slices(Sq, Lk, left, Hq, Hkv, D, math):
    torch.manual_seed(Sq * 7 + Lk)
    q = torch.randn(2, Sq, Hq, D).half()
    kc = torch.randn(3, Lk + 7, Hkv, D).half()
    vc = torch.randn(3, Lk + 7, Hkv, D).half()
    idx = torch.tensor([2, 0], dtype=torch.int32)
    got, lse = window_attn_ref(q, kc, vc, left, cache_seqlens=Lk, cache_batch_idx=idx, math=math, return_lse=True)
    off = Lk - Sq
    worst = 0.0
    for b in range(2):
        for i in range(Sq):
            s, e = max(0, i + off - left), i + off
            ref, rl = flash_attn_with_kvcache_ref(q[b:b + 1, i:i + 1], kc[idx[b]:idx[b] + 1, s:e + 1].clone(), vc[idx[b]:idx[b] + 1, s:e + 1].clone(),
                                                  cache_seqlens=e + 1 - s, math=math, return_lse=True)
            worst = max(worst, (ref[0, 0].double() - got[b, i].double()).abs().max().item())
            assert (rl[0, :, 0].double() - lse[b, :, i].double()).abs().max().item() < (1e-12 if math == "f64" else 1e-5)
    # f64: the same sums in another order; f32: both round P and the output to fp16 (one ulp of the output at most apart)
    assert worst <= (1e-13 if math == "f64" else 2e-3), worst
    if left >= Lk:
        full = flash_attn_with_kvcache_ref(q, kc.clone(), vc.clone(), cache_seqlens=Lk, cache_batch_idx=idx, causal=True, math=math)
        assert (full.double() - got.double()).abs().max().item() <= (1e-13 if math == "f64" else 2e-3)


def test_helper_rows_and_q_lens_select_what_they_say():
    torch.manual_seed(3)
    q = torch.randn(2, 600, 4, 64).half()
    kc, vc = torch.randn(2, 900, 2, 64).half(), torch.randn(2, 900, 2, 64).half()
    lens, qls = [900, 500], [600, 130]
    full = window_attn_ref(q, kc, vc, 100, cache_seqlens=lens, q_lens=qls)
    rows = torch.tensor([0, 1, 99, 100, 101, 129, 130, 255, 256, 511, 599])
    part = window_attn_ref(q, kc, vc, 100, cache_seqlens=lens, q_lens=qls, rows=rows)
    assert (part - full[:, rows]).abs().max().item() < 1e-13      # (other key slices: the same float64 sums in another order)
    assert not bool(full[1, 130:].any()) and bool(full[1, 129].any())
    for b in range(2):      # every entry is its own one-entry call
        one = window_attn_ref(q[b:b + 1, :qls[b]], kc[b:b + 1], vc[b:b + 1], 100, cache_seqlens=lens[b])
        assert (one[0] - full[b, :qls[b]]).abs().max().item() < 1e-13


@pytest.mark.parametrize("Sq,Lk,left", [(2, 5, 1), (5, 2, 0), (5, 5, 2), (6, 9, 0), (6, 9, 3), (6, 9, 100), (1, 9, 4), (8, 20, 7)])
def test_docstring_formula_read_back(Sq, Lk, left):
    """q = 0 and one-hot value rows: output element j of query i is non-zero iff i + Lk - Sq - left <= j <= i + Lk - Sq
    (flash_attn_interface.py:1204-1206, right = 0), and then equals 1 / (visible keys of i)."""
    D = 32
    q = torch.zeros(1, Sq, 1, D, dtype=torch.float16)
    k = torch.randn(1, Lk, 1, D).half()
    v = torch.zeros(1, Lk, 1, D, dtype=torch.float16)
    for j in range(Lk):
        v[0, j, 0, j] = 1.0
    out = window_attn_ref(q, k, v, left, cache_seqlens=Lk)
    for i in range(Sq):
        vis = [j for j in range(Lk) if i + Lk - Sq - left <= j <= i + Lk - Sq]
        for j in range(Lk):
            want = 1.0 / len(vis) if j in vis else 0.0
            assert abs(out[0, i, 0, j].item() - want) < 1e-12, (i, j)
    assert first_visible_key(Sq, Lk, left) == max(0, Lk - Sq - left)


# ---- the C ABI's host side ----

def _params(b, sq, sk, h, hk, d=128, causal=1, left=None, knew=0, hint=0):
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = b, sq, sk, knew, h, hk, d
    p.is_causal, p.dtype, p.max_seqlen_k_hint = causal, 0, hint
    if left is not None:
        p.window_left_plus1 = left + 1
    return p


def _tensors(p):
    """validate() wants non-null, aligned tensor pointers; nothing is launched and nothing dereferences them"""
    p.q = p.out = p.k_cache = p.v_cache = 4096
    p.q_row_stride = p.o_row_stride = p.h * p.d
    p.q_head_stride = p.o_head_stride = p.k_head_stride = p.v_head_stride = p.d
    p.k_row_stride = p.v_row_stride = p.h_k * p.d
    return p


def test_abi_carries_the_window_at_the_end_of_the_block():
    assert K.ABI_VERSION == 6
    names = [n for n, _ in K.AttnParams._fields_]
    assert names[-2:] == ["window_left_plus1", "window_reserved"]
    assert K.AttnParams.window_left_plus1.offset == K.AttnParams.pf_wg_first.offset + 8
    assert C.sizeof(K.AttnParams) == K.AttnParams.window_left_plus1.offset + 8
    assert K.AttnParams().window_left_plus1 == 0          # a zeroed block: no window


def test_the_three_planners_answer_default_launch_for_a_window():
    lib = K.klib()
    # a ragged decode batch and a whole prompt on a tensor-parallel shard: both get a plan without a window
    lens = [30000, 4000, 4100, 3900, 28000, 4000, 4000, 4000]
    items, seq = (K.DecodeItem * 4096)(), (C.c_int32 * 16)()
    cl = (C.c_int32 * 8)(*lens)
    assert lib.vattn_decode_plan(C.byref(_params(8, 1, 32768, 32, 4)), cl, items, 4096, seq) > 0
    assert lib.vattn_decode_plan(C.byref(_params(8, 1, 32768, 32, 4, left=4095)), cl, items, 4096, seq) == 0
    pit, pbl = (K.PrefillItem * 8192)(), (K.PrefillItem * 1024)()
    kl = (C.c_int32 * 1)(8192)
    for left, want_list in ((None, True), (1023, False)):
        p = _params(1, 8192, 8192, 8, 1, left=left)
        counts = (C.c_int32 * 3)(7, 7, 7)
        n = lib.vattn_prefill_plan(C.byref(p), None, kl, pit, 8192, pbl, 1024, counts)
        assert (n > 0) == want_list and (want_list or list(counts) == [0, 0, 0])
        counts4, wg_first = (C.c_int32 * 4)(7, 7, 7, 7), (C.c_int32 * 257)()
        n = lib.vattn_prefill_plan_wg(C.byref(p), None, kl, pit, 8192, pbl, 1024, wg_first, 0, counts4)
        assert (n > 0) == want_list and (want_list or list(counts4) == [0, 0, 0, 0])
        n = lib.vattn_prefill_plan_wg(C.byref(p), None, kl, pit, 8192, pbl, 1024, None, 0, counts4)
        assert (n > 0) == want_list


def test_decode_plan_and_workspace_are_sized_by_visible_keys():
    lib = K.klib()
    for (b, h, hk, d) in ((16, 32, 4, 128), (1, 32, 4, 128), (64, 8, 1, 128), (8, 71, 1, 64), (16, 32, 1, 128)):
        win = _params(b, 1, 32768, h, hk, d, left=4095)
        short = _params(b, 1, 4096 + 32, h, hk, d)          # the same visible keys + one decode tile of alignment slack
        full = _params(b, 1, 32768, h, hk, d)
        dw, ds, df = K.describe(win), K.describe(short), K.describe(full)
        assert dw["form"] == 1 and dw["path"] == ds["path"] and dw["tiling"] == ds["tiling"]
        assert dw["workgroups"] <= ds["workgroups"] and dw["workspace_bytes"] <= ds["workspace_bytes"], (dw, ds)
        assert dw["workspace_bytes"] == lib.vattn_attn_workspace_bytes(C.byref(win))
        if df["workspace_bytes"] > ds["workspace_bytes"]:
            assert dw["workspace_bytes"] < df["workspace_bytes"] and dw["workgroups"] < df["workgroups"], (dw, df)
    # strictly smaller wherever the window-less launch at 32 768 is sized by its length and not by the chip (B16 x 4 kv heads fills the
    # resident workgroups at 4 128 keys already: equal there, as the loop above allows)
    for b in (1, 4):
        dw, df = K.describe(_params(b, 1, 32768, 32, 4, left=4095)), K.describe(_params(b, 1, 32768, 32, 4))
        assert dw["workspace_bytes"] < df["workspace_bytes"] and dw["workgroups"] < df["workgroups"], (b, dw, df)
    # a window wider than the view changes nothing
    assert K.describe(_params(16, 1, 2048, 32, 4, left=4095)) == K.describe(_params(16, 1, 2048, 32, 4))


def test_prefill_plan_counts_visible_keys():
    # a 2 k chunk on a 30 k prefix of a tensor-parallel shard: four key-range shares without a window; with left = 1 023 a query block sees
    # (1 023 + 256) keys = 20 tiles — nothing worth four shares, and the workspace shrinks with them
    full, win = K.describe(_params(1, 2048, 32768, 8, 1, hint=32768)), K.describe(_params(1, 2048, 32768, 8, 1, hint=32768, left=1023))
    assert full["nsplit"] == 4 and win["nsplit"] < full["nsplit"] and win["workspace_bytes"] < full["workspace_bytes"]
    assert win["path"] == 0
    # the 32 k prompt with left = 4 095 keeps prefill64 on the grid path, unsplit
    d = K.describe(_params(1, 32702, 32702, 32, 4, left=4095))
    assert (d["path"], d["tiling"], d["nsplit"]) == (0, 7, 1)


def test_window_argument_rules_of_the_c_abi():
    lib = K.klib()
    ok = _tensors(_params(2, 1, 4096, 8, 2, left=100))
    # (no launch here: a block that passes validate() is only described)
    assert lib.vattn_attn_plan_describe(C.byref(ok), C.byref(K.PlanDesc())) == 0
    noncausal = _tensors(_params(1, 512, 4096, 8, 2, causal=0, left=100))
    assert lib.vattn_flash_attn_with_kvcache(C.byref(noncausal), None) == -10 and "causal" in K.last_error()
    with_items = _tensors(_params(4, 1, 4096, 8, 2, left=100))
    with_items.split_items, with_items.split_seq, with_items.num_split_items = 4096, 4096, 4
    assert lib.vattn_flash_attn_with_kvcache(C.byref(with_items), None) == -11 and "split_items" in K.last_error()
    with_list = _tensors(_params(1, 2048, 4096, 8, 2, left=100))
    with_list.pf_items, with_list.num_pf_items = 4096, 8
    assert lib.vattn_flash_attn_with_kvcache(C.byref(with_list), None) == -11 and "pf_items" in K.last_error()
    neg = _tensors(_params(2, 1, 4096, 8, 2))
    neg.window_left_plus1 = -3
    assert lib.vattn_flash_attn_with_kvcache(C.byref(neg), None) == -11


def test_a_zeroed_window_describes_exactly_as_before():
    """the committed plan tables (tests/test_plan_table.py) hold for a block whose window words are zero — spot-checked here with the
    values of that table, so a window default that is not "none" cannot hide behind a regenerated table"""
    assert K.describe(_params(16, 1, 32768, 32, 4))["workspace_bytes"] == 6922368
    d = K.describe(_params(1, 2048, 32768, 8, 1, hint=32768))
    assert (d["path"], d["tiling"], d["nsplit"], d["workgroups"], d["merge_launch"], d["workspace_bytes"]) == (0, 7, 4, 256, 1, 33816576)


def test_python_window_argument_rules():
    from vattention_amd.flash_attn import _window_left_plus1 as w
    assert w((-1, -1), True, 8, 100) == (0, True) and w((-1, -1), False, 8, 100) == (0, False)
    assert w((10, 5), True, 8, 100) == (11, True)            # causal forces right = 0 (flash_api.cpp:1368)
    assert w((10, 77), False, 1, 100) == (11, True)          # a one-token query ignores right
    assert w((100, 0), True, 8, 100) == (0, True)            # left >= the view's rows: no window (:1380)
    assert w((99, 0), True, 8, 100) == (100, True)
    assert w((0, 0), True, 8, 100) == (1, True)              # left = 0: the own position only
    assert w((-1, 0), True, 8, 100) == (0, True)             # plain causal
    assert w((5, 0), False, 8, 100) == (6, True)             # (left, 0) is the causal mask with a left limit
    for ws in ((-1, 0), (-1, 3), (5, 3)):
        with pytest.raises(NotImplementedError, match="causal windows"):
            w(ws, False, 8, 100)
