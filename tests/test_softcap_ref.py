"""Logit soft-capping without a GPU: (1) the softcap helper of the GPU tests (tests/softcap_ref.py) against the oracle and the window
helper — with a cap so large that tanh is the identity to float64 precision it IS the uncapped call — and against a row worked by hand;
(2) the host side of the C ABI with a cap (include/vattn_kernels.h, "Logit soft-capping"): the block and the ABI number are untouched,
softcap = 0 is the plain call, softcap > 0 describes the plain call's plan without prefill64, every refusal of the gate names its rule
— in the style of tests/test_window_ref.py (pure host arithmetic of libvattn_amd.so, nothing is launched)."""
import ctypes as C
import math

import pytest
import torch

from oracle.attn import flash_attn_with_kvcache_ref
from tests.softcap_ref import softcap_attn_ref
from tests.window_ref import window_attn_ref
from vattention_amd import kernels as K

HUGE = 1e6      # |s| <= ~60 here: tanh(s / 1e6) * 1e6 = s (1 - (s / 1e6)^2 / 3 ...), a relative 1e-9 at most


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Sq,Lk,Hq,Hkv,D", [(1, 300, 8, 2, 64), (5, 5, 4, 4, 128), (33, 200, 4, 1, 64), (8, 3, 8, 2, 64), (70, 333, 7, 1, 64)])
def test_a_huge_cap_is_the_oracle(Sq, Lk, Hq, Hkv, D, causal):
    torch.manual_seed(Sq * 7 + Lk)
    q = torch.randn(2, Sq, Hq, D).half()
    kc, vc = torch.randn(3, Lk + 7, Hkv, D).half(), torch.randn(3, Lk + 7, Hkv, D).half()
    idx = torch.tensor([2, 0], dtype=torch.int32)
    got, lse = softcap_attn_ref(q, kc, vc, HUGE, causal=causal, cache_seqlens=Lk, cache_batch_idx=idx, return_lse=True)
    ref, rl = flash_attn_with_kvcache_ref(q, kc.clone(), vc.clone(), cache_seqlens=Lk, cache_batch_idx=idx, causal=causal, math="f64", return_lse=True)
    assert (got - ref.double()).abs().max().item() < 1e-9
    live = torch.isfinite(rl.double())
    assert bool((torch.isfinite(lse) == live).all()) and (lse[live] - rl.double()[live]).abs().max().item() < 1e-9
    # softcap = 0 is "no cap" exactly
    zero = softcap_attn_ref(q, kc, vc, 0.0, causal=causal, cache_seqlens=Lk, cache_batch_idx=idx)
    assert (zero - ref.double()).abs().max().item() < 1e-12
    if Sq > Lk and causal:      # rows without a visible key: 0 and LSE +inf
        assert not bool(got[:, :Sq - Lk].any()) and bool(torch.isinf(lse[:, :, :Sq - Lk]).all())


@pytest.mark.parametrize("Sq,Lk,left", [(1, 300, 64), (70, 333, 100), (33, 200, 0), (40, 40, 7)])
def test_a_huge_cap_is_the_window_helper(Sq, Lk, left):
    torch.manual_seed(Lk + left)
    q = torch.randn(2, Sq, 8, 64).half()
    kc, vc = torch.randn(2, Lk + 3, 2, 64).half(), torch.randn(2, Lk + 3, 2, 64).half()
    lens, qls = [Lk, Lk - 1], [Sq, max(1, Sq - 3)]
    got, lse = softcap_attn_ref(q, kc, vc, HUGE, left=left, cache_seqlens=lens, q_lens=qls, return_lse=True)
    ref, rl = window_attn_ref(q, kc, vc, left, cache_seqlens=lens, q_lens=qls, return_lse=True)
    assert (got - ref).abs().max().item() < 1e-9
    live = torch.isfinite(rl)
    assert bool((torch.isfinite(lse) == live).all()) and (lse[live] - rl[live]).abs().max().item() < 1e-9
    # the f32 statement rounds where the window helper's does
    g32, r32 = softcap_attn_ref(q, kc, vc, HUGE, left=left, cache_seqlens=lens, q_lens=qls, math="f32"), window_attn_ref(q, kc, vc, left, cache_seqlens=lens, q_lens=qls, math="f32")
    assert (g32.double() - r32.double()).abs().max().item() <= 2e-3


def test_one_row_by_hand():
    """one query, three keys, d = 2, cap 2, scale 1: scores q.k = (4, 0, -1) -> 2 tanh(s / 2)"""
    q = torch.tensor([[[[2.0, 0.0]]]]).half()
    kc = torch.tensor([[[[2.0, 1.0]], [[0.0, 3.0]], [[-0.5, 1.0]]]]).half()
    vc = torch.tensor([[[[1.0, 0.0]], [[0.0, 1.0]], [[1.0, 1.0]]]]).half()
    t = [2 * math.tanh(4 / 2), 2 * math.tanh(0.0), 2 * math.tanh(-1 / 2)]
    w = [math.exp(x) for x in t]
    want = [(w[0] + w[2]) / sum(w), (w[1] + w[2]) / sum(w)]
    got, lse = softcap_attn_ref(q, kc, vc, 2.0, causal=False, softmax_scale=1.0, return_lse=True)
    assert abs(got[0, 0, 0, 0].item() - want[0]) < 1e-12 and abs(got[0, 0, 0, 1].item() - want[1]) < 1e-12
    assert abs(lse.item() - math.log(sum(w))) < 1e-12
    # the cap binds: without it the first key would take nearly all the weight
    plain = softcap_attn_ref(q, kc, vc, 0.0, causal=False, softmax_scale=1.0)
    assert plain[0, 0, 0, 0].item() > 0.97 > want[0]
    # causal with a window of one key to the left: the last two keys only
    got = softcap_attn_ref(q, kc, vc, 2.0, left=1, softmax_scale=1.0)
    assert abs(got[0, 0, 0, 0].item() - w[2] / (w[1] + w[2])) < 1e-12


# ---- the C ABI's host side ----

def _params(b, sq, sk, h, hk, d=128, causal=1, left=None, knew=0, hint=0, splits=0, variant=0):
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = b, sq, sk, knew, h, hk, d
    p.is_causal, p.dtype, p.max_seqlen_k_hint, p.num_splits, p.variant = causal, 0, hint, splits, variant
    p.softmax_scale = d ** -0.5
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


# decode (one token: stream path, one sequence, wide groups, forced splits), multi-token, prefill (chunk on a prefix, short prompt, forced
# split, explicit tilings, d = 64), each also with a window
BLOCKS = [dict(b=16, sq=1, sk=32768, h=32, hk=4), dict(b=1, sq=1, sk=32768, h=32, hk=4), dict(b=8, sq=1, sk=8192, h=32, hk=1), dict(b=3, sq=1, sk=301, h=8, hk=2, splits=-3),
          dict(b=4, sq=1, sk=4096, h=8, hk=2, d=64, splits=4), dict(b=16, sq=1, sk=32768, h=32, hk=4, left=4095),
          dict(b=3, sq=4, sk=301, h=8, hk=2), dict(b=16, sq=8, sk=32768, h=32, hk=4, causal=0), dict(b=16, sq=8, sk=32768, h=32, hk=4, left=40),
          dict(b=1, sq=300, sk=300, h=8, hk=2), dict(b=1, sq=130, sk=330, h=8, hk=2, splits=2), dict(b=1, sq=300, sk=300, h=8, hk=2, variant=2),
          dict(b=1, sq=300, sk=300, h=8, hk=2, variant=8), dict(b=1, sq=2048, sk=2048, h=32, hk=4), dict(b=2, sq=512, sk=4096, h=8, hk=2, d=64, causal=0),
          dict(b=1, sq=300, sk=300, h=8, hk=2, left=100), dict(b=1, sq=2048, sk=32768, h=8, hk=1, hint=32768, left=1023)]


def test_abi_is_untouched():
    assert K.ABI_VERSION == 6 and C.sizeof(K.AttnParams) == 400
    assert [n for n, _ in K.AttnParams._fields_][-2:] == ["window_left_plus1", "window_reserved"]      # nothing was added to the block


@pytest.mark.parametrize("kw", BLOCKS, ids=lambda kw: "-".join("%s%s" % kv for kv in kw.items()))
def test_softcap_describes_the_plain_calls_plan(kw):
    lib = K.klib()
    p = _params(**kw)
    plain = K.describe(p)
    assert K.describe_softcap(p, 0.0) == plain                               # softcap = 0: exactly vattn_attn_plan_describe
    assert lib.vattn_softcap_attn_workspace_bytes(C.byref(p), 0.0) == plain["workspace_bytes"]
    capped = K.describe_softcap(p, 50.0)
    assert capped["workspace_bytes"] == lib.vattn_softcap_attn_workspace_bytes(C.byref(p), 50.0)
    if plain["tiling"] != 7:
        assert capped == plain, (capped, plain)
    else:      # no prefill64 with a cap: the same rules with that branch skipped (what the fp8 prefill call gets)
        assert capped["form"] == 0 and capped["path"] == 0 and capped["tiling"] in (1, 4)
        assert capped == K.describe_fp8kv_prefill(p)


def test_a_chip_filling_prompt_leaves_prefill64():
    p = _params(1, 32702, 32702, 32, 4)
    assert K.describe(p)["tiling"] == 7
    d = K.describe_softcap(p, 50.0)
    assert d["form"] == 0 and d["path"] == 0 and d["tiling"] in (1, 4), d
    assert d["workspace_bytes"] == K.klib().vattn_softcap_attn_workspace_bytes(C.byref(p), 50.0)
    # ... and the other fields of a block the plain call does NOT give to prefill64 are the plain call's (the table above); the cap's
    # value does not enter the plan
    assert K.describe_softcap(p, 1.5) == d


def _refused(p, softcap, code, word, gate=True):
    lib = K.klib()
    assert lib.vattn_softcap_attn_with_kvcache(C.byref(p), softcap, None) == code, K.last_error()
    assert word in K.last_error(), K.last_error()
    if gate:      # outside the softcap gate: no plan, no workspace
        assert lib.vattn_softcap_attn_workspace_bytes(C.byref(p), softcap) == 0
        assert lib.vattn_softcap_attn_plan_describe(C.byref(p), softcap, C.byref(K.PlanDesc())) == -10 and word in K.last_error()


def test_every_refusal_of_the_gate_names_its_rule():
    rot = _tensors(_params(2, 1, 4096, 8, 2))
    rot.rotary_cos_sin, rot.rotary_dim, rot.rotary_row_stride = 4096, 128, 128
    _refused(rot, 50.0, -10, "rotary")
    rot_pf = _tensors(_params(1, 512, 4096, 8, 2))
    rot_pf.rotary_cos_sin, rot_pf.rotary_dim, rot_pf.rotary_row_stride = 4096, 128, 128
    _refused(rot_pf, 50.0, -10, "rotary")
    items = _tensors(_params(4, 1, 4096, 8, 2))
    items.split_items, items.split_seq, items.num_split_items = 4096, 4096, 4
    _refused(items, 50.0, -10, "split_items")
    lst = _tensors(_params(1, 2048, 4096, 8, 2))
    lst.pf_items, lst.num_pf_items = 4096, 8
    _refused(lst, 50.0, -10, "pf_items")
    lst.pf_num_wg = 8
    _refused(lst, 50.0, -10, "pf_num_wg")
    _refused(_tensors(_params(1, 2048, 4096, 8, 2, variant=14)), 50.0, -10, "tiling 7")
    _refused(_tensors(_params(1, 2048, 4096, 8, 2, d=256)), 50.0, -10, "head dimensions")
    _refused(_tensors(_params(2, 1, 4096, 8, 2, d=96)), 50.0, -10, "head dimensions")
    # the window's own rules still hold under a cap (the plain call's argument check, not the softcap gate: a non-causal window on a prefill block)
    _refused(_tensors(_params(1, 512, 4096, 8, 2, causal=0, left=100)), 50.0, -10, "causal", gate=False)
    # inside the gate: a block that passes is described (no launch here)
    ok = _tensors(_params(2, 1, 4096, 8, 2, left=100))
    assert K.klib().vattn_softcap_attn_plan_describe(C.byref(ok), 50.0, C.byref(K.PlanDesc())) == 0


@pytest.mark.parametrize("bad", [-1.0, -0.001, float("nan"), float("inf"), -float("inf")])
def test_bad_softcap_values_are_invalid(bad):
    lib = K.klib()
    p = _tensors(_params(2, 1, 4096, 8, 2))
    assert lib.vattn_softcap_attn_with_kvcache(C.byref(p), bad, None) == -11 and "softcap" in K.last_error()
    assert lib.vattn_softcap_attn_plan_describe(C.byref(p), bad, C.byref(K.PlanDesc())) == -11
    assert lib.vattn_softcap_attn_workspace_bytes(C.byref(p), bad) == 0


def test_a_cap_whose_pre_overflows_is_invalid():
    """a denormal cap is finite and > 0, but pre = softmax_scale / softcap is not a finite fp32 number: refused, not multiplied into every score"""
    lib = K.klib()
    p = _tensors(_params(2, 1, 4096, 8, 2))
    for tiny in (1e-45, 1e-40):
        assert lib.vattn_softcap_attn_with_kvcache(C.byref(p), tiny, None) == -11 and "too small" in K.last_error()
        assert lib.vattn_softcap_attn_plan_describe(C.byref(p), tiny, C.byref(K.PlanDesc())) == -11
        assert lib.vattn_softcap_attn_workspace_bytes(C.byref(p), tiny) == 0
    assert lib.vattn_softcap_attn_plan_describe(C.byref(p), 1.2e-38, C.byref(K.PlanDesc())) == 0      # the smallest normal numbers still divide


def test_a_mismatched_block_is_refused_before_anything_else():
    p = _tensors(_params(2, 1, 4096, 8, 2))
    p.abi_version = 5
    assert K.klib().vattn_softcap_attn_with_kvcache(C.byref(p), 50.0, None) == -11
    assert K.klib().vattn_softcap_attn_workspace_bytes(C.byref(p), 50.0) == 0


@pytest.mark.lab
def test_the_measurement_build_has_no_softcap_kernels():
    """the -DVATTN_LAB rule of the gate: refused by name before anything else is looked at; no plan, no workspace; softcap = 0 still delegates"""
    lab = K.klib_lab()
    for p in (_tensors(_params(2, 1, 4096, 8, 2)), _tensors(_params(3, 4, 301, 8, 2)), _tensors(_params(1, 512, 4096, 8, 2))):
        assert lab.vattn_softcap_attn_with_kvcache(C.byref(p), 50.0, None) == -10
        assert "measurement build" in K.last_error(lab)
        assert lab.vattn_softcap_attn_workspace_bytes(C.byref(p), 50.0) == 0
        assert lab.vattn_softcap_attn_plan_describe(C.byref(p), 50.0, C.byref(K.PlanDesc())) == -10 and "measurement build" in K.last_error(lab)
        # softcap = 0 is the lab library's own plain call: its plan, its workspace ...
        assert K.describe_softcap(p, 0.0, lab) == K.describe(p, lab)
        assert lab.vattn_softcap_attn_workspace_bytes(C.byref(p), 0.0) == lab.vattn_attn_workspace_bytes(C.byref(p))
    # ... and its own argument checks, reached THROUGH the new entry (a block the plain call refuses before any launch: null tensors)
    null = _params(2, 1, 4096, 8, 2)
    want = lab.vattn_flash_attn_with_kvcache(C.byref(null), None)
    msg = K.last_error(lab)
    assert want == -11 and lab.vattn_softcap_attn_with_kvcache(C.byref(null), 0.0, None) == want and K.last_error(lab) == msg
    # a bad value is INVALID there as everywhere
    assert lab.vattn_softcap_attn_with_kvcache(C.byref(_tensors(_params(2, 1, 4096, 8, 2))), -1.0, None) == -11


def test_python_softcap_argument_rules():
    """ValueError for anything that is not 0 or a NORMAL fp32 number > 0: the library takes the cap as a C float, where a value above FLT_MAX
    would arrive as inf and one below FLT_MIN would make pre = softmax_scale / softcap overflow"""
    from vattention_amd.flash_attn import _softcap_value
    assert _softcap_value(0) == 0.0 and _softcap_value(50) == 50.0 and _softcap_value(-0.0) == 0.0
    assert _softcap_value(1.5) == 1.5 and _softcap_value(3.4e38) > 0 and _softcap_value(1.2e-38) > 0
    for bad in (-1.0, float("nan"), float("inf"), -float("inf"), 3.5e38, 1e300, 1e-39, 1e-45, 5e-324):
        with pytest.raises(ValueError, match="softcap"):
            _softcap_value(bad)
