"""Routing of the MULTI-TOKEN decode form (include/vattn_kernels.h: 2 <= seqlen_q <= 8 query rows per entry on the split-KV decode kernels,
(token, head) columns), pinned through vattn_attn_plan_describe — pure host arithmetic, no GPU.  The gate lives in ONE function of the
library (csrc/attn_common.h, multitoken_form); the launch, the workspace size, the plan description and the Python drop-in all ask it."""
import ctypes as C

import pytest

from vattention_amd import kernels as K


def _params(b, sq, sk, h, hk, d=128, causal=1, splits=0, variant=0, knew=None):
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = b, sq, sk, sq if knew is None else knew, h, hk, d
    p.is_causal, p.dtype, p.num_splits, p.variant = causal, 0, splits, variant
    return p


def _workspace(p):
    return int(K.klib().vattn_attn_workspace_bytes(C.byref(p)))


def test_verify_step_shapes_take_the_decode_kernels():
    # B16, 4 draft tokens, Yi-6B heads (G = 8: 32 columns): two 16-column blocks per workgroup, one pass over K/V
    d = K.describe(_params(16, 4, 32768, 32, 4))
    assert d["form"] == 1 and d["tiling"] == 2, d
    # Llama-3-8B heads (G = 4: 16 columns): the one-token instruction stream, device-planned stream decomposition
    d = K.describe(_params(16, 4, 32768, 32, 8))
    assert d["form"] == 1 and d["tiling"] == 1 and d["path"] == 2, d
    # one sequence: the uniform split of the grid heuristics
    d = K.describe(_params(1, 2, 131072, 8, 1))
    assert d["form"] == 1 and d["path"] == 0 and d["nsplit"] > 1 and d["merge_launch"] == 1, d


@pytest.mark.parametrize("p", [
    _params(16, 9, 32768, 32, 8),                       # seqlen_q 9
    _params(16, 8, 32768, 16, 1),                       # 8 tokens x G = 16: 128 columns
    _params(16, 4, 32768, 32, 8, variant=4 << 1),       # an explicit prefill tiling (the A/B selector)
    _params(16, 4, 32768, 32, 8, splits=3),             # an explicit prefill key-range split
], ids=["sq9", "R128", "explicit_tiling", "num_splits_3"])
def test_outside_the_gate_keeps_the_prefill_form(p):
    assert K.describe(p)["form"] == 0


def test_pointer_fields_outside_the_gate_keep_the_prefill_form():
    buf = (C.c_int32 * 64)()              # (describe only tests the pointers for NULL)
    p = _params(16, 4, 32768, 32, 8, knew=0)
    assert K.describe(p)["form"] == 1
    p.q_lens = p.q_start = C.addressof(buf)
    assert K.describe(p)["form"] == 0
    p = _params(16, 4, 32768, 32, 8)
    p.rotary_cos_sin, p.rotary_dim = C.addressof(buf), 128
    assert K.describe(p)["form"] == 0


@pytest.mark.parametrize("args", [(16, 4, 32768, 32, 4), (16, 4, 32768, 32, 8), (1, 2, 131072, 8, 1), (3, 8, 4096, 8, 1), (2, 5, 2000, 28, 4)],
                         ids=["B16_G8", "B16_G4", "B1", "R64", "G7"])
def test_workspace_is_what_describe_reports(args):
    p = _params(*args)
    d = K.describe(p)
    assert d["form"] == 1 and d["workspace_bytes"] == _workspace(p) > 0, d
    if d["path"] == 0:
        # grid heuristics: fp32 partial rows [split][b][token][head] + their LSEs
        assert d["workspace_bytes"] == d["nsplit"] * p.b * p.seqlen_q * p.h * (p.d + 1) * 4, d


def test_boundaries_of_the_gate():
    assert K.describe(_params(4, 2, 4096, 8, 2))["form"] == 1 and K.describe(_params(4, 8, 4096, 8, 1))["form"] == 1      # 2 and 8 rows, 64 columns
    assert K.describe(_params(4, 8, 4096, 9, 1, d=64))["form"] == 0                                                          # 72 columns
    assert K.describe(_params(4, 1, 4096, 8, 2, knew=1))["form"] == 1                                                        # one token: decode, as ever
    f = K.describe(_params(16, 4, 32768, 32, 8, splits=-100))            # num_splits < 0 keeps its decode meaning: forced workgroups per kv head
    assert f["form"] == 1 and f["path"] == 2 and f["workgroups"] == 800, f
    w = _params(16, 4, 32768, 32, 8)
    w.window_left_plus1 = 1024
    d = K.describe(w)
    assert d["form"] == 1 and d["path"] == 2, d
