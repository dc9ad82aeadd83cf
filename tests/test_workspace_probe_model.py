"""The workspace probes on the host (tests/workspace_probe.py; the GPU file is tests/test_gpu_workspace.py): the plan descriptions and the
`*_workspace_bytes` exports are pure host arithmetic, so coverage, sizes, the dead-entry cases and the launch count of the GPU file are
proved here, and the fills and the guarded allocator are exercised on CPU tensors — a workspace answer that is 128 bytes short damages the
high guard, and the allocator says where.

NULL-WORKSPACE REFUSALS, read in the sources (test_every_split_launch_refuses_a_null_workspace keeps them there): every launch of a plan with
workspace_bytes > 0 is behind one of
  csrc/decode_kernels.hip launch_decode_stream   `if (!p->workspace) return fail(...)`                      decode path 2, every build
  csrc/decode_kernels.hip launch_decode_nb       `if (splits > 1 && !p->workspace) return fail(...)`        decode path 0 with nsplit > 1 and path 1 (host items: splits = 2), every build
  csrc/prefill_kernels.hip launch_prefill_t      `num_pf_blocks > 0 && (!p->pf_blocks || !p->workspace)`   the work list with split blocks, per piece and persistent
  csrc/prefill_kernels.hip launch_prefill_t      `if (pl.nsplit > 1 && !p->workspace) return fail(...)`     the KV-split prefill, tilings 1 / 4 / 7, plain, fp8 and softcap
each in front of the first launch of its function (the append launch included).  No test passes a NULL or short workspace to a launch."""
import inspect
import os
import re

import pytest
import torch

from tests import workspace_probe as W
from tests.test_plan_table import DECODE, PREFILL, _params

CASES = W.cases()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vattention_amd", "csrc")


def _grid_blocks():
    """the shape grid of tests/test_plan_table.py: its prefill shapes as they stand, its decode shapes as one-token calls and — for the multi-token
    and tree-masked entries — with 2 and 4 query rows; each also with the forced stream grid and an explicit split count the probes use"""
    for (_n, Hq, Hkv, n, c) in PREFILL:
        for splits in (0, 2):
            yield "pre", _params(1, n, c + n, Hq, Hkv, hint=c + n, splits=splits)
    for (name, Hq, Hkv, B, ctx) in DECODE:
        for sq in (1, 2, 4):
            for splits in (0, -37, 5):
                yield ("dec" if sq == 1 else "mt"), _params(B, sq, ctx, Hq, Hkv, d=64 if "d64" in name else 128, knew=sq, splits=splits)


def _describe(entry, form, p):
    from vattention_amd import kernels as K
    c = dict(form="tree" if entry in ("tree", "fp8tree") else form, fp8=entry.startswith("fp8"), cap=50.0 if entry == "cap" else None)
    if W.entry_of(c) != entry:
        return None
    if entry in ("tree", "fp8tree"):
        p.is_causal = 0
    p.cache_seqlens = W.DUMMY
    p.softmax_scale = p.d ** -0.5
    try:
        return W.describe_block(c, p)
    except RuntimeError:          # outside the entry's gate
        return None


def test_every_plan_with_a_workspace_is_probed():
    """every (entry point, form, path, tiling, merge launch) the plan descriptions answer with workspace_bytes > 0 on the plan-table grid is
    reached by a case of the probe table: a future plan with a workspace and no probe fails here"""
    have = {W.coverage_key(c, d) for c, d in CASES}
    want = {}
    for form, p in _grid_blocks():
        for entry in ("plain", "cap", "fp8", "fp8pre", "tree", "fp8tree"):
            d = _describe(entry, form, p)
            if d is not None and d["workspace_bytes"] > 0:
                want.setdefault((entry, d["form"], d["path"], d["tiling"], d["merge_launch"]), (p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.num_splits))
    assert len(want) >= 20, sorted(want)
    missing = {k: v for k, v in want.items() if k not in have}
    assert not missing, "plans with a workspace and no probe (key: a shape b, sq, sk, h, hk, d, splits that takes it): %s" % missing
    # and the paths only host plans reach, which the grid cannot: host items, the work list per piece, assigned and drawn
    for k in (("plain", 1, 1, 1, 1), ("plain", 1, 1, 2, 1), ("plain", 0, 1, 7, 1)):
        assert k in have, k
    assert {W.queue_of(c) for c, _ in CASES} >= {"per_piece", "assigned", "drawn"}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c, _ in CASES])
def test_layout_sizes_add_up(case):
    c, d = case
    p = W.host_block(c)
    assert W.describe_block(c, p) == d
    regions = W.layout(c, d, p)
    assert d["workspace_bytes"] == W.workspace_bytes_export(c, p) > 0
    assert sum(r["nbytes"] for r in regions) == d["workspace_bytes"], (c["name"], d, regions)
    off = 0
    for r in regions:
        assert r["offset"] == off and r["nbytes"] > 0 and r["offset"] % 4 == 0
        off += r["nbytes"]
        if r["kind"] == "float":
            assert r["nbytes"] % r["unit"] == 0, "the float region is a whole number of records / rows: %s" % r
        else:
            assert r["name"] == "table" and r["nbytes"] == (8 * p.b + 127) & ~127 and r["used"] == 8 * p.b
    assert [r["kind"] for r in regions] in (["float", "float"], ["int", "float"])
    assert (regions[0]["kind"] == "int") == (d["form"] == 1 and d["path"] == 2)


def test_a_dead_entry_case_for_every_decode_build():
    """an entry with cache_seqlens == 0 and no append beside live entries, on the device-planned stream path, per build and form"""
    dead = {}
    for c, d in CASES:
        if min(c["lens"]) == 0 and not c["append"] and max(c["lens"]) > 0 and d["path"] == 2:
            dead.setdefault(W.build_of(c), set()).add((c["form"], c["dt"]))
    assert set(dead) == {"plain", "tree", "fp8", "fp8tree", "softcap"}, dead
    for b in ("plain", "fp8", "softcap"):
        assert {f for f, _ in dead[b]} == {"dec", "mt"}, (b, dead[b])
    assert all({dt for _, dt in v} == {"f16", "bf16"} for v in dead.values()), dead
    assert all(c["sq"] * c["G"] == 16 for c, _ in CASES if min(c["lens"]) == 0 and c["form"] != "dec")      # the multi-token form at R = 16


def test_the_window_share_cases_are_in_the_table():
    """a windowed one-token decode cut into more shares than it has visible tiles, and its multi-token twins (tests/census.py numerics_cases)"""
    names = {c["name"] for c, _ in CASES}
    for dt in ("f16", "bf16"):
        assert {"num_empty_piece_%s_dec" % dt, "num_empty_piece_%s_mt" % dt, "num_empty_piece_%s_mt_R32" % dt} <= names
    c = next(c for c, _ in CASES if c["name"] == "num_empty_piece_f16_dec")
    d = W.describe_host(c)
    tiles = max((min(n, c["left"] + 1) + 31 + 31) // 32 for n in c["lens"])
    assert d["path"] == 0 and d["nsplit"] == 16 > tiles


def test_the_gpu_file_stays_within_its_launch_budget():
    n = W.total_kernels()
    print("%d cases x %d calls: %d kernel launches" % (len(CASES), W.CALLS_PER_CASE, n))
    assert n <= W.MAX_KERNELS == 1500
    assert len(W.FILLS) == 4 and W.CALLS_PER_CASE == 1 + 2 + 2 + 2


def test_every_drop_in_launch_takes_its_workspace_from__workspace():
    """_issue is the one place that sets p.workspace, from _workspace; every entry point and relaunch()'s fast path end in _issue"""
    from vattention_amd import flash_attn as FA
    src = inspect.getsource(FA)
    assert len(re.findall(r"p\.workspace\s*=", src)) == 1
    assert "p.workspace = _workspace(need, dev, st).data_ptr()" in inspect.getsource(FA._issue)
    assert "_issue(p, dev, *fast)" in inspect.getsource(FA.relaunch)
    assert "_issue(" in inspect.getsource(FA._launch) and "_issue(" in inspect.getsource(FA._launch_tree)
    for fn in (FA.flash_attn_fp8kv_with_kvcache, FA.flash_attn_fp8kv_tree_with_kvcache, FA.flash_attn_fp8kv_prefill_with_kvcache, FA.flash_attn_fp8kv_varlen_with_kvcache):
        assert "_issue(" in inspect.getsource(fn)
    for fn in (FA.flash_attn_with_kvcache, FA.flash_attn_varlen_with_kvcache):
        assert "_launch(" in inspect.getsource(fn)
    assert "_launch_tree(" in inspect.getsource(FA.flash_attn_tree_with_kvcache)


def _function_body(text, head):
    i = text.index(head)
    j = text.index("\n}\n", i)
    return text[i:j]


def test_every_split_launch_refuses_a_null_workspace():
    """module docstring: the refusal stands in front of the first launch of every function that launches a plan with a workspace"""
    dec = open(os.path.join(CSRC, "decode_kernels.hip")).read()
    pre = open(os.path.join(CSRC, "prefill_kernels.hip")).read()
    stream = _function_body(dec, "int launch_decode_stream(")
    assert stream.index('if (!p->workspace) return fail(') < stream.index("begin_decode_launch<") < stream.index("hipLaunchKernelGGL(")
    nb = _function_body(dec, "int launch_decode_nb(")
    assert "const int splits = planned ? 2 : pick_splits(" in nb
    assert nb.index("if (splits > 1 && !p->workspace) return fail(") < nb.index("begin_decode_launch<") < nb.index("hipLaunchKernelGGL(")
    pf = _function_body(pre, "int launch_prefill_t(")
    lst = pf.index("p->num_pf_blocks > 0 && (!p->pf_blocks || !p->workspace)")
    assert lst < pf.index("launch_prefill64p(") and lst < pf.index("launch_prefill64(p, st, 1)")
    split = pf.index("if (pl.nsplit > 1 && !p->workspace) return fail(")
    assert split < pf.index("launch_prefill<") and split < pf.index("launch_prefill64(p, st, pl.nsplit)")
    # every case of the table is on a plan one of the four guards: decode path 2 | decode path 0 / 1 | the list | the KV split
    for c, d in CASES:
        assert (d["form"], d["path"]) in ((1, 2), (1, 0), (1, 1), (0, 1), (0, 0)), c["name"]
        if (d["form"], d["path"]) == (1, 0) or (d["form"], d["path"]) == (0, 0):
            assert d["nsplit"] > 1, c["name"]


# ---- the fills and the guarded allocator, on CPU tensors ----
def test_the_guarded_allocator_and_its_fills():
    c, d = next((c, d) for c, d in CASES if d["form"] == 1 and d["path"] == 2)
    p = W.host_block(c)
    regions, need = W.layout(c, d, p), d["workspace_bytes"]
    g = W.GuardedWorkspace()
    g.regions = regions
    tb = regions[0]["nbytes"]
    for fill in ("zero", "ones", "loud"):
        g.fill = fill
        v = g(need, torch.device("cpu"))
        assert v.numel() * 4 == need and v.dtype == torch.float32 and g.buf.numel() * 4 == W.GUARD + need + max(W.GUARD, need)
        assert g.guards_intact() and g.first_damage() is None
        w = g.words()
        table, floats = w[:tb // 4].view(-1, 2), w[tb // 4:]
        if fill == "zero":
            assert not w.any()
        elif fill == "ones":
            assert bool((w == -1).all()) and bool(torch.isnan(floats.view(torch.float32)).all())
        else:
            assert bool((table[:, 0] == 0).all()) and bool((table[:, 1] == 1).all()) and bool((floats.view(torch.float32) == 88.0).all())
    assert g.requests == [need] * 3
    first = v.data_ptr()
    g.fill = None                                        # leftover: the same bytes, untouched
    assert g(need, torch.device("cpu")).data_ptr() == first and bool((g.words()[tb // 4:].view(torch.float32) == 88.0).all())
    # a write 4 bytes past the view — what a `*_workspace_bytes` answer that is 128 bytes short lets the last record's tail do — is seen and located
    g.buf[(W.GUARD + need) // 4] = 0
    assert not g.guards_intact() and g.first_damage() == need
    g.buf[(W.GUARD + need) // 4] = W.CANARY_I32
    g.buf[W.GUARD // 4 - 1] = 0
    assert not g.guards_intact() and g.first_damage() == -4


def test_other_lens_change_something_and_stay_in_range():
    changed = 0
    for c, _ in CASES:
        cl = W.lens_before(c)
        o = W.other_lens(c)
        assert len(o) == len(cl) and max(o) <= max(cl) and min(o) >= 0, c["name"]
        if c["form"] in ("pre", "var"):
            assert all(n + W.appended_rows(c) >= min(m + W.appended_rows(c), q) for n, m, q in zip(o, cl, W.C.case_qlens(c))), c["name"]
        else:
            assert o != cl or max(cl) <= 1, c["name"]
        changed += o != cl
    assert changed >= len(CASES) - 2
