"""The twin-call rotary probe (tests/rope_twin.py) proved without a GPU: the identity table is exact on every case's operands; the positions
of the case table are the header's rule, restated here independently, and end at the last table row; a position off by one for one query row
or one new key row, an un-rotated second head block and a piece rotated at its piece-relative row each change output BITS in the affected
rows (f32-math oracle, cast to the I/O dtype); every case's plan description on a host-only parameter block is the one it names — a
table-carrying persistent work list describes as one workgroup per piece; an injected single-bit difference fails the comparison by name."""
import pytest
import torch

from tests import census as C
from tests import rope_twin as RT
from vattention_amd import kernels as K

CASES = RT.cases()
IDS = [c["name"] for c in CASES]
_twins = {}


def _twin(c):
    if c["name"] not in _twins:
        _twins.clear()          # (one at a time: the tests of a case run back to back)
        _twins[c["name"]] = RT.build(c)
    return _twins[c["name"]]


def test_case_table_shape():
    assert 150 <= len(CASES) <= 400
    for c in CASES:
        assert max(c["lens"]) <= 1100 and max(C.case_qlens(c)) <= 600, c["name"]
        assert c["dt"] in C.DT and c["D"] in (64, 128)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_identity_table_is_exact_and_positions_follow_the_header(case):
    c, t = case, _twin(case)
    ident = RT.table_view(t["I"], c)
    ql, s = C.case_qlens(c), RT.sn(c)
    # include/vattn_kernels.h: "Token i of batch entry b sits at position cache_seqlens[b] + i (new keys) resp. (visible keys - seqlen_q) + i
    # (queries)", restated: visible keys = cache_seqlens + seqlen_knew; the batched-chunk form: cache_seqlens[i] - q_lens[i] + row
    kpos, qpos = RT.positions(c)
    top = -1
    for b, cache_len in enumerate(t["cl"]):
        visible = cache_len + s
        assert visible == c["lens"][b]
        for i in range(s):
            assert kpos[b][i] == cache_len + i
        for i in range(ql[b]):
            assert qpos[b][i] == (visible - ql[b]) + i
        top = max([top] + [x for x in kpos[b] + qpos[b]])
    P = RT.table_rows(c)
    assert P - 1 == max(top, 0) and ident.shape == (P, c["D"]) and RT.table_view(t["R"], c).shape == (P, c["D"])
    # the guard rows and the column slice
    for a in (t["R"], t["I"]):
        assert bool(torch.isnan(a[:RT.GUARD].float()).all()) and bool(torch.isnan(a[-RT.GUARD:].float()).all())
        assert RT.table_view(a, c).stride(0) == (2 if c["colslice"] else 1) * c["D"] and (RT.table_view(a, c).stride(0) * 2) % 16 == 0
    for x in (t["q_raw"], t["knew_raw"]):
        assert x is None or bool((x != 0).all()), "the un-rotated operands hold no zero"
    for x in (t["q_rot"], t["knew_rot"], t["k_clean"]):
        assert x is None or RT.neg_zeros(x) == 0, "a rotated operand holds -0, which the identity rotation does not preserve"
    # rotary_embedding_ref with the identity table returns its input bit for bit, at every live position, for q and the new keys of both sides
    for b in range(len(ql)):
        for x, pos in ((t["q_raw"][b, :ql[b]], qpos[b]), (t["q_rot"][b, :ql[b]], qpos[b])) + (((t["knew_raw"][b], kpos[b]), (t["knew_rot"][b], kpos[b])) if s else ()):
            assert not RT.bit_diff(RT.rotate(x, pos, ident), x, "identity rotation, entry %d" % b)
    # the rows the call appends hold the rotated keys and the un-rotated values; in front of the call they are poisoned
    for b, slot in enumerate(c["slots"]):
        L = c["lens"][b]
        if s:
            assert torch.equal(t["k_after"][slot, L - s:L], t["knew_rot"][b]) and torch.equal(t["v_after"][slot, L - s:L], t["v_new"][b])
            assert bool(torch.isnan(t["k_before"][slot, L - s:L].float()).all()) and bool(torch.isinf(t["v_before"][slot, L - s:L].float()).all())
        assert bool(torch.isnan(t["k_after"][slot, L:].float()).all()) and bool(torch.isinf(t["v_after"][slot, L:].float()).all())


def _rows_differ(c, a, b, rows, what):
    """out a / b [B, Sq, Hq, D] differ in bits in every (entry, row) of `rows` — in the heads `heads` when given"""
    assert rows, what
    for b_, r, heads in rows:
        x, y = a[b_, r], b[b_, r]
        if heads is not None:
            x, y = x[heads], y[heads]
        assert RT.bit_diff(x.unsqueeze(0).unsqueeze(0), y.unsqueeze(0).unsqueeze(0), what), "%s: %s: entry %d row %d is blind to it" % (c["name"], what, b_, r)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_sees_each_fault_the_probe_is_for(case):
    c, t = case, _twin(case)
    ql, s, G = C.case_qlens(c), RT.sn(c), c["G"]
    kpos, qpos = RT.positions(c)
    tab = RT.table_view(t["R"], c)
    P = tab.shape[0]
    base, _ = RT.oracle(c, t, "f32")
    # one query row at position +- 1 (a live row of the longest entry)
    b = max(range(len(ql)), key=lambda i: c["lens"][i])
    r = ql[b] - 1
    ran = {"query": 0, "key": 0}
    for step in (1, -1):
        if not 0 <= qpos[b][r] + step < P:
            continue
        q2 = [list(x) for x in qpos]
        q2[b][r] += step
        o, _ = RT.oracle(c, t, "f32", q=RT.build(c, qpos=q2)["q_rot"])
        _rows_differ(c, base, o, [(b, r, None)], "query row at position %+d" % step)
        ran["query"] += 1
    # one new key row at position +- 1: every row that sees it
    if s:
        for step in (1, -1):
            if not 0 <= kpos[b][s - 1] + step < P:
                continue
            k2 = [list(x) for x in kpos]
            k2[b][s - 1] += step
            o, _ = RT.oracle(c, t, "f32", k=RT.build(c, kpos=k2)["k_clean"])
            j = c["lens"][b] - 1
            see = [(b, i, None) for i in range(ql[b]) if (lambda lo_hi: lo_hi[0] <= j < lo_hi[1])(C.visible_interval(ql[b], c["lens"][b], i, c["causal"], c.get("left")))]
            _rows_differ(c, base, o, see, "new key row at position %+d" % step)
            ran["key"] += 1
    assert ran["query"] >= 1 and (ran["key"] >= 1 or not s), "%s: no position +- 1 lies inside the table: nothing was perturbed (%s)" % (c["name"], ran)
    # the second head block (heads 16 .. of a kv head) left un-rotated
    if G > 16:
        def second_block_raw(b_, q_b, pos, table):
            out = RT.rotate(q_b, pos, table)
            hq = out.shape[1]
            keep = [h for h in range(hq) if 16 <= h % G < 32]
            out[:, keep] = q_b[:, keep]
            return out
        o, _ = RT.oracle(c, t, "f32", q=RT.build(c, rot_q=second_block_raw)["q_rot"])
        # per head and per row of every entry that sees at least two keys (with one key the output is that key's value whatever q holds):
        # ONE head of the block left raw must show
        two = lambda e, i: (lambda lo_hi: lo_hi[1] - lo_hi[0] >= 2)(C.visible_interval(ql[e], c["lens"][e], i, c["causal"], c.get("left")))
        _rows_differ(c, base, o, [(e, i, [h]) for e in range(len(ql)) for i in range(ql[e]) if two(e, i) for h in range(c["Hkv"] * G) if 16 <= h % G < 32],
                     "second head block un-rotated")
    # a piece's rows at their piece-relative position: the rows of a query block behind the first (128-row blocks of the 4-wave tiling,
    # 256-row blocks of the others and of the work list) rotated as if the block started at row 0
    bm = 128 if c["tiling"] == 4 else 256
    if c["form"] in ("pre", "var") and ql[b] > bm:
        q2 = [list(x) for x in qpos]
        for i in range(bm, ql[b]):
            q2[b][i] = max(qpos[b][i] - bm, 0)
        o, _ = RT.oracle(c, t, "f32", q=RT.build(c, qpos=q2)["q_rot"])
        _rows_differ(c, base, o, [(b, i, None) for i in range(bm, ql[b]) if qpos[b][i] - bm >= 0 and qpos[b][i] >= 0], "a piece rotated at its piece-relative rows")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_on_a_host_only_block(case):
    c = case
    p, lst = RT.host_block(c)
    d = K.describe(p)
    RT.check_plan(c, p, d, lst)
    nb, groups = RT.head_blocks(c)
    if c["form"] == "dec":
        assert d["form"] == 1 and d["tiling"] == nb
    else:
        assert d["form"] == 0      # (2 - 8 query rows with a table: the multi-token gate keeps the prefill form)
    if c.get("pf"):
        # the same list WITHOUT a table keeps its persistent workgroups; with one it is one workgroup per piece
        bare, _ = RT.host_block(c, with_table=False)
        assert K.describe(bare)["workgroups"] == (lst[3] if c["pf"]["persistent"] else lst[0])
        assert d["workgroups"] == lst[0] and d["path"] == 1 and d["tiling"] == 7
        assert any(it.qb > 0 for it in lst[4]), "no piece starts behind the first query block"
        if c["pf"]["persistent"]:
            assert 0 < lst[3] < lst[0], "the persistent request must group several pieces per workgroup, or the rule is not exercised"
    if c["form"] == "pre" and 2 <= c["sq"] <= 8:
        bare, _ = RT.host_block(c, with_table=False)
        assert K.describe(bare)["form"] == 1, "without a table the same block takes the multi-token form"


def test_coverage_list_is_satisfiable_by_the_table():
    reached = {}
    for c in CASES:
        p, _ = RT.host_block(c)
        reached[RT.union_key(c, K.describe(p))] = 1
    assert not RT.missing(reached), RT.missing(reached)
    assert RT.missing({k: 1 for k in reached if k[0] != "var"}), "the coverage check must notice a missing family"
    assert sum(1 for c in CASES if c["lab"]) <= 4 and all(K.needs_lab(c["variant"]) == c["lab"] for c in CASES)
    for fam in ("dec", "pre", "var"):
        assert any(c["form"] == fam and c["table"] == "real" for c in CASES) and any(c["form"] == fam and c["colslice"] for c in CASES)
    assert any(c["form"] == "dec" and not c["append"] and 0 in c["lens"] for c in CASES), "one decode case carries a dead entry"
    # rows in front of position 0 (the side of the kernels' position test that skips the rotation): every prefill build — dtype, head
    # dimension, tiling — runs them causal (no visible key) and non-causal (every key, un-rotated q); the dead decode entry in every dtype / d
    for dt in C.DT:
        for D in (64, 128):
            assert any(c["form"] == "dec" and c["dt"] == dt and c["D"] == D and 0 in c["lens"] for c in CASES), (dt, D)
            for tiling in (1, 4, 7) if D == 128 else (1, 4):
                for causal in (True, False):
                    assert any(c["form"] == "pre" and (c["dt"], c["D"], c["tiling"], c["causal"]) == (dt, D, tiling, causal) and
                               min(min(x) for x in RT.positions(c)[1]) < 0 for c in CASES), (dt, D, tiling, causal)
    # every row of the table exists in both dtypes
    strip = lambda n: n.replace("bf16", "f16")
    assert sorted(strip(c["name"]) for c in CASES if c["dt"] == "bf16") == sorted(c["name"] for c in CASES if c["dt"] == "f16")


def test_an_injected_bit_fails_the_comparison_by_name():
    c = next(x for x in CASES if x["name"] == "pre_few_f16_d128_sq5_hkv2")
    t = _twin(c)
    out, lse = RT.oracle(c, t, "f32")
    bad = out.clone()
    bad.view(torch.int16)[2, 3, 5, 17] ^= 1
    msg = RT.bit_diff(out, bad, "out")
    assert msg and "1 of" in msg[0] and "entry 2 row 3 head 5 element 17" in msg[1]
    assert not RT.bit_diff(out, out.clone(), "out")
    l32 = lse.float()
    bad = l32.clone()
    bad.view(torch.int32)[1, 6, 4] ^= 1
    msg = RT.bit_diff(l32, bad, "lse", "bhs")
    assert msg and "entry 1 row 4 head 6" in msg[1]
    k = t["k_after"]
    bad = k.clone()
    bad.view(torch.int16)[c["slots"][0], 2, 1, 9] ^= 1
    assert "slot %d row 2 head 1 element 9" % c["slots"][0] in RT.bit_diff(k, bad, "k cache", "cache")[1]
    nan = torch.full((1, 1, 1, 4), float("nan"), dtype=torch.float16)
    assert not RT.bit_diff(nan, nan.clone(), "NaN rows compare by their bits")

