"""The prefill host path, pinned on a CPU (no stopwatch, no device): what vattn_attn_plan_describe and vattn_attn_workspace_bytes answer for
~400 prefill-form blocks, which work lists vattn_prefill_plan / vattn_prefill_plan_wg build for ~200 launches, and the argument errors the
prefill launch returns before it touches the device.  tests/golden/prefill_plan_pins.json holds the blocks AND the answers; it was written
by the library of the commit it names (`parent`), before the host code of csrc/prefill*_kernels.hip was restructured, and a later change
of that host code must keep every answer.  test_plan_table.py pins the shapes the benchmarks launch; this file pins the corners: every
value of variant bits 1-3 (also the tilings only the measurement build runs, which describe still normalises) x bits 5-6, forced share
counts, windows, the work-list fields with the persistent-eligibility rules, caps that make the planner give up, d = 64.
Regenerate ONLY after a deliberate change of the plans: VATTN_REGEN_PLAN_PINS=<commit id of the library that answers> pytest <this file>."""
import ctypes as C
import hashlib
import json
import os
import random

from vattention_amd import kernels as K

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "prefill_plan_pins.json")
HEADS = [(32, 4), (8, 1), (32, 8), (28, 4), (14, 2), (32, 1), (64, 1), (71, 1)]      # test_plan_table.py's head pairs, and Falcon's 71 / 1
DESC = ("form", "path", "tiling", "nsplit", "workgroups", "merge_launch", "workspace_bytes")
PTR = 4096      # a fake, non-null, 16-byte-aligned pointer: describe, the workspace query and the checks below never dereference one


def _block(fields):
    p = K.AttnParams()
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _answer(fields):
    p = _block(fields)
    d = K.describe(p)
    return [d[n] for n in DESC] + [int(K.klib().vattn_attn_workspace_bytes(C.byref(p)))]


def _describe_cases(n_want=400):
    """Seeded draw; blocks that take the multi-token form (describe: form 1) are skipped and counted."""
    rnd = random.Random(20261018)
    out, skipped, i = [], 0, 0
    while len(out) < n_want:
        h, h_k = rnd.choice(HEADS)
        sq = rnd.choice([rnd.randint(2, 8), rnd.randint(2, 300), rnd.randint(2, 4096), rnd.randint(2, 32768), rnd.choice([128, 256, 257, 2048, 8192, 32768])])
        cache = rnd.choice([0, 0, rnd.randint(0, 4096), rnd.randint(0, 131072), 131072])
        causal = rnd.choice([1, 1, 0])
        f = dict(d=rnd.choice([64, 128, 128]), h=h, h_k=h_k, b=rnd.randint(1, 4), seqlen_q=sq, seqlen_k=cache + sq, is_causal=causal,
                 num_splits=rnd.choice([0, 0, 1, 2, 5, 16, 40]), variant=((i % 8) << 1) | (((i // 8) % 4) << 5),      # bits 1-3 x bits 5-6: all 32
                 o_row_stride=h * 128, o_head_stride=128, o_batch_stride=sq * h * 128)
        if rnd.random() < 0.5:
            f["max_seqlen_k_hint"] = cache + sq
        if causal:
            f["window_left_plus1"] = rnd.choice([0, 0, 1, 300, 5000])
        if rnd.random() < 0.1:
            f["seqlen_knew"] = rnd.choice([1, sq])
        # the work-list fields (a window excludes them at validate(); describe answers for whatever it is given) and the rules of the
        # persistent form: pf_num_wg > 0, no fused rotary, output strides in multiples of 8
        if rnd.random() < 0.35:
            items = rnd.randint(1, 3000)
            f.update(pf_items=PTR, num_pf_items=items, num_pf_blocks=rnd.choice([0, 0, rnd.randint(1, 400)]), pf_part_rows=rnd.choice([0, 256 * rnd.randint(2, 900)]))
            if f["num_pf_blocks"]:
                f["pf_blocks"] = PTR
            if rnd.random() < 0.7:
                f["pf_num_wg"] = rnd.choice([8, 64, 256, min(items, 248)])
                if rnd.random() < 0.5:
                    f["pf_wg_first"] = PTR
        if rnd.random() < 0.2:
            f.update(rotary_cos_sin=PTR, rotary_dim=f["d"], rotary_row_stride=f["d"])
        if rnd.random() < 0.15:
            f[rnd.choice(["o_row_stride", "o_head_stride", "o_batch_stride"])] = rnd.choice([4, 132, h * 128 + 4])
        if rnd.random() < 0.1:
            f.update(q_lens=PTR, q_start=PTR)
        i += 1
        ans = _answer(f)
        if ans[0] != 0:
            skipped += 1
            continue
        out.append({"p": f, "want": ans})
    return out, skipped


def _work_list(c):
    """One planner call -> [return value, counts..., digest of the items, the blocks and the queue table] (as test_plan_table._work_list_digest)."""
    p = K.AttnParams()
    B, q_lens, k_lens = len(c["k"]), c["q"], c["k"]
    p.b, p.seqlen_q, p.h, p.h_k, p.d, p.is_causal, p.seqlen_k, p.num_splits = B, max(q_lens), c["h"], c["h_k"], c["d"], c["causal"], max(k_lens), -c["T"]
    items, blocks = (K.PrefillItem * max(c["cap_i"], 1))(), (K.PrefillItem * max(c["cap_b"], 1))()
    ql = None if c["q_null"] else (C.c_int32 * B)(*q_lens)
    kl = (C.c_int32 * B)(*k_lens)
    if c["mode"] == 0:
        counts = (C.c_int32 * 3)()
        n = K.klib().vattn_prefill_plan(C.byref(p), ql, kl, items, c["cap_i"], blocks, c["cap_b"], counts)
        wf = b""
    else:
        counts = (C.c_int32 * 4)()
        wg = (C.c_int32 * 257)()
        n = K.klib().vattn_prefill_plan_wg(C.byref(p), ql, kl, items, c["cap_i"], blocks, c["cap_b"], wg if c["mode"] == 1 else None, c["max_wg"], counts)
        wf = bytes(wg)
    h = hashlib.sha256()
    h.update(bytes(items)[:max(n, 0) * C.sizeof(K.PrefillItem)] + bytes(blocks)[:counts[1] * C.sizeof(K.PrefillItem)] + wf)
    return [n] + list(counts) + [h.hexdigest()[:16]]


def _work_list_cases(n_want=200):
    """mode 0 per piece, 1 assigned queues, 2 drawn queues; T > 0 forces the piece length (num_splits = -T)."""
    rnd = random.Random(20261019)
    out = []
    for i in range(n_want):
        h, h_k = rnd.choice(HEADS[:5] + [(64, 8), (16, 16), (12, 3)])      # (kv heads that do and do not divide the 8 XCDs; heads that are no multiple of 8)
        B = rnd.choice([1, 1, 2, 3, 4])
        top = rnd.choice([700, 5000, 12000, 30000])
        q_lens = [rnd.randint(2, top) for _ in range(B)]
        kind = rnd.random()
        q_null = kind < 0.12
        if q_null or kind < 0.3:
            q_lens = [q_lens[0]] * B                                     # an equal batch; with q_lens NULL every entry has seqlen_q rows
        k_lens = [q + (rnd.randint(0, 100000) if rnd.random() < 0.3 else 0) for q in q_lens]
        if rnd.random() < 0.05:
            k_lens[0] = max(1, q_lens[0] - rnd.randint(1, 300))          # fewer keys than rows: the first blocks see nothing
        mode = i % 3
        nblk = sum((q + 255) // 256 for q in q_lens) * h
        c = dict(h=h, h_k=h_k, q=q_lens, k=k_lens, q_null=q_null, mode=mode, max_wg=rnd.choice([0, 8, 64, 256]) if mode else 0,
                 T=rnd.choice([0, 0, 0, 4, 9, 16, 40]), causal=rnd.choice([1, 1, 1, 0]), d=64 if rnd.random() < 0.04 else 128,
                 cap_i=17 * nblk + 16, cap_b=nblk + 16)
        cap = rnd.random()
        if cap < 0.06:
            c["cap_i"] = max(1, nblk // 2)                               # too few items: the planner gives up (returns 0)
        elif cap < 0.12:
            c["cap_b"], c["T"] = 1, c["T"] or 9                          # too few blocks for a list that cuts
        elif cap < 0.16:
            c["cap_i"] = nblk + rnd.randint(0, 3)                        # room for the uncut list only
        out.append(c)
    return out


def _fake_tensors(f):
    f.update(q=PTR, out=PTR, k_cache=PTR, v_cache=PTR, q_row_stride=f["h"] * f["d"], o_row_stride=f["h"] * f["d"], q_head_stride=f["d"],
             o_head_stride=f["d"], k_head_stride=f["d"], v_head_stride=f["d"], k_row_stride=f["h_k"] * f["d"], v_row_stride=f["h_k"] * f["d"])
    return f


def _error_cases():
    """Returns of launch_prefill_t in front of its first launch.  k_new stays NULL (no append launch), so nothing here reaches the device:
    validate() passes, then the argument check of the work-list launch or the workspace check of the KV split answers."""
    base = dict(b=1, seqlen_q=2048, seqlen_k=32768, h=8, h_k=1, d=128, is_causal=1)
    return [
        _fake_tensors(dict(base, pf_items=PTR, num_pf_items=0)),                                             # a list without a length
        _fake_tensors(dict(base, pf_items=PTR, num_pf_items=64, num_pf_blocks=8)),                           # split blocks without pf_blocks
        _fake_tensors(dict(base, pf_items=PTR, num_pf_items=64, num_pf_blocks=8, pf_blocks=PTR)),            # ... and without a workspace
        _fake_tensors(dict(base, max_seqlen_k_hint=32768)),                                                  # the plan splits the key range; no workspace
        _fake_tensors(dict(base, d=64, h=32, h_k=8, seqlen_q=512, num_splits=4)),                            # forced shares, d = 64
    ]


def _error(f):
    rc = K.klib().vattn_flash_attn_with_kvcache(C.byref(_block(f)), None)
    return [rc, K.last_error()]


def _golden():
    regen = os.environ.get("VATTN_REGEN_PLAN_PINS")
    if regen:
        blocks, skipped = _describe_cases()
        lists = _work_list_cases()
        errors = _error_cases()
        json.dump({"parent": regen, "multitoken_blocks_skipped": skipped, "describe_fields": list(DESC) + ["vattn_attn_workspace_bytes"], "blocks": blocks,
                   "work_lists": [{"case": c, "want": _work_list(c)} for c in lists], "errors": [{"p": f, "want": _error(f)} for f in errors]},
                  open(GOLDEN, "w"), separators=(",", ":"))
    return json.load(open(GOLDEN))


def test_describe_and_workspace_answers_are_the_pinned_ones():
    g = _golden()
    assert len(g["blocks"]) >= 400 and len(g["parent"]) >= 7
    bad = [(c["p"], c["want"], _answer(c["p"])) for c in g["blocks"] if _answer(c["p"]) != c["want"]]
    assert not bad, (len(bad), bad[:3])
    # the draw covers what it is there for: both head dimensions, every tiling x order selector, splits, windows, lists on persistent workgroups or not
    ps = [c["p"] for c in g["blocks"]]
    assert {(p["variant"] >> 1) & 7 for p in ps} == set(range(8)) and {(p["variant"] >> 5) & 3 for p in ps} == set(range(4)) and {p["d"] for p in ps} == {64, 128}
    assert {c["want"][2] for c in g["blocks"]} == {1, 4, 7} and max(c["want"][3] for c in g["blocks"]) == 16
    lists = [c for c in g["blocks"] if c["want"][1] == 1]
    assert any(c["want"][4] == c["p"].get("pf_num_wg", 0) > 0 for c in lists)
    assert any(c["p"].get("pf_num_wg", 0) > 0 and c["p"].get("rotary_cos_sin") and c["want"][4] == c["p"]["num_pf_items"] for c in lists)
    assert any(c["p"].get("pf_num_wg", 0) > 0 and not c["p"].get("rotary_cos_sin") and c["want"][4] == c["p"]["num_pf_items"] != c["p"]["pf_num_wg"] for c in lists)


def test_work_lists_are_the_pinned_ones():
    g = _golden()
    assert len(g["work_lists"]) >= 200
    bad = [(c["case"], c["want"], _work_list(c["case"])) for c in g["work_lists"] if _work_list(c["case"]) != c["want"]]
    assert not bad, (len(bad), bad[:3])
    want = [c for c in g["work_lists"]]
    for mode in (0, 1, 2):
        assert sum(1 for c in want if c["case"]["mode"] == mode and c["want"][0] > 0) >= 20, mode
    assert sum(1 for c in want if c["want"][2] > 0) >= 40                                  # lists that cut blocks
    assert any(c["want"][0] == 0 and c["case"]["d"] == 64 for c in want)
    nblk = lambda c: sum((q + 255) // 256 for q in c["q"]) * c["h"]
    assert any(c["want"][0] == 0 and c["case"]["d"] == 128 and c["case"]["cap_i"] < nblk(c["case"]) for c in want)      # cap_items hit
    assert any(c["want"][0] == 0 and c["case"]["d"] == 128 and c["case"]["cap_b"] == 1 and c["case"]["cap_i"] > nblk(c["case"]) for c in want)      # cap_blocks hit
    assert any(c["want"][0] > 0 and c["case"]["q_null"] for c in want) and any(c["want"][0] > 0 and c["case"]["T"] for c in want)


def test_prefill_launch_argument_errors_are_the_pinned_ones():
    g = _golden()
    assert [c["p"] for c in g["errors"]] == _error_cases()                                   # (exactly these blocks: none of them reaches a launch)
    got = [_error(c["p"]) for c in g["errors"]]
    assert got == [c["want"] for c in g["errors"]]
    assert [rc for rc, _ in got] == [-11] * 5
    assert {msg for _, msg in got} == {"pf_items needs num_pf_items, and pf_blocks + a workspace when blocks are split",
                                       "KV-split prefill needs a workspace (vattn_attn_workspace_bytes)"}
