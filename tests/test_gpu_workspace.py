"""Workspace probes on the GPU (tests/workspace_probe.py: the case table, the layout, the fills, the guarded allocator; the host side is
tests/test_workspace_probe_model.py).  One test per case.  The case runs once through the unpatched drop-in (its 1 MiB workspace); then the
very parameter block it launched is issued again through flash_attn._issue — with flash_attn._workspace replaced by the guarded allocator
(monkeypatch), a fresh `out` whose rows carry one extra head of padding, and a fresh softmax_lse, both preset to the canary between 4 KiB
bands — under each fill.  Every call runs on the current stream and is synchronised before anything is compared.

1. CONTROL: two calls with zero-filled exact-size workspaces give `out`, softmax_lse and the caches bit for bit equal to each other and to the
   unpatched drop-in's (the batched-chunk entry returns no LSE: there the two zero fills are compared); the result passes the case's own
   expectation — the closed-form census (tests/census.py / tests/census_fp8_tree.py `compare`, <= 1 ulp), or for the score-range cases
   tests/census.py `check` / `check_lse` against the float64 reference.
2. SIZE AND FOOTPRINT, after every call: both 64 KiB+ guards of the workspace are the canary; the request equals the plan description's
   workspace_bytes (of the launched block, and of the host-only block) and the matching `*_workspace_bytes` export; the bands round `out` and
   softmax_lse, the padding head of every `out` row and the LSE rows beyond an entry's q_lens are untouched; the caches — appended rows and
   every byte outside them — are the expected ones.
3. FILL INDEPENDENCE: `ones`, `loud` and `leftover` give `out` and softmax_lse bit for bit equal to the control.
4. WINDOW SHARES: the windowed one-token decode cut into more shares than it has visible tiles and its multi-token twins
   (num_empty_piece_*) are cases of the table and get the same fills.

PLANS PROBED, by plan description — (entry point, form, path, tiling, merge launch); form 1 = decode (one token, multi-token, tree), 0 =
prefill; entry points plain / cap (softcap) / tree / fp8 / fp8tree / fp8pre (prefill over an fp8 cache):
  decode path 0 (uniform grid split, nsplit > 1), tilings 1 and 2: plain, cap, tree, fp8, fp8tree — windowed and not (plain, cap)
  decode path 1 (host items), tilings 1 and 2: plain
  decode path 2 (device-planned stream: the int2 table and the records), tilings 1 and 2: plain, cap, tree, fp8, fp8tree — windowed and not
      (plain, cap); with an entry of cache_seqlens == 0 beside live ones: every build, one-token and multi-token (R = 16), f16 and bf16
  prefill path 0 (KV split, nsplit > 1): tilings 1, 4, 7 plain; 1, 4 cap and fp8pre; batched chunks with two shares: plain, cap, fp8pre
  prefill path 1 (work list with split blocks, tiling 7): one workgroup per piece, persistent with assigned and with drawn queues
88 cases, one (dtype, d) per plan (see tests/workspace_probe.py), 7 calls each.

BIT EQUALITY: no plan fell back.  Every plan — the persistent prefill with drawn queues included, which nobody had measured: its merge adds the
shares in share order whichever workgroup drew them — gives the same bits on two identical calls and under every fill.

BUGS FOUND: none.  No fill changes a bit of `out` or softmax_lse on any of the 88 cases, no call writes outside its workspace bytes, the
padding and bands of `out` / softmax_lse or the cache rows it does not append, and every request equals the plan description's
workspace_bytes.  In particular the table entry of a sequence without a visible key IS written (the stream plan gives an empty sequence one
masked tile, csrc/decode_body.h:711, whose owner publishes it), and every workgroup of a grid split writes its partial rows, -inf for an empty
key range.  The fill-independence tests found nothing; they were not run against a mutant.
SENSITIVITY of the guard assertion, without a fault: on a scratch copy whose decode path-0 workspace formula answers 128 bytes less,
num_empty_piece_f16_dec fails with "the call wrote outside its 264064 workspace bytes, first at byte offset 264064" (the last 32 lse_part
words land in the high guard, inside the test's own buffer); the stream-path case beside it, whose formula was left alone, passes.

MEASURED on one MI355X: 88 cases, whole file 4.2 s; tests/test_gpu_census.py on the same box in the same visit: 697 tests, 7.7 s.
"""
import pytest
import torch

from tests import census as C
from tests import census_fp8_tree as X
from tests import workspace_probe as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = W.cases()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _dead_note(c, b):
    notes = []
    if c["lens"][b] == 0:
        notes.append("entry %d has no visible key" % b)
    elif "empty" in c["name"]:
        notes.append("a piece of this case is empty by construction")
    if c["form"] in ("mt", "tree") and c["lens"][b] < C.case_qlens(c)[b]:
        notes.append("entry %d has rows without a visible key" % b)
    return "; ".join(notes) or "entry %d and its pieces all have visible keys, as far as the table knows" % b


def _same(call, c, d, fill, got, ref):
    """out and lse of a fill against the control, bit for bit; the message names case, plan, fill, the first differing (entry, row, head) and
    whether that entry is dead"""
    (out, lse), (out_r, lse_r) = got, ref
    where = call.first_difference(out, out_r)
    if where is None and not torch.equal(_bits(lse), _bits(lse_r)):
        i = torch.nonzero(_bits(lse) != _bits(lse_r))[0]
        where = (int(i[0]), int(i[2]), int(i[1]))
        what = "softmax_lse %r vs %r" % (float(lse[tuple(i)]), float(lse_r[tuple(i)]))
    elif where is not None:
        o, r = call.canonical(out, None)[0][where], call.canonical(out_r, None)[0][where]
        what = "out max |diff| %.6g (first elements %s vs %s)" % (float((o.float() - r.float()).abs().nan_to_num(nan=float("inf")).max()), o[:4].tolist(), r[:4].tolist())
    assert where is None, "%s: plan %s: fill %r changes the result: first difference at (entry %d, row %d, head %d): %s; %s" % (
        c["name"], d, fill, where[0], where[1], where[2], what, _dead_note(c, where[0]))


def _expectation(call, c, out, lse, numerics, what):
    out_c, lse_c = call.canonical(out, lse)
    if numerics is not None:
        q, kc, vc = numerics
        ref64, lse64 = C.reference(c, q, kc, vc, "f64", return_lse=True)
        ref32 = C.reference(c, q, kc, vc, "f32")
        assert bool(torch.isfinite(out_c.float()).all()), what
        C.check(out_c, ref64, ref32, C.DT[c["dt"]], what)
        C.check_lse(lse_c, lse64, what)
        return
    fails, stats = X.compare(out_c, lse_c, c)
    assert not fails, what + "\n  " + "\n  ".join(fails)
    assert stats["max_ulp"] <= 1.0, what


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c, _ in CASES])
def test_workspace(case, monkeypatch):
    from vattention_amd import flash_attn as FA
    c, d_host = case
    numerics = C.numerics_inputs(c) if c.get("kind") else None
    call = W.Call(c, DEV, numerics)
    out0, lse0 = call.first_call()                                        # the unpatched drop-in: its own (1 MiB) workspace
    p = call.issued[0]
    d = W.describe_block(c, p)
    what = "%s: plan %s" % (c["name"], d)
    assert d == d_host, "%s: the host-only block describes %s" % (what, d_host)
    need = d["workspace_bytes"]
    assert need == W.workspace_bytes_export(c, p) > 0, what
    assert call.caches_intact(), what + ": the caches after the drop-in's call"
    regions = W.layout(c, d, p)
    guard = W.GuardedWorkspace()
    guard.regions = regions
    monkeypatch.setattr(FA, "_workspace", guard)

    def run(fill, block=None):
        guard.fill = fill
        n = len(guard.requests)
        out, lse, damage = call.reissue(block)
        assert guard.requests[n:] == [need], "%s: fill %r: the call asked for %s bytes" % (what, fill, guard.requests[n:])
        assert guard.guards_intact(), "%s: fill %r: the call wrote outside its %d workspace bytes, first at byte offset %s" % (what, fill, need, guard.first_damage())
        assert not damage, "%s: fill %r: %s" % (what, fill, "; ".join(damage))
        return out, lse

    # 1. control
    a, b = run("zero"), run("zero")
    _same(call, c, d, "zero (second call)", b, a)
    assert call.first_difference(a[0], out0) is None, what + ": the exact-size zero-filled workspace gives another `out` than the drop-in's own"
    if lse0 is not None:
        assert torch.equal(_bits(a[1]), _bits(lse0)), what + ": softmax_lse differs from the drop-in's own"
    _expectation(call, c, a[0], a[1], numerics, what)
    # 3. fill independence (2. is asserted by run() after every call)
    for fill in ("ones", "loud"):
        _same(call, c, d, fill, run(fill), a)
    block, hold = call.leftover_block()
    run("zero", block)                                                    # the same plan with other lengths and V negated ...
    _same(call, c, d, "leftover", run(None), a)                           # ... then the case in the bytes it left
    del hold
    assert len(guard.requests) == W.CALLS_PER_CASE - 1
