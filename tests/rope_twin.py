"""Twin-call probes of the fused rotary embedding — shared by tests/test_rope_twin_model.py (CPU: proves the probe) and
tests/test_gpu_rope_twin.py.  The key census (tests/census.py) runs with q = 0 and cannot see a rotation; the parity tests hold a real
cos/sin table to 2e-3, where neighbouring table rows are nearly equal in the low-frequency half.

THE TWIN.  Two calls through the SAME entry point with identical shapes, strides, plan arguments, `_variant`, num_splits, window and host
hints — so the same gate, plan, kernel build and code path (a table changes the route in three places: the multi-token gate, the
persistent-list rule, the bf16 decode_stream_kernel build):
    A  un-rotated q / k_new and a table R of random finite values, uniform in [-1, 1], every row distinct.  The kernels do arithmetic on
       table rows, not trigonometry: a wrong row, element or partner moves every element of the rotated operand.
    B  q / k_new rotated beforehand on the CPU (oracle.attn.rotary_embedding_ref, R) at the positions include/vattn_kernels.h states —
       new key i of entry b at cache_seqlens[b] + i, query row i at (visible keys - seqlen_q) + i — and the IDENTITY table cos = 1, sin = 0.
Under the identity table the kernel's rotation is exact: cvt(x * 1) = x, cvt(y * 0) = +-0, and both sums return their operand unless the
operand is itself +-0 — so the inputs are drawn without zero elements.  A and B then feed bit-equal operands to the same build: out, LSE and
the caches must be BIT-IDENTICAL.  A is anchored to the f64 oracle on the pre-rotated operands with the project's own check.

GUARD ROWS.  Each table is the view [8 : 8 + P) of a NaN-filled allocation, P = the largest position the case uses + 1: a read of row -1 or
row P poisons the output instead of faulting.  `colslice`: the view is also a column slice (row stride 2 D != rotary_dim).

A query row in front of position 0 (an entry without a visible key; Sq > Lk) has no position and no table row: the kernels leave it
un-rotated and read no table row for it (include/vattn_kernels.h).  In a causal or windowed call it sees no key and its output is 0 whatever
q holds; in a non-causal call it attends to every key with its un-rotated q.  The twin leaves such rows un-rotated too, so the oracle states
exactly that."""
import ctypes as CT

import torch

from oracle.attn import make_cos_sin_cache, rotary_embedding_ref
from tests import census as C

SPARE = 8      # poisoned rows of the cache VIEW behind the longest entry
PAD = 4        # poisoned rows of the ALLOCATION behind the view (every call passes a [:, :rows] view)
GUARD = 8      # NaN rows in front of and behind a table


def sn(c):
    """rows the call appends per entry"""
    return (1 if c["form"] == "dec" else c["sq"]) if c["append"] else 0


def positions(c):
    """(positions of the new keys, positions of the query rows) per entry; a negative query position: a row without a visible key"""
    s, ql = sn(c), C.case_qlens(c)
    kpos = [[L - s + i for i in range(s)] for L in c["lens"]]
    qpos = [[L - n + t for t in range(n)] for L, n in zip(c["lens"], ql)]
    return kpos, qpos


def table_rows(c):
    kpos, qpos = positions(c)
    return max([x for e in kpos + qpos for x in e if x >= 0] + [0]) + 1


def head_blocks(c):
    """(16-column head blocks per workgroup, sibling head-block groups) of a decode-form case; (0, 0) for the prefill form"""
    if c["form"] != "dec":
        return 0, 0
    nb = 2 if c["G"] > 16 else 1
    return nb, ((c["G"] + 15) // 16 + nb - 1) // nb


def _case(name, form, dt, D, Hkv, G, sq, lens, path, **kw):
    kw.setdefault("table", "random")
    kw.setdefault("colslice", False)
    kw.setdefault("knew_strided", False)
    kw.setdefault("wg", None)
    kw.setdefault("lab", False)
    return C._case(name, form, dt, D, Hkv, G, sq, lens, path, **kw)


def cases():
    cs = []
    n = 0

    def add(*a, **kw):
        nonlocal n
        n += 1
        kw.setdefault("colslice", n % 3 == 0)
        cs.append(_case(*a, **kw))
    CL = [5, 31, 32, 33, 1000]           # cache_seqlens in FRONT of the call: the new key alone in / last in / first in a tile (0: below)
    for dt in ("f16", "bf16"):
        for D in (128, 64):
            tag = "%s_d%d" % (dt, D)
            # ---------------- one-token decode ----------------
            after = [0 + 1] + [x + 1 for x in CL[1:]]           # visible keys with an append at cache_seqlens 0, 31, 32, 33, 1000
            for ap in (True, False):
                a = "ap" if ap else "noap"
                # G = 4: the stream by default (no append: entry 0 is DEAD — no visible key, q at position -1), a forced grid of one-tile
                # pieces (40 > 32 tiles), the uniform split (B = 1 with num_splits; variant bit 19), host items of one tile
                add("dec_stream_%s_g4_%s" % (tag, a), "dec", dt, D, 2, 4, 1, after if ap else [0] + CL[1:], 2, tiling=1, append=ap, idx=ap, knew_strided=ap)
                add("dec_forced_%s_g4_%s" % (tag, a), "dec", dt, D, 2, 4, 1, after if ap else CL, 2, splits=-40, tiling=1, append=ap, idx=not ap, wg=80)
                add("dec_items_%s_g4_%s" % (tag, a), "dec", dt, D, 2, 4, 1, after if ap else CL, 1, host_tiles=1, tiling=1, append=ap, idx=ap)
            add("dec_split3_%s_g4" % tag, "dec", dt, D, 2, 4, 1, [1001], 0, splits=3, tiling=1, merge=1, append=True, wg=6)
            add("dec_bit19_%s_g4" % tag, "dec", dt, D, 2, 4, 1, after, 0, variant=1 << 19, tiling=1, append=True, idx=True)
            add("dec_real_%s_g4" % tag, "dec", dt, D, 2, 4, 1, after, 2, tiling=1, append=True, idx=True, table="real")
            # G = 20: two head blocks per workgroup (the `for nb` loop rotates the second)
            for Hkv in (1, 2):
                h = "g20_hkv%d" % Hkv
                add("dec_grid_%s_%s" % (tag, h), "dec", dt, D, Hkv, 20, 1, after, 0, tiling=2, append=True, idx=True, knew_strided=True)
                add("dec_forced_%s_%s" % (tag, h), "dec", dt, D, Hkv, 20, 1, CL, 2, splits=-40, tiling=2, wg=40 * Hkv)
                add("dec_items_%s_%s" % (tag, h), "dec", dt, D, Hkv, 20, 1, after, 1, host_tiles=1, tiling=2, append=True)
                add("dec_split3_%s_%s" % (tag, h), "dec", dt, D, Hkv, 20, 1, [1000], 0, splits=3, tiling=2, merge=1, wg=3 * Hkv)
            # sibling head-block groups: 71/1 at d = 64 (three groups), 40/1 at d = 128 (two)
            Gs = 40 if D == 128 else 71
            add("dec_sib_%s_g%d" % (tag, Gs), "dec", dt, D, 1, Gs, 1, after, 0, tiling=2, append=True, idx=True)
            add("dec_sib_split3_%s_g%d" % (tag, Gs), "dec", dt, D, 1, Gs, 1, [1000], 0, splits=3, tiling=2, merge=1, wg=3 * head_blocks(dict(form="dec", G=Gs))[1])
            # the WIN builds: cache_seqlens 39 / left 5 puts the new key (39) into the window's first tile (34 .. 39: tile 1); left 5 is
            # shorter than most sequences, 100 than one, 1005 longer than every sequence (and still below the view's rows: a window)
            wl = [1, 32, 33, 34, 40, 1001]
            for left in (5, 100, 1005):
                add("dec_win%d_%s_g4_stream" % (left, tag), "dec", dt, D, 2, 4, 1, wl, 2, left=left, tiling=1, append=True, idx=bool(left & 1))
                add("dec_win%d_%s_g4_forced" % (left, tag), "dec", dt, D, 2, 4, 1, wl, 2, splits=-40, left=left, tiling=1, append=True, knew_strided=True, wg=80)
                add("dec_win%d_%s_g20_grid" % (left, tag), "dec", dt, D, 1, 20, 1, wl, 0, left=left, tiling=2, append=left != 100, idx=True)
            # ---------------- the prefill form ----------------
            # 2 - 8 query rows with k_new and a table: the gate keeps the prefill form, the multi-row append rotates the new keys
            for sq, Hkv, G in ((2, 1, 4), (5, 2, 4), (8, 3, 2)):
                add("pre_few_%s_sq%d_hkv%d" % (tag, sq, Hkv), "pre", dt, D, Hkv, G, sq, [sq, sq + 31, sq + 700], 0, tiling=4, append=True, idx=True, knew_strided=sq != 5)
            add("pre_few_real_%s" % tag, "pre", dt, D, 2, 4, 5, [5, 36, 705], 0, tiling=4, append=True, idx=True, table="real")
            # chunks with Sn = Sq: 300 rows = a second query block of the 4-wave tiling and a ragged last wave; prefixes 0, 33, 700
            big, small = [300, 333, 1000], [70, 103, 770]
            add("pre_chunk300_%s" % tag, "pre", dt, D, 2, 4, 300, big, 0, tiling=4, append=True, idx=True)
            add("pre_chunk70_%s" % tag, "pre", dt, D, 2, 2, 70, small, 0, tiling=4, append=True, knew_strided=True)
            add("pre_incache_%s" % tag, "pre", dt, D, 2, 4, 300, big, 0, tiling=4, idx=True)      # the keys are in the cache already: q alone rotates
            for variant, tiling in ((2, 1), (8, 4), (14, 7)):
                if tiling == 7 and D != 128:
                    continue
                vt = "%s_t%d" % (tag, tiling)
                bm = 128 if tiling == 4 else 256
                add("pre_chunk300_%s" % vt, "pre", dt, D, 2, 4, 300, big, 0, variant=variant, tiling=tiling, append=True, knew_strided=tiling == 4)
                add("pre_prefix500_%s" % vt, "pre", dt, D, 2, 4, 300, [800], 0, variant=variant, tiling=tiling, append=True)
                add("pre_split3_%s" % vt, "pre", dt, D, 2, 4, 300, big, 0, variant=variant, tiling=tiling, splits=3, merge=1, append=True, idx=True,
                    wg=-(-300 // bm) * 8 * 3 * 3)
                add("pre_full_%s" % vt, "pre", dt, D, 1, 4, 300, big, 0, variant=variant, tiling=tiling, causal=False, append=True)
                add("pre_win100_%s" % vt, "pre", dt, D, 2, 4, 300, big, 0, variant=variant, tiling=tiling, left=100, append=True)
                add("pre_chunk70_%s" % vt, "pre", dt, D, 2, 4, 70, small, 0, variant=variant, tiling=tiling, append=True, idx=True)
                # rows in front of position 0 (Sq > Lk): causal — they see no key — and non-causal — they attend to every key with their un-rotated q
                add("pre_sq_gt_lk_%s" % vt, "pre", dt, D, 2, 2, 150, [90, 149, 150, 1], 0, variant=variant, tiling=tiling)
                add("pre_full_sq_gt_lk_%s" % vt, "pre", dt, D, 2, 2, 150, [90, 149, 150, 1], 0, variant=variant, tiling=tiling, causal=False)
            if D == 128:
                add("pre_real_%s_t7" % tag, "pre", dt, D, 2, 4, 300, big, 0, variant=14, tiling=7, append=True, table="real")
                add("pre_chunk300_%s_v782" % tag, "pre", dt, D, 2, 4, 300, big, 0, variant=782, tiling=7, append=True, lab=True)
            # the batched-chunk entry point: position cache_seqlens[i] - q_lens[i] + row
            vl, vq = [41, 137, 557], [1, 37, 300]
            for variant, tiling in ((0, 4), (2, 1), (14, 7)):
                if tiling == 7 and D != 128:
                    continue
                add("var_%s_t%d" % (tag, tiling), "var", dt, D, 2, 4, 300, vl, 0, qlens=vq, variant=variant, tiling=tiling, idx=tiling != 1)
            add("var_win64_%s" % tag, "var", dt, D, 2, 4, 300, vl, 0, qlens=vq, variant=8, tiling=4, left=64, idx=True)
            if D == 128:
                # work lists: a table sends EVERY list to one workgroup per piece (csrc/prefill_kernels.hip, persistent_list) — also the two
                # persistent kinds, whose tables are built here as for a call without a table
                for pf, kw in (("per_piece", dict(persistent=False, force_tiles=3)), ("assigned", dict(persistent=True, force_tiles=3, drawn=False, max_wg=8)),
                               ("drawn", dict(persistent=True, force_tiles=3, drawn=True, max_wg=8))):
                    add("var_list_%s_%s" % (pf, tag), "var", dt, D, 2, 4, 300, vl, 1, qlens=vq, pf=kw, tiling=7, idx=True, table="real" if pf == "assigned" else "random")
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


# ---------------------------------------------------------------------------------------------------------------------------------------
# twin construction (CPU)
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_table(c, kind, seed=0):
    """the NaN-guarded allocation of a table [GUARD + P + GUARD, D or 2 D]; table_view() is what the call gets"""
    D, dtype, P = c["D"], C.DT[c["dt"]], table_rows(c)
    if kind == "identity":
        body = torch.cat((torch.ones(P, D // 2), torch.zeros(P, D // 2)), dim=1).to(dtype)
    elif kind == "real":
        body = make_cos_sin_cache(D, P, dtype=dtype)
    else:
        g = torch.Generator().manual_seed(90_000 + seed + P + D)
        body = (torch.rand(P, D, generator=g) * 2 - 1).to(dtype)
        assert torch.unique(body, dim=0).shape[0] == P and bool(torch.isfinite(body.float()).all())
    alloc = torch.full((GUARD + P + GUARD, 2 * D if c["colslice"] else D), float("nan"), dtype=dtype)
    alloc[GUARD:GUARD + P, :D] = body
    return alloc


def table_view(alloc, c):
    return alloc[GUARD:alloc.shape[0] - GUARD, :c["D"]]


def rotate(x, pos, table):
    """x [T, H, D] rotated at positions pos (rows with a negative position stay as they are): a new tensor"""
    out = x.clone()
    live = [i for i, p in enumerate(pos) if p >= 0]
    if live:
        D = x.shape[-1]
        sel = x[live].reshape(len(live), -1).clone()
        rotary_embedding_ref(torch.tensor([pos[i] for i in live]), sel, torch.zeros(len(live), D, dtype=x.dtype), D, table)
        out[live] = sel.view(len(live), x.shape[1], D)
    return out


def _nonzero(x):
    return torch.where(x == 0, torch.ones_like(x), x)


def neg_zeros(x):
    """number of -0 elements of a 2-byte float tensor"""
    return int((x.contiguous().view(torch.int16) == -32768).sum())


def build(c, seed=0, kpos=None, qpos=None, rot_q=None):
    """CPU tensors of the twin of case c.  kpos / qpos: other positions than the header's (the sensitivity tests); rot_q(b, q_b, pos, table):
    another rotation of entry b's query rows.  Keys: q_raw / q_rot [B, Sq, Hq, D]; knew_raw / knew_rot / v_new [B, sn, Hkv, D] or None;
    k_before / v_before and k_after / v_after: the whole ALLOCATION [slots, rows + PAD, Hkv, D] in front of and behind the call (rows behind
    the visible keys NaN / Inf); k_clean / v_clean: the view after the call without the poison (what the oracle reads); R, I: the table
    allocations; cl: cache_seqlens.
    ZEROS.  The un-rotated operands are drawn without a zero element.  A ROTATED element can still be an exact zero — the difference of two
    rounded products that coincide (about one element in 10^4) — but that zero is +0 (x - x = +0 in round-to-nearest), and the identity
    rotation preserves +0: +0 * 1 - (+-0) = +0, +0 * 1 + (+-0) = +0.  Only -0 is not preserved (-0 - (-0) = +0); it needs an underflowing
    product and is asserted absent from both sides' operands."""
    dtype, D, Hkv, G, lens, slots = C.DT[c["dt"]], c["D"], c["Hkv"], c["G"], c["lens"], c["slots"]
    ql = C.case_qlens(c)
    B, Sq, Hq, s = len(lens), max(ql), Hkv * G, sn(c)
    rows = max(lens) + SPARE
    g = torch.Generator().manual_seed(31_000 + 1000 * seed + 7 * B + Sq + G)
    rnd = lambda *shape: _nonzero(torch.randn(*shape, generator=g).to(dtype))
    R, I = make_table(c, c["table"], seed), make_table(c, "identity")
    tab = table_view(R, c)
    hk, hq = positions(c)
    kpos, qpos = kpos or hk, qpos or hq
    q_raw = rnd(B, Sq, Hq, D)
    q_rot = q_raw.clone()
    for b in range(B):
        q_rot[b, :ql[b]] = (rot_q(b, q_raw[b, :ql[b]], qpos[b], tab) if rot_q else rotate(q_raw[b, :ql[b]], qpos[b], tab))
    k_clean, v_clean = rnd(c["n_slots"], rows, Hkv, D), rnd(c["n_slots"], rows, Hkv, D)
    t = dict(q_raw=q_raw, q_rot=q_rot, knew_raw=None, knew_rot=None, v_new=None, R=R, I=I, cl=[n - s for n in lens], rows=rows)
    if s:
        t["knew_raw"], t["v_new"] = rnd(B, s, Hkv, D), rnd(B, s, Hkv, D)
        t["knew_rot"] = torch.stack([rotate(t["knew_raw"][b], kpos[b], tab) for b in range(B)])
        for b in range(B):
            k_clean[slots[b], lens[b] - s:lens[b]], v_clean[slots[b], lens[b] - s:lens[b]] = t["knew_rot"][b], t["v_new"][b]
    for x in (q_raw, t["knew_raw"]):
        assert x is None or bool((x != 0).all()), "the un-rotated operands are drawn without zero elements"
    for x in (q_rot, t["knew_rot"], k_clean):
        assert x is None or neg_zeros(x) == 0, "the identity rotation does not preserve -0"
    k_after = torch.full((c["n_slots"], rows + PAD, Hkv, D), float("nan"), dtype=dtype)
    v_after = torch.full((c["n_slots"], rows + PAD, Hkv, D), float("inf"), dtype=dtype)
    k_after[:, :rows], v_after[:, :rows] = k_clean, v_clean
    for b in range(B):
        k_after[slots[b], lens[b]:], v_after[slots[b], lens[b]:] = float("nan"), float("inf")
    k_before, v_before = k_after.clone(), v_after.clone()
    for b in range(B):
        k_before[slots[b], lens[b] - s:lens[b]], v_before[slots[b], lens[b] - s:lens[b]] = float("nan"), float("inf")
    t.update(k_clean=k_clean, v_clean=v_clean, k_after=k_after, v_after=v_after, k_before=k_before, v_before=v_before)
    return t


def oracle(c, t, math, q=None, k=None):
    """the project's CPU statement of the case on the pre-rotated operands: (out [B, Sq, Hq, D], LSE [B, Hq, Sq])"""
    out, lse = C.reference(c, t["q_rot"] if q is None else q, t["k_clean"] if k is None else k, t["v_clean"], math=math, return_lse=True)
    for b, n in enumerate(c["lens"]):
        if n <= 0:      # an entry WITHOUT any key: the oracle skips it and leaves its LSE at the initial -inf; include/vattn_kernels.h: "A row
            lse[b] = float("inf")      # without a visible key gives 0 and LSE +inf" (what it returns for a fully masked row of a live entry)
    return out, lse


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------------
def bit_diff(a, b, what, layout="bshd"):
    """[] when a and b are bit-identical, else strings naming entry, row and head of the first differences.  layout "bshd": out
    [B, Sq, Hq, D]; "bhs": LSE [B, Hq, Sq]; "cache": [slot, row, kv head, D]"""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    ne = a.contiguous().view(iv) != b.contiguous().view(iv)
    if not bool(ne.any()):
        return []
    out = ["%s: %d of %d elements differ in bits" % (what, int(ne.sum()), ne.numel())]
    for ix in ne.nonzero()[:6].tolist():
        if layout == "bhs":
            out.append("  entry %d row %d head %d: %r vs %r" % (ix[0], ix[2], ix[1], a[tuple(ix)].item(), b[tuple(ix)].item()))
        else:
            out.append("  %s %d row %d head %d element %d: %r vs %r" % ("slot" if layout == "cache" else "entry", ix[0], ix[1], ix[2], ix[3], a[tuple(ix)].item(), b[tuple(ix)].item()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch plan of a case on a host-only parameter block (no GPU) and on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def window_arg(c):
    return (c["left"], 0) if c.get("left") is not None else (-1, -1)


def list_plan(c, p):
    """vattn_prefill_plan / _plan_wg for the case's `pf` request on block p (WITHOUT a table, as the caller of a table-less layer builds it):
    (items, split blocks, partial rows, workgroups, item list) — pure host arithmetic, what flash_attn.prefill_plan uploads"""
    from vattention_amd import kernels as K
    kw, ql, lens = c["pf"], C.case_qlens(c), c["lens"]
    B = len(lens)
    n_blk = sum((x + 255) // 256 for x in ql) * p.h
    cap_i, cap_b = 17 * n_blk + 16, n_blk + 16
    items, blocks = (K.PrefillItem * cap_i)(), (K.PrefillItem * cap_b)()
    counts = (CT.c_int32 * 4)()
    qa, ka = (CT.c_int32 * B)(*ql), (CT.c_int32 * B)(*lens)
    keep = p.num_splits
    p.num_splits = -int(kw["force_tiles"])
    if kw["persistent"]:
        first = None if kw.get("drawn") else (CT.c_int32 * 257)()
        n = K.klib().vattn_prefill_plan_wg(CT.byref(p), qa, ka, items, cap_i, blocks, cap_b, first, int(kw.get("max_wg", 0)), counts)
    else:
        n = K.klib().vattn_prefill_plan(CT.byref(p), qa, ka, items, cap_i, blocks, cap_b, counts)
    p.num_splits = keep
    assert n > 0, c["name"]
    return n, int(counts[1]), int(counts[2]), int(counts[3]) if kw["persistent"] else 0, [items[i] for i in range(n)]


def host_block(c, with_table=True):
    """The parameter block the drop-in builds for the case, on fake aligned pointers (nothing is launched or dereferenced): shapes, causal /
    window rule, num_splits, variant, hint, the table fields, host items / the work list — what vattn_attn_plan_describe reads."""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    D, Hkv, G, lens = c["D"], c["Hkv"], c["G"], c["lens"]
    ql = C.case_qlens(c)
    B, Sq, Hq, s = len(lens), max(ql), Hkv * G, sn(c)
    rows = max(lens) + SPARE
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = B, Sq, rows, s, Hq, Hkv, D
    p.q = p.out = p.k_cache = p.v_cache = p.cache_seqlens = 4096
    p.q_row_stride = p.o_row_stride = Hq * D
    p.q_head_stride = p.o_head_stride = p.k_head_stride = p.v_head_stride = D
    p.k_row_stride = p.v_row_stride = Hkv * D
    p.k_batch_stride = p.v_batch_stride = (rows + PAD) * Hkv * D
    if c["form"] == "var":
        p.q_start = p.q_lens = 4096
        p.max_seqlen_k_hint = min(max(lens), rows)
    else:
        p.q_batch_stride = p.o_batch_stride = Sq * Hq * D
    if s:
        p.k_new = p.v_new = 4096
        p.knew_row_stride = p.vnew_row_stride = Hkv * D * (2 if c["knew_strided"] else 1)
        p.knew_head_stride = p.vnew_head_stride = D * (2 if c["knew_strided"] else 1)
        p.knew_batch_stride = p.vnew_batch_stride = s * p.knew_row_stride
    p.window_left_plus1, causal = FA._window_left_plus1(window_arg(c), bool(c["causal"]), Sq, rows)
    p.is_causal, p.dtype, p.num_splits, p.variant, p.softmax_scale = int(causal), 0 if c["dt"] == "f16" else 1, c["splits"], c["variant"], D ** -0.5
    lst = None
    if c.get("pf"):
        lst = list_plan(c, p)
        p.pf_items, p.num_pf_items, p.num_pf_blocks, p.pf_part_rows, p.pf_num_wg = 4096, lst[0], lst[1], lst[2], lst[3]
        p.pf_blocks = 4096 if lst[1] else None
        p.pf_wg_first = 4096 if lst[3] and not c["pf"].get("drawn") else None
    if with_table:
        p.rotary_cos_sin, p.rotary_row_stride, p.rotary_dim = 4096, D * (2 if c["colslice"] else 1), D
    if c.get("host_tiles") and B > 1 and c["splits"] == 0 and not p.window_left_plus1:
        cl = (CT.c_int32 * B)(*[n - s for n in lens])
        items, seq = (K.DecodeItem * (4 * B + 1024))(), (CT.c_int32 * (2 * B))()
        p.num_splits = -c["host_tiles"]
        n = K.klib().vattn_decode_plan(CT.byref(p), cl, items, 4 * B + 1024, seq)
        p.num_splits = 0
        assert n > 0, c["name"]
        p.split_items, p.split_seq, p.num_split_items = 4096, 4096, n
    return p, lst


def named_workgroups(c, d):
    """The workgroups of the main launch the case names.  A literal (`wg`) for forced grids and explicit split counts; restated here from
    include/vattn_kernels.h / csrc/decode_kernels.hip for the device-planned stream (one round of 768 resident workgroups over the kv heads,
    at most min(48, tiles / 4) pieces per sequence) and for host items of T tiles (one piece per T tiles of every entry); a work list: one
    per piece.  Where the split count comes out of the tuning heuristics (pick_splits, plan_prefill: pinned by tests/test_plan_table.py,
    not restated a third time) the case names the GRID — head-block groups x kv heads x entries, or query blocks x heads x entries — times
    the key-range shares the description reports."""
    Hkv, G, lens = c["Hkv"], c["G"], c["lens"]
    B, rows = len(lens), max(lens) + SPARE
    nb, groups = head_blocks(c)
    if c["wg"] is not None:
        return c["wg"]
    if c.get("pf"):
        return None          # (check_plan: the number of pieces)
    if c["form"] == "dec":
        if c["path"] == 2:
            vis = rows
            if c.get("left") is not None and c["left"] + 1 + 31 < rows:
                vis = c["left"] + 1 + 31
            per_seq = min(48, max(1, ((vis + 31) // 32) // 4))
            return min(max(1, 768 // Hkv), B * per_seq) * Hkv
        if c["path"] == 1:
            T = c["host_tiles"]
            return sum(max(1, -(-((n + 31) // 32) // T)) for n in lens) * Hkv * groups
        return d["nsplit"] * Hkv * groups * B
    bm = 128 if c["tiling"] == 4 else 256
    return -(-max(C.case_qlens(c)) // bm) * Hkv * G * B * d["nsplit"]


def check_plan(c, p, d, lst=None):
    """the form, path, tiling, merge launch (C.assert_plan) and workgroups (named_workgroups) the case names; a work list beside a table: one
    workgroup per piece"""
    what = C.assert_plan(c, p, d, max(c["lens"]) + SPARE)
    if c.get("pf"):
        assert d["workgroups"] == p.num_pf_items and (lst is None or p.num_pf_items == lst[0]), what
    else:
        assert d["workgroups"] == named_workgroups(c, d), "%s: names %s workgroups" % (what, named_workgroups(c, d))
    return what


def union_key(c, d):
    nb, groups = head_blocks(c)
    return (c["form"], d["path"], d["tiling"], d["merge_launch"], nb, groups, c.get("left") is not None, c["D"], c["dt"])


# what the table must reach (test_rope_twin_plans_reached): partial keys — every listed field must match one reached combination
NEED = [dict(form="dec", path=2, nb=1), dict(form="dec", path=2, nb=2), dict(form="dec", path=0, nb=1), dict(form="dec", path=0, nb=2, groups=1),
        dict(form="dec", path=0, groups=2, D=128), dict(form="dec", path=0, groups=3, D=64), dict(form="dec", path=1, nb=1), dict(form="dec", path=1, nb=2),
        dict(form="dec", path=2, win=True), dict(form="dec", path=0, win=True, nb=2),
        dict(form="pre", tiling=1, merge=1), dict(form="pre", tiling=4, merge=1), dict(form="pre", tiling=7, merge=1, D=128),
        dict(form="pre", tiling=1, win=True), dict(form="pre", tiling=4, win=True), dict(form="pre", tiling=7, win=True),
        dict(form="var", path=0, tiling=1), dict(form="var", path=0, tiling=4), dict(form="var", path=0, tiling=7), dict(form="var", path=1, tiling=7),
        dict(form="var", win=True)]
NEED = [dict(n, D=D, dt=dt) for n in NEED for D in (64, 128) for dt in ("f16", "bf16") if n.get("D", D) == D and not (D == 64 and n.get("tiling") == 7)] + \
       [dict(form="pre", tiling=t, merge=0, D=D, dt=dt) for t in (1, 4, 7) for D in (64, 128) for dt in ("f16", "bf16") if not (D == 64 and t == 7)]
FIELDS = ("form", "path", "tiling", "merge", "nb", "groups", "win", "D", "dt")


def missing(reached):
    keys = [dict(zip(FIELDS, k)) for k in reached]
    return [n for n in NEED if not any(all(k[f] == v for f, v in n.items()) for k in keys)]


def launch(c, t, side, dev):
    """One call of the twin on the GPU: side "A" (un-rotated operands, table R) or "B" (pre-rotated, identity).  Returns (out [B, Sq, Hq, D],
    LSE [B, Hq, Sq] or None, the k / v ALLOCATIONS after the call, the launched parameter block, its plan description, the list plan)."""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    dtype, D, Hkv, G, lens, slots = C.DT[c["dt"]], c["D"], c["Hkv"], c["G"], c["lens"], c["slots"]
    ql = C.case_qlens(c)
    B, Sq, Hq, rows = len(lens), max(ql), Hkv * G, t["rows"]
    q = t["q_raw" if side == "A" else "q_rot"].to(dev)
    tab = table_view(t["R" if side == "A" else "I"].to(dev), c)
    ka, va = t["k_before"].to(dev), t["v_before"].to(dev)
    kc, vc = ka[:, :rows], va[:, :rows]
    new = (None, None)
    if t["v_new"] is not None:
        kn, vn = t["knew_raw" if side == "A" else "knew_rot"].to(dev), t["v_new"].to(dev)
        if c["knew_strided"]:
            wide = torch.full(kn.shape[:-1] + (2 * D,), float("nan"), dtype=dtype, device=dev)
            wide[..., :D] = kn
            kn = wide[..., :D]
        new = (kn, vn)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    idx = i32(slots) if c["idx"] else None
    lse, lst = None, None
    if c["form"] == "var":
        starts = [sum(ql[:i]) for i in range(B)]
        plan = None
        if c.get("pf"):
            pp = K.AttnParams()
            pp.b, pp.seqlen_q, pp.h, pp.h_k, pp.d, pp.is_causal = B, Sq, Hq, Hkv, D, int(c["causal"])
            pp.o_row_stride, pp.o_head_stride = Hq * D, D
            plan = FA.prefill_plan(pp, ql, lens, torch.device(dev), **c["pf"])
            assert plan.t is not None and (plan.n_wg > 0) == c["pf"]["persistent"] and plan.drawn == bool(c["pf"].get("drawn")), c["name"]
            lst = (plan.n_items,)
        flat = torch.full((sum(ql), Hq, D), 7.0, dtype=dtype, device=dev)
        qf = torch.cat([q[b, :ql[b]] for b in range(B)])
        _, p = C.spy_call(FA.flash_attn_varlen_with_kvcache, qf, kc, vc, i32(starts), i32(ql), Sq, i32(lens), idx, causal=c["causal"], out=flat,
                         num_splits=c["splits"], _variant=c["variant"], _max_seqlen_k=max(lens), _pf_plan=plan, window_size=window_arg(c), _rotary_cos_sin=tab)
        out = torch.zeros(B, Sq, Hq, D, dtype=dtype, device=dev)
        for b in range(B):
            out[b, :ql[b]] = flat[starts[b]:starts[b] + ql[b]]
    else:
        host = dict(_cache_seqlens_host=t["cl"], _plan_tiles=c["host_tiles"]) if c.get("host_tiles") else {}
        (out, lse), p = C.spy_call(FA.flash_attn_with_kvcache, q, kc, vc, *new, cache_seqlens=i32(t["cl"]), cache_batch_idx=idx, causal=c["causal"],
                                  window_size=window_arg(c), num_splits=c["splits"], return_softmax_lse=True, _variant=c["variant"], _rotary_cos_sin=tab, **host)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu() if lse is not None else None, ka.cpu(), va.cpu(), p, K.describe(p, K.klib_for(c["variant"])), lst

