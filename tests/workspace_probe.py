"""Workspace probes: the case table, the workspace layout of every split plan, the layout-aware fills and the guarded allocator.  Plain
Python / ctypes / torch, no GPU at import; shared by tests/test_workspace_probe_model.py (CPU: coverage, sizes, dead entries, launch count,
NULL-workspace refusals) and tests/test_gpu_workspace.py (GPU: exact-size guarded workspaces under every fill).

Every split-KV plan sends fp32 partials through the caller's workspace; the device-planned stream decode also keeps an int2 table there.
The drop-in allocates max(need, 1 MiB) with torch.empty and reuses the buffer, so neither a `*_workspace_bytes` answer that is too small nor a
merge that reads a word this call never wrote is visible to the other suites.  Here every call gets a workspace of EXACTLY the bytes the
library asked for, with canaries on both sides and contents the test controls.

OUT OF SCOPE: the hybrid entry point (vattn_hybrid_attn).  Its contract requires a zeroed workspace (include/vattn_kernels.h) and
tests/test_gpu_hybrid_fused.py owns it.

THE CASE TABLE (`cases()`) is taken from the existing tables — tests/census.py gpu_cases() and the "empty" kinds of numerics_cases(),
tests/census_fp8_tree.py fp8_cases() / tree_cases(), tests/census_softcap.py zero_cases() / signed_cases() (run here as zero-query censuses
under their cap) — keeping the cases whose plan description (pure host arithmetic: `describe_host`) has workspace_bytes > 0, thinned to the
first case per `plan_key` = (entry point, form, path, tiling, nsplit > 1, merge launch, one or two head blocks, windowed, work-list queue) in
ONE (dtype, d) combination that cycles from key to key through (f16, 128), (bf16, 64), (f16, 64), (bf16, 128), plus every case with a dead
entry or a piece that is empty by construction, in both dtypes (`has_dead`), plus the additions of `extra_cases()`: an entry with
cache_seqlens == 0 and no append beside live entries on the stream path of every decode-family build (the tables have none), and the
batched-chunk prefill with two key-range shares.
[One (dtype, d) per plan, not all four: a case is seven calls of two or three launches, and one f16 and one bf16 case per plan and head size —
166 cases — would be 2 618 launches against the budget of 1 500 that tests/test_workspace_probe_model.py asserts; the table as it stands is 88
cases, 1 358 launches.  Neither the dtype nor d changes which workspace words a plan writes and reads — d only scales the rows — and both
values of each are spread over the plans of every entry point.  A piece "empty by construction" is known for the numerics table's "empty"
kinds only; the planners' pieces are not modelled here.]

THE LAYOUT (`layout()`), restated from the kernel sources.  Every word is an fp32 partial except the stream plan's table.
  decode path 0, nsplit S > 1 (csrc/decode_kernels.hip:27, csrc/decode_body.h:583-590): float o_part[S][b][sq][h][d], then float
      lse_part[S][b][sq][h] (log2 domain).  Row (split, b, token, head) is written by workgroup (split, kv head, head-block group, b) of
      decode_kernel — every workgroup of the grid writes its rows, an empty key range gives lse -inf — and read by combine_kernel's block
      (b, token, head), which reads the S lse words and the S o rows of ITS row only.
  decode path 1, host items (decode_body.h:585-587, decode_kernels.hip:86): float o_part[n_items][h][d], then float lse_part[n_items][h].
      Row (item, head) is written by workgroup (item, kv head x group); combine_items_kernel's block (b, head) reads rows [first, first + cnt)
      of split_seq — host tables, not workspace words.
  decode path 2, device-planned stream (decode_body.h:633-638, 754-758, 900-916; decode_kernels.hip:202): int2 table[b] = (first record,
      record count), padded to stream_table_bytes(b) = (8 b + 127) & ~127 bytes — THE ONLY INTEGER WORDS — then (nwg + b) x h_k records of
      16 NB d + 32 floats: o[16 NB][d], lse[16 NB] padded to a 128-byte line.  table[b] is written by the workgroup that owns the first tile
      of sequence b on kv head 0 (an empty sequence owns one masked tile: decode_body.h:711) and read by decode_stream_combine_kernel's
      workgroup (b, kv head), which returns at count <= 1 and else walks records [first, first + count).  Record (w + b, kv head) is written by
      workgroup w for its piece of sequence b when the sequence has more than one piece (one piece: the final rows are written directly,
      st_mode 1, and no record); only columns below R = seqlen_q G are written and read.  The table padding and the 32 - 16 NB pad floats of a
      record are never touched.
  prefill, nsplit > 1 (csrc/prefill_body.h:376-379, csrc/prefill64_kernel.inc:303-306, csrc/prefill_kernels.hip:28-66): float
      o_part[nsplit][b][seqlen_q][h][d], then float lse_part[nsplit][b][seqlen_q][h].  Row (share, b, q, head) is written by the workgroup of
      (share, b, head, query block of q); combine_rows_kernel's wave (b, q, head) reads the nsplit words of its row.  Batched chunks: rows
      q >= q_lens[b] are neither written nor read.
  prefill work list (prefill64_kernel.inc:303, csrc/prefill64p_kernels.hip:412-413, prefill_kernels.hip:72-110): float o_part[pf_part_rows][d],
      then float lse_part[pf_part_rows]; share s of split block sb holds rows [part_row + 256 s, + 256), written by the workgroup (or the
      persistent workgroup's queue entry) of that piece, read by combine_blocks_kernel's wave of (block, row) for rows q < q_lens[b].

THE FILLS (`FILLS`) are layout-aware so that none can turn an unwritten integer into an out-of-range walk: integer words only ever hold 0,
-1 (an empty loop: count <= 1 returns) or the in-range decoy (first record 0, count 1).
  zero      all bytes 0
  ones      all bytes 0xFF: floats NaN, integers -1
  loud      floats +88.0 — as a stale log2-domain LSE it outweighs every real partial by 2^60 or more, as a stale accumulator it is a large
            finite value: a stale read gives a finite, grossly wrong answer that no NaN-sanitising path swallows; integers the decoy (0, 1)
  leftover  no fill: the same plan runs first with other lengths and V negated, then the case, in the same bytes

THE GUARDED ALLOCATOR (`GuardedWorkspace`) replaces flash_attn._workspace (monkeypatch, inside the test).  Every drop-in entry point reaches
the workspace through flash_attn._issue and so through _workspace — relaunch()'s fast path too (tests/test_workspace_probe_model.py reads the
source) — so no call needs its workspace set by hand.
"""
import ctypes

import torch

from tests import census as C
from tests import census_fp8_tree as X
from tests import census_softcap as S

SPARE = 8                        # rows of the cache view behind the longest entry
GUARD = 64 << 10                 # bytes of the low guard (a multiple of 256)
CANARY = 0xA5A5A5A5
CANARY_I32 = CANARY - (1 << 32)
CANARY_I16 = 0xA5A5 - (1 << 16)
LOUD_BITS = 0x42B00000           # +88.0f
FILLS = ("zero", "ones", "loud", "leftover")
CALLS_PER_CASE = 7               # the unpatched drop-in, two zero fills, ones, loud, and the two calls of leftover
MAX_KERNELS = 1500
DUMMY = 4096                     # a non-NULL pointer value for fields the plan description only tests for presence


# ---------------------------------------------------------------------------------------------------------------------------------------
# host-only parameter blocks and plan descriptions
# ---------------------------------------------------------------------------------------------------------------------------------------
def entry_of(c):
    """the C entry point a case calls: plain | cap | tree | fp8 | fp8tree | fp8pre"""
    if c.get("cap"):
        return "cap"
    if c["form"] == "tree":
        return "fp8tree" if c.get("fp8") else "tree"
    if c.get("fp8"):
        return "fp8pre" if c["form"] in ("pre", "var") else "fp8"
    return "plain"


def build_of(c):
    """the decode-family build: plain | tree | fp8 | fp8tree | softcap (None: a prefill-form case)"""
    if c["form"] in ("pre", "var"):
        return None
    return {"plain": "plain", "cap": "softcap", "tree": "tree", "fp8": "fp8", "fp8tree": "fp8tree"}[entry_of(c)]


def rows_of(c):
    return max(c["lens"]) + SPARE


def appended_rows(c):
    return (1 if c["form"] == "dec" else c["sq"]) if c["append"] else 0


def lens_before(c):
    """cache_seqlens as the call gets them (the table's lens are the VISIBLE keys, after the append)"""
    sn = appended_rows(c)
    return [n - sn for n in c["lens"]]


def host_list_plan(c):
    """the work list of a `pf` case through the library's planner, on the host: (items, split blocks, partial rows, workgroups, drawn)"""
    from vattention_amd import kernels as K
    kw, ql, lens = c["pf"], C.case_qlens(c), c["lens"]
    B, Hq = len(lens), c["Hkv"] * c["G"]
    p = K.AttnParams()
    p.b, p.seqlen_q, p.h, p.h_k, p.d, p.is_causal = B, max(ql), Hq, c["Hkv"], c["D"], int(c["causal"])
    p.o_row_stride, p.o_head_stride = Hq * c["D"], c["D"]
    p.num_splits = -int(kw.get("force_tiles", 0))
    n_blk = sum((q + 255) // 256 for q in ql) * Hq
    cap_i, cap_b = 17 * n_blk + 16, n_blk + 16
    items, blocks = (K.PrefillItem * cap_i)(), (K.PrefillItem * cap_b)()
    qa, ka = (ctypes.c_int32 * B)(*ql), (ctypes.c_int32 * B)(*lens)
    if kw["persistent"]:
        counts = (ctypes.c_int32 * 4)()
        wg_first = None if kw.get("drawn") else (ctypes.c_int32 * 257)()
        n = K.klib().vattn_prefill_plan_wg(ctypes.byref(p), qa, ka, items, cap_i, blocks, cap_b, wg_first, 0, counts)
    else:
        counts = (ctypes.c_int32 * 3)()
        n = K.klib().vattn_prefill_plan(ctypes.byref(p), qa, ka, items, cap_i, blocks, cap_b, counts)
    assert n > 0, c["name"]
    return int(n), int(counts[1]), int(counts[2]), int(counts[3]) if kw["persistent"] else 0, bool(kw["persistent"] and kw.get("drawn"))


def host_block(c):
    """the parameter block of case c as far as the plan descriptions and the workspace queries read it (shapes, flags, which optional pointers
    are set, the host plans' counts): what the drop-in call of tests/test_gpu_workspace.py builds — no device, nothing is dereferenced"""
    from vattention_amd import kernels as K
    lens, rows = c["lens"], rows_of(c)
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = len(lens), max(C.case_qlens(c)), rows, appended_rows(c), c["Hkv"] * c["G"], c["Hkv"], c["D"]
    left = c.get("left")
    p.window_left_plus1 = left + 1 if left is not None and left < rows else 0
    p.is_causal = 0 if c["form"] == "tree" else int(c["causal"] or p.window_left_plus1 > 0)
    p.dtype, p.num_splits, p.variant, p.softmax_scale = (0 if c["dt"] == "f16" else 1), c["splits"], c["variant"], c["D"] ** -0.5
    p.cache_seqlens = DUMMY
    if c["idx"]:
        p.cache_batch_idx = DUMMY
    if c["form"] == "var":
        p.q_lens = p.q_start = DUMMY
        p.max_seqlen_k_hint = min(max(lens), rows)
        p.o_row_stride, p.o_head_stride = p.h * p.d, p.d
    if c.get("pf"):
        n, nb, part_rows, nwg, drawn = host_list_plan(c)
        p.pf_items, p.num_pf_items, p.num_pf_blocks, p.pf_part_rows, p.pf_num_wg = DUMMY, n, nb, part_rows, nwg
        p.pf_blocks = DUMMY if nb else None
        p.pf_wg_first = DUMMY if nwg and not drawn else None
    if c.get("host_tiles") and c.get("left") is None and not c.get("cap"):
        B = p.b
        cap = 4 * B + 1024
        items, seq = (K.DecodeItem * cap)(), (ctypes.c_int32 * (2 * B))()
        p.num_splits = -int(c["host_tiles"])
        n = K.klib().vattn_decode_plan(ctypes.byref(p), (ctypes.c_int32 * B)(*lens_before(c)), items, cap, seq)
        p.num_splits = 0
        assert n >= 0, c["name"]
        if n:
            p.split_items, p.split_seq, p.num_split_items = DUMMY, DUMMY, n
    return p


def describe_block(c, p):
    """the plan description of block p through the describe entry of the call case c makes"""
    from vattention_amd import kernels as K
    e = entry_of(c)
    if e == "cap":
        return K.describe_softcap(p, c["cap"])
    return {"plain": K.describe, "tree": K.describe_tree, "fp8": K.describe_fp8kv, "fp8tree": K.describe_fp8kv_tree, "fp8pre": K.describe_fp8kv_prefill}[e](p)


def workspace_bytes_export(c, p):
    """the answer of the `*_workspace_bytes` export that matches the call of case c"""
    from vattention_amd import kernels as K
    lib, e = K.klib(), entry_of(c)
    if e == "cap":
        return int(lib.vattn_softcap_attn_workspace_bytes(ctypes.byref(p), c["cap"]))
    fn = {"plain": lib.vattn_attn_workspace_bytes, "tree": lib.vattn_tree_attn_workspace_bytes, "fp8": lib.vattn_fp8kv_attn_workspace_bytes,
          "fp8tree": lib.vattn_fp8kv_tree_attn_workspace_bytes, "fp8pre": lib.vattn_fp8kv_prefill_workspace_bytes}[e]
    return int(fn(ctypes.byref(p)))


def describe_host(c):
    return describe_block(c, host_block(c))


def queue_of(c):
    pf = c.get("pf")
    return "" if not pf else ("drawn" if pf.get("drawn") else "assigned") if pf["persistent"] else "per_piece"


def head_blocks(c):
    """16-column head blocks per workgroup in the decode forms: 1 or 2 (R = seqlen_q G > 16 columns per kv head); 0: prefill forms"""
    if c["form"] in ("pre", "var"):
        return 0
    return 1 if c["sq"] * c["G"] <= 16 else 2


def plan_key(c, d, windowed):
    return (entry_of(c), c["form"], d["path"], d["tiling"], d["nsplit"] > 1, d["merge_launch"], head_blocks(c), windowed, queue_of(c))


def coverage_key(c, d):
    """(entry point, form, path, tiling, merge launch): what tests/test_workspace_probe_model.py compares with the plan-table grid"""
    return (entry_of(c), d["form"], d["path"], d["tiling"], d["merge_launch"])


def has_dead(c):
    """some entry has no visible key, or some piece is empty by construction (the numerics table's "empty" kinds)"""
    return min(c["lens"]) == 0 or "empty" in c["name"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------
DEAD_LENS = [0, 200, 33]
VAR_SPLIT = dict(qlens=[1, 70, 130], lens=[41, 70, 330], slots=[3, 0, 2], n_slots=4)      # tests/test_gpu_softcap.py test_prefill_batched_chunks


def extra_cases():
    """what the existing tables do not hold: a dead entry (cache_seqlens == 0, no append) beside live ones on the device-planned stream path of
    every decode-family build, one-token (R = 4) and multi-token (R = 16), in the closed-form census style; the batched-chunk prefill with
    num_splits = 2 through the plain, softcap and fp8 entry points"""
    cs = []
    for dt in ("f16", "bf16"):
        for D in (128, 64):
            tag = "%s_d%d" % (dt, D)
            if D == 128:
                cs.append(C._case("ws_dead_dec_%s" % tag, "dec", dt, D, 2, 4, 1, DEAD_LENS, 2, tiling=1, merge=1))
                cs.append(C._case("ws_dead_mt_%s" % tag, "mt", dt, D, 2, 4, 4, DEAD_LENS, 2, tiling=1, merge=1))
            if D != 128:
                continue
            cs.append(dict(C._case("ws_dead_cap_dec_%s" % tag, "dec", dt, D, 2, 4, 1, DEAD_LENS, 2, tiling=1, merge=1), cap=50.0))
            cs.append(dict(C._case("ws_dead_cap_mt_%s" % tag, "mt", dt, D, 2, 4, 4, DEAD_LENS, 2, tiling=1, merge=1), cap=1.0))
            cs.append(X._xcase("ws_dead_fp8_dec_%s" % tag, "dec", dt, D, 2, 4, 1, DEAD_LENS, 2, True, tiling=1, merge=1))
            cs.append(X._xcase("ws_dead_fp8_mt_%s" % tag, "mt", dt, D, 2, 4, 4, DEAD_LENS, 2, True, tiling=1, merge=1))
            for fp8 in (False, True):
                cs.append(X._xcase("ws_dead_tree_%s_%s" % ("fp8" if fp8 else "2b", tag), "tree", dt, D, 2, 4, 4, DEAD_LENS, 2, fp8, mask="tree7", tiling=1, merge=1))
            for entry in ("plain", "cap", "fp8pre"):
                c = C._case("ws_var_split2_%s_%s" % (entry, tag), "var", dt, D, 2, 4, 130, VAR_SPLIT["lens"], 0, qlens=VAR_SPLIT["qlens"], splits=2, merge=1, idx=True,
                            fp8=entry == "fp8pre")
                c["slots"], c["n_slots"] = list(VAR_SPLIT["slots"]), VAR_SPLIT["n_slots"]
                if entry == "cap":
                    c["cap"] = 50.0
                cs.append(c)
    return cs


def source_cases():
    """every case of the existing tables this file draws from, and the additions, in table order"""
    cs = list(C.gpu_cases()) + [c for c in C.numerics_cases() if "empty" in c["name"]]
    cs += X.fp8_cases() + X.tree_cases()
    cs += [dict(c, name="cap_" + c["name"]) for c in S.zero_cases()] + [dict(c, name="capsigned_" + c["name"]) for c in S.signed_cases()]
    return cs + extra_cases()


_CASES = None


def cases():
    """the thinned table (module docstring): [(case, plan description of its host-only block)]"""
    global _CASES
    if _CASES is not None:
        return _CASES
    split, have = [], {}
    for c in source_cases():
        if c.get("fp8") is None:
            c = dict(c, fp8=False)
        p = host_block(c)
        d = describe_block(c, p)
        if d["workspace_bytes"] <= 0:
            continue
        key = plan_key(c, d, p.window_left_plus1 > 0)
        split.append((c, d, key))
        if not has_dead(c):
            have.setdefault(key, []).append((c["dt"], c["D"]))
    # one (dtype, d) per plan, cycling from plan to plan (the nearest other one where the tables do not hold the plan in that combination)
    cycle = [("f16", 128), ("bf16", 64), ("f16", 64), ("bf16", 128)]
    want = {}
    for i, (key, combos) in enumerate(have.items()):
        want[key] = next(cycle[(i + j) % 4] for j in range(4) if cycle[(i + j) % 4] in combos)
    out = []
    for c, d, key in split:
        if has_dead(c):
            out.append((c, d))
        elif want.get(key) == (c["dt"], c["D"]):
            want[key] = None
            out.append((c, d))
    names = [c["name"] for c, _ in out]
    assert len(set(names)) == len(names)
    _CASES = out
    return out


def kernels_per_call(c, d):
    """launches of one call: the attention kernel, the merge launch, and the append launch where the rows are not appended by the attention
    kernel itself (csrc/decode_kernels.hip begin_decode_launch: fused for ONE new row of a 2-byte cache; csrc/prefill_kernels.hip:296)"""
    fused = c["form"] == "dec" and entry_of(c) in ("plain", "cap")
    return 1 + d["merge_launch"] + (1 if c["append"] and not fused else 0)


def total_kernels():
    return sum(CALLS_PER_CASE * kernels_per_call(c, d) for c, d in cases())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the layout
# ---------------------------------------------------------------------------------------------------------------------------------------
def stream_table_bytes(b):
    return (8 * b + 127) & ~127


def layout(c, d, p):
    """the regions of the workspace of case c under plan description d of block p: a list of dicts
    (name, kind 'int' | 'float', offset, nbytes, unit = bytes of one record / row, writer, reader); their sizes add up to workspace_bytes"""
    D, H, B, Sq = c["D"], p.h, p.b, p.seqlen_q
    if d["form"] == 1 and d["path"] == 2:
        nwg = d["workgroups"] // p.h_k
        assert nwg * p.h_k == d["workgroups"]
        rf = 16 * d["tiling"] * D + 32
        tb = stream_table_bytes(B)
        return [dict(name="table", kind="int", offset=0, nbytes=tb, unit=8, used=8 * B,
                     writer="decode_stream_kernel: the workgroup that owns the first tile of sequence b on kv head 0", reader="decode_stream_combine_kernel (b, kv head)"),
                dict(name="records", kind="float", offset=tb, nbytes=(nwg + B) * p.h_k * rf * 4, unit=rf * 4,
                     writer="decode_stream_kernel: workgroup w, record (w + b, kv head) of a sequence with more than one piece", reader="decode_stream_combine_kernel (b, kv head)")]
    if d["form"] == 1 and d["path"] == 1:
        rows, writer, reader = p.num_split_items * H, "decode_kernel: workgroup (item, kv head x group)", "combine_items_kernel (b, head)"
    elif d["form"] == 1:
        rows, writer, reader = d["nsplit"] * B * Sq * H, "decode_kernel: workgroup (split, kv head, group, b)", "combine_kernel (b, token, head)"
    elif d["path"] == 1:
        rows, writer, reader = p.pf_part_rows, "prefill64 / prefill64p: the piece (block, share)", "combine_blocks_kernel (block, row)"
    else:
        rows, writer, reader = d["nsplit"] * B * Sq * H, "prefill kernel: workgroup (share, b, head, query block)", "combine_rows_kernel (b, q, head)"
    return [dict(name="o_part", kind="float", offset=0, nbytes=rows * D * 4, unit=D * 4, writer=writer, reader=reader),
            dict(name="lse_part", kind="float", offset=rows * D * 4, nbytes=rows * 4, unit=4, writer=writer, reader=reader)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the guarded allocator
# ---------------------------------------------------------------------------------------------------------------------------------------
class GuardedWorkspace:
    """Replacement for vattention_amd.flash_attn._workspace: a view of EXACTLY nbytes bytes that starts GUARD bytes into a buffer with a low
    guard of GUARD bytes and a high guard of max(GUARD, nbytes), both filled with CANARY.  Every request is recorded.  `fill` / `regions`
    (set by the test before the call) decide the contents; fill None keeps the buffer of the previous request of the same size (leftover)."""

    def __init__(self):
        self.requests, self.fill, self.regions = [], "zero", None
        self.buf, self.nbytes = None, 0

    def __call__(self, nbytes, device, stream_ptr=None):
        nbytes = int(nbytes)
        self.requests.append(nbytes)
        assert nbytes > 0 and nbytes % 4 == 0
        if self.fill is None:
            assert self.buf is not None and self.nbytes == nbytes, "leftover: the two calls must ask for the same bytes (%d, %d)" % (self.nbytes, nbytes)
            return self.view()
        hi = max(GUARD, nbytes)
        self.buf = torch.full(((GUARD + nbytes + hi) // 4,), CANARY_I32, dtype=torch.int32, device=device)
        self.nbytes = nbytes
        w = self.words()
        if self.fill == "zero":
            w.zero_()
        elif self.fill == "ones":
            w.fill_(-1)
        else:
            assert self.fill == "loud" and self.regions is not None
            assert sum(r["nbytes"] for r in self.regions) == nbytes
            for r in self.regions:
                seg = w[r["offset"] // 4:(r["offset"] + r["nbytes"]) // 4]
                if r["kind"] == "float":
                    seg.fill_(LOUD_BITS)
                else:                                  # (first record 0, count 1): in range whatever the record count
                    seg.view(-1, 2)[:, 0] = 0
                    seg.view(-1, 2)[:, 1] = 1
        return self.view()

    def words(self):
        return self.buf[GUARD // 4:(GUARD + self.nbytes) // 4]

    def view(self):
        v = self.words().view(torch.float32)
        assert v.numel() * 4 == self.nbytes and (not v.is_cuda or v.data_ptr() % 256 == 0)
        return v

    def guards_intact(self):
        lo, hi = self.buf[:GUARD // 4], self.buf[(GUARD + self.nbytes) // 4:]
        return bool((lo == CANARY_I32).all()) and bool((hi == CANARY_I32).all())

    def first_damage(self):
        """byte offset relative to the view's start of the first damaged guard word (negative: the low guard), or None"""
        bad = (self.buf != CANARY_I32)
        bad[GUARD // 4:(GUARD + self.nbytes) // 4] = False
        i = torch.nonzero(bad)
        return None if i.numel() == 0 else int(i[0]) * 4 - GUARD


# ---------------------------------------------------------------------------------------------------------------------------------------
# the call: device inputs of a case, the drop-in call, and the re-issue of the very block it launched
# ---------------------------------------------------------------------------------------------------------------------------------------
def other_lens(c):
    """cache_seqlens of the leftover fill's first call.  Decode forms: the case's own, rotated by one entry (halved where that changes nothing) —
    a dead entry moves to another sequence, the records and the table change.  Prefill forms: every entry 37 keys shorter, never below its
    query rows (a work list built for the case's lengths then runs on stale ones within the regime tests/test_gpu_prefill_persistent.py
    test_stale_host_lengths_cost_balance_never_keys covers)."""
    cl, sn = lens_before(c), appended_rows(c)
    if c["form"] in ("pre", "var"):
        return [max(min(n + sn, q), n + sn - 37) - sn for n, q in zip(cl, C.case_qlens(c))]
    r = cl[1:] + cl[:1]
    return r if r != cl else [n // 2 for n in cl]


def _copy_block(p):
    from vattention_amd import kernels as K
    q = K.AttnParams()
    ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(K.AttnParams))
    return q


class Call:
    """One case on the GPU.  Holds every tensor the launched parameter block points to (the drop-in drops its own references when it returns),
    so that the block can be issued again through flash_attn._issue with another `out`, LSE buffer and — through the patched _workspace —
    another workspace.  An appending call is idempotent: the same rows land on the same cache rows."""

    def __init__(self, c, dev, numerics=None):
        from vattention_amd import flash_attn as FA
        self.c, self.dev, self.FA = c, dev, FA
        dtype, D, Hkv, G, lens, slots = C.DT[c["dt"]], c["D"], c["Hkv"], c["G"], c["lens"], c["slots"]
        self.ql = ql = C.case_qlens(c)
        self.B, self.Sq, self.Hq, self.D = len(lens), max(ql), Hkv * G, D
        B, Sq, Hq = self.B, self.Sq, self.Hq
        rows, fp8, e = rows_of(c), bool(c.get("fp8")), entry_of(c)
        self.fp8, self.var = fp8, c["form"] == "var"
        g = torch.Generator(device=dev).manual_seed(D + Hkv + B)
        if numerics is not None:                                   # score-range inputs (tests/census.py numerics_inputs): CPU tensors, caches after the append
            q, k_fin, v_fin = (t.to(dev) for t in numerics)
            pk = pv = 0.0
        elif fp8:
            q = torch.zeros(B, Sq, Hq, D, dtype=dtype, device=dev)
            k_fin, v_fin = X.fp8_random_keys(c["n_slots"], rows, Hkv, D, D + Hkv, device=dev), X.fp8_census_values(c["n_slots"], rows, Hkv, D, device=dev)
            pk = pv = X.FP8_NAN
        else:
            q = torch.zeros(B, Sq, Hq, D, dtype=dtype, device=dev)
            k_fin, v_fin = torch.randn(c["n_slots"], rows, Hkv, D, device=dev, dtype=dtype, generator=g), C.census_values(c["n_slots"], rows, Hkv, D, dtype, device=dev)
            pk, pv = float("nan"), float("inf")
        if numerics is None:                                       # rows at or behind Lk are poisoned, the rows an append will fill included
            for b in range(B):
                k_fin[slots[b], lens[b]:], v_fin[slots[b], lens[b]:] = pk, pv
        self.k_fin, self.v_fin = k_fin, v_fin
        kc, vc, new, cl = C.cut_out_appended(c, k_fin, v_fin, pk, pv)
        if new[0] is None:
            kc, vc = kc.clone(), vc.clone()
        self.cl = cl
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
        self.t_cl, self.t_idx = i32(cl), (i32(slots) if c["idx"] else None)
        self.scales = None
        if fp8:
            ks, vs = X.case_scales(c)
            self.scales = (torch.tensor(ks, dtype=torch.float32, device=dev), torch.tensor(vs, dtype=torch.float32, device=dev))
            if new[0] is not None:
                new = (X.dequantize_bytes(new[0], self.scales[0], dtype), X.dequantize_bytes(new[1], self.scales[1], dtype))
            kc, vc = kc.view(torch.float8_e4m3fn), vc.view(torch.float8_e4m3fn)
        self.kc, self.vc, self.new = kc, vc, new
        self.mask = X.mask_tensor(c, dev) if c["form"] == "tree" else None
        self.starts = [sum(ql[:i]) for i in range(B)]
        self.q = torch.cat([q[b, :ql[b]] for b in range(B)]).contiguous() if self.var else q
        self.t_starts, self.t_ql = i32(self.starts), i32(ql)
        self.plan = None
        if c.get("pf"):
            from vattention_amd import kernels as K
            pp = K.AttnParams()
            pp.b, pp.seqlen_q, pp.h, pp.h_k, pp.d, pp.is_causal = B, Sq, Hq, Hkv, D, int(c["causal"])
            pp.o_row_stride, pp.o_head_stride = Hq * D, D
            self.plan = FA.prefill_plan(pp, ql, lens, torch.device(dev), **c["pf"])
            assert self.plan.t is not None
        self.issued, self.kept = None, None
        self.out0 = self.lse0 = None

    # -- the drop-in call, spied at _issue (what the launch was issued with) and _launch (the tensors the entry point keeps alive only until it returns)
    def first_call(self):
        FA, c = self.FA, self.c
        seen, kept, real_issue, real_launch = [], [], FA._issue, FA._launch

        def spy_issue(p, dev, lib, need=None, mask=None, scales=None, fp8_prefill=False, softcap=0.0):
            seen.append((p, dev, lib, mask, scales, fp8_prefill, softcap))
            return real_issue(p, dev, lib, need, mask, scales, fp8_prefill, softcap)

        def spy_launch(p, dev, keep=()):
            kept.append(keep)
            return real_launch(p, dev, keep)
        FA._issue, FA._launch = spy_issue, spy_launch
        try:
            out, lse = self._dropin()
        finally:
            FA._issue, FA._launch = real_issue, real_launch
        torch.cuda.synchronize()
        assert len(seen) == 1, "%s: the drop-in issued %d launches" % (c["name"], len(seen))
        self.issued, self.kept = seen[0], kept
        self.out0, self.lse0 = out, lse
        return out, lse

    def _dropin(self):
        FA, c = self.FA, self.c
        e = entry_of(c)
        win = (c["left"], 0) if c.get("left") is not None else (-1, -1)
        newkw = dict(k=self.new[0], v=self.new[1]) if self.new[0] is not None else {}
        if e in ("plain", "cap"):
            if self.var:
                out = torch.full_like(self.q, 7.0)
                FA.flash_attn_varlen_with_kvcache(self.q, self.kc, self.vc, self.t_starts, self.t_ql, self.Sq, self.t_cl, self.t_idx, softmax_scale=c.get("scale"), causal=c["causal"],
                                                  out=out, num_splits=c["splits"], _variant=c["variant"], _max_seqlen_k=max(c["lens"]), _pf_plan=self.plan, window_size=win,
                                                  softcap=c.get("cap") or 0.0)
                return out, None
            host = {}
            if c.get("host_tiles") and c.get("left") is None and not c.get("cap"):
                host = dict(_cache_seqlens_host=self.cl, _plan_tiles=c["host_tiles"])
            return FA.flash_attn_with_kvcache(self.q, self.kc, self.vc, cache_seqlens=self.t_cl, cache_batch_idx=self.t_idx, softmax_scale=c.get("scale"), causal=c["causal"],
                                              window_size=win, num_splits=c["splits"], return_softmax_lse=True, _variant=c["variant"], softcap=c.get("cap") or 0.0, **host, **newkw)
        if e in ("tree", "fp8tree"):
            if e == "tree":
                return FA.flash_attn_tree_with_kvcache(self.q, self.kc, self.vc, self.mask, cache_seqlens=self.t_cl, cache_batch_idx=self.t_idx, softmax_scale=c.get("scale"),
                                                       return_softmax_lse=True, _num_splits=c["splits"], **newkw)
            return FA.flash_attn_fp8kv_tree_with_kvcache(self.q, self.kc, self.vc, self.scales[0], self.scales[1], self.mask, cache_seqlens=self.t_cl, cache_batch_idx=self.t_idx,
                                                         softmax_scale=c.get("scale"), return_softmax_lse=True, _num_splits=c["splits"], **newkw)
        if self.var:
            out = torch.full_like(self.q, 7.0)
            FA.flash_attn_fp8kv_varlen_with_kvcache(self.q, self.kc, self.vc, self.scales[0], self.scales[1], self.t_starts, self.t_ql, self.Sq, self.t_cl, self.t_idx,
                                                    softmax_scale=c.get("scale"), causal=c["causal"], out=out, _num_splits=c["splits"], _variant=c["variant"], _max_seqlen_k=max(c["lens"]))
            return out, None
        fn = FA.flash_attn_fp8kv_prefill_with_kvcache if e == "fp8pre" else FA.flash_attn_fp8kv_with_kvcache
        return fn(self.q, self.kc, self.vc, self.scales[0], self.scales[1], cache_seqlens=self.t_cl, cache_batch_idx=self.t_idx, softmax_scale=c.get("scale"), causal=c["causal"],
                  return_softmax_lse=True, _num_splits=c["splits"], _variant=c["variant"], **newkw)

    # -- the same block once more, with guard bands round a padded `out` and round the LSE
    OUT_BAND, LSE_BAND = 4096, 4096

    def reissue(self, block=None):
        """Issue the launched block (or `block`, a modified copy) through flash_attn._issue with a fresh `out` whose rows carry one extra head of
        padding and a fresh LSE buffer, both preset to the canary and set between 4 KiB bands.  Returns (out, lse, damage): out in the
        drop-in's own shape ([B, Sq, Hq, D], batched chunks [T, Hq, D]), lse [B, Hq, Sq], damage a list of strings naming what was written
        outside them."""
        p0, dev, lib, mask, scales, fp8_prefill, softcap = self.issued
        p = p0 if block is None else block
        Hq, D, Sq, B = self.Hq, self.D, self.Sq, self.B
        rows = self.q.shape[0] if self.var else B * Sq
        eo, el = self.OUT_BAND // 2, self.LSE_BAND // 4
        obuf = torch.full((2 * eo + rows * (Hq + 1) * D,), CANARY_I16, dtype=torch.int16, device=self.dev)
        lbuf = torch.full((2 * el + B * Hq * Sq,), CANARY_I32, dtype=torch.int32, device=self.dev)
        keep = (p.out, p.softmax_lse, p.o_batch_stride, p.o_row_stride, p.o_head_stride)
        p.out, p.softmax_lse = obuf.data_ptr() + self.OUT_BAND, lbuf.data_ptr() + self.LSE_BAND
        p.o_head_stride, p.o_row_stride, p.o_batch_stride = D, (Hq + 1) * D, 0 if self.var else Sq * (Hq + 1) * D
        try:
            self.FA._issue(p, dev, lib, None, mask, scales, fp8_prefill, softcap)
            torch.cuda.synchronize()
        finally:
            p.out, p.softmax_lse, p.o_batch_stride, p.o_row_stride, p.o_head_stride = keep
        body = obuf[eo:eo + rows * (Hq + 1) * D].view(rows, Hq + 1, D)
        damage = []
        if not bool((obuf[:eo] == CANARY_I16).all()) or not bool((obuf[eo + rows * (Hq + 1) * D:] == CANARY_I16).all()):
            damage.append("a 4 KiB band round `out` was written")
        if not bool((body[:, Hq] == CANARY_I16).all()):
            damage.append("the padding head of an `out` row was written")
        if not bool((lbuf[:el] == CANARY_I32).all()) or not bool((lbuf[el + B * Hq * Sq:] == CANARY_I32).all()):
            damage.append("a 4 KiB band round softmax_lse was written")
        lse_i = lbuf[el:el + B * Hq * Sq].view(B, Hq, Sq)
        for b in range(B):
            if self.ql[b] < Sq and not bool((lse_i[b, :, self.ql[b]:] == CANARY_I32).all()):
                damage.append("softmax_lse rows beyond q_lens[%d] = %d were written" % (b, self.ql[b]))
        out = body[:, :Hq].contiguous().view(self.q.dtype)
        if not self.var:
            out = out.view(B, Sq, Hq, D)
        if not self.caches_intact():
            damage.append("the caches differ from their expected state (appended rows, or bytes outside them)")
        return out, lse_i.clone().view(torch.float32), damage

    def caches_intact(self):
        bits = (lambda t: t.view(torch.uint8)) if self.fp8 else (lambda t: t.view(torch.int16))
        return torch.equal(bits(self.kc), bits(self.k_fin)) and torch.equal(bits(self.vc), bits(self.v_fin))

    def leftover_block(self):
        """a copy of the launched block for the first call of the leftover fill: the same plan over other lengths and V negated, on copies of the
        caches (an appending call writes its rows elsewhere).  Returns (block, tensors to hold while it runs)."""
        p = _copy_block(self.issued[0])
        # (the poisoned rows behind Lk become plausible finite ones: with other lengths the first call sees some of them)
        if self.fp8:
            k8, v8 = self.kc.view(torch.uint8), self.vc.view(torch.uint8)
            k2 = torch.where(k8 == X.FP8_NAN, torch.full_like(k8, X.FP8_ONE), k8).view(torch.float8_e4m3fn)
            v2 = (torch.where(v8 == X.FP8_NAN, torch.full_like(v8, X.FP8_ONE), v8) ^ 0x80).view(torch.float8_e4m3fn)
        else:
            k2, v2 = torch.nan_to_num(self.kc, nan=0.5), -torch.nan_to_num(self.vc, posinf=1.0)
        cl2 = torch.tensor(other_lens(self.c), dtype=torch.int32, device=self.dev)
        p.k_cache, p.v_cache, p.cache_seqlens = k2.data_ptr(), v2.data_ptr(), cl2.data_ptr()
        return p, (k2, v2, cl2)

    def canonical(self, out, lse):
        """(out [B, Sq, Hq, D], lse [B, Hq, Sq] or None) on the CPU: batched chunks entry by entry, rows an entry does not have 0"""
        if self.var:
            o = torch.zeros(self.B, self.Sq, self.Hq, self.D, dtype=out.dtype, device=out.device)
            for b in range(self.B):
                o[b, :self.ql[b]] = out[self.starts[b]:self.starts[b] + self.ql[b]]
            out = o
        return out.cpu(), (lse.cpu() if lse is not None else None)

    def first_difference(self, out, ref):
        """(entry, row, head) of the first element in which two outputs of the drop-in's shape differ bit for bit, or None"""
        a, b = self.canonical(out.view(torch.int16), None)[0], self.canonical(ref.view(torch.int16), None)[0]
        i = torch.nonzero(a != b)
        return None if i.numel() == 0 else tuple(int(x) for x in i[0][:3])
