"""The key census (tests/census.py, tests/census_fp8_tree.py, tests/census_softcap.py) with the cache view placed FAR into one large allocation: K/V
byte offsets beyond 2, 4 and 8 GiB, where a 32-bit product or sum in a kernel's address arithmetic wraps.  The closed forms (`expected`, `compare`),
the case constructor and the spies are the census modules', untouched; what is new is where the view sits, a sparse address model of the buffer
(tests/test_far_address_model.py: the probe SEES a wrap at 2^31 / 2^32 / 2^33 bytes) and the launcher (tests/test_gpu_far_address.py).

ONE raw uint8 buffer for K and one for V (BUF_BYTES each), plain device memory, filled with a finite constant per dtype group: K 0.5, V 3.0 —
neither 0 nor 1, so a value row read from a wrapped address moves an output element by >= 3 / n and stays finite: a failed comparison that names the
entry, never a fault.  A case writes its payload (random K, one-hot census V) through a strided view and puts the fill back afterwards; rows behind
Lk keep the fill.  K addresses show too: every query row is (Q0, 0, 0, ...) with Q0 = 64 and every payload key row holds 0 in element 0, so
every visible key still scores exactly 0 (the census's arithmetic stays exact: 64 x 0 plus zeros), while a key row read from a wrapped address is
fill, scores 64 x 0.5 x softmax_scale (x k_scale) > 0 and weighs e^score, >= 2, instead of 1: its residue counts double or more, >= 1 / n.

BUILDS AND PLANS the table reaches (`cases`, `needed_plans`), each in f16 and bf16 at d = 64 and 128 where the build exists, in geometry `slot`
and `row`: one-token decode on the device-planned stream (path 2), the uniform split with forced num_splits (0) and host items (1, `slot` only:
it needs a batch), one and two head blocks, windowed, with the in-kernel one-row append; multi-token at R = 16 / 32 / 64 columns, causal and
not, windowed, with the append launch; tree-masked with a chain and a non-trivial mask over a 2-byte and an fp8 cache; fp8 decode (one-token,
multi-token), fp8 prefill tilings 1 and 4 with and without the key-range merge, fp8 batched chunks, appends through the call; softcap (cap 50)
decode, multi-token, prefill tilings 1 and 4 with and without a window; prefill tilings 1, 4 and 7, the KV-split merge, batched chunks, the
work list per piece and persistent with assigned and with drawn queues, windowed tilings.  Geometry `deep`: the windowed one-token, multi-token,
prefill (1, 4, 7) and softcap builds.  The writers (cache_flat, cache_flat_rope, cache_flat_fp8, keep_rows, keep_rows_fp8) are in
tests/test_gpu_far_address.py.

THREE GEOMETRIES (byte strides; `geometry`):
  slot   [9, rows, Hkv, D], row pitch 64 KiB (fp8: 32 KiB) as in production, batch stride 1 GiB + 5 KiB; the entries use, through cache_batch_idx,
         slots 8, 0, 4, 2, 6: starts at >= 8 GiB, < 2 GiB, in [4, 8) GiB, in [2, 4) GiB, in [4, 8) GiB
  row    one slot, row pitch 8 MiB + 4 KiB, first row 16 pitches in: rows 239 | 240, 495 | 496 and 1007 | 1008 straddle the 2, 4 and 8 GiB marks —
         inside the 32-row tiles 224.., 480.., 992.. and the 64-row tiles 192.., 448.., 960..; Lk = 1061 (n <= 2048: admissible for bf16 at d = 64)
  deep   windowed builds, one slot, production pitch 64 KiB, Lk = 65536 + 500 and 131072 + 500 rows, left 0 / 31 / 255: the visible tail and the
         no-read line align_down(first visible key, 64) lie beyond 4 GiB and beyond 8 GiB; only the tail from that line on is payload
The buffers are 8.5 GiB each, not "8 GiB plus one row pitch": 1061 rows of 8 MiB + 4 KiB end at 8.42 GiB, and torch.as_strided wants the whole
view inside its storage.

PITCH CONDITION (`pitch_violations`, asserted by the model test for every case): for every payload byte range [A, A + len) of a case and every w in
2^31, 2^32, 2^33 with A >= w, neither A - w nor A mod w meets any payload of the case — a wrapped read lands on fill, never on another one-hot row
that might carry the same residue.  (A row pitch of exactly 8 MiB fails it: the 2^32 alias of row j is row j - 512.)

OUT OF SCOPE: the lab build and the fused hybrid kernel; fused-rotary attention calls (rotation does not change K/V addressing; the rotating WRITER
cache_flat_rope is here); q / out offsets beyond 2^31 elements (not reachable at realistic shapes)."""
import numpy as np
import torch

from tests import census as C
from tests import census_fp8_tree as X

GiB = 1 << 30
BUF_BYTES = 8 * GiB + 512 * (1 << 20)
MARKS = (2 * GiB, 4 * GiB, 8 * GiB)
WRAPS = (1 << 31, 1 << 32, 1 << 33)      # bytes; for a 2-byte cache ELEMENT offsets modulo 2^31 / 2^32 are byte offsets modulo 2^32 / 2^33: the same set
ROW_PITCH = 8 * (1 << 20) + 4096
SLOT_PITCH = GiB + 5120          # (k x 5 KiB, k <= 8, never lands within a payload row of a 32- or 64-KiB pitch)
SLOTS = [8, 0, 4, 2, 6]
CAP = 50.0
K_FILL, V_FILL = 0.5, 3.0
Q0 = 64.0                                # element 0 of every query row; every other element is 0
K_FILL8, V_FILL8 = 0x30, 0x44            # e4m3 0.5 and 3.0
DEEP_LENS = (65536 + 500, 131072 + 500)


def esize(c):
    return 1 if c.get("fp8") else 2


def group(c):
    """the dtype group a case's buffers are filled for"""
    return "fp8" if c.get("fp8") else c["dt"]


def view_rows(c):
    return max(c["lens"]) + 8


def geometry(c):
    """byte strides and byte offset of the [n_slots, rows, Hkv, D] cache view of case c (K and V alike, each in its own buffer)"""
    es, geo = esize(c), c["geo"]
    g = dict(es=es, hs=c["D"] * es, rows=view_rows(c), n_slots=c["n_slots"], base=0)
    if geo == "slot":
        g.update(rs=(64 << 10) // (2 // es), bs=SLOT_PITCH)
    elif geo == "row":
        g.update(rs=ROW_PITCH, bs=ROW_PITCH * 8, base=16 * ROW_PITCH)
    else:
        g.update(rs=(64 << 10) // (2 // es), bs=(64 << 10) * 8)
    g["row_bytes"] = c["Hkv"] * c["D"] * es
    end = g["base"] + (g["n_slots"] - 1) * g["bs"] + (g["rows"] - 1) * g["rs"] + g["row_bytes"]
    assert end <= BUF_BYTES and all(g[k] % 16 == 0 for k in ("rs", "bs", "hs", "base")), (c["name"], g)
    return g


def payload_rows(c, b):
    """[r0, r1) of entry b: the rows that hold data (AFTER the call); a deep-window case holds only the tail from its no-read line on"""
    Lk = c["lens"][b]
    if c["geo"] != "deep":
        return 0, Lk
    ql = C.case_qlens(c)[b]
    first = min(C.visible_interval(ql, Lk, t, c["causal"], c["left"])[0] for t in range(ql))
    return first // 64 * 64, Lk


def row_address(c, g, b, j):
    """byte offset of row j (any integer array) of entry b's slot, kv head 0"""
    return g["base"] + c["slots"][b] * g["bs"] + np.asarray(j, dtype=np.int64) * g["rs"]


def payload_ranges(c):
    """int64 [N] sorted start addresses of every payload row of the case (each g['row_bytes'] long: the kv heads of a row are contiguous)"""
    g = geometry(c)
    a = np.concatenate([row_address(c, g, b, np.arange(*payload_rows(c, b))) for b in range(len(c["lens"]))])
    return np.sort(a), g["row_bytes"]


def _meets(starts, n, x):
    """which of the ranges [x, x + n) meet one of the sorted payload ranges [starts, starts + n)"""
    i = np.searchsorted(starts, x, side="right")
    below = (i > 0) & (starts[np.maximum(i - 1, 0)] + n > x)
    above = (i < len(starts)) & (starts[np.minimum(i, len(starts) - 1)] < x + n)
    return below | above


def pitch_violations(c):
    """[(w, address, alias)] that break the pitch condition"""
    starts, n = payload_ranges(c)
    bad = []
    for w in WRAPS:
        far = starts[starts >= w]
        for alias in (far - w, far % w):
            hit = _meets(starts, n, alias)
            bad += [(w, int(a), int(x)) for a, x in zip(far[hit][:3], alias[hit][:3])]
    return bad


def zones_touched(c):
    """zones (0: below 2 GiB, 1: [2, 4) GiB, 2: [4, 8) GiB, 3: at or beyond 8 GiB) in which at least one payload row of the case lies"""
    g = geometry(c)
    z = set()
    for b in range(len(c["lens"])):
        r0, r1 = payload_rows(c, b)
        if r1 > r0:
            a = row_address(c, g, b, np.arange(r0, r1))
            z |= {int(x) for x in np.unique(sum((a >= m).astype(np.int64) for m in MARKS))}
    return z


def far_entries(c, w):
    """entries that see a row at or beyond byte offset w"""
    g = geometry(c)
    return [b for b in range(len(c["lens"])) if payload_rows(c, b)[1] > payload_rows(c, b)[0] and int(row_address(c, g, b, c["lens"][b] - 1)) >= w]


def straddlers(c, w):
    """entries with a query row that sees keys on both sides of byte offset w: there a wrapped K offset changes the OUTPUT, not only the LSE"""
    g = geometry(c)
    out = []
    for b in range(len(c["lens"])):
        for t in range(C.case_qlens(c)[b]):
            lo, hi, singles = X.row_keys(c, b, t)
            keys = ([lo, hi - 1] if hi > lo else []) + list(singles)
            side = {int(row_address(c, g, b, j)) >= w for j in keys}
            if len(side) == 2:
                out.append(b)
                break
    return out


def fill_key_weight(c, hk):
    """exp(score) of a key whose K row is the fill, for a query row (Q0, 0, 0, ...): what a wrapped K address turns a key's weight of 1 into"""
    ks, _ = X.case_scales(c)
    s = Q0 * K_FILL * (ks[hk] if ks else 1.0) * c["D"] ** -0.5
    if c.get("cap"):
        s = c["cap"] * np.tanh(s / c["cap"])
    return float(np.exp(s))


def model_output(c, wrap=None, tensor="v"):
    """the census output [B, Sq, Hq, D] (float64) of case c computed from a sparse address -> payload model of the K and the V buffer: every
    key's row of `tensor` ("v" / "k") is looked up at its byte address, reduced modulo `wrap` when given.  An address outside every payload
    reads the fill: a value row of V_FILL in every element; a key row of K_FILL, whose score against the probe's query (Q0 in element 0) is
    not 0 — the key then weighs fill_key_weight instead of 1 (every payload key row holds 0 in element 0, whichever row it is).  Returns
    (out, lse [B, Hq, Sq]): when EVERY key of a row wraps (a far slot) the weights cancel in the output and only the LSE, ln n + score, shows it —
    the batched-chunk entry returns no LSE, so for K addresses its far-slot cases rest on the `pre` cases of the same kernels and tilings."""
    g = geometry(c)
    D, Hkv, G, ql = c["D"], c["Hkv"], c["G"], C.case_qlens(c)
    B, Sq = len(c["lens"]), max(ql)
    _, vs = X.case_scales(c)
    where = {}
    for b in range(B):
        for j in range(*payload_rows(c, b)):
            where[int(row_address(c, g, b, j))] = (c["slots"][b], j)
    out = np.zeros((B, Sq, Hkv * G, D))
    lse = np.full((B, Hkv * G, Sq), np.inf)
    for b in range(B):
        r0, r1 = payload_rows(c, b)
        rows = np.arange(r0, max(r1, r0))
        addr = row_address(c, g, b, rows)
        src = addr % wrap if wrap else addr
        for hk in range(Hkv):
            M = np.zeros((len(rows) + 1, D + 1))          # M[i + 1]: what key r0 + i adds to the numerator (D) and the denominator; then prefix sums
            for i, a in enumerate(src):
                hit = where.get(int(a))
                if tensor == "v":
                    M[i + 1, D] = 1.0
                    if hit is None:
                        M[i + 1, :D] = V_FILL
                    else:
                        M[i + 1, C.residue(hit[1], hk, hit[0], D)] = 1.0
                else:
                    wgt = 1.0 if hit is not None else fill_key_weight(c, hk)
                    M[i + 1, D] = wgt
                    M[i + 1, C.residue(int(rows[i]), hk, c["slots"][b], D)] = wgt
            cum = np.cumsum(M, axis=0)
            for t in range(ql[b]):
                lo, hi, singles = X.row_keys(c, b, t)
                if not max(hi - lo, 0) + len(singles):
                    continue
                assert hi <= lo or lo >= r0, "a visible key below the payload"
                acc = (cum[hi - r0] - cum[lo - r0]) if hi > lo else np.zeros(D + 1)
                for j in singles:
                    acc = acc + M[j - r0 + 1]
                out[b, t, hk * G:(hk + 1) * G] = acc[:D] / acc[D] * vs[hk]
                lse[b, hk * G:(hk + 1) * G, t] = np.log(acc[D])
    return out, lse


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------
def _place(c, geo, zones):
    c = dict(c, geo=geo, zones=tuple(zones), name="%s_%s" % (geo, c["name"]))
    B = len(c["lens"])
    if geo == "slot":
        assert B == len(SLOTS)
        c.update(slots=list(SLOTS), n_slots=9, idx=True)
    else:
        assert B == 1
        c.update(slots=[0], n_slots=1, idx=False)
    return c


def _family(dt, D, geo):
    """every build and plan of the module docstring's list for one (dtype, head size) in geometry `slot` or `row`"""
    tag = "%s_d%d" % (dt, D)
    one = geo == "row"
    B = 1 if one else 5
    dl = [1061] if one else [1034, 33, 1033, 97, 1032]
    mtl = lambda sq: [1061] if one else [1025, 33, 64 + sq - 1, 96 + sq // 2, 1034]
    pl = [1061] if one else [300, 1034, 363, 131, 1000]
    vl, vq = ([1061], [130]) if one else ([300, 701, 577, 1034, 261], [130, 1, 77, 37, 64])
    # a window of 32 keys whose rows straddle a mark (geometry `row`: Lk = 256 / 512 / 1024 puts rows 224.. / 480.. / 992.. in it)
    wl = [[256], [512], [1024]] if one else [dl]
    wz = [(0, 1), (1, 2), (2, 3)] if one else [(0, 1, 2, 3)]
    allz = (0, 1, 2, 3)
    cs = []
    add = lambda c, z=allz: cs.append(_place(c, geo, z))
    # ---- one-token decode: stream (2), uniform split (0), host items (1); one and two head blocks; windowed; the in-kernel one-row append ----
    for G in (4, 17):
        two = 2 if G > 16 else 1
        s = -3 if (one or G > 16) else 0
        add(C._case("dec_stream_%s_g%d" % (tag, G), "dec", dt, D, 2, G, 1, dl, 2, splits=s, tiling=two, append=G == 4))
        add(C._case("dec_grid_%s_g%d" % (tag, G), "dec", dt, D, 2, G, 1, dl, 0, splits=5, tiling=two, append=G == 17))
        add(X._xcase("fp8_dec_stream_%s_g%d" % (tag, G), "dec", dt, D, 2, G, 1, dl, 2, True, splits=s, tiling=two, append=G == 17))
        add(X._xcase("fp8_dec_grid_%s_g%d" % (tag, G), "dec", dt, D, 2, G, 1, dl, 0, True, splits=5, tiling=two, append=G == 4))
        add(dict(C._case("cap_dec_%s_g%d" % (tag, G), "dec", dt, D, 2, G, 1, dl, 2 if G == 4 else 0, splits=s if G == 4 else 5, tiling=two, append=G == 4), cap=CAP))
    if not one:      # (the host item plan needs a batch)
        for tiles in (1, 5):
            add(C._case("dec_items_%s_t%d" % (tag, tiles), "dec", dt, D, 2, 4, 1, dl, 1, host_tiles=tiles, tiling=1, append=tiles == 5))
    for lens, z in zip(wl, wz):
        for G, s, path in ((4, -37, 2), (17, 3, 0)):
            add(C._case("dec_win31_%s_g%d_L%d" % (tag, G, lens[0]), "dec", dt, D, 2, G, 1, lens, path, splits=s, left=31, tiling=2 if G > 16 else 1, append=G == 17), z)
        add(dict(C._case("cap_dec_win31_%s_L%d" % (tag, lens[0]), "dec", dt, D, 2, 4, 1, lens, 2, splits=-37, left=31, tiling=1), cap=CAP), z)
    # ---- multi-token: R = 16 / 32 / 64, causal and not, windowed, with the append launch; tree-masked; over an fp8 cache ----
    for sq, G in ((4, 4), (8, 4), (8, 8)):
        R = sq * G
        Hkv, two = (1 if R > 32 else 2), (2 if R > 16 else 1)
        s = 0 if R > 32 else (-5 if (one or R > 16) else 0)
        path = C.decode_path(R, B, s)
        for causal in (True, False):
            kw = dict(splits=s, causal=causal, tiling=two, append=causal)
            add(C._case("mt_%s_sq%d_g%d_%s" % (tag, sq, G, "causal" if causal else "full"), "mt", dt, D, Hkv, G, sq, mtl(sq), path, **kw))
            add(X._xcase("fp8_mt_%s_sq%d_g%d_%s" % (tag, sq, G, "causal" if causal else "full"), "mt", dt, D, Hkv, G, sq, mtl(sq), path, True, **dict(kw, append=not causal)))
        add(dict(C._case("cap_mt_%s_sq%d_g%d" % (tag, sq, G), "mt", dt, D, Hkv, G, sq, mtl(sq), path, splits=s, tiling=two, append=R == 32), cap=CAP))
        for lens, z in zip(wl, wz):
            add(C._case("mt_win31_%s_sq%d_g%d_L%d" % (tag, sq, G, lens[0]), "mt", dt, D, Hkv, G, sq, lens, path, splits=s, left=31, tiling=two, append=R == 16), z)
        for i, kind in enumerate(("chain", "tree7")):
            for fp8 in (False, True):
                add(X._xcase("tree_%s_%s_sq%d_g%d_%s" % ("fp8" if fp8 else "2b", tag, sq, G, kind), "tree", dt, D, Hkv, G, sq, mtl(sq), path, fp8, mask=kind, splits=s,
                             tiling=two, append=bool(i) ^ fp8))
    # ---- prefill: tilings 1, 4, 7; the KV-split merge; batched chunks; windowed; fp8 and softcap (tilings 1 and 4) ----
    for variant, tiling in ((2, 1), (8, 4), (14, 7)):
        if tiling == 7 and D != 128:
            continue
        vt = "%s_t%d" % (tag, tiling)
        for splits in (1, 3):
            kw = dict(variant=variant, tiling=tiling, merge=int(splits > 1), splits=splits)
            add(C._case("pre_%s_s%d" % (vt, splits), "pre", dt, D, 2, 4, 130, pl, 0, append=splits == 1, **kw))
            add(C._case("pre_win64_%s_s%d" % (vt, splits), "pre", dt, D, 2, 4, 130, pl, 0, left=64, **kw))
            if tiling != 7:
                add(X._xcase("fp8_pre_%s_s%d" % (vt, splits), "pre", dt, D, 2, 4, 130, pl, 0, True, append=splits == 3, **kw))
                add(dict(C._case("cap_pre_%s_s%d" % (vt, splits), "pre", dt, D, 2, 4, 130, pl, 0, **kw), cap=CAP))
                add(dict(C._case("cap_pre_win64_%s_s%d" % (vt, splits), "pre", dt, D, 2, 4, 130, pl, 0, left=64, **kw), cap=CAP))
        kw = dict(qlens=vq, variant=variant, tiling=tiling, merge=0, splits=1)
        add(C._case("var_%s" % vt, "var", dt, D, 2, 4, max(vq), vl, 0, **kw))
        add(C._case("var_win64_%s" % vt, "var", dt, D, 2, 4, max(vq), vl, 0, left=64, **kw))
        if tiling != 7:
            add(X._xcase("fp8_var_%s" % vt, "var", dt, D, 2, 4, max(vq), vl, 0, True, **kw))
    if D == 128:      # the work list: one workgroup per piece, and its persistent form with assigned and with drawn queues
        for pf, kw in (("per_piece", dict(persistent=False, force_tiles=3)), ("assigned", dict(persistent=True, force_tiles=3, drawn=False)),
                       ("drawn", dict(persistent=True, force_tiles=3, drawn=True))):
            add(C._case("list_%s_%s" % (pf, tag), "var", dt, D, 2, 4, max(vq), vl, 1, qlens=vq, pf=kw, tiling=7, merge=1))
    return cs


def _deep(dt, D):
    """windowed builds over a view whose visible tail lies beyond 4 GiB / 8 GiB at the production pitch"""
    tag = "%s_d%d" % (dt, D)
    cs = []
    for Lk, z in zip(DEEP_LENS, (2, 3)):
        for i, left in enumerate((0, 31, 255)):
            nm = "%s_L%d_left%d" % (tag, Lk, left)
            add = lambda c: cs.append(_place(c, "deep", (z,)))
            add(C._case("dec_win_%s" % nm, "dec", dt, D, 2, 4, 1, [Lk], 2, splits=-37, left=left, tiling=1, append=i == 1))
            add(C._case("dec_win_grid_%s" % nm, "dec", dt, D, 2, 17, 1, [Lk], 0, splits=3, left=left, tiling=2))
            add(C._case("mt_win_%s" % nm, "mt", dt, D, 2, 4, 4, [Lk], 0, splits=0, left=left, tiling=1, append=i == 2))
            add(dict(C._case("cap_dec_win_%s" % nm, "dec", dt, D, 2, 4, 1, [Lk], 2, splits=-37, left=left, tiling=1), cap=CAP))
            for variant, tiling in ((2, 1), (8, 4), (14, 7)):
                if (tiling == 7 and D != 128) or (tiling + i) % 3 == 0:      # (each left on two of the three tilings)
                    continue
                kw = dict(variant=variant, tiling=tiling, merge=0, splits=1, left=left)
                add(C._case("pre_win_t%d_%s" % (tiling, nm), "pre", dt, D, 2, 4, 130, [Lk], 0, **kw))
                if tiling != 7:
                    add(dict(C._case("cap_pre_win_t%d_%s" % (tiling, nm), "pre", dt, D, 2, 4, 130, [Lk], 0, **kw), cap=CAP))
    return cs


def cases():
    """the table, ordered by dtype group (f16, bf16, fp8) so that the buffers are filled three times"""
    cs = []
    for dt in ("f16", "bf16"):
        for D in (128, 64):
            cs += _family(dt, D, "slot") + _family(dt, D, "row") + _deep(dt, D)
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return sorted(cs, key=lambda c: ("f16", "bf16", "fp8").index(group(c)))


def entry_point(c):
    """which drop-in / describe entry the case goes through"""
    if c["form"] == "tree":
        return "fp8_tree" if c.get("fp8") else "tree"
    if c.get("fp8"):
        return {"dec": "fp8", "mt": "fp8", "pre": "fp8_prefill", "var": "fp8_varlen"}[c["form"]]
    return ("softcap_" if c.get("cap") else "") + ("varlen" if c["form"] == "var" else "kvcache")


def plan_key(c, queue=""):
    """(geometry, form, path, tiling, merge launch or None, queue, windowed, entry point): what the table names and the launcher asserts"""
    merge = c.get("merge")
    if merge is None and c["form"] in ("dec", "mt", "tree") and (c["path"] in (1, 2) or c["splits"] > 1):
        merge = 1
    if c.get("pf"):
        queue = ("assigned" if not c["pf"].get("drawn") else "drawn") if c["pf"]["persistent"] else "per_piece"
    return (c["geo"], c["form"], c["path"], c["tiling"], merge, queue, c.get("left") is not None, entry_point(c))


def needed_plans():
    """every (geometry, form, path, tiling, merge, queue, windowed, entry point) of the module docstring's list; the table must name each (model test) and the GPU
    run must reach each (test_gpu_far_address.py)"""
    need = set()
    for geo in ("slot", "row"):
        for til in (1, 2):
            need |= {(geo, "dec", 2, til, 1, "", False, e) for e in ("kvcache", "fp8")} | {(geo, "dec", 0, til, 1, "", False, e) for e in ("kvcache", "fp8")}
            need |= {(geo, "dec", 2, 1, 1, "", True, e) for e in ("kvcache", "softcap_kvcache")} | {(geo, "dec", 0, 2, 1, "", True, "kvcache")}
            need |= {(geo, "tree" if "tree" in e else "mt", 2, til, 1, "", False, e)
                     for e in ("kvcache", "fp8", "tree", "fp8_tree", "softcap_kvcache")}
            need |= {(geo, "tree" if "tree" in e else "mt", 0, 2, None, "", False, e) for e in ("kvcache", "fp8", "tree", "fp8_tree", "softcap_kvcache")}
        need |= {(geo, "mt", 2, til, 1, "", True, "kvcache") for til in (1, 2)} | {(geo, "mt", 0, 2, None, "", True, "kvcache")}
        need |= {(geo, "dec", 2, 1, 1, "", False, "softcap_kvcache"), (geo, "dec", 0, 2, 1, "", False, "softcap_kvcache"), (geo, "mt", 2, 1, 1, "", False, "softcap_kvcache")}
        for til in (1, 4):
            for m in (0, 1):
                need |= {(geo, "pre", 0, til, m, "", w, e) for w, e in ((False, "kvcache"), (True, "kvcache"), (False, "fp8_prefill"), (False, "softcap_kvcache"), (True, "softcap_kvcache"))}
            need |= {(geo, "var", 0, til, 0, "", False, "varlen"), (geo, "var", 0, til, 0, "", True, "varlen"), (geo, "var", 0, til, 0, "", False, "fp8_varlen")}
        need |= {(geo, "pre", 0, 7, m, "", w, "kvcache") for m in (0, 1) for w in (False, True)} | {(geo, "var", 0, 7, 0, "", w, "varlen") for w in (False, True)}
        need |= {(geo, "var", 1, 7, 1, q, False, "varlen") for q in ("per_piece", "assigned", "drawn")}
    need |= {("slot", "dec", 1, 1, 1, "", False, "kvcache")}
    need |= {("deep", "dec", 2, 1, 1, "", True, e) for e in ("kvcache", "softcap_kvcache")} | {("deep", "dec", 0, 2, 1, "", True, "kvcache"), ("deep", "mt", 0, 1, None, "", True, "kvcache")}
    need |= {("deep", "pre", 0, til, 0, "", True, "kvcache") for til in (1, 4, 7)} | {("deep", "pre", 0, til, 0, "", True, "softcap_kvcache") for til in (1, 4)}
    return need


def compare(out, lse, c):
    """the census's own bounds: |out - closed form| <= 1 ulp of the output dtype, |lse - ln n| n < 0.25, dead rows 0 and +inf"""
    return X.compare(out, lse, c)


def admissible(c):
    return X.admissible(c)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the buffers and the launcher (GPU)
# ---------------------------------------------------------------------------------------------------------------------------------------
CHUNK = 256 << 20


class Buffers:
    """the K and the V buffer, the fill of the current dtype group, and the whole-buffer check"""

    def __init__(self, dev):
        self.dev = dev
        self.k = torch.empty(BUF_BYTES, dtype=torch.uint8, device=dev)
        self.v = torch.empty(BUF_BYTES, dtype=torch.uint8, device=dev)
        self.group = None

    def fills(self, grp):
        if grp == "fp8":
            return K_FILL8, V_FILL8
        return K_FILL, V_FILL

    def typed(self, buf, grp):
        return buf if grp == "fp8" else buf.view(C.DT[grp])

    def enter(self, grp):
        if grp != self.group:
            kf, vf = self.fills(grp)
            self.typed(self.k, grp).fill_(kf)
            self.typed(self.v, grp).fill_(vf)
            self.group = grp

    def view(self, buf, c):
        g = geometry(c)
        es = g["es"]
        flat = buf.view(torch.float8_e4m3fn) if es == 1 else buf.view(C.DT[c["dt"]])
        return torch.as_strided(flat, (g["n_slots"], g["rows"], c["Hkv"], c["D"]), (g["bs"] // es, g["rs"] // es, g["hs"] // es, 1), g["base"] // es)

    def dirty(self):
        """number of 256-MiB chunks of either buffer that differ from the fill (one host synchronisation)"""
        kf, vf = self.fills(self.group)
        bad = torch.zeros((), dtype=torch.int64, device=self.dev)
        for buf, f in ((self.k, kf), (self.v, vf)):
            t = self.typed(buf, self.group)
            bits = t.view(torch.uint8) if self.group == "fp8" else t.view(torch.int16)
            pat = (torch.tensor(f, dtype=torch.uint8) if self.group == "fp8" else torch.tensor(f, dtype=C.DT[self.group]).view(torch.int16)).item()
            step = CHUNK // bits.element_size()
            for i in range(0, bits.numel(), step):
                bad += (bits[i:i + step] != pat).any()
        return int(bad.item())


def _bits(x):
    return x.view(torch.uint8) if x.element_size() == 1 else x.view(torch.int16)


def run(c, bufs):
    """Run case c through its real drop-in over the far view.  Returns (out, lse or None, plan key reached, view K, view V).  Asserts the plan the
    case names on the block launched; after an appending call the appended rows bit for bit; and — payload saved, fill put back — that the whole
    of both buffers holds the fill again (nothing else was written)."""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    dev = bufs.dev
    bufs.enter(group(c))
    fp8, form, dtype, D, Hkv, G = bool(c.get("fp8")), c["form"], C.DT[c["dt"]], c["D"], c["Hkv"], c["G"]
    lens, slots, ql = c["lens"], c["slots"], C.case_qlens(c)
    B, Sq, Hq = len(lens), max(ql), Hkv * G
    kv, vv = bufs.view(bufs.k, c), bufs.view(bufs.v, c)
    rows = kv.shape[1]
    sn = X.appended_rows(c)
    gen = torch.Generator(device=dev).manual_seed(len(c["name"]) + D)
    ks, vs = X.case_scales(c)
    sc = (torch.tensor(ks, dtype=torch.float32, device=dev), torch.tensor(vs, dtype=torch.float32, device=dev)) if fp8 else ()
    k_new, v_new, want = [], [], []
    for b in range(B):
        r0, r1 = payload_rows(c, b)
        n = r1 - r0
        j = torch.arange(r0, r1, device=dev).view(-1, 1)
        h = torch.arange(Hkv, device=dev).view(1, -1)
        vd = torch.zeros(n, Hkv, D, dtype=torch.float32, device=dev)
        vd.scatter_(2, ((j + 17 * h + 5 * slots[b]) % D).unsqueeze(-1), 1.0)          # tests/census.py census_values, rows r0 .. r1 of one slot
        if fp8:
            kd = X.fp8_random_keys(1, n, Hkv, D, 7 + b, device=dev)[0].view(torch.float8_e4m3fn)
            vd = (vd * X.FP8_ONE).to(torch.uint8).view(torch.float8_e4m3fn)
        else:
            kd = torch.randn(n, Hkv, D, device=dev, dtype=dtype, generator=gen)
            vd = vd.to(dtype)
        _bits(kd)[..., 0] = 0          # element 0 of every payload key row is 0: against q = (Q0, 0, ...) its score is exactly 0, a fill row's is not
        want.append((kd, vd))
        keep = n - sn
        _bits(kv[slots[b], r0:r0 + keep]).copy_(_bits(kd[:keep]))
        _bits(vv[slots[b], r0:r0 + keep]).copy_(_bits(vd[:keep]))
        if sn:
            if fp8:
                k_new.append(X.dequantize_bytes(_bits(kd[keep:]), sc[0], dtype))
                v_new.append(X.dequantize_bytes(_bits(vd[keep:]), sc[1], dtype))
            else:
                k_new.append(kd[keep:].clone())
                v_new.append(vd[keep:].clone())
    newkw = dict(k=torch.stack(k_new), v=torch.stack(v_new)) if sn else {}
    cl = [n - sn for n in lens]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    idx = i32(slots) if c["idx"] else None
    win = (c["left"], 0) if c.get("left") is not None else (-1, -1)
    cap = float(c.get("cap") or 0.0)
    q = torch.zeros(B, Sq, Hq, D, dtype=dtype, device=dev)
    q[..., 0] = Q0
    lse, queue = None, ""
    wrong = []
    try:
        if form == "var":
            T = sum(ql)
            starts = [sum(ql[:i]) for i in range(B)]
            flat_q = torch.zeros(T, Hq, D, dtype=dtype, device=dev)
            flat_q[..., 0] = Q0
            flat = torch.full((T, Hq, D), 7.0, dtype=dtype, device=dev)
            if fp8:
                _, p, mask, scl, pre = X.spy_issue(FA.flash_attn_fp8kv_varlen_with_kvcache, flat_q, kv, vv, *sc, i32(starts), i32(ql), Sq, i32(cl), idx, causal=c["causal"], out=flat,
                                                   _num_splits=c["splits"], _variant=c["variant"], _max_seqlen_k=max(lens))
                assert mask is None and scl is not None and pre is True
            else:
                plan = None
                if c.get("pf"):
                    pb = K.AttnParams()
                    pb.b, pb.seqlen_q, pb.h, pb.h_k, pb.d, pb.is_causal = B, Sq, Hq, Hkv, D, int(c["causal"])
                    pb.o_row_stride, pb.o_head_stride = Hq * D, D
                    plan = FA.prefill_plan(pb, ql, lens, torch.device(dev), **c["pf"])
                    assert plan.t is not None and (plan.n_wg > 0) == c["pf"]["persistent"] and plan.drawn == bool(c["pf"].get("drawn")), c["name"]
                _, p = C.spy_call(FA.flash_attn_varlen_with_kvcache, flat_q, kv, vv, i32(starts), i32(ql), Sq, i32(cl), idx, causal=c["causal"], out=flat, num_splits=c["splits"],
                                  _variant=c["variant"], _max_seqlen_k=max(lens), _pf_plan=plan, window_size=win, softcap=cap)
                if plan is not None:
                    queue = ("assigned" if p.pf_wg_first else "drawn") if p.pf_num_wg else "per_piece"
            out = torch.zeros(B, Sq, Hq, D, dtype=dtype, device=dev)
            for b in range(B):
                out[b, :ql[b]] = flat[starts[b]:starts[b] + ql[b]]
        elif form == "tree":
            fn = FA.flash_attn_fp8kv_tree_with_kvcache if fp8 else FA.flash_attn_tree_with_kvcache
            (out, lse), p, mask, scl, pre = X.spy_issue(fn, q, kv, vv, *sc, X.mask_tensor(c, dev), cache_seqlens=i32(cl), cache_batch_idx=idx, return_softmax_lse=True,
                                                        _num_splits=c["splits"], **newkw)
            assert mask is not None and (scl is not None) == fp8
        elif fp8:
            fn = FA.flash_attn_fp8kv_prefill_with_kvcache if form == "pre" else FA.flash_attn_fp8kv_with_kvcache
            (out, lse), p, mask, scl, pre = X.spy_issue(fn, q, kv, vv, *sc, cache_seqlens=i32(cl), cache_batch_idx=idx, causal=c["causal"], return_softmax_lse=True,
                                                        _num_splits=c["splits"], _variant=c["variant"], **newkw)
            assert mask is None and scl is not None and pre is (form == "pre")
        else:
            host = dict(_cache_seqlens_host=cl, _plan_tiles=c["host_tiles"]) if c.get("host_tiles") else {}
            (out, lse), p = C.spy_call(FA.flash_attn_with_kvcache, q, kv, vv, *(newkw.get("k"), newkw.get("v")), cache_seqlens=i32(cl), cache_batch_idx=idx, causal=c["causal"],
                                       window_size=win, num_splits=c["splits"], return_softmax_lse=True, _variant=c["variant"], softcap=cap, **host)
        torch.cuda.synchronize()
        # ---- the plan, through the describe entry of THIS call, on the block it launched ----
        if form == "tree" or fp8:
            d = X.describe_case(c, p)
            what = X.assert_plan_ext(c, d)
        else:
            d = K.describe_softcap(p, cap) if cap else K.describe(p)
            assert getattr(p, "_softcap", 0.0) == cap
            what = C.assert_plan(c, p, d, rows)
        key = plan_key(c, queue)
        assert key[5] == queue, what
        # ---- what the call wrote ----
        out, lse = out.cpu(), (lse.cpu() if lse is not None else None)
        for b in range(B):
            r0, r1 = payload_rows(c, b)
            kd, vd = want[b]
            if sn and not (torch.equal(_bits(kv[slots[b], r1 - sn:r1]), _bits(kd[r1 - r0 - sn:])) and torch.equal(_bits(vv[slots[b], r1 - sn:r1]), _bits(vd[r1 - r0 - sn:]))):
                wrong.append("entry %d (slot %d): the %d appended rows at %d.. (byte offset %d) are not the given ones" % (b, slots[b], sn, r1 - sn, int(row_address(c, geometry(c), b, r1 - sn))))
    finally:          # whatever happened, the fill goes back over the payload: a failing case must not fail the cases behind it
        kf, vf = bufs.fills(group(c))
        for b in range(B):
            r0, r1 = payload_rows(c, b)
            (kv[slots[b], r0:r1].view(torch.uint8) if fp8 else kv[slots[b], r0:r1]).fill_(kf)
            (vv[slots[b], r0:r1].view(torch.uint8) if fp8 else vv[slots[b], r0:r1]).fill_(vf)
    assert not wrong, what + "\n  " + "\n  ".join(wrong)
    if sn:          # ... and nothing else
        n_bad = bufs.dirty()
        assert n_bad == 0, "%s: after the appending call and with the fill put back over the payload, %d 256-MiB chunks of the buffers differ from the fill" % (what, n_bad)
    return out, lse, key, d
