"""Probes whose expected result is known in closed form — shared by tests/test_census_model.py (CPU: proves the model and the inputs) and the
GPU files tests/test_gpu_census.py, test_gpu_decoy_keys.py, test_gpu_decode_numerics.py.  Plain Python / numpy / torch, no GPU; the census model
imports neither oracle (only `reference`, the fp64 / f32-math expectation of the decoy and score-range inputs, calls them).

THE CENSUS.  q = 0, k arbitrary finite data, one-hot value rows that encode the key's position, kv head and cache slot:
    v[slot, j, h, (j + 17 h + 5 slot) % D] = 1, everything else 0.
Every visible key then has score 0, exp2(0) = 1 exactly (fp32, fp16, bf16), the MFMA accumulates integers in fp32 and the row sum is the integer
n.  Output element d of a row that sees keys [lo, hi) of kv head h in slot s is round_to_dtype(count_d / n), count_d = #{j in [lo, hi) :
(j + 17 h + 5 s) % D == d}, n = hi - lo; its LSE is ln n; n = 0 gives exactly 0 and LSE +inf.  One key dropped, read twice, taken from the
neighbouring kv head or slot, or admitted at a mask edge moves an element by ~1/n: >= 4 ulp of the output dtype while ceil(n / D) <= 256
(fp16) / 32 (bf16) — `admissible`.

THE VISIBLE INTERVAL (include/vattn_kernels.h, VISIBILITY, restated here as a per-row function — a third statement of the rule beside
oracle/attn.py and tests/window_ref.py, imported from neither): with Lk visible keys and Sq query rows, row t sees keys j <= Lk - Sq + t
when causal (a one-row call: all of them) and all j < Lk otherwise; with a window also j >= max(0, Lk - Sq + t - left).
"""
import random

import numpy as np
import torch

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
MANT = {"f16": 10, "bf16": 7}
MAX_KEYS_PER_RESIDUE = {"f16": 256, "bf16": 32}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------
def visible_interval(sq, Lk, t, causal, left):
    """[lo, hi) of query row t (0-based) of an entry with sq query rows and Lk visible keys; left = None: no window."""
    if Lk <= 0:
        return 0, 0
    hi = Lk
    if causal and sq > 1:
        hi = Lk - sq + t + 1
    lo = 0
    if left is not None:
        lo = Lk - sq + t - left
        if lo < 0:
            lo = 0
    if hi > Lk:
        hi = Lk
    if hi <= lo:
        return 0, 0
    return lo, hi


def residue(j, h, slot, D):
    return (j + 17 * h + 5 * slot) % D


def counts(lo, hi, h, slot, D):
    """count_d for keys [lo, hi) of kv head h in slot `slot`: int64[D]"""
    n = hi - lo
    if n <= 0:
        return np.zeros(D, dtype=np.int64)
    d = np.arange(D)
    return n // D + (((d - residue(lo, h, slot, D)) % D) < n % D).astype(np.int64)


def ulp(x, dt):
    """unit in the last place of dtype `dt` ("f16" / "bf16") at the float64 magnitudes x (> 0; fp16 subnormals: 2^-24)"""
    x = np.asarray(x, dtype=np.float64)
    e = np.floor(np.log2(np.where(x > 0, x, 1.0)))
    if dt == "f16":
        e = np.maximum(e, -14)
    return np.exp2(e - MANT[dt])


def case_qlens(c):
    """query rows per entry"""
    return list(c["qlens"]) if c.get("qlens") else [c["sq"]] * len(c["lens"])


def expected(c):
    """(exp float64 [B, Sq, Hq, D], n int64 [B, Sq, Hq]) of case c; Sq = max query rows, rows an entry does not have stay 0 / n = -1"""
    D, Hkv, G = c["D"], c["Hkv"], c["G"]
    lens, ql = c["lens"], case_qlens(c)
    B, Sq = len(lens), max(ql)
    slots = c.get("slots") or list(range(B))
    exp = np.zeros((B, Sq, Hkv * G, D))
    n = np.full((B, Sq, Hkv * G), -1, dtype=np.int64)
    for b in range(B):
        for t in range(ql[b]):
            lo, hi = visible_interval(ql[b], lens[b], t, c["causal"], c.get("left"))
            for hk in range(Hkv):
                cnt = counts(lo, hi, hk, slots[b], D)
                n[b, t, hk * G:(hk + 1) * G] = hi - lo
                if hi > lo:
                    exp[b, t, hk * G:(hk + 1) * G] = cnt / float(hi - lo)
    return exp, n


def census_values(n_slots, rows, Hkv, D, dtype, device="cpu"):
    """v[slot, j, h, (j + 17 h + 5 slot) % D] = 1"""
    j = torch.arange(rows, device=device).view(1, rows, 1)
    h = torch.arange(Hkv, device=device).view(1, 1, Hkv)
    s = torch.arange(n_slots, device=device).view(n_slots, 1, 1)
    r = (j + 17 * h + 5 * s) % D
    v = torch.zeros(n_slots, rows, Hkv, D, dtype=dtype, device=device)
    v.scatter_(3, r.unsqueeze(-1), 1.0)
    return v


def admissible(c):
    """ceil(n / D) <= 256 (fp16) / 32 (bf16) for every row of the case"""
    _, n = expected(c)
    return int(n.max()) <= MAX_KEYS_PER_RESIDUE[c["dt"]] * c["D"]


def compare(out, lse, c, lse_factor=0.25):
    """out [B, Sq, Hq, D] (any float tensor on the CPU), lse [B, Hq, Sq] or None, against the closed form.  Returns (failures, stats):
    failures is a list of strings naming the element — entry, row, head, residue, and the key positions that residue stands for."""
    exp, n = expected(c)
    got = out.double().numpy()
    ql = case_qlens(c)
    live = n >= 0
    fails = []
    err = np.abs(got - exp)
    u = ulp(exp, c["dt"])
    zero_bad = (exp == 0) & (got != 0) & live[..., None]
    # written as "not within", so that a NaN (a masked P = 0 times a poisoned V = Inf) fails like any other wrong element
    bad = (~(err <= u) & (exp > 0)) | zero_bad | ~np.isfinite(got)
    ulps = np.where(np.isfinite(got), err / u, np.inf)[exp > 0]
    stats = {"max_ulp": float(ulps.max()) if ulps.size else 0.0, "lse_worst_times_n": 0.0}
    if not np.isfinite(got).all():
        fails.append("%d output elements are not finite (a read of the poisoned rows behind the visible keys?)" % (~np.isfinite(got)).sum())
    if bad.any():
        for b, t, h, d in np.argwhere(bad)[:6]:
            lo, hi = visible_interval(ql[b], c["lens"][b], t, c["causal"], c.get("left"))
            slot = (c.get("slots") or list(range(len(c["lens"]))))[b]
            hk = h // c["G"]
            j0 = (d - 17 * hk - 5 * slot) % c["D"]
            fails.append("entry %d row %d head %d (kv head %d, slot %d) element %d: got %.9g, expected %d/%d = %.9g (%.2f ulp); keys [%d, %d), this residue = keys %d + %d i"
                         % (b, t, h, hk, slot, d, got[b, t, h, d], round(exp[b, t, h, d] * max(n[b, t, h], 1)), n[b, t, h], exp[b, t, h, d],
                            err[b, t, h, d] / u[b, t, h, d], lo, hi, j0, c["D"]))
    if lse is not None:
        l = lse.double().numpy().transpose(0, 2, 1)          # [B, Sq, Hq]
        dead = n == 0
        if not np.array_equal(np.isposinf(l) & live, dead):
            fails.append("LSE: rows without a visible key must be +inf, and only those (%d dead rows, %d +inf)" % (dead.sum(), (np.isposinf(l) & live).sum()))
        ok = n > 0
        if ok.any():
            with np.errstate(invalid="ignore"):
                e = np.abs(l - np.log(np.maximum(n, 1)))[ok] * n[ok]
            e = np.where(np.isfinite(e), e, np.inf)
            stats["lse_worst_times_n"] = float(e.max())
            if e.max() >= lse_factor:
                fails.append("LSE: |lse - ln n| * n = %.4f >= %.2f" % (e.max(), lse_factor))
    return fails, stats


# ---------------------------------------------------------------------------------------------------------------------------------------
# the shared case table of the GPU census (tests/test_gpu_census.py runs it, tests/test_census_model.py proves it admissible)
#   form   "dec" one-token decode | "mt" multi-token | "pre" prefill (flash_attn_with_kvcache) | "var" batched chunks (varlen)
#   lens   VISIBLE keys per entry (after the append, when there is one)
#   path   what vattn_attn_plan_describe must answer: decode 0 uniform grid split / 1 host items / 2 device-planned stream; prefill 0 grid / 1 list
# ---------------------------------------------------------------------------------------------------------------------------------------
# Lk % 32 in {0, 1, 31}, Lk % 64 in {0, 1, 63}; with left = 31 / 1000 the one-token window start Lk - 1 - left sits on a 32-key tile edge
# (64, 96, 1033) and one to either side (63, 65, 95, 97, 1032, 1034)
DEC_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 1032, 1033, 1034, 4095, 16384]
RAGGED16 = [100, 20000, 257, 4096, 31, 9999, 12345, 1024, 16000, 700, 19999, 3, 5000, 2048, 8191, 64]      # test_gpu_multitoken_decode._ragged16


def cut(lens, dt, D):
    """the lengths cut to what is admissible with comfortable margin: ceil(n / D) <= 128 (fp16) / 23 (bf16)"""
    cap = (128 if dt == "f16" else 23) * D
    return [x if x <= cap else cap - 37 * i for i, x in enumerate(lens)]


def _case(name, form, dt, D, Hkv, G, sq, lens, path, **kw):
    c = dict(name=name, form=form, dt=dt, D=D, Hkv=Hkv, G=G, sq=sq, lens=list(lens), path=path, causal=True, left=None, append=False, idx=False,
             splits=0, variant=0)
    c.update(kw)
    if c["append"]:                                    # the call appends sq rows (decode: one): every entry then sees at least those
        c["lens"] = [max(x, sq) for x in c["lens"]]
    B = len(c["lens"])
    c["n_slots"] = B + 3 if c["idx"] else B
    c["slots"] = random.Random(B * 7 + sq + G).sample(range(c["n_slots"]), B) if c["idx"] else list(range(B))
    return c


def _lefts(lens):
    """the issue's list; the entry '> Lk' as max(lens) + 5 (a window wider than every sequence that the library still runs as a window: the
    view has more rows than that)"""
    return [0, 1, 31, 32, 33, 1000, max(lens) + 5]


def gpu_cases():
    cs = []
    flip = 0
    for dt in ("f16", "bf16"):
        for D in (128, 64):
            tag = "%s_d%d" % (dt, D)
            dl = cut(DEC_LENS, dt, D)
            rg = cut(RAGGED16, dt, D)
            # ---- one-token decode ----
            for G in (1, 4, 7, 16, 17, 32, 40):
                Hkv = 1 if G >= 32 else 2
                two = 2 if G > 16 else 1
                flip += 1
                ap, ix = bool(flip & 1), bool(flip & 2)
                # device-planned stream: default grid for G <= 16 (wider groups take it only with a forced grid), forced grids for G <= 32
                for s in (0, -1, -3, -37):
                    if G > 32 or (s == 0 and G > 16):
                        continue
                    if dt == "bf16" and s in (-1, -3) and G not in (4, 17):
                        continue
                    cs.append(_case("dec_stream_%s_g%d_s%d" % (tag, G, s), "dec", dt, D, Hkv, G, 1, dl, 2, splits=s, tiling=two, merge=1, append=ap, idx=ix))
                # uniform grid split: wide groups by default, explicit split counts for all
                for s in ((0, 5) if G > 16 else (5,)):
                    cs.append(_case("dec_grid_%s_g%d_s%d" % (tag, G, s), "dec", dt, D, Hkv, G, 1, dl, 0, splits=s, tiling=two, merge=1 if s > 1 else None,
                                    append=not ap, idx=not ix))
                # host item plan: pieces of one and of five tiles (a seam at every tile edge / every fifth)
                if G <= 32:
                    for tiles in (1, 5):
                        cs.append(_case("dec_items_%s_g%d_t%d" % (tag, G, tiles), "dec", dt, D, Hkv, G, 1, dl, 1, host_tiles=tiles, tiling=two, merge=1, append=ap, idx=not ix))
            cs.append(_case("dec_one_sequence_%s" % tag, "dec", dt, D, 2, 4, 1, cut([16384], dt, D), 0, tiling=1, merge=1))
            cs.append(_case("dec_ragged16_%s" % tag, "dec", dt, D, 2, 4, 1, rg, 2, tiling=1, merge=1, idx=True, append=True))
            # windowed one-token decode
            for left in _lefts(dl):
                for G, s, path in ((4, 0, 2), (4, -37, 2), (7, 3, 0), (17, 0, 0), (17, -3, 2)):
                    if dt == "bf16" and (G, s) not in ((4, 0), (17, -3)):
                        continue
                    cs.append(_case("dec_win%d_%s_g%d_s%d" % (left, tag, G, s), "dec", dt, D, 2, G, 1, dl, path, splits=s, left=left, tiling=2 if G > 16 else 1,
                                    merge=1 if (path == 2 or s > 1) else None, append=bool(left & 1), idx=bool(left & 2)))
            # ---- multi-token form: R = sq G in <= 16, 17..32, 33..64; Lk < sq (dead rows); a tail that spans two tiles (1 <= Lk % 32 < sq) ----
            for sq, G in ((2, 4), (3, 1), (5, 2), (8, 2), (2, 16), (3, 7), (8, 4), (5, 8), (8, 8), (8, 7)):
                R = sq * G
                ml = cut([sq - 1, sq, 1, 32, 33, 64 + sq - 1, 96 + sq // 2, 127, 1025, 2048 + 1, 4095, 9000 + sq - 1], dt, D)
                Hkv = 1 if R > 32 else 2
                two = 2 if R > 16 else 1
                flip += 1
                ap, ix = bool(flip & 1), bool(flip & 2)
                for causal in (True, False):
                    if R <= 32:
                        for s in ((0, -3, -400) if R <= 16 else (-3, -400)):
                            if (dt == "bf16" or not causal) and s == -3:
                                continue
                            cs.append(_case("mt_stream_%s_sq%d_g%d_s%d_%s" % (tag, sq, G, s, "causal" if causal else "full"), "mt", dt, D, Hkv, G, sq, ml, 2, splits=s,
                                            causal=causal, tiling=two, merge=1, append=ap, idx=ix))
                    if R > 16:      # uniform grid split (two-block workgroups; R > 32: sibling head-block groups)
                        cs.append(_case("mt_grid_%s_sq%d_g%d_%s" % (tag, sq, G, "causal" if causal else "full"), "mt", dt, D, Hkv, G, sq, ml, 0, causal=causal,
                                        tiling=2, merge=None, append=not ap, idx=not ix))
                if ((sq, G) in ((2, 4), (5, 2), (8, 2), (3, 7), (8, 4), (8, 8)) and dt == "f16") or (sq, G) in ((2, 4), (8, 8)):
                    for left in _lefts(ml):
                        s = -400 if left in (31, 32, 1000) else 0
                        path = 2 if (R <= 16 or (R <= 32 and s < 0)) else 0
                        cs.append(_case("mt_win%d_%s_sq%d_g%d_s%d" % (left, tag, sq, G, s), "mt", dt, D, Hkv, G, sq, ml, path, splits=s, left=left, tiling=two,
                                        merge=1 if path == 2 else None, append=bool(left & 1) ^ ap, idx=ix))
            cs.append(_case("mt_one_sequence_%s" % tag, "mt", dt, D, 2, 4, 4, cut([16001], dt, D), 0, tiling=1, merge=1, append=True))
            cs.append(_case("mt_ragged16_%s" % tag, "mt", dt, D, 2, 4, 4, rg, 2, tiling=1, merge=1, append=True, idx=True))
            # ---- prefill: explicit tilings (variant 2 / 8 / 14 -> tiling 1 / 4 / 7), the two-launch KV split, non-causal, Sq > Lk, windows on
            # the 64-key tile (window start on a tile edge and one to either side: Lk - Sq - left = 64, 63, 65 for row 0) ----
            for variant, tiling in ((2, 1), (8, 4), (14, 7)):
                if tiling == 7 and D != 128:
                    continue
                vt = "%s_t%d" % (tag, tiling)
                pl = cut([300, 301, 363, 364, 1500 + 300, 2111], dt, D)
                cs.append(_case("pre_%s" % vt, "pre", dt, D, 2, 4, 300, pl, 0, variant=variant, tiling=tiling, merge=0, splits=1, idx=True))
                cs.append(_case("pre_append_%s" % vt, "pre", dt, D, 2, 2, 130, [130, 131, 700], 0, variant=variant, tiling=tiling, merge=0, splits=1, append=True))
                cs.append(_case("pre_split3_%s" % vt, "pre", dt, D, 2, 4, 300, pl, 0, variant=variant, tiling=tiling, merge=1, splits=3))
                cs.append(_case("pre_full_%s" % vt, "pre", dt, D, 1, 4, 257, [257, 64, 1, 1000], 0, variant=variant, tiling=tiling, merge=0, splits=1, causal=False))
                cs.append(_case("pre_sq_gt_lk_%s" % vt, "pre", dt, D, 2, 2, 150, [90, 149, 150, 1], 0, variant=variant, tiling=tiling, merge=0, splits=1))
                cs.append(_case("var_%s" % vt, "var", dt, D, 2, 4, 513, [300, 701, 577, 1037, 261], 0, qlens=[300, 1, 513, 37, 256], variant=variant, tiling=tiling,
                                merge=0, splits=1, idx=True))
                for left, s in ((0, 1), (1, 1), (63, 1), (64, 2), (65, 1), (1000, 1), (236, 1), (235, 3), (237, 1)):
                    if dt == "bf16" and left not in (0, 64, 236):
                        continue
                    cs.append(_case("pre_win%d_%s_s%d" % (left, vt, s), "pre", dt, D, 2, 4, 300, [300, 600, 601, 663, 1800], 0, variant=variant, tiling=tiling,
                                    merge=1 if s > 1 else 0, splits=s, left=left))
                cs.append(_case("var_win64_%s" % vt, "var", dt, D, 2, 4, 513, [300, 701, 577, 1037, 261], 0, qlens=[300, 1, 513, 37, 256], variant=variant,
                                tiling=tiling, merge=0, splits=1, left=64))
            # the work list (d = 128): one workgroup per piece, and its persistent form with assigned and with drawn queues
            if D == 128:
                for pf, kw in (("per_piece", dict(persistent=False, force_tiles=3)), ("assigned", dict(persistent=True, force_tiles=3, drawn=False)),
                               ("drawn", dict(persistent=True, force_tiles=3, drawn=True)), ("per_piece_t1", dict(persistent=False, force_tiles=1))):
                    for causal in (True, False):
                        if not causal and pf != "assigned":
                            continue
                        cs.append(_case("list_%s_%s_%s" % (pf, tag, "causal" if causal else "full"), "var", dt, D, 2, 4, 600, [600, 1300, 257, 41, 2000],
                                        1, qlens=[600, 300, 257, 1, 64], pf=kw, tiling=7, merge=1, causal=causal, idx=True))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def decode_path(R, B, splits, host_items=False):
    """the path a decode-form call is meant to take (include/vattn_kernels.h, vattn_plan_desc; R = seqlen_q G columns per kv head): host items
    when given; the device-planned stream for R <= 32 with a forced grid (num_splits < 0) and, by default, for batches of R <= 16; else the
    uniform grid split (one sequence, wide groups, sibling head-block groups of R > 32, explicit split counts)"""
    if host_items:
        return 1
    if splits > 0 or R > 32:
        return 0
    if splits < 0:
        return 2
    return 2 if (B >= 2 and R <= 16) else 0


def sweep_case(seed):
    """one random draw of the census sweep: form, sq, heads, D, dtype, lengths, left, num_splits, append and slots"""
    rng = random.Random(50_000 + seed)
    dt = rng.choice(["f16", "f16", "bf16"])
    D = rng.choice([64, 128, 128])
    form = rng.choice(["dec", "dec", "mt", "mt", "mt", "pre"])
    cap = (128 if dt == "f16" else 23) * D
    if form == "pre":
        sq = rng.choice([2, 17, 64, 100, 129, 257, 300])
        Hkv, G = rng.choice([1, 2]), rng.choice([1, 2, 4, 7])
        B = rng.choice([1, 2, 3])
        lens = [rng.choice([0, 1, 30, 64, 333, 600, 1200]) + (sq if rng.random() < 0.85 else rng.randrange(1, sq + 1)) for _ in range(B)]
        causal = rng.random() < 0.8
        left = rng.choice([None, None, 0, 1, 63, 64, 65, 200, 1000]) if causal else None
        variant = rng.choice([2, 8] + ([14, 14] if D == 128 else []))
        splits = rng.choice([1, 1, 2, 3])
        return _case("sweep%d" % seed, "pre", dt, D, Hkv, G, sq, [min(x, cap) for x in lens], 0, causal=causal, left=left, variant=variant, splits=splits,
                     tiling={2: 1, 8: 4, 14: 7}[variant], merge=1 if splits > 1 else 0, idx=rng.random() < 0.5, append=False)
    sq = 1 if form == "dec" else rng.choice([2, 3, 4, 5, 8])
    G = rng.choice([g for g in (1, 2, 4, 7, 8, 16, 17, 32, 40) if sq * g <= 64])
    Hkv = rng.choice([1, 2, 4]) if sq * G <= 32 else 1
    B = rng.choice([1, 2, 5, 9, 16])
    top = rng.choice([40, 700, 2100, 6000, 16384])
    lens = [min(cap, rng.randrange(1, top)) for _ in range(B)]          # (multi-token: Lk < sq gives dead rows)
    left = rng.choice([None, None, 0, 1, 31, 32, 33, 100, 1000, top + 7])
    causal = True if (left is not None or form == "dec") else rng.random() < 0.8
    splits = rng.choice([0, 0, -1, -3, -37, -200, 2, 9]) if form == "dec" else rng.choice([0, 0, -1, -3, -37, -200])
    path = decode_path(sq * G, B, splits)
    c = _case("sweep%d" % seed, form, dt, D, Hkv, G, sq, lens, path, causal=causal, left=left, splits=splits, tiling=2 if sq * G > 16 else 1,
              merge=1 if (path == 2 or splits > 1) else None, idx=rng.random() < 0.6, append=rng.random() < 0.6)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------
# decoy keys (tests/test_gpu_decoy_keys.py): a needle k[j*] = 2 q_row at an admitted position, decoys 3 q_row at the excluded ones
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_to_plant(c):
    """(entry, row t, needle kind) triples: which rows of the call carry a needle, and where in their interval"""
    out = []
    for b, spec in enumerate(c["needles"]):
        for t, kind in spec:
            out.append((b, t, kind))
    return out


def decoy_inputs(c, seed=0):
    """CPU tensors of a decoy case: q [B, Sq, Hq, D], the caches AFTER the append kc / vc [slots, rows, Hkv, D] (all rows finite), and
    `plants`: (entry, row, head, slot, kv head, j*) of every needle.  Every planted cell is registered: two plants never share a cell."""
    g = torch.Generator().manual_seed(1000 + seed)
    dtype, D, Hkv, G, lens = DT[c["dt"]], c["D"], c["Hkv"], c["G"], c["lens"]
    ql = case_qlens(c)
    B, Sq, Hq = len(lens), max(ql), Hkv * G
    rows = max(lens) + 8
    q = torch.randn(B, Sq, Hq, D, generator=g).to(dtype)
    kc = (0.1 * torch.randn(c["n_slots"], rows, Hkv, D, generator=g)).to(dtype)
    vc = torch.randn(c["n_slots"], rows, Hkv, D, generator=g).to(dtype)
    cells, plants = {}, []

    def plant(slot, j, hk, vec, who, unused_slot=False):
        if j < 0 or j >= rows:
            return
        key = (slot, j, hk)
        # (cells of a slot no entry uses may be re-planted: whatever row reads one is wrong already)
        assert unused_slot or key not in cells, "decoy construction: %s and %s share cache cell %s" % (cells[key], who, key)
        cells[key] = who
        kc[slot, j, hk] = vec.to(dtype)

    for n_, (b, t, kind) in enumerate(_rows_to_plant(c)):
        lo, hi = visible_interval(ql[b], lens[b], t, c["causal"], c.get("left"))
        if hi <= lo:
            continue
        hk = (t + b) % Hkv
        h = hk * G + (t % G)
        js = {"last": hi - 1, "first": lo, "0": 0, "31": 31, "32": 32, "63": 63, "64": 64}.get(kind, kind if isinstance(kind, int) else None)
        if js is None or not lo <= js < hi or (kind == "first" and lo == 0 and t > 0):      # (a window clamped at key 0: one row per entry takes key 0)
            js = hi - 1
        slot = c["slots"][b]
        # the needle's query row is scaled to |q|^2 = 12 sqrt(D): its needle scores 2 |q|^2 D^-0.5 = 24 (probability > 1 - 1e-4 among a few
        # thousand background keys of score ~0), an admitted decoy would score 36
        qr = q[b, t, h].float()
        q[b, t, h] = (qr * (12 * D ** 0.5 / (qr * qr).sum()) ** 0.5).to(dtype)
        qr = q[b, t, h].float()
        plant(slot, js, hk, 2 * qr, "needle(%d,%d)" % (b, t))
        plants.append((b, t, h, slot, hk, js))
        plant(slot, hi, hk, 3 * qr, "decoy hi(%d,%d)" % (b, t))                       # the next row: a later draft token's, or the next cache row
        if lo > 0:
            plant(slot, lo - 1, hk, 3 * qr, "decoy lo-1(%d,%d)" % (b, t))
        # the same position under another kv head: hk + 2, because the direct neighbours are taken at this position — consecutive rows use
        # consecutive kv heads, so (js, hk - 1) may hold the previous row's hi decoy and (js, hk + 1) the next row's lo - 1 decoy (a needle on
        # the first key of a window; the registry above refuses hk + 1 there).  Needs four kv heads: every decoy case has them.
        if Hkv > 2:
            plant(slot, js, (hk + 2) % Hkv, 3 * qr, "decoy kv head(%d,%d)" % (b, t))
        other = next(s for s in range(c["n_slots"]) if s not in c["slots"])
        plant(other, js, hk, 3 * qr, "decoy slot(%d,%d)" % (b, t), unused_slot=True)                     # the same position in another slot
    return q, kc, vc, plants


def decoy_cases():
    cs = []
    kinds = ["last", "first", "0", "31", "32", "63", "64", 95, 96, 159, 160]      # 95 / 96, 159 / 160: last / first key of a piece of three / five 32-key tiles
    for dt, D in (("f16", 128), ("bf16", 128), ("f16", 64)):
        tag = "%s_d%d" % (dt, D)
        lens = [700, 33, 64, 65, 300, 161, 97, 1000, 450, 129, 200]
        for left in (None, 200):
            w = "win%d" % left if left is not None else "nowin"
            # one-token decode: entry b carries needle kind b.  (windowed: a kind outside the window falls back to the window's last key)
            for G, s, path in ((4, 0, 2), (4, -50, 2), (4, 3, 0), (17, 0, 0)):
                cs.append(_case("decoy_dec_%s_%s_g%d_s%d" % (tag, w, G, s), "dec", dt, D, 4, G, 1, lens, path, splits=s, left=left, idx=True, append=(G == 4),
                                tiling=2 if G > 16 else 1, needles=[[(0, kinds[b])] for b in range(len(lens))]))
            cs.append(_case("decoy_dec_%s_%s_items_t3" % (tag, w), "dec", dt, D, 4, 4, 1, lens, 1 if left is None else 2, host_tiles=3, left=left, idx=True, tiling=1,
                            needles=[[(0, kinds[b])] for b in range(len(lens))]))
            # multi-token: hi - 1 for EVERY token of entries 0-3 (the decoy at hi is the next draft token's row), other kinds for the rest
            for sq, G, s in ((4, 4, 0), (4, 4, -50), (8, 4, -50), (8, 8, 0)):
                R = sq * G
                path = 2 if (R <= 16 or (R <= 32 and s < 0)) else 0
                nd = [[(t, "last") for t in range(sq)] if b < 4 else [(b % sq, kinds[b])] for b in range(len(lens))]
                cs.append(_case("decoy_mt_%s_%s_sq%d_g%d_s%d" % (tag, w, sq, G, s), "mt", dt, D, 4, G, sq, lens, path, splits=s, left=left, idx=True, append=True,
                                tiling=2 if R > 16 else 1, needles=nd))
            # prefill tilings 1, 4, 7
            for variant, tiling in ((2, 1), (8, 4), (14, 7)):
                if tiling == 7 and D != 128:
                    continue
                pl = [300, 364, 900]
                rows_ = [0, 31, 63, 64, 127, 128, 255, 256, 299]
                nd = [[(t, "last" if left is None else ("last", "first")[(i + b) & 1]) for i, t in enumerate(rows_)] for b in range(len(pl))]      # (no window: every row's first key is key 0)
                cs.append(_case("decoy_pre_%s_%s_t%d" % (tag, w, tiling), "pre", dt, D, 4, 2, 300, pl, 0, variant=variant, tiling=tiling, splits=1, left=left, idx=True,
                                needles=nd))
    return cs


# ---------------------------------------------------------------------------------------------------------------------------------------
# score-range inputs of the decode and merge kernels (tests/test_gpu_decode_numerics.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
SPIKE = 110.0      # score of a spiked key in natural-log units: exp(-110) underflows to 0 in fp32, so every other piece's merge weight is exactly 0
# Scaling written down (the admissibility rule: the oracle's f32 math within half the tolerance of its f64 math, asserted for every set by
# tests/test_census_model.py): background keys 0.3 randn — scores of unit size; a spike k = SPIKE unit(q_row) D^0.5 / |q_row| puts exactly one
# key SPIKE above the rest for its own row (for the other rows of the kv head it is a score of about +-10: a moderate spike of their own).
# The 3e4 value rows: magnitudes 3e4 (0.9 + 0.1 u) with ONE sign per (slot, kv head, d), so that every output element is near 3e4 in
# magnitude and the relative part of the tolerance applies.  [First tried with a random sign per element: the averages cancel to ~1e3 with
# absolute errors of a few units from rounding P and the output to fp16 — the f32-math oracle itself missed half the tolerance by 1.9.]


def numerics_cases():
    cs = []
    lens = [700, 1023, 96, 33, 400, 1200]
    forms = [("dec", 1, 4), ("dec", 1, 17), ("mt", 4, 4), ("mt", 4, 8), ("mt", 8, 8)]      # R = 4, 17 (two blocks), 16, 32, 64
    for dt in ("f16", "bf16"):
        for form, sq, G in forms:
            R = sq * G
            Hkv = 1 if R > 32 else 2
            for kind in ("late", "early", "one_piece", "v3e4"):
                if kind == "v3e4" and dt != "f16":
                    continue
                for left in (None, 300):
                    if left is not None and kind in ("one_piece", "v3e4") and form == "dec":
                        continue
                    for s in ((0, -2, -50) if kind == "one_piece" else (0, -50)):
                        if dt == "bf16" and s == -50 and kind != "late":
                            continue
                        path = 2 if ((R <= 16 and s == 0) or (R <= 32 and s < 0)) else 0
                        cs.append(_case("num_%s_%s_%s_sq%d_g%d_%s_s%d" % (kind, dt, form, sq, G, "win%d" % left if left is not None else "nowin", s), form, dt, 128,
                                        Hkv, G, sq, lens, path, splits=s, left=left, kind=kind, tiling=2 if R > 16 else 1, append=(form == "mt"), idx=True, scale=None))
        # no visible key in a piece: windowed multi-token calls with one-tile pieces whose first tile holds a key for row 0 only (Lk - sq - left
        # = 31 mod 32: row 1's window starts in the next tile, its partial of the first piece is -inf), entries with dead rows, and a windowed
        # one-token call cut into more shares than it has visible tiles
        cs.append(_case("num_empty_piece_%s_mt" % dt, "mt", dt, 128, 2, 4, 4, [3, 4 + 31 + 100, 4 + 63 + 100, 1000, 4 + 95 + 100], 2, splits=-200, left=100, kind="plain", tiling=1,
                        append=True, idx=True, scale=None))
        cs.append(_case("num_empty_piece_%s_mt_R32" % dt, "mt", dt, 128, 2, 8, 4, [3, 4 + 31 + 100, 4 + 63 + 100, 1000, 4 + 95 + 100], 2, splits=-200, left=100, kind="plain",
                        tiling=2, append=True, idx=True, scale=None))
        cs.append(_case("num_empty_piece_%s_dec" % dt, "dec", dt, 128, 2, 4, 1, [700, 40, 1023, 1], 0, splits=16, left=40, kind="plain", tiling=1, idx=True, scale=None))
        for sc in (1.0, 0.02, 1.7):
            for form, sq, G, s in (("dec", 1, 4, 0), ("dec", 1, 17, 0), ("mt", 4, 4, 0), ("mt", 4, 8, -50), ("mt", 8, 8, 0)):
                R = sq * G
                path = 2 if ((R <= 16 and s == 0) or (R <= 32 and s < 0)) else 0
                for left in (None, 300):
                    if left is not None and form == "dec" and G == 17:
                        continue
                    cs.append(_case("num_scale%g_%s_%s_sq%d_g%d_%s" % (sc, dt, form, sq, G, "win" if left is not None else "nowin"), form, dt, 128, 1 if R > 32 else 2, G, sq,
                                    lens, path, splits=s, left=left, kind="plain", tiling=2 if R > 16 else 1, append=(form == "mt"), idx=True,
                                    scale=sc if sc != 1.7 else 1.7 * 128 ** -0.5))
    return cs


def numerics_inputs(c, seed=0):
    """q, kc, vc (caches after the append, every row finite) of a score-range case"""
    g = torch.Generator().manual_seed(7000 + seed + c["sq"] * 131 + c["G"] * 17 + (c["left"] or 0))
    dtype, D, Hkv, G, lens = DT[c["dt"]], c["D"], c["Hkv"], c["G"], c["lens"]
    sq = c["sq"]
    B, Hq = len(lens), Hkv * G
    rows = max(lens) + 8
    q = torch.randn(B, sq, Hq, D, generator=g).to(dtype)
    kc = (0.3 * torch.randn(c["n_slots"], rows, Hkv, D, generator=g)).to(dtype)
    vc = torch.randn(c["n_slots"], rows, Hkv, D, generator=g).to(dtype)
    kind = c["kind"]
    if kind == "v3e4":
        mag = 3e4 * (0.9 + 0.1 * torch.rand(vc.shape, generator=g))
        sign = torch.where(torch.rand(c["n_slots"], 1, Hkv, D, generator=g) < 0.5, -1.0, 1.0)      # one sign per (slot, kv head, d): no cancellation
        vc = (mag * sign).to(dtype)
    if kind in ("late", "early", "one_piece", "v3e4"):
        for b in range(B):
            for hk in range(Hkv):
                t = (b + hk) % sq
                h = hk * G + (b % G)
                lo, hi = visible_interval(sq, lens[b], t, c["causal"], c.get("left"))
                if hi <= lo:
                    continue
                j = {"late": hi - 1 - (b % 3), "early": lo + (b % 3), "one_piece": (lo + hi) // 2, "v3e4": (lo + hi) // 2}[kind]
                j = min(max(j, lo), hi - 1)
                qr = q[b, t, h].float()
                kc[c["slots"][b], j, hk] = (SPIKE * D ** 0.5 * qr / (qr * qr).sum()).to(dtype)
    return q, kc, vc


def reference(c, q, kc, vc, math="f64", return_lse=False):
    """the oracle's statement of case c on CPU tensors (caches AFTER the append): oracle/attn.py, or tests/window_ref.py with a window.
    Returns out [B, Sq, Hq, D] (+ LSE [B, Hq, Sq]); the batched-chunk form entry by entry, rows an entry does not have stay 0."""
    from oracle.attn import flash_attn_with_kvcache_ref
    from tests.window_ref import window_attn_ref
    idx = torch.tensor(c["slots"], dtype=torch.int32)

    def one(q_, lens_, idx_):
        if c.get("left") is None:
            return flash_attn_with_kvcache_ref(q_, kc, vc, cache_seqlens=torch.tensor(lens_, dtype=torch.int32), cache_batch_idx=idx_, softmax_scale=c.get("scale"),
                                               causal=c["causal"], math=math, return_lse=True)
        return window_attn_ref(q_, kc, vc, c["left"], cache_seqlens=lens_, cache_batch_idx=idx_, softmax_scale=c.get("scale"), math=math, return_lse=True)
    if not c.get("qlens"):
        out, lse = one(q, c["lens"], idx)
    else:
        B, Sq = len(c["lens"]), max(c["qlens"])
        out = torch.zeros(B, Sq, q.shape[2], q.shape[3], dtype=torch.float64 if math == "f64" else q.dtype)
        lse = torch.zeros(B, q.shape[2], Sq, dtype=torch.float64)
        for b, n in enumerate(c["qlens"]):
            o, l = one(q[b:b + 1, :n], [c["lens"][b]], idx[b:b + 1])
            out[b, :n], lse[b, :, :n] = o[0], l[0]
    return (out, lse) if return_lse else out


def inputs_key(c):
    """what the inputs (and so the oracle's answers) of a decoy / score-range case depend on: everything but how the launch is planned"""
    return (c["form"], c["dt"], c["D"], c["Hkv"], c["G"], c["sq"], c["left"], c["causal"], tuple(c["lens"]), tuple(c["slots"]), c.get("kind"), c.get("scale"), str(c.get("needles")))


def tol(dtype):
    """the project's tolerance (tests/test_gpu_attention.py): atol = rtol = 2e-3 for fp16, 1.6e-2 for bf16"""
    return (2e-3, 2e-3) if dtype in (torch.float16, "f16") else (1.6e-2, 1.6e-2)


def check(out_gpu, ref64, ref32, dtype, what):
    """tests/test_gpu_attention.py `_check`, restated once for the probe files: the tolerance, and 2 x the error of the f32-math oracle"""
    atol, rtol = tol(dtype)
    got = out_gpu.double().cpu()
    err = (got - ref64).abs()
    bound = atol + rtol * ref64.abs()
    assert bool((err <= bound).all()), "%s: max err %.3e (allowed %.3e)" % (what, err.max().item(), bound.max().item())
    e_ref = (ref32.double() - ref64).abs().max().item()
    assert err.max().item() <= 2 * e_ref + 1e-5 + (0 if dtype == torch.float16 else 4e-3), \
        "%s: kernel err %.3e vs reference-numerics err %.3e" % (what, err.max().item(), e_ref)


def check_lse(lse, lse64, what):
    """tests/test_gpu_multitoken_decode.py `_check_lse`, restated: 2e-3 absolute, rows without a visible key +inf"""
    lse = lse.double().cpu()
    dead = torch.isinf(lse64)
    assert torch.equal(torch.isinf(lse) & (lse > 0), dead & (lse64 > 0)), what + ": rows without a visible key have LSE +inf"
    assert ((lse - lse64)[~dead]).abs().max().item() < 2e-3, what


def spy_call(fn, *a, **kw):
    """fn(*a, **kw) of the drop-in, and the ONE parameter block it launched (seen at its launch point)"""
    from vattention_amd import flash_attn as FA
    seen, real = [], FA._launch

    def spy(p, dev, keep=()):
        seen.append(p)
        return real(p, dev, keep)
    FA._launch = spy
    try:
        r = fn(*a, **kw)
    finally:
        FA._launch = real
    assert len(seen) == 1
    return r, seen[0]


def cut_out_appended(c, k_fin, v_fin, fill_k, fill_v):
    """caches given AS AFTER the call -> (k cache, v cache, (k, v) to append or (None, None), cache_seqlens): the rows the call appends are cut
    out into k / v and hold fill_k / fill_v before the call"""
    lens, slots = c["lens"], c["slots"]
    sn = (1 if c["form"] == "dec" else c["sq"]) if c["append"] else 0
    if not sn:
        return k_fin, v_fin, (None, None), list(lens)
    B = len(lens)
    new = (torch.stack([k_fin[slots[b], lens[b] - sn:lens[b]] for b in range(B)]), torch.stack([v_fin[slots[b], lens[b] - sn:lens[b]] for b in range(B)]))
    kc, vc = k_fin.clone(), v_fin.clone()
    for b in range(B):
        kc[slots[b], lens[b] - sn:lens[b]], vc[slots[b], lens[b] - sn:lens[b]] = fill_k, fill_v
    return kc, vc, new, [n - sn for n in lens]


def assert_plan(c, p, d, rows):
    """the form, path, tiling, merge launch and window field the case meant to reach"""
    what = "%s: plan %s" % (c["name"], d)
    assert d["form"] == (0 if c["form"] in ("pre", "var") else 1), what
    assert p.window_left_plus1 == (c["left"] + 1 if c.get("left") is not None and c["left"] < rows else 0), what
    assert d["tiling"] == c["tiling"] and d["path"] == c["path"], what
    merge = c.get("merge")
    if merge is None and c["form"] in ("dec", "mt") and (c["path"] in (1, 2) or c["splits"] > 1):
        merge = 1            # items and stream pieces are always merged by a second launch; so are explicit split counts
    if merge is not None:
        assert d["merge_launch"] == merge, what
    return what


def launch(c, q, kc, vc, dev):
    """Run a decode / multi-token / prefill case on CPU inputs whose caches are given AS AFTER the append.  Asserts the launch plan the case
    names (assert_plan) through the plan description of the parameter block the drop-in launches, and that the cache after the call is the
    given one bit for bit.  Returns (out, lse, plan description)."""
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    kf, vf = kc.to(dev), vc.to(dev)
    kg, vg, new, cl = cut_out_appended(c, kf, vf, 0.5, -0.25)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    host = dict(_cache_seqlens_host=cl, _plan_tiles=c["host_tiles"]) if c.get("host_tiles") and c["left"] is None else {}
    (out, lse), p = spy_call(FA.flash_attn_with_kvcache, q.to(dev), kg, vg, *new, cache_seqlens=i32(cl), cache_batch_idx=i32(c["slots"]) if c["idx"] else None,
                             causal=c["causal"], window_size=(c["left"], 0) if c["left"] is not None else (-1, -1), num_splits=c["splits"],
                             softmax_scale=c.get("scale"), return_softmax_lse=True, _variant=c["variant"], **host)
    torch.cuda.synchronize()
    d = K.describe(p)
    what = assert_plan(c, p, d, kc.shape[1])
    if new[0] is not None:
        assert torch.equal(kg, kf) and torch.equal(vg, vf), what + ": the cache after the append"
    return out, lse, d
