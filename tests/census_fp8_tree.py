"""The closed-form probes of tests/census.py for the builds it does not reach: FP8 (e4m3) decode and prefill, tree-masked multi-token decode over
a 2-byte and over an FP8 cache.  Beside tests/census.py, which it imports and leaves as it is: the model (`expected` / `compare` here take a
per-row key SET and per-head value scales, and hand every other case to tests/census.py), the case tables, the seeded sweep, the decoy
constructions and the launcher through the real drop-ins.  Plain Python / numpy / torch, no GPU; the model imports neither tests/tree_ref.py
nor the oracle (only `xreference`, the fp64 / f32-math expectation the CPU proof compares the model with, calls the references).
Shared by tests/test_census_fp8_tree_model.py (CPU: proves the model and the inputs), tests/test_gpu_census_fp8_tree.py and
tests/test_gpu_decoy_keys_fp8_tree.py."""
import random

import numpy as np
import torch

from tests import census as _census
from tests.census import (DEC_LENS, DT, MAX_KEYS_PER_RESIDUE, RAGGED16, _case, case_qlens, census_values, check, counts, cut, cut_out_appended, decode_path,  # noqa: F401
                          decoy_inputs, inputs_key, residue, tol, ulp, visible_interval)


def expected(c):
    """tests/census.py `expected`, also for a per-row key SET (tree masks) and per-head value scales (fp8 caches)"""
    return _expected_ext(c) if is_ext(c) else _census.expected(c)


def compare(out, lse, c, lse_factor=0.25):
    """tests/census.py `compare`, also for those cases: a tree row's message names the draft keys of the wrong residue and their mask bits"""
    return _compare_ext(out, lse, c, lse_factor) if is_ext(c) else _census.compare(out, lse, c, lse_factor)


def admissible(c):
    """ceil(n / D) <= 256 (fp16) / 32 (bf16) for every row of the case"""
    _, n = expected(c)
    return int(n.max()) <= MAX_KEYS_PER_RESIDUE[c["dt"]] * c["D"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the FP8-cache (e4m3) and tree-masked builds (tests/test_census_fp8_tree_model.py proves what follows on the CPU; the GPU files are
# tests/test_gpu_census_fp8_tree.py and tests/test_gpu_decoy_keys_fp8_tree.py).  A case of these tables is a `_case` dict with more keys:
#   form   also "tree": the tree-masked multi-token call            fp8    the caches are float8_e4m3fn bytes with one scale per kv head
#   masks  tree only: [B][sq] mask words as Python ints in [0, 2^32) — bits >= sq are garbage on purpose
#
# THE TREE RULE (include/vattn_kernels.h, "tree-masked multi-token form", restated as a per-row set; a third statement beside
# tests/tree_ref.py and the kernels, imported from neither): with Lk visible keys, sq nodes and base = Lk - sq, node t sees the interval
# [0, max(base, 0)) and the single keys base + s, 0 <= s < sq, with bit s of word t set and base + s >= 0.
#
# FP8 CENSUS INPUTS.  V bytes 0x38 (stored 1.0) at residue (j + 17 h + 5 slot) % D, 0x00 elsewhere; v_scale[h] = 1, 2, 4, 8: a row's
# output is round(count_d / n * v_scale[h]) — the ulp is taken at that magnitude, so admissibility is unchanged, and a scale taken from
# another head is off by a factor >= 2.  K bytes uniformly random over the 254 non-NaN bytes (+-448, subnormals, -0 included), k_scale[h]
# distinct powers of two in [1/4, 4]: with q = 0 every score is +-0.  Powers of two make "dequantise, hand to the call as k / v,
# requantise" the identity, so the cache after an appending call is the given one, every byte.
# ---------------------------------------------------------------------------------------------------------------------------------------
FP8_ONE, FP8_NAN = 0x38, 0x7F
E4M3_FINITE = [b for b in range(256) if (b & 0x7F) != 0x7F]
K_SCALES = [0.25, 4.0, 0.5, 2.0]
V_SCALES = [1.0, 2.0, 4.0, 8.0]
TREE7 = [0b1, 0b11, 0b101, 0b1011, 0b10011, 0b100101, 0b1100101, 0b11100101]      # tools/kbench.py's 7-node tree 0-1-{3,4}, 0-2-5-6 (+ a child of node 6)
XSPARE = 8          # rows of the cache view behind the longest entry
MASK_KINDS = ("chain", "ones", "zero", "tree7", "noself", "last0", "rand")


def e4m3_value(byte):
    """the value of an OCP e4m3fn byte (sign, 4 exponent bits of bias 7, 3 mantissa bits; S.1111.111 is NaN, there is no infinity)"""
    s = -1.0 if byte & 0x80 else 1.0
    e, m = (byte >> 3) & 15, byte & 7
    if e == 15 and m == 7:
        return float("nan")
    return s * (m / 8.0) * 2.0 ** -6 if e == 0 else s * (1 + m / 8.0) * 2.0 ** (e - 7)


def is_ext(c):
    return bool(c.get("fp8")) or c.get("masks") is not None


def case_scales(c):
    """(k_scale, v_scale) lists per kv head of an fp8 case; (None, [1.0] * Hkv) for a 2-byte cache"""
    if not c.get("fp8"):
        return None, [1.0] * c["Hkv"]
    return list(c.get("k_scale") or K_SCALES[:c["Hkv"]]), list(c.get("v_scale") or V_SCALES[:c["Hkv"]])


def tree_visible(sq, Lk, word):
    """(hi of the committed interval [0, hi), [visible draft keys]) of a node whose mask word is `word`"""
    if Lk <= 0:
        return 0, []
    base = Lk - sq
    w = word & ((1 << sq) - 1)
    return max(base, 0), [base + s for s in range(sq) if (w >> s) & 1 and base + s >= 0]


def row_keys(c, b, t):
    """the key SET of row t of entry b: (lo, hi, [single keys]) — an interval and a few keys beside it"""
    ql = case_qlens(c)
    if c.get("masks") is not None:
        hi, singles = tree_visible(ql[b], c["lens"][b], c["masks"][b][t])
        return 0, hi, singles
    lo, hi = visible_interval(ql[b], c["lens"][b], t, c["causal"], c.get("left"))
    return lo, hi, []


def set_counts(lo, hi, singles, h, slot, D):
    cnt = counts(lo, hi, h, slot, D)
    for j in singles:
        cnt[residue(j, h, slot, D)] += 1
    return cnt


def _expected_ext(c):
    D, Hkv, G = c["D"], c["Hkv"], c["G"]
    lens, ql = c["lens"], case_qlens(c)
    B, Sq = len(lens), max(ql)
    slots = c.get("slots") or list(range(B))
    _, vs = case_scales(c)
    exp = np.zeros((B, Sq, Hkv * G, D))
    n = np.full((B, Sq, Hkv * G), -1, dtype=np.int64)
    for b in range(B):
        for t in range(ql[b]):
            lo, hi, singles = row_keys(c, b, t)
            m = max(hi - lo, 0) + len(singles)
            for hk in range(Hkv):
                n[b, t, hk * G:(hk + 1) * G] = m
                if m:
                    exp[b, t, hk * G:(hk + 1) * G] = set_counts(lo, hi, singles, hk, slots[b], D) / float(m) * vs[hk]
    return exp, n


def _row_story(c, b, t, hk, slot, d):
    """which keys residue d stands for in row (b, t): the interval's, and for a tree row every draft key of that residue with its mask bit"""
    lo, hi, singles = row_keys(c, b, t)
    j0 = (d - 17 * hk - 5 * slot) % c["D"]
    s = "keys [%d, %d)%s, this residue = keys %d + %d i" % (lo, hi, (" + " + str(singles)) if singles else "", j0, c["D"])
    if c.get("masks") is not None:
        sq, word = case_qlens(c)[b], c["masks"][b][t]
        base = c["lens"][b] - sq
        hit = ["draft key %d = base %d + %d: bit %d of mask word 0x%08x is %s" % (base + k, base, k, k, word, "SET" if (word >> k) & 1 else "clear")
               for k in range(sq) if base + k >= 0 and residue(base + k, hk, slot, c["D"]) == d]
        if base >= 1 and residue(base - 1, hk, slot, c["D"]) == d:
            hit.append("key %d = base - 1, the last committed key" % (base - 1))
        if residue(base + sq, hk, slot, c["D"]) == d:
            hit.append("key %d = base + sq, the first row behind the draft" % (base + sq))
        s += "; " + ("; ".join(hit) if hit else "no draft key has this residue")
    return s


def _compare_ext(out, lse, c, lse_factor=0.25):
    """`compare` for a per-row key SET and per-head value scales: the ulp is taken at count_d / n * v_scale"""
    exp, n = _expected_ext(c)
    got = out.double().numpy()
    live = n >= 0
    _, vs = case_scales(c)
    fails = []
    err = np.abs(got - exp)
    u = ulp(exp, c["dt"])
    zero_bad = (exp == 0) & (got != 0) & live[..., None]
    bad = (~(err <= u) & (exp > 0)) | zero_bad | ~np.isfinite(got)
    ulps = np.where(np.isfinite(got), err / u, np.inf)[exp > 0]
    stats = {"max_ulp": float(ulps.max()) if ulps.size else 0.0, "lse_worst_times_n": 0.0}
    if not np.isfinite(got).all():
        fails.append("%d output elements are not finite (a read of the poisoned rows behind the visible keys?)" % (~np.isfinite(got)).sum())
    if bad.any():
        slots = c.get("slots") or list(range(len(c["lens"])))
        where = np.argwhere(bad)
        # the worst elements first: the residue of the one key that is missing or extra, ahead of the elements that only feel the changed n
        rank = np.where(np.isfinite(got) & ~zero_bad, err / u, np.inf)[bad]
        for b, t, h, d in where[np.argsort(-rank, kind="stable")[:6]]:
            hk = h // c["G"]
            fails.append("entry %d row %d head %d (kv head %d, slot %d, v_scale %g) element %d: got %.9g, expected %d/%d x %g = %.9g (%.2f ulp); %s"
                         % (b, t, h, hk, slots[b], vs[hk], d, got[b, t, h, d], round(exp[b, t, h, d] / vs[hk] * max(n[b, t, h], 1)), n[b, t, h], vs[hk], exp[b, t, h, d],
                            err[b, t, h, d] / u[b, t, h, d], _row_story(c, b, t, hk, slots[b], d)))
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
                b, t, h = np.argwhere(ok)[int(np.argmax(e))]
                fails.append("LSE: |lse - ln n| * n = %.4f >= %.2f (entry %d row %d head %d, n = %d)" % (e.max(), lse_factor, b, t, h, n[b, t, h]))
    return fails, stats


def fp8_census_values(n_slots, rows, Hkv, D, device="cpu"):
    """uint8 [slots, rows, Hkv, D]: 0x38 (1.0) at residue (j + 17 h + 5 slot) % D, 0x00 elsewhere"""
    return (census_values(n_slots, rows, Hkv, D, torch.float32, device) * FP8_ONE).to(torch.uint8)


def fp8_random_keys(n_slots, rows, Hkv, D, seed, device="cpu"):
    """uint8 [slots, rows, Hkv, D], uniform over the 254 non-NaN e4m3 bytes"""
    g = torch.Generator(device=device).manual_seed(seed)
    table = torch.tensor(E4M3_FINITE, dtype=torch.uint8, device=device)
    return table[torch.randint(0, len(E4M3_FINITE), (n_slots, rows, Hkv, D), generator=g, device=device)]


def dequantize_bytes(u8, scale, dtype):
    """bytes [..., Hkv, D] -> stored * scale[h] in `dtype` (exact for power-of-two scales; fp32 product otherwise)"""
    return (u8.view(torch.float8_e4m3fn).float() * torch.as_tensor(scale, dtype=torch.float32, device=u8.device).view(-1, 1)).to(dtype)


def mask_words(kind, B, sq, seed=0):
    """[B][sq] mask words of the table's mask kinds"""
    rng = random.Random(9000 + seed)
    full = (1 << sq) - 1
    out = []
    for b in range(B):
        if kind == "chain":
            w = [(2 << t) - 1 for t in range(sq)]
        elif kind == "ones":
            w = [0xFFFFFFFF] * sq
        elif kind == "zero":
            w = [0] * sq
        elif kind == "tree7":
            w = TREE7[:sq]
        elif kind == "noself":                         # the ancestors of a chain without the node itself (node 0: a word of 0)
            w = [((2 << t) - 1) & ~(1 << t) for t in range(sq)]
        elif kind == "last0":                          # the last node sees draft key 0 only
            w = [(2 << t) - 1 for t in range(sq - 1)] + [1]
        else:                                          # random words, garbage in bits >= sq (every third entry: the sign bit too)
            w = [rng.randrange(0, full + 1) | (rng.randrange(0, 1 << (31 - sq)) << sq) | (0x80000000 if b % 3 == 2 else 0)
                 for t in range(sq)]
        out.append([int(x) & 0xFFFFFFFF for x in w])
    return out


def _xcase(name, form, dt, D, Hkv, G, sq, lens, path, fp8, mask=None, **kw):
    c = _case(name, form, dt, D, Hkv, G, sq, lens, path, fp8=bool(fp8), **kw)
    if form == "tree":
        c["causal"] = False
        c["mask_kind"] = mask if isinstance(mask, str) else "given"
        c["masks"] = mask_words(mask, len(c["lens"]), sq, seed=sq * 100 + G) if isinstance(mask, str) else [list(m) for m in mask]
    return c


def tree_lens(sq):
    """the issue's list: Lk = sq (base 0), sq - 1 (base < 0), the draft rows inside one tile, straddling a 32-key edge (base = 29 / 31 mod 32), a
    full last tile, and lengths that several pieces share"""
    return [sq, sq - 1, 40 + sq, 93 + sq, 95 + sq, 64, 1025, 4095, 9000]


def fp8_cases():
    """FP8 decode (one token, multi-token) and FP8 prefill (tilings 1 and 4, batched chunks); bf16 trimmed as in gpu_cases()"""
    cs = []
    flip = 0
    for dt in ("f16", "bf16"):
        for D in (128, 64):
            tag = "%s_d%d" % (dt, D)
            dl = cut(DEC_LENS, dt, D)
            rg = cut(RAGGED16, dt, D)
            for G in (1, 4, 16, 17, 40):
                if dt == "bf16" and G not in (4, 17):
                    continue
                Hkv = 4 if G <= 4 else 1 if G >= 32 else 2
                two = 2 if G > 16 else 1
                flip += 1
                ap, ix = bool(flip & 1), bool(flip & 2)
                for s in (0, -3, -37):
                    if G > 32 or (s == 0 and G > 16):
                        continue
                    cs.append(_xcase("fp8_dec_stream_%s_g%d_s%d" % (tag, G, s), "dec", dt, D, Hkv, G, 1, dl, 2, True, splits=s, tiling=two, merge=1, append=ap, idx=ix))
                for s in ((0, 5) if G > 16 else (5,)):
                    cs.append(_xcase("fp8_dec_grid_%s_g%d_s%d" % (tag, G, s), "dec", dt, D, Hkv, G, 1, dl, 0, True, splits=s, tiling=two, merge=1 if s > 1 else None,
                                     append=not ap, idx=not ix))
            cs.append(_xcase("fp8_dec_one_sequence_%s" % tag, "dec", dt, D, 2, 4, 1, cut([16384], dt, D), 0, True, tiling=1, merge=1))
            cs.append(_xcase("fp8_dec_ragged16_%s" % tag, "dec", dt, D, 2, 4, 1, rg, 2, True, tiling=1, merge=1, idx=True, append=True))
            for sq, G in ((2, 4), (5, 2), (8, 2), (3, 7), (8, 4), (8, 8)):
                R = sq * G
                ml = cut([sq - 1, sq, 1, 32, 33, 64 + sq - 1, 96 + sq // 2, 127, 1025, 2048 + 1, 4095, 9000 + sq - 1], dt, D)
                Hkv = 1 if R > 32 else 2
                two = 2 if R > 16 else 1
                flip += 1
                ap, ix = bool(flip & 1), bool(flip & 2)
                for causal in (True, False):
                    if R <= 32:
                        for s in ((0, -400) if R <= 16 else (-400,)):
                            if dt == "bf16" and s == -400 and R <= 16 and not causal:
                                continue
                            cs.append(_xcase("fp8_mt_stream_%s_sq%d_g%d_s%d_%s" % (tag, sq, G, s, "causal" if causal else "full"), "mt", dt, D, Hkv, G, sq, ml, 2, True,
                                             splits=s, causal=causal, tiling=two, merge=1, append=ap, idx=ix))
                    if R > 16:
                        cs.append(_xcase("fp8_mt_grid_%s_sq%d_g%d_%s" % (tag, sq, G, "causal" if causal else "full"), "mt", dt, D, Hkv, G, sq, ml, 0, True, causal=causal,
                                         tiling=2, merge=None, append=not ap, idx=not ix))
            cs.append(_xcase("fp8_mt_one_sequence_%s" % tag, "mt", dt, D, 2, 4, 4, cut([16001], dt, D), 0, True, tiling=1, merge=1, append=True))
            for variant, tiling in ((2, 1), (8, 4)):
                vt = "%s_t%d" % (tag, tiling)
                pl = cut([300, 301, 363, 364, 1500 + 300, 2111], dt, D)
                cs.append(_xcase("fp8_pre_%s" % vt, "pre", dt, D, 2, 4, 300, pl, 0, True, variant=variant, tiling=tiling, merge=0, splits=1, idx=True))
                cs.append(_xcase("fp8_pre_split3_%s" % vt, "pre", dt, D, 2, 4, 300, pl, 0, True, variant=variant, tiling=tiling, merge=1, splits=3))
                cs.append(_xcase("fp8_var_%s" % vt, "var", dt, D, 2, 4, 513, [300, 701, 577, 1037, 261], 0, True, qlens=[300, 1, 513, 37, 256], variant=variant,
                                 tiling=tiling, merge=0, splits=1, idx=True))
                if dt == "bf16":
                    continue
                cs.append(_xcase("fp8_pre_append_%s" % vt, "pre", dt, D, 2, 2, 130, [130, 131, 700], 0, True, variant=variant, tiling=tiling, merge=0, splits=1, append=True))
                cs.append(_xcase("fp8_pre_full_%s" % vt, "pre", dt, D, 1, 4, 257, [257, 64, 1, 1000], 0, True, variant=variant, tiling=tiling, merge=0, splits=1, causal=False))
                cs.append(_xcase("fp8_pre_sq_gt_lk_%s" % vt, "pre", dt, D, 2, 2, 150, [90, 149, 150, 1], 0, True, variant=variant, tiling=tiling, merge=0, splits=1))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def tree_cases():
    """tree-masked multi-token decode over a 2-byte and over an FP8 cache (`fp8`): every (sq, G) x mask kind for fp16, three mask kinds for
    bf16; the cache kind and the plan (default / forced stream grid) alternate so that D = 128 and D = 64 hold the two halves"""
    cs = []
    for ti, (dt, D) in enumerate((("f16", 128), ("f16", 64), ("bf16", 128), ("bf16", 64))):
        tag = "%s_d%d" % (dt, D)
        for i, (sq, G) in enumerate(((2, 4), (5, 2), (8, 2), (8, 4), (8, 8), (2, 24))):
            R = sq * G
            Hkv = 1 if R > 32 else 2
            for m, kind in enumerate(MASK_KINDS):
                if dt == "bf16" and kind not in ("rand", "tree7", "chain"):
                    continue
                fp8 = bool((i + m + ti) & 1)
                forced = bool(((i + m) >> 1 ^ ti) & 1)
                s = -5 if forced else 0
                path = decode_path(R, 9, s)
                cs.append(_xcase("tree_%s_%s_sq%d_g%d_%s_s%d" % ("fp8" if fp8 else "2b", tag, sq, G, kind, s), "tree", dt, D, Hkv, G, sq, cut(tree_lens(sq), dt, D), path,
                                 fp8, mask=kind, splits=s, tiling=2 if R > 16 else 1, merge=1 if path == 2 else None, append=bool((i + m) & 1), idx=bool((i + m) & 2)))
        # one sequence has nothing to balance: the grid heuristics with ONE 16-column block per workgroup and striped pieces; the three draft
        # rows straddle a tile edge (4095 - 3 = 28 mod 32 ... 4094: keys 28-30 of a tile; 1054 - 3 = 27 mod 32 likewise: 2049 puts them on 30, 31 | 0)
        for fp8 in (False, True):
            cs.append(_xcase("tree_%s_%s_one_sequence" % ("fp8" if fp8 else "2b", tag), "tree", dt, D, 2, 4, 3, cut([2049], dt, D), 0, fp8,
                             mask=[[0b100, 0b011, 0b101]], tiling=1, merge=1, append=fp8))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def xsweep_case(seed):
    """one random draw of the FP8 / tree census sweep: form, cache kind, sq, heads, D, dtype, lengths, mask words, num_splits, append and slots"""
    rng = random.Random(70_000 + seed)
    dt = rng.choice(["f16", "f16", "bf16"])
    D = rng.choice([64, 128, 128])
    form = rng.choice(["dec", "mt", "mt", "tree", "tree", "tree", "pre"])
    fp8 = True if form != "tree" else rng.random() < 0.5
    cap = (128 if dt == "f16" else 23) * D
    name = "xsweep%d" % seed
    if form == "pre":
        sq = rng.choice([9, 17, 64, 100, 129, 257, 300])
        Hkv, G = rng.choice([1, 2, 4]), rng.choice([1, 2, 4, 7])
        B = rng.choice([1, 2, 3])
        lens = [rng.choice([0, 1, 30, 64, 333, 600, 1200]) + (sq if rng.random() < 0.85 else rng.randrange(1, sq + 1)) for _ in range(B)]
        variant = rng.choice([2, 8])
        splits = rng.choice([1, 1, 2, 3])
        return _xcase(name, "pre", dt, D, Hkv, G, sq, [min(x, cap) for x in lens], 0, True, causal=rng.random() < 0.8, variant=variant, splits=splits,
                      tiling={2: 1, 8: 4}[variant], merge=1 if splits > 1 else 0, idx=rng.random() < 0.5, append=rng.random() < 0.3)
    sq = 1 if form == "dec" else rng.choice([2, 3, 4, 5, 7, 8])
    G = rng.choice([g for g in (1, 2, 4, 7, 8, 16, 17, 24, 32, 40) if sq * g <= 64])
    Hkv = rng.choice([1, 2, 4]) if sq * G <= 32 else 1
    B = rng.choice([1, 2, 5, 9, 16])
    top = rng.choice([40, 700, 2100, 6000, 16384])
    lens = [min(cap, rng.choice([sq, max(sq - 1, 1), rng.randrange(1, top), rng.randrange(1, top)])) for _ in range(B)]
    if form == "dec":
        splits = rng.choice([0, 0, -1, -3, -37, -200, 2, 9])
    else:
        splits = rng.choice([0, 0, -1, -3, -37, -200])
    path = decode_path(sq * G, B, splits)
    kw = dict(splits=splits, tiling=2 if sq * G > 16 else 1, merge=1 if (path == 2 or splits > 1) else None, idx=rng.random() < 0.6, append=rng.random() < 0.6)
    if form != "tree":
        return _xcase(name, form, dt, D, Hkv, G, sq, lens, path, True, causal=True if form == "dec" else rng.random() < 0.7, **kw)
    c = _xcase(name, "tree", dt, D, Hkv, G, sq, lens, path, fp8, mask=rng.choice(MASK_KINDS + ("rand", "rand", "rand")), **kw)
    return c


def small_twin(c, limit=2100):
    """the case without its entries of more than `limit` keys (None: nothing is left)"""
    keep = [b for b, n in enumerate(c["lens"]) if n <= limit]
    if not keep:
        return None
    t = dict(c)
    for k in ("lens", "slots", "qlens", "masks", "needles"):
        if c.get(k):
            t[k] = [c[k][b] for b in keep]
    return t


def mask_tensor(c, device="cpu"):
    """int32 [B, sq] mask words of a tree case"""
    return torch.tensor([[w - (1 << 32) if w >= 1 << 31 else w for w in row] for row in c["masks"]], dtype=torch.int32, device=device)


def xreference(c, q, kc, vc, math="f64", return_lse=False):
    """tests/fp8kv_ref.py, tests/tree_ref.py or tests/fp8kv_tree_ref.py on CPU tensors of case c (caches AFTER the append; an fp8 case: the
    float8_e4m3fn tensors and the case's scales).  Returns out [B, Sq, Hq, D] (+ LSE [B, Hq, Sq]); batched chunks entry by entry."""
    from tests.fp8kv_ref import fp8kv_attn_ref
    from tests.fp8kv_tree_ref import fp8kv_tree_ref
    from tests.tree_ref import tree_attn_ref
    idx = torch.tensor(c["slots"], dtype=torch.int32)
    ks, vs = case_scales(c)
    if c.get("fp8"):
        ks, vs = torch.tensor(ks, dtype=torch.float32), torch.tensor(vs, dtype=torch.float32)
    if c["form"] == "tree":
        cl = torch.tensor(c["lens"], dtype=torch.int32)
        if c.get("fp8"):
            return fp8kv_tree_ref(q, kc, vc, ks, vs, mask_tensor(c), cache_seqlens=cl, cache_batch_idx=idx, softmax_scale=c.get("scale"), math=math, return_lse=return_lse)
        return tree_attn_ref(q, kc, vc, mask_tensor(c), cache_seqlens=cl, cache_batch_idx=idx, softmax_scale=c.get("scale"), math=math, return_lse=return_lse)
    assert c.get("fp8") and c.get("left") is None

    def one(q_, lens_, idx_):
        return fp8kv_attn_ref(q_, kc, vc, ks, vs, cache_seqlens=torch.tensor(lens_, dtype=torch.int32), cache_batch_idx=idx_, softmax_scale=c.get("scale"),
                              causal=c["causal"], math=math, return_lse=True)
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


def appended_rows(c):
    return (1 if c["form"] == "dec" else c["sq"]) if c["append"] else 0


def plan_block(c, rows=None):
    """the parameter block of case c as far as the library's plan description reads it (shapes, flags, which optional pointers are set): the
    host-only statement of what launch_ext's drop-in call builds — no device, nothing is dereferenced"""
    from vattention_amd import kernels as K
    lens = c["lens"]
    rows = rows or max(lens) + XSPARE
    p = K.AttnParams()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = len(lens), max(case_qlens(c)), rows, appended_rows(c), c["Hkv"] * c["G"], c["Hkv"], c["D"]
    p.is_causal = 0 if c["form"] == "tree" else int(c["causal"])
    p.dtype, p.num_splits, p.variant = (0 if c["dt"] == "f16" else 1), c["splits"], c["variant"]
    p.cache_seqlens = 4096
    if c["idx"]:
        p.cache_batch_idx = 4096
    if c["form"] == "var":
        p.q_lens = p.q_start = 4096
        p.max_seqlen_k_hint = min(max(lens), rows)
    return p


def describe_case(c, p):
    """the plan description of block p through the describe entry of the call case c makes"""
    from vattention_amd import kernels as K
    if c["form"] == "tree":
        return K.describe_fp8kv_tree(p) if c.get("fp8") else K.describe_tree(p)
    assert c.get("fp8")
    return K.describe_fp8kv_prefill(p) if c["form"] in ("pre", "var") else K.describe_fp8kv(p)


def assert_plan_ext(c, d):
    """the form, path, tiling and merge launch the case meant to reach"""
    what = "%s: plan %s" % (c["name"], d)
    assert d["form"] == (0 if c["form"] in ("pre", "var") else 1), what
    assert d["tiling"] == c["tiling"] and d["path"] == c["path"], what
    merge = c.get("merge")
    if merge is None and c["form"] in ("dec", "mt", "tree") and (c["path"] == 2 or c["splits"] > 1):
        merge = 1
    if merge is not None:
        assert d["merge_launch"] == merge, what
    return what


def spy_issue(fn, *a, **kw):
    """fn(*a, **kw) of an fp8 / tree drop-in, and what its ONE launch was issued with: (result, parameter block, mask, scales, prefill selector)"""
    from vattention_amd import flash_attn as FA
    seen, real = [], FA._issue

    def spy(p, dev, lib, need=None, mask=None, scales=None, fp8_prefill=False):
        seen.append((p, mask, scales, fp8_prefill))
        return real(p, dev, lib, need, mask, scales, fp8_prefill)
    FA._issue = spy
    try:
        r = fn(*a, **kw)
    finally:
        FA._issue = real
    assert len(seen) == 1
    return (r,) + seen[0]


def launch_ext(c, q, k_fin, v_fin, dev, fill_k, fill_v, scales=None):
    """Run an fp8 / tree case through the real drop-in.  k_fin / v_fin: DEVICE caches [slots, rows, Hkv, D] AS AFTER the call (uint8 bytes of an
    fp8 case, the I/O dtype otherwise); the rows the call appends are cut out, handed to it as k / v (an fp8 case: dequantised with the
    case's scales) and hold fill_k / fill_v before the call.  The call runs over a strided [:, :rows] view of a larger allocation.  Asserts
    the plan the case names on the block the drop-in launched, that the host-only block (plan_block) describes the same plan, and that the
    cache after an appending call is the given one, every byte.  Returns (out [B, Sq, Hq, D], lse or None, plan description)."""
    from vattention_amd import flash_attn as FA
    fp8, form, dtype = bool(c.get("fp8")), c["form"], DT[c["dt"]]
    ql = case_qlens(c)
    B, Sq, rows = len(c["lens"]), max(ql), k_fin.shape[1]
    kb, vb, new, cl = cut_out_appended(c, k_fin, v_fin, fill_k, fill_v)
    views = []
    for t, fill in ((kb, fill_k), (vb, fill_v)):
        alloc = torch.full((t.shape[0], rows + 3) + tuple(t.shape[2:]), fill, dtype=t.dtype, device=dev)
        alloc[:, :rows] = t
        views.append((alloc.view(torch.float8_e4m3fn) if fp8 else alloc)[:, :rows])
    kv, vv = views
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    idx = i32(c["slots"]) if c["idx"] else None
    sc = ()
    if fp8:
        ks, vs = scales if scales is not None else case_scales(c)
        sc = (torch.as_tensor(ks, dtype=torch.float32).to(dev), torch.as_tensor(vs, dtype=torch.float32).to(dev))
        if new[0] is not None:
            new = (dequantize_bytes(new[0], sc[0], dtype), dequantize_bytes(new[1], sc[1], dtype))
    newkw = dict(k=new[0], v=new[1]) if new[0] is not None else {}
    qd = q.to(dev)
    lse = None
    if form == "tree":
        fn = FA.flash_attn_fp8kv_tree_with_kvcache if fp8 else FA.flash_attn_tree_with_kvcache
        (out, lse), p, mask, scl, pre = spy_issue(fn, qd, kv, vv, *sc, mask_tensor(c, dev), cache_seqlens=i32(cl), cache_batch_idx=idx, softmax_scale=c.get("scale"),
                                                  return_softmax_lse=True, _num_splits=c["splits"], **newkw)
        assert mask is not None and (scl is not None) == fp8
    elif form == "var":
        T = sum(ql)
        starts = [sum(ql[:i]) for i in range(B)]
        flat_q = torch.cat([qd[b, :ql[b]] for b in range(B)])
        flat = torch.full((T,) + tuple(qd.shape[2:]), 7.0, dtype=dtype, device=dev)
        _, p, mask, scl, pre = spy_issue(FA.flash_attn_fp8kv_varlen_with_kvcache, flat_q, kv, vv, *sc, i32(starts), i32(ql), Sq, i32(cl), idx, softmax_scale=c.get("scale"),
                                         causal=c["causal"], out=flat, _num_splits=c["splits"], _variant=c["variant"], _max_seqlen_k=max(c["lens"]))
        assert mask is None and scl is not None and pre is True
        out = torch.zeros(B, Sq, qd.shape[2], qd.shape[3], dtype=dtype, device=dev)
        for b in range(B):
            out[b, :ql[b]] = flat[starts[b]:starts[b] + ql[b]]
    else:
        fn = FA.flash_attn_fp8kv_prefill_with_kvcache if form == "pre" else FA.flash_attn_fp8kv_with_kvcache
        (out, lse), p, mask, scl, pre = spy_issue(fn, qd, kv, vv, *sc, cache_seqlens=i32(cl), cache_batch_idx=idx, softmax_scale=c.get("scale"), causal=c["causal"],
                                                  return_softmax_lse=True, _num_splits=c["splits"], _variant=c["variant"], **newkw)
        assert mask is None and scl is not None and pre is (form == "pre")
    torch.cuda.synchronize()
    d = describe_case(c, p)
    what = assert_plan_ext(c, d)
    dh = describe_case(c, plan_block(c, rows))
    assert all(dh[f] == d[f] for f in ("form", "path", "tiling", "merge_launch")), "%s: the host-only block describes %s" % (what, dh)
    if new[0] is not None:
        assert torch.equal(kv.view(torch.uint8) if fp8 else kv.view(torch.int16), k_fin.view(torch.uint8) if fp8 else k_fin.view(torch.int16)) and \
            torch.equal(vv.view(torch.uint8) if fp8 else vv.view(torch.int16), v_fin.view(torch.uint8) if fp8 else v_fin.view(torch.int16)), \
            what + ": the cache after the append, every row, bit for bit"
    return out, lse, d


# ---------------------------------------------------------------------------------------------------------------------------------------
# decoy keys of the FP8 / tree builds (tests/test_gpu_decoy_keys_fp8_tree.py): the construction of decoy_inputs, quantised for an fp8 cache
# with amax scales that are no powers of two, and for a tree row the decoys the MASK excludes
# ---------------------------------------------------------------------------------------------------------------------------------------
def tree_decoy_inputs(c, seed=0):
    """decoy_inputs for a tree case: c["needles"][b] = [(row t, kind)], kind ("bit", i): the i-th set draft bit of the row's word (modulo their
    number), "base-1", or a key position (clamped into the committed context).  Decoys 3 q_row at every draft key base + s whose bit is clear
    in the row's word, at base + sq (a real finite row behind the draft), at the needle's position under another kv head and in another slot.
    The two planted rows of an entry use kv heads hk, hk + 1 and their other-head decoys hk + 2, hk + 3: four kv heads, no shared cell."""
    g = torch.Generator().manual_seed(3000 + seed)
    dtype, D, Hkv, G, lens, sq = DT[c["dt"]], c["D"], c["Hkv"], c["G"], c["lens"], c["sq"]
    B, Hq = len(lens), Hkv * G
    rows = max(lens) + XSPARE
    q = torch.randn(B, sq, Hq, D, generator=g).to(dtype)
    kc = (0.1 * torch.randn(c["n_slots"], rows, Hkv, D, generator=g)).to(dtype)
    vc = torch.randn(c["n_slots"], rows, Hkv, D, generator=g).to(dtype)
    cells, plants = {}, []

    def plant(slot, j, hk, vec, who, unused_slot=False):
        key = (slot, j, hk)
        assert 0 <= j < rows
        assert unused_slot or key not in cells, "decoy construction: %s and %s share cache cell %s" % (cells[key], who, key)
        cells[key] = who
        kc[slot, j, hk] = vec.to(dtype)

    assert Hkv == 4
    other = next(s for s in range(c["n_slots"]) if s not in c["slots"])
    for b, spec in enumerate(c["needles"]):
        assert len(spec) <= 2
        for i, (t, kind) in enumerate(spec):
            ctx, singles = tree_visible(sq, lens[b], c["masks"][b][t])
            if ctx == 0 and not singles:
                continue
            base = lens[b] - sq
            if isinstance(kind, tuple):
                js = singles[kind[1] % len(singles)] if singles else ctx - 1
            elif kind == "base-1":
                js = ctx - 1 if ctx > 0 else singles[-1]
            else:
                js = min(int(kind), ctx - 1) if ctx > 0 else singles[0]
            hk = (2 * b + i) % 2 + 2 * (b % 2)          # (0, 1) for even entries, (2, 3) for odd ones
            h = hk * G + (t % G)
            qr = q[b, t, h].float()
            q[b, t, h] = (qr * (12 * D ** 0.5 / (qr * qr).sum()) ** 0.5).to(dtype)
            qr = q[b, t, h].float()
            slot = c["slots"][b]
            plant(slot, js, hk, 2 * qr, "needle(%d,%d)" % (b, t))
            plants.append((b, t, h, slot, hk, js))
            for s in range(sq):                           # the draft keys this row's word excludes
                if base + s >= 0 and base + s not in singles:
                    plant(slot, base + s, hk, 3 * qr, "decoy clear bit %d (%d,%d)" % (s, b, t))
            plant(slot, base + sq, hk, 3 * qr, "decoy base+sq(%d,%d)" % (b, t))
            plant(slot, js, (hk + 2) % Hkv, 3 * qr, "decoy kv head(%d,%d)" % (b, t))
            plant(other, js, hk, 3 * qr, "decoy slot(%d,%d)" % (b, t), unused_slot=True)
    return q, kc, vc, plants


def xdecoy_inputs(c, seed=0):
    """(q, kc, vc, scales, plants) of a decoy case of the FP8 / tree tables, caches AFTER the append.  An fp8 case: kc / vc are the
    float8_e4m3fn tensors quantised (tests/fp8kv_ref.py's quantiser) with amax scales — no powers of two — and `scales` = (k_scale, v_scale)
    float32 [Hkv]; a needle's value row is then the DEQUANTISED row.  A 2-byte case: scales is None."""
    from tests.fp8kv_ref import amax_scales, quantize_ref
    q, kc, vc, plants = tree_decoy_inputs(c, seed) if c["form"] == "tree" else decoy_inputs(c, seed)
    if not c.get("fp8"):
        return q, kc, vc, None, plants
    ks, vs = amax_scales(kc), amax_scales(vc)
    return q, quantize_ref(kc, ks), quantize_ref(vc, vs), (ks, vs), plants


def xdecoy_reference(c, q, kc, vc, scales, math="f64"):
    t = dict(c)
    if scales is not None:
        t["k_scale"], t["v_scale"] = scales[0].tolist(), scales[1].tolist()
    return xreference(t, q, kc, vc, math)


def xdecoy_cases():
    cs = []
    kinds = ["last", "first", "0", "31", "32", "63", "64", 95, 96, 159, 160]
    lens = [700, 33, 64, 65, 300, 161, 97, 1000, 450, 129, 200]
    for dt, D in (("f16", 128), ("bf16", 128), ("f16", 64)):
        tag = "%s_d%d" % (dt, D)
        nd1 = [[(0, kinds[b])] for b in range(len(lens))]
        for G, s, path in ((4, 0, 2), (4, 3, 0)):          # FP8 one-token: stream and grid
            cs.append(_xcase("decoy_fp8_dec_%s_g%d_s%d" % (tag, G, s), "dec", dt, D, 4, G, 1, lens, path, True, splits=s, idx=True, append=(s == 0), tiling=1, needles=nd1))
        for sq, G, s in ((4, 4, 0), (8, 4, -50), (8, 8, 0)):      # FP8 multi-token: R = 16, 32, 64
            R = sq * G
            path = 2 if (R <= 16 or (R <= 32 and s < 0)) else 0
            nd = [[(t, "last") for t in range(sq)] if b < 4 else [(b % sq, kinds[b])] for b in range(len(lens))]
            cs.append(_xcase("decoy_fp8_mt_%s_sq%d_g%d_s%d" % (tag, sq, G, s), "mt", dt, D, 4, G, sq, lens, path, True, splits=s, idx=True, append=True,
                             tiling=2 if R > 16 else 1, needles=nd))
        for variant, tiling in ((2, 1), (8, 4)):          # FP8 prefill tilings 1 and 4
            pl = [300, 364, 900]
            nd = [[(t, "last") for t in (0, 31, 63, 64, 127, 128, 255, 256, 299)] for b in range(len(pl))]
            cs.append(_xcase("decoy_fp8_pre_%s_t%d" % (tag, tiling), "pre", dt, D, 4, 2, 300, pl, 0, True, variant=variant, tiling=tiling, splits=1, idx=True, needles=nd))
        # tree, 2-byte and FP8: each set draft bit of the deepest node in turn (entries 0-3), base - 1, keys 0, 31 / 32, and 95 / 96, 159 / 160:
        # the last / first key of a piece of three / five tiles under the forced grids.  The draft rows of entry 2 (Lk = 93 + sq) straddle a tile edge.
        for fp8 in (False, True):
            for sq, G, s, kind in ((7, 4, 0, "tree7"), (7, 4, -50, "tree7"), (4, 4, 0, "rand")):
                R = sq * G
                path = decode_path(R, 11, s)
                tl = [700, sq, 93 + sq, 40 + sq, 300, 161, 97 + sq, 1000, 450, 129, 200]
                deep = sq - 1
                tk = [("bit", 0), ("bit", 1), ("bit", 2), ("bit", 3), "base-1", 0, 31, 32, 95, 96, 159]
                nd = [[(deep, tk[b]), ((deep + b) % (sq - 1), ("bit", b) if b & 1 else ["base-1", 160, 96][b % 3])] for b in range(len(tl))]
                cs.append(_xcase("decoy_tree_%s_%s_sq%d_g%d_%s_s%d" % ("fp8" if fp8 else "2b", tag, sq, G, kind, s), "tree", dt, D, 4, G, sq, tl, path, fp8, mask=kind,
                                 splits=s, idx=True, append=(s == 0), tiling=2 if R > 16 else 1, needles=nd))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def xinputs_key(c):
    """inputs_key for the FP8 / tree tables: also the cache kind and the mask words"""
    return inputs_key(c) + (bool(c.get("fp8")), str(c.get("masks")))


# what the two tables together must reach (tests/test_census_fp8_tree_model.py on the host-only blocks, tests/test_gpu_census_fp8_tree.py on the
# blocks the drop-ins launched): (form, cache kind, tree mask, path, tiling, merge launch)
XNEED = [("dec", "fp8", False, 0, 1, 1), ("dec", "fp8", False, 0, 2, 1), ("dec", "fp8", False, 2, 1, 1), ("dec", "fp8", False, 2, 2, 1),
         ("mt", "fp8", False, 0, 1, 1), ("mt", "fp8", False, 0, 2, 1), ("mt", "fp8", False, 2, 1, 1), ("mt", "fp8", False, 2, 2, 1),
         ("mt", "2b", True, 0, 1, 1), ("mt", "2b", True, 0, 2, 1), ("mt", "2b", True, 2, 1, 1), ("mt", "2b", True, 2, 2, 1),
         ("mt", "fp8", True, 0, 1, 1), ("mt", "fp8", True, 0, 2, 1), ("mt", "fp8", True, 2, 1, 1), ("mt", "fp8", True, 2, 2, 1),
         ("pre", "fp8", False, 0, 1, 0), ("pre", "fp8", False, 0, 1, 1), ("pre", "fp8", False, 0, 4, 0), ("pre", "fp8", False, 0, 4, 1),
         ("var", "fp8", False, 0, 1, 0), ("var", "fp8", False, 0, 4, 0)]


def plan_key(c, d):
    """(form, cache kind, tree, path, tiling, merge launch) of a case that ran with plan description d"""
    return ("mt" if c["form"] == "tree" else c["form"], "fp8" if c.get("fp8") else "2b", c["form"] == "tree", d["path"], d["tiling"], d["merge_launch"])
