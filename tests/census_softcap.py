"""Closed-form probes for the SOFTCAP builds of the decode and prefill kernels (logit soft-capping: scores = cap * tanh(q.k * softmax_scale / cap)),
beside tests/census.py, which it imports and leaves as it is.  Plain Python / numpy / torch, no GPU; shared by tests/test_census_softcap_model.py
(CPU: proves the models and the inputs) and tests/test_gpu_census_softcap.py.  Four parts:

1. ZERO-QUERY CENSUS UNDER A CAP.  q = 0 and the census one-hot V: every score is tanh(0), the same for all visible keys, so the output is
   tests/census.py `expected` unchanged and the LSE ln n (if tanh_exp2(0) were a tiny c instead of 0, only the LSE moved, by cap * c).  The tanh
   sits in front of every mask: a key masked BEFORE the tanh would come back with weight exp(-cap - score) — e^-1 at cap 1.0.

2. SIGNED (SATURATED) CENSUS.  q = 16 in every element, k[slot, j, hk, :] = sigma(slot, j, hk) * 16, sigma = +-1, census V, default scale,
   cap 64: q.k = +-256 D exactly, the tanh argument is +-32 (d 64) / +-45.3 (d 128) and the fp32 expression 1 - 2 / (1 + exp2(x2)) is exactly
   +-1 there (`tanh_exp2_f32`, asserted on the CPU).  A "-" key beside any "+" key weighs exp2(-2 * 64 * log2e) = 0 in fp32, a "+" key 1:
   a row with n+ >= 1 visible "+" keys gives count_d over the "+" keys / n+ and LSE 64 + ln n+; a row with visible keys but no "+" key the plain
   census over its n keys and LSE -64 + ln n; a row without a visible key 0 and +inf.  This ties K row j to V row j exactly.

3. SCALE TWIN.  (2 q, softmax_scale s, cap) and (q, 2 s, cap) must give the same bits: the scale may enter only through pre = softmax_scale /
   cap, behind the tanh the cap stands where the scale stood.  `tile_step_f32` is the CPU statement of why, and of what breaks it.

4. THE TANH READ OUT.  A row with exactly one visible key has LSE = cap * tanh(s * pre) and nothing else in it; q row = a e_i makes s = a k_i
   exact.  |lse - cap tanh64(x)| <= cap * 6e-7 + ulp_fp32(|lse|): 1.85e-7 for the expression in IEEE fp32 (roundings of s * k2 included), 2.4e-7 for
   a 1-ulp reciprocal, 6e-8 for a 1-ulp exp2, 0.45 * 2^-23 for the rounding of k2 — 5.4e-7, rounded up.
"""
import math
import random

import numpy as np
import torch

from tests import census as C
from tests.census import DT, case_qlens, visible_interval
from tests.softcap_ref import softcap_attn_ref

SPARE = 8                  # rows of the cache view behind the longest entry
LEN_CAP = 4095             # part 1: longer walks run the plain builds' planner and are covered there
ZERO_CAPS = (1.0, 50.0)    # part 1, alternating by case index
SWEEP_CAPS = (0.5, 1.0, 30.0, 50.0)
SIGNED_CAP = 64.0
SIGNED_Q = 16.0
TWIN_CAPS = (1.5, 50.0)
TANH_CAPS = (1.5, 30.0, 50.0)
TANH_FIXED = [s * x for x in (1e-3, 1e-2, 0.1, 0.5, 1, 2, 4, 8, 12, 20, 40) for s in (1, -1)]
TANH_BOUND = 6e-7          # x cap (+ one fp32 ulp of the LSE)
LOG2E_F32 = np.float32(1.4426950408889634)


def ulp32(x):
    """one fp32 ulp at the float64 magnitudes x (normal range)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.exp2(np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 23)


# ---------------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' expressions (csrc/attn_common.h tanh_exp2 / softcap_k2; the host's pre): IEEE roundings, exp2 and the
# reciprocal correctly rounded — what the hardware's 1-ulp units are measured against
# ---------------------------------------------------------------------------------------------------------------------------------------
def host_pre(scale, cap):
    """pre = softmax_scale / softcap as the host forms it: both fp32, IEEE fp32 division"""
    return np.float32(np.float32(scale) / np.float32(cap))


def cap_k2(pre):
    return np.float32(np.float32(pre) * np.float32(np.float32(2.0) * LOG2E_F32))


def tanh_exp2_f32(x2):
    """fma(-2, rcp(1 + exp2(x2)), 1) on fp32 x2 (the fma exact in float64: 2 r and 1 - 2 r need fewer than 53 bits)"""
    x2 = np.asarray(x2, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2(x2.astype(np.float64)).astype(np.float32)
        d = (np.float32(1.0) + e).astype(np.float32)
        r = (1.0 / d.astype(np.float64)).astype(np.float32)
    return (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)


def capped_lse_f32(s, scale, cap):
    """the LSE of a one-key row in fp32: cap * tanh_exp2(s * k2) (one more rounding)"""
    t = tanh_exp2_f32(np.asarray(s, dtype=np.float32) * cap_k2(host_pre(scale, cap)))
    return (t * np.float32(cap)).astype(np.float32)


def tile_step_f32(s, scale, cap, sc_from_scale=False):
    """one tile step of the capped online softmax on raw fp32 scores s [rows, keys]: (P fp32, LSE fp32) bit patterns.  sc_from_scale: the
    FAULT the scale twin is there to catch — sc and the LSE built from softmax_scale instead of the cap."""
    s = np.asarray(s, dtype=np.float32)
    t = tanh_exp2_f32(s * cap_k2(host_pre(scale, cap)))
    scl = np.float32(scale) if sc_from_scale else np.float32(cap)
    sc = np.float32(scl * LOG2E_F32)
    m = t.max(axis=-1, keepdims=True)
    with np.errstate(under="ignore"):
        arg = ((t.astype(np.float64) * sc).astype(np.float32) - (m * sc).astype(np.float32)).astype(np.float32)      # (no fma contraction assumed either way: both calls alike)
        p = np.exp2(arg.astype(np.float64)).astype(np.float32)
    l = p.sum(axis=-1, dtype=np.float32)
    lse = ((m[..., 0] * scl).astype(np.float32) + np.log(l.astype(np.float64)).astype(np.float32)).astype(np.float32)
    return p, lse


# ---------------------------------------------------------------------------------------------------------------------------------------
# part 1: the plain census table under a cap
# ---------------------------------------------------------------------------------------------------------------------------------------
def gate_admits(c):
    """what the softcap gate takes of tests/census.py's table: no host item plan, no prefill work list, no tiling 7 (variant 14)"""
    return not c.get("host_tiles") and not c.get("pf") and c.get("tiling") != 7 and c.get("variant") != 14


def with_cap(c, cap):
    """the case with every length above LEN_CAP replaced as tests/census.py `cut` does it, and its cap"""
    t = dict(c, cap=float(cap))
    t["lens"] = [x if x <= LEN_CAP else LEN_CAP - 37 * i for i, x in enumerate(c["lens"])]
    return t


def zero_cases():
    return [with_cap(c, ZERO_CAPS[i & 1]) for i, c in enumerate(c for c in C.gpu_cases() if gate_admits(c))]


def zero_sweep_case(seed):
    """draw `seed` of tests/census.py's sweep mapped through the same filter: a draw the gate refuses (tiling 7) is drawn again"""
    rng = random.Random(90_000 + seed)
    cap = rng.choice(SWEEP_CAPS)
    for i in range(64):
        c = C.sweep_case(seed + 1_000_003 * i)
        if gate_admits(c):
            return with_cap(dict(c, name="capsweep%d" % seed), cap)
    raise AssertionError("no admitted draw for seed %d" % seed)


# ---------------------------------------------------------------------------------------------------------------------------------------
# part 2: the signed census
# ---------------------------------------------------------------------------------------------------------------------------------------
SIGNS = ("default", "lo", "hi-1", "lo-1", "hi", "neighbour")


def _xcase(name, form, dt, D, Hkv, G, sq, lens, path, **kw):
    c = C._case(name, form, dt, D, Hkv, G, sq, lens, path, **kw)
    if not c["idx"]:
        c["n_slots"] = len(c["lens"]) + 1          # one slot no entry uses (the "neighbour" signs, and a wrong slot is then a wrong answer)
    c["cap"] = SIGNED_CAP
    return c


def target_rows(n):
    """the query rows of an n-row entry whose edges get a sign of their own: first, last, middle, and the rows on either side of a 64-row block"""
    return sorted({0, n - 1, n // 2, 63, 64} & set(range(n)))


def sign_modes(c):
    """the named sign entries that mean something for case c"""
    ms = ["default", "lo", "hi-1", "neighbour"]
    rows = max(c["lens"]) + SPARE
    if c.get("left") is not None and plus_cells(c, "lo-1", rows).any():      # (not under a window wider than every entry: lo is 0)
        ms.append("lo-1")
    if c["causal"] and max(case_qlens(c)) > 1 and plus_cells(c, "hi", rows).any():
        ms.append("hi")
    return ms


def plus_cells(c, mode, rows):
    """bool [n_slots, rows, Hkv]: where sigma = +1.  "default": (j + 3 hk + slot) % 3 == 0.  The named entries are all "-" except, for every
    target row of every entry: "lo" its first visible key, "hi-1" its last, "lo-1" / "hi" the key just outside (never a row at or behind Lk:
    those stay poisoned), "neighbour" its last visible key under kv head 1 only (kv head 0 must not see it) and under every head of a slot no
    entry uses."""
    n_slots, Hkv = c["n_slots"], c["Hkv"]
    if mode == "default":
        j = np.arange(rows).reshape(1, rows, 1)
        return (j + 3 * np.arange(Hkv).reshape(1, 1, Hkv) + np.arange(n_slots).reshape(n_slots, 1, 1)) % 3 == 0
    plus = np.zeros((n_slots, rows, Hkv), dtype=bool)
    unused = next(s for s in range(n_slots) if s not in c["slots"])
    ql = case_qlens(c)
    for b, Lk in enumerate(c["lens"]):
        for t in target_rows(ql[b]):
            lo, hi = visible_interval(ql[b], Lk, t, c["causal"], c.get("left"))
            if hi <= lo:
                continue
            j = {"lo": lo, "hi-1": hi - 1, "lo-1": lo - 1, "hi": hi, "neighbour": hi - 1}[mode]
            if not 0 <= j < Lk:
                continue
            if mode == "neighbour":
                plus[unused, j, :] = True
                if Hkv > 1:
                    plus[c["slots"][b], j, 1] = True
            else:
                plus[c["slots"][b], j, :] = True
    return plus


def signed_expected(c, plus):
    """(exp float64 [B, Sq, Hq, D], n int64 [B, Sq, Hq] keys that count (-1: no such row), lse float64 [B, Sq, Hq])"""
    D, Hkv, G, cap = c["D"], c["Hkv"], c["G"], c["cap"]
    lens, ql = c["lens"], case_qlens(c)
    B, Sq = len(lens), max(ql)
    exp = np.zeros((B, Sq, Hkv * G, D))
    n = np.full((B, Sq, Hkv * G), -1, dtype=np.int64)
    lse = np.full((B, Sq, Hkv * G), np.inf)
    for b in range(B):
        slot = c["slots"][b]
        for t in range(ql[b]):
            lo, hi = visible_interval(ql[b], lens[b], t, c["causal"], c.get("left"))
            for hk in range(Hkv):
                sl = slice(hk * G, (hk + 1) * G)
                if hi <= lo:
                    n[b, t, sl] = 0
                    continue
                keys = np.arange(lo, hi)
                sel = plus[slot, lo:hi, hk]
                sign = 1.0 if sel.any() else -1.0
                if sel.any():
                    keys = keys[sel]
                m = len(keys)
                n[b, t, sl] = m
                exp[b, t, sl] = np.bincount((keys + 17 * hk + 5 * slot) % D, minlength=D) / float(m)
                lse[b, t, sl] = sign * cap + math.log(m)
    return exp, n, lse


def signed_lse_tol(c, n):
    """0.25 / n + 2 ulp_fp32(cap + ln n): one fp32 ulp at 64 is 7.6e-6, no longer small against 0.25 / n at n in the thousands"""
    n = np.maximum(n, 1).astype(np.float64)
    return 0.25 / n + 2 * ulp32(c["cap"] + np.log(n))


def compare_closed(out, lse, c, exp, n, lse_exp, lse_tol):
    """tests/census.py `compare` against a GIVEN closed form: out [B, Sq, Hq, D], lse [B, Hq, Sq] or None.  Returns (failures, stats); a
    failure names entry, row, head and element.  stats: max_ulp, lse_worst_times_n (|lse - expected| * n)."""
    got = out.double().numpy()
    live = n >= 0
    fails = []
    err = np.abs(got - exp)
    u = C.ulp(exp, c["dt"])
    zero_bad = (exp == 0) & (got != 0) & live[..., None]
    bad = (~(err <= u) & (exp > 0)) | zero_bad | (~np.isfinite(got) & live[..., None])
    ulps = np.where(np.isfinite(got), err / u, np.inf)[exp > 0]
    stats = {"max_ulp": float(ulps.max()) if ulps.size else 0.0, "lse_worst_times_n": 0.0}
    if not np.isfinite(got[live]).all():
        fails.append("%d output elements are not finite (a read of the poisoned rows behind the visible keys?)" % (~np.isfinite(got[live])).sum())
    if bad.any():
        ql = case_qlens(c)
        where = np.argwhere(bad)
        rank = np.where(np.isfinite(got) & ~zero_bad, err / u, np.inf)[bad]
        for b, t, h, d in where[np.argsort(-rank, kind="stable")[:6]]:
            lo, hi = visible_interval(ql[b], c["lens"][b], t, c["causal"], c.get("left"))
            hk, slot = h // c["G"], c["slots"][b]
            fails.append("entry %d row %d head %d (kv head %d, slot %d) element %d: got %.9g, expected %d/%d = %.9g (%.2f ulp); keys [%d, %d), this residue = keys %d + %d i"
                         % (b, t, h, hk, slot, d, got[b, t, h, d], round(exp[b, t, h, d] * max(n[b, t, h], 1)), n[b, t, h], exp[b, t, h, d], err[b, t, h, d] / u[b, t, h, d],
                            lo, hi, (d - 17 * hk - 5 * slot) % c["D"], c["D"]))
    if lse is not None:
        l = lse.double().numpy().transpose(0, 2, 1)
        dead = n == 0
        if not np.array_equal(np.isposinf(l) & live, dead):
            fails.append("LSE: rows without a visible key must be +inf, and only those (%d dead rows, %d +inf)" % (dead.sum(), (np.isposinf(l) & live).sum()))
        ok = n > 0
        if ok.any():
            with np.errstate(invalid="ignore"):
                e = np.abs(l - np.where(ok, lse_exp, 0.0))
            e = np.where(np.isfinite(e), e, np.inf)
            stats["lse_worst_times_n"] = float((e[ok] * n[ok]).max())
            over = ok & ~(e <= lse_tol)
            if over.any():
                b, t, h = np.argwhere(over)[int(np.argmax((e / lse_tol)[over]))]
                fails.append("LSE: entry %d row %d head %d: got %.9g, expected %.9g (n = %d): off by %.3e > %.3e"
                             % (b, t, h, l[b, t, h], lse_exp[b, t, h], n[b, t, h], e[b, t, h], lse_tol[b, t, h]))
    return fails, stats


def signed_compare(out, lse, c, plus):
    exp, n, lse_exp = signed_expected(c, plus)
    return compare_closed(out, lse, c, exp, n, lse_exp, signed_lse_tol(c, n))


def signed_n(c, plus):
    """the keys that count per (entry, row, kv head) — n+ of a row with "+" keys, n of a row without — by cumulative sums: int64 list"""
    ql, out = case_qlens(c), []
    for b, Lk in enumerate(c["lens"]):
        cs = np.concatenate([np.zeros((1, c["Hkv"]), dtype=np.int64), np.cumsum(plus[c["slots"][b]], axis=0)])
        for t in range(ql[b]):
            lo, hi = visible_interval(ql[b], Lk, t, c["causal"], c.get("left"))
            npl = cs[hi] - cs[lo]
            out.append(np.where(npl > 0, npl, hi - lo))
    return np.asarray(out)


def signed_admissible(c, plus):
    """tests/census.py's rule on the keys that count, for every row of the case"""
    return int(signed_n(c, plus).max()) <= C.MAX_KEYS_PER_RESIDUE[c["dt"]] * c["D"]


def emulate_row(keys, c, cap, score, out_dtype=None):
    """What a kernel that walks the key LIST `keys` of one row returns — the CPU emulation the sensitivity tests inject faults into.  keys:
    (slot, j, kv head) triples, repeats allowed; score(slot, j, hk) the capped score cap * tanh(.) of that cell, -inf for none.  Returns
    (out float64 [D] rounded to the I/O dtype, lse)."""
    sc = np.asarray([score(*k) for k in keys], dtype=np.float64)
    if not len(keys) or not np.isfinite(sc).any():
        return np.zeros(c["D"]), np.inf
    m = sc.max()
    w = np.exp(sc - m).astype(np.float32).astype(np.float64)          # (exp(-128) is 0 in fp32, as in the kernels)
    o = np.zeros(c["D"])
    for (slot, j, hk), wk in zip(keys, w):
        o[C.residue(j, hk, slot, c["D"])] += wk
    o = torch.tensor(o / w.sum()).to(DT[c["dt"]] if out_dtype is None else out_dtype).double().numpy()
    return o, m + math.log(w.sum())


def signed_inputs(c, plus, rows, device="cpu", q_value=SIGNED_Q):
    """q = 16 everywhere, k = +-16 by `plus`, census V; the caches as AFTER the call, nothing poisoned yet"""
    dtype = DT[c["dt"]]
    B, Sq, Hq, D = len(c["lens"]), max(case_qlens(c)), c["Hkv"] * c["G"], c["D"]
    q = torch.full((B, Sq, Hq, D), q_value, dtype=dtype, device=device)
    sgn = torch.from_numpy(np.where(plus, SIGNED_Q, -SIGNED_Q)).to(device=device, dtype=dtype)
    k = sgn.unsqueeze(-1).expand(c["n_slots"], rows, c["Hkv"], D).contiguous()
    return q, k, C.census_values(c["n_slots"], rows, c["Hkv"], D, dtype, device=device)


DEC_LENS = [1, 2, 31, 32, 33, 64, 65, 97, 300, 1033]
PRE_A, PRE_B = [130 + x for x in (0, 1, 63, 64, 200)], [90, 149]
VAR_Q, VAR_L = [130, 1, 70, 37], [130, 701, 270, 1037]


def _mt_path(R, s):
    return 2 if (R <= 16 or (R <= 32 and s < 0)) else 0


def _family(dts=("f16", "bf16"), Ds=(64, 128), short=False):
    """the plans of the issue's table, one _xcase per (plan, mask): the signed census runs all of it, the scale twin (short: lengths <= 300)
    one per build family"""
    cs = []
    flip = 0
    for dt in dts:
        for D in Ds:
            tag = "%s_d%d" % (dt, D)
            dl = [x for x in DEC_LENS if x <= 300] if short else DEC_LENS
            for G in (4, 17):
                for s in ((0, 3) if short and G == 4 else (0, -3) if short else (0, -3, -37, 3)):
                    for left in ((None, 31) if short else (None, 0, 31, 32, 100)):
                        flip += 1
                        path = C.decode_path(G, len(dl), s)
                        cs.append(_xcase("dec_%s_g%d_s%d_%s" % (tag, G, s, "full" if left is None else "win%d" % left), "dec", dt, D, 2, G, 1, dl, path, splits=s, left=left,
                                         tiling=2 if G > 16 else 1, merge=1 if (path == 2 or s > 1) else None, append=bool(flip & 1), idx=bool(flip & 2)))
            for sq, G in ((4, 4), (8, 4), (8, 8)):
                R = sq * G
                ml = [sq - 1, sq, 33, 64 + sq - 1, 127, 300 if short else 1025]
                for s in ((0 if R != 32 else -400,) if short else (0, -400)):
                    for causal, left in (((True, None), (True, 32)) if short else ((True, None), (False, None), (True, 0), (True, 32), (True, 100))):
                        flip += 1
                        path = _mt_path(R, s)
                        cs.append(_xcase("mt_%s_sq%d_g%d_s%d_%s" % (tag, sq, G, s, ("causal" if causal else "full") if left is None else "win%d" % left), "mt", dt, D,
                                         1 if R > 32 else 2, G, sq, ml, path, splits=s, causal=causal, left=left, tiling=2 if R > 16 else 1, merge=1 if path == 2 else None,
                                         append=bool(flip & 1), idx=bool(flip & 2)))
            # one sequence has nothing to balance: the uniform grid split with ONE 16-column block per workgroup (path 0, tiling 1)
            for left in (None, 100):
                cs.append(_xcase("mt_one_sequence_%s_%s" % (tag, "causal" if left is None else "win%d" % left), "mt", dt, D, 2, 4, 4, [300 if short else 1025], 0, left=left,
                                 tiling=1, merge=None, append=left is None))
            for variant, tiling in ((2, 1), (8, 4)):
                vt = "%s_t%d" % (tag, tiling)
                for s in (1, 3):
                    masks = ((True, None), (True, 64)) if short else ((True, None), (False, None), (True, 0), (True, 63), (True, 64), (True, 65), (True, 236))
                    for causal, left in masks:
                        m = ("causal" if causal else "full") if left is None else "win%d" % left
                        flip += 1
                        pa = [130 + x for x in (0, 1, 63, 64, 170)] if short else PRE_A
                        cs.append(_xcase("pre_%s_s%d_%s" % (vt, s, m), "pre", dt, D, 2, 4, 130, pa, 0, variant=variant, tiling=tiling, merge=1 if s > 1 else 0, splits=s, causal=causal,
                                         left=left, append=bool(flip & 1) and not short, idx=bool(flip & 2)))
                        if not short:
                            cs.append(_xcase("pre_sq_gt_lk_%s_s%d_%s" % (vt, s, m), "pre", dt, D, 2, 4, 150, PRE_B, 0, variant=variant, tiling=tiling, merge=1 if s > 1 else 0,
                                             splits=s, causal=causal, left=left, idx=not bool(flip & 2)))
                for left in (None, 64):
                    cs.append(_xcase("var_%s_%s" % (vt, "full" if left is None else "win%d" % left), "var", dt, D, 2, 4, max(VAR_Q), [130, 300, 270, 237] if short else VAR_L, 0,
                                     qlens=VAR_Q, variant=variant, tiling=tiling, merge=0, splits=1, left=left, idx=True))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def signed_cases():
    return _family()


def twin_cases():
    return _family(short=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# part 3: the scale twin
# ---------------------------------------------------------------------------------------------------------------------------------------
def twin_scale(D):
    return 0.7 * D ** -0.5


def twin_inputs(c, rows, seed=0):
    """(q_A = 2 q_B, q_B = 2 randn in the I/O dtype, k, v = randn), CPU; caches as AFTER the call"""
    g = torch.Generator().manual_seed(3000 + seed + c["D"] + 7 * c["G"] + c["sq"])
    dtype = DT[c["dt"]]
    B, Sq, Hq, D = len(c["lens"]), max(case_qlens(c)), c["Hkv"] * c["G"], c["D"]
    qb = (2 * torch.randn(B, Sq, Hq, D, generator=g)).to(dtype)
    qa = (qb.float() * 2).to(dtype)
    assert bool(torch.isfinite(qa).all()) and torch.equal(qa.float(), qb.float() * 2)
    k = torch.randn(c["n_slots"], rows, c["Hkv"], D, generator=g).to(dtype)
    v = torch.randn(c["n_slots"], rows, c["Hkv"], D, generator=g).to(dtype)
    return qa, qb, k, v


def capped_reference(c, q, kc, vc, cap, scale=None, math="f64"):
    """tests/softcap_ref.py on the CPU tensors of case c (caches AFTER the append): (out [B, Sq, Hq, D], lse [B, Hq, Sq])"""
    return softcap_attn_ref(q, kc, vc, cap, left=c.get("left"), causal=c["causal"] or max(case_qlens(c)) == 1, cache_seqlens=c["lens"],
                            cache_batch_idx=torch.tensor(c["slots"]), softmax_scale=scale, math=math, return_lse=True, q_lens=c.get("qlens"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# part 4: the tanh read out through rows with exactly one visible key
# ---------------------------------------------------------------------------------------------------------------------------------------
def tanh_targets():
    """the 22 fixed arguments and 400 seeded ones in [-12, 12]"""
    rng = random.Random(4242)
    return TANH_FIXED + [rng.uniform(-12.0, 12.0) for _ in range(400)]


def tanh_cases():
    """the configurations whose sample rows see ONE key.  `sample`: "all" every row of the call, "row0" row 0 of every entry"""
    cs = []
    for dt in ("f16", "bf16"):
        for D in (64, 128):
            tag = "%s_d%d" % (dt, D)
            for G, s in ((4, 0), (4, 3), (17, 0), (17, -3)):
                path = C.decode_path(G, 13, s)
                kw = dict(splits=s, tiling=2 if G > 16 else 1, merge=1 if (path == 2 or s > 1) else None, sample="all")
                B = 13 if G == 17 else 53
                cs.append(_xcase("tanh_dec_lk1_%s_g%d_s%d" % (tag, G, s), "dec", dt, D, 2, G, 1, [1] * B, path, idx=True, **kw))
                cs.append(_xcase("tanh_dec_win0_%s_g%d_s%d" % (tag, G, s), "dec", dt, D, 2, G, 1, [33, 300] * (B // 2 + 1), path, left=0, append=True, **kw))
            for sq, G, s in ((4, 4, 0), (8, 4, -400), (8, 8, 0)):
                R = sq * G
                path = _mt_path(R, s)
                cs.append(_xcase("tanh_mt_win0_%s_sq%d_g%d" % (tag, sq, G), "mt", dt, D, 1 if R > 32 else 2, G, sq, [sq, 33, 64 + sq - 1, 300] * 4, path, splits=s, left=0,
                                 tiling=2 if R > 16 else 1, merge=1 if path == 2 else None, append=True, sample="all"))
            for variant, tiling in ((2, 1), (8, 4)):
                vt = "%s_t%d" % (tag, tiling)
                cs.append(_xcase("tanh_pre_win0_%s" % vt, "pre", dt, D, 2, 4, 130, [130, 194], 0, variant=variant, tiling=tiling, merge=0, splits=1, left=0, sample="all"))
                cs.append(_xcase("tanh_var_win0_%s" % vt, "var", dt, D, 2, 4, max(VAR_Q), [130, 300, 270, 237], 0, qlens=VAR_Q, variant=variant, tiling=tiling, merge=0, splits=1,
                                 left=0, idx=True, sample="all"))
                cs.append(_xcase("tanh_pre_row0_%s" % vt, "pre", dt, D, 2, 4, 130, [130] * 8, 0, variant=variant, tiling=tiling, merge=0, splits=1, sample="row0"))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def tanh_inputs(c, cap, rows, seed=0):
    """CPU tensors of a read-out case: q [B, Sq, Hq, D] with row (b, t, h) = a e_g (g = h % G), k / v = randn (caches AFTER the call) with
    k[slot, j(b, t), hk, g] set so that a * k is the sample's score, and `samples`: arrays b, t, h, slot, hk, j, x — x the tanh argument in
    float64 computed from the STORED values with pre formed in fp32 as the host does."""
    g_ = torch.Generator().manual_seed(5000 + seed + c["D"] + c["G"])
    dtype, D, Hkv, G = DT[c["dt"]], c["D"], c["Hkv"], c["G"]
    ql, lens = case_qlens(c), c["lens"]
    B, Sq, Hq = len(lens), max(ql), Hkv * G
    q = torch.zeros(B, Sq, Hq, D, dtype=dtype)
    k = torch.randn(c["n_slots"], rows, Hkv, D, generator=g_).to(dtype)
    v = torch.randn(c["n_slots"], rows, Hkv, D, generator=g_).to(dtype)
    targets = np.asarray(tanh_targets())
    pre = float(host_pre(D ** -0.5, cap))
    cells = []
    for b in range(B):
        for t in range(ql[b] if c["sample"] == "all" else 1):
            lo, hi = visible_interval(ql[b], lens[b], t, c["causal"], c.get("left"))
            assert hi - lo == 1, (c["name"], b, t, lo, hi)
            cells += [(b, t, h, c["slots"][b], h // G, lo) for h in range(Hq)]
    S = dict(zip(("b", "t", "h", "slot", "hk", "j"), np.asarray(cells).T))
    first = (seed * 101 + len(c["name"]) * 37) % len(targets)
    s = targets[(first + np.arange(len(cells))) % len(targets)] / pre
    a = np.exp2(np.round(0.5 * np.log2(np.abs(s))))                      # a power of two: exact in either dtype
    kv = torch.from_numpy(s / a).to(dtype)
    gi = torch.from_numpy(S["h"] % G)
    # (the heads of a group share the key row: element g of it is theirs alone; every sample row (b, t) has a key row of its own)
    ix = lambda n: torch.from_numpy(S[n])
    q[ix("b"), ix("t"), ix("h"), gi] = torch.from_numpy(a).to(dtype)
    k[ix("slot"), ix("j"), ix("hk"), gi] = kv
    S["s"] = a * kv.double().numpy()                                     # exact: the product of two stored values
    S["x"] = S["s"] * pre
    assert np.array_equal(q[ix("b"), ix("t"), ix("h"), gi].double().numpy(), a)
    if c["sample"] == "row0":      # the other rows of the call run unchecked: give them a query too
        q[:, 1:] = torch.randn(B, Sq - 1, Hq, D, generator=g_).to(dtype)
    return q, k, v, S


def tanh_check(out, lse, c, cap, v, S):
    """the two assertions of part 4 on CPU tensors out [B, Sq, Hq, D], lse [B, Hq, Sq].  Returns (failures, worst |err| / cap)."""
    b, t, h = S["b"], S["t"], S["h"]
    got = lse.double().numpy()[b, h, t]
    want = cap * np.tanh(S["x"])
    err = np.abs(got - want)
    tol = cap * TANH_BOUND + ulp32(got)
    fails = []
    for i in np.argwhere(~(err <= tol))[:4, 0]:
        fails.append("entry %d row %d head %d: x = %.9g, lse %.9g, cap tanh(x) = %.9g: |err| / cap = %.3e > %.1e (+ ulp %.2e)"
                     % (b[i], t[i], h[i], S["x"][i], got[i], want[i], err[i] / cap, TANH_BOUND, ulp32(got[i]) / cap))
    o = out.double().numpy()[b, t, h]
    vrow = v.double().numpy()[S["slot"], S["j"], S["hk"]]
    u = C.ulp(np.maximum(np.abs(vrow), 1e-30), c["dt"])
    badrow = ~(np.abs(o - vrow) <= u).all(axis=-1)
    for i in np.argwhere(badrow)[:4, 0]:
        fails.append("entry %d row %d head %d: the output is not value row %d of slot %d, kv head %d (max %.2f ulp)"
                     % (b[i], t[i], h[i], S["j"][i], S["slot"][i], S["hk"][i], (np.abs(o[i] - vrow[i]) / u[i]).max()))
    return fails, float(np.where(np.isfinite(err), err, np.inf).max() / cap)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launcher
# ---------------------------------------------------------------------------------------------------------------------------------------
def plan_block(c, rows):
    """the parameter block of case c as far as vattn_softcap_attn_plan_describe reads it: host-only, nothing is dereferenced"""
    from vattention_amd import kernels as K
    lens = c["lens"]
    p = K.AttnParams()
    sn = (1 if c["form"] == "dec" else c["sq"]) if c["append"] else 0
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = len(lens), max(case_qlens(c)), rows, sn, c["Hkv"] * c["G"], c["Hkv"], c["D"]
    left = c.get("left")
    p.window_left_plus1 = left + 1 if left is not None and left < rows else 0
    p.is_causal = int(c["causal"] or p.window_left_plus1 > 0)
    p.dtype, p.num_splits, p.variant, p.softmax_scale = (0 if c["dt"] == "f16" else 1), c["splits"], c["variant"], c["D"] ** -0.5
    p.cache_seqlens = 4096
    if c["idx"]:
        p.cache_batch_idx = 4096
    if c["form"] == "var":
        p.q_lens = p.q_start = 4096
        p.max_seqlen_k_hint = min(max(lens), rows)
    return p


def describe_host(c, rows=None):
    from vattention_amd import kernels as K
    rows = rows or max(c["lens"]) + SPARE
    p = plan_block(c, rows)
    d = K.describe_softcap(p, c["cap"])
    C.assert_plan(c, p, d, rows)
    return d


def plan_key(c, d):
    return (c["form"], d["path"], d["tiling"], d["merge_launch"], c.get("left") is not None)


# what the tables must reach (merge launch None: either — the grid heuristics decide it for the decode forms)
NEED = ([(f, path, tiling, None, w) for f in ("dec", "mt") for path in (0, 2) for tiling in (1, 2) for w in (False, True)]
        + [("pre", 0, tiling, m, w) for tiling in (1, 4) for m in (0, 1) for w in (False, True)] + [("var", 0, tiling, 0, w) for tiling in (1, 4) for w in (False, True)])


def missing_plans(reached):
    return [k for k in NEED if not any(r[:3] == k[:3] and r[4] == k[4] and k[3] in (None, r[3]) for r in reached)]


def poison(c, k_fin, v_fin):
    """rows at or behind Lk of every slot an entry uses: NaN (K) and Inf (V), in place"""
    for b, Lk in enumerate(c["lens"]):
        k_fin[c["slots"][b], Lk:], v_fin[c["slots"][b], Lk:] = float("nan"), float("inf")


def launch(c, q, k_fin, v_fin, dev, scale=None):
    """Run case c under its cap through the real drop-in (flash_attn_with_kvcache / flash_attn_varlen_with_kvcache, softcap=c["cap"]).  q
    [B, Sq, Hq, D]; k_fin / v_fin: DEVICE caches [slots, rows, Hkv, D] AS AFTER the call, poisoned behind Lk; the rows the call appends are cut
    out, handed to it as k / v and hold NaN / Inf before it.  Asserts, on the ONE block the drop-in launched, the cap, and through
    kernels.describe_softcap the form, path, tiling, merge launch and window field the case names; that a host-only block describes the same
    plan; and after an appending call the whole cache, bit for bit.  The batched entry returns no LSE: the very block it launched is issued
    once more through the C ABI with an LSE buffer (rows an entry does not have stay +inf) and must give the same output.
    Returns (out [B, Sq, Hq, D], lse [B, Hq, Sq], plan description)."""
    import ctypes
    from vattention_amd import flash_attn as FA
    from vattention_amd import kernels as K
    dtype, cap = DT[c["dt"]], c["cap"]
    ql = case_qlens(c)
    B, Sq, rows = len(c["lens"]), max(ql), k_fin.shape[1]
    kc, vc, new, cl = C.cut_out_appended(c, k_fin, v_fin, float("nan"), float("inf"))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    idx = i32(c["slots"]) if c["idx"] else None
    win = (c["left"], 0) if c.get("left") is not None else (-1, -1)
    qd = q.to(dev)
    Hq, D = qd.shape[2], qd.shape[3]
    if c["form"] == "var":
        starts = [sum(ql[:i]) for i in range(B)]
        flat_q = torch.cat([qd[b, :ql[b]] for b in range(B)])
        flat = torch.full_like(flat_q, 7.0)
        index = (i32(starts), i32(ql), i32(cl))          # held to the end: the block is issued twice and points into them
        _, p = C.spy_call(FA.flash_attn_varlen_with_kvcache, flat_q, kc, vc, index[0], index[1], Sq, index[2], idx, softmax_scale=scale, causal=c["causal"], out=flat,
                          num_splits=c["splits"], _variant=c["variant"], _max_seqlen_k=max(c["lens"]), window_size=win, softcap=cap)
        lse = torch.full((B, Hq, Sq), float("inf"), dtype=torch.float32, device=dev)
        again = torch.full_like(flat, 9.0)
        p.softmax_lse, p.out = lse.data_ptr(), again.data_ptr()
        assert K.klib().vattn_softcap_attn_with_kvcache(ctypes.byref(p), cap, K.current_stream_ptr(qd.device)) == 0, K.last_error()
        torch.cuda.synchronize()
        assert torch.equal(flat.view(torch.int16), again.view(torch.int16)), c["name"] + ": the same block with an LSE buffer gives another output"
        del index
        out = torch.zeros(B, Sq, Hq, D, dtype=dtype, device=dev)
        for b in range(B):
            out[b, :ql[b]] = flat[starts[b]:starts[b] + ql[b]]
    else:
        (out, lse), p = C.spy_call(FA.flash_attn_with_kvcache, qd, kc, vc, *new, cache_seqlens=i32(cl), cache_batch_idx=idx, softmax_scale=scale, causal=c["causal"],
                                  window_size=win, num_splits=c["splits"], return_softmax_lse=True, _variant=c["variant"], softcap=cap)
    torch.cuda.synchronize()
    assert p._softcap == cap
    d = K.describe_softcap(p, cap)
    what = C.assert_plan(c, p, d, rows)
    dh = K.describe_softcap(plan_block(c, rows), cap)
    assert all(dh[f] == d[f] for f in ("form", "path", "tiling", "merge_launch")), "%s: the host-only block describes %s" % (what, dh)
    if new[0] is not None:
        assert torch.equal(kc.view(torch.int16), k_fin.view(torch.int16)) and torch.equal(vc.view(torch.int16), v_fin.view(torch.int16)), \
            what + ": the cache after the append, every row, bit for bit"
    return out, lse, d
