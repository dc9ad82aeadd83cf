"""The far-address census on the GPU (tests/far_address.py; the CPU proof is tests/test_far_address_model.py): every attention build and launch plan
over cache views whose K/V byte offsets lie beyond 2, 4 and 8 GiB of one 8.5-GiB buffer each for K and V — far slots through cache_batch_idx, far
rows of one sequence at a row pitch of 8 MiB + 4 KiB (the marks inside a tile), and windowed builds deep in a 65 536- / 131 072-row view at the
production pitch.  The census's own bounds, no new tolerance: |out - count_d / n| <= 1 ulp of the output dtype, |lse - ln n| n < 0.25, dead rows 0 and
+inf; rows behind Lk hold the fill (K 0.5, V 3.0) and must leave no trace; a value row read from a wrapped address is fill and moves an element by
3 / n; a key row read from one is fill too and, against the query (64, 0, 0, ...), weighs e^score >= 2 where every payload key weighs exactly 1 (seen
in the output where a row sees keys on both sides of the wrap, in the LSE where all of its keys wrap; the batched-chunk entry returns no LSE).  Every case asserts the plan it names on the block its drop-in launched, through the describe entry of that call; after every call that
writes, the written rows are compared bit for bit, the fill is put back and BOTH whole buffers are compared with the fill.

The writers (cache_flat vector and 2-byte element path, cache_flat_rope, cache_flat_fp8, keep_rows, keep_rows_fp8) are checked bit for bit at far
rows and in far slots in the same way.  The buffers are allocated once per module and released at its end.

Measured on one MI355X (whole file): see README.md, "Tests"."""
import time

import pytest
import torch

from tests import census as C
from tests import census_fp8_tree as X
from tests import far_address as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = F.cases()
REACHED = {}
WORST = {"max_ulp": 0.0, "lse_worst_times_n": 0.0, "lse_case": "", "seconds": 0.0, "t0": None}


@pytest.fixture(scope="module")
def bufs():
    WORST["t0"] = time.time()
    b = F.Buffers(DEV)
    yield b
    del b.k, b.v
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_far_address_census(case, bufs):
    c = case
    t0 = time.time()
    out, lse, key, d = F.run(c, bufs)
    REACHED[key] = REACHED.get(key, 0) + 1
    fails, stats = F.compare(out, lse, c)
    WORST["max_ulp"] = max(WORST["max_ulp"], stats["max_ulp"])
    if stats["lse_worst_times_n"] > WORST["lse_worst_times_n"]:
        WORST["lse_worst_times_n"], WORST["lse_case"] = stats["lse_worst_times_n"], c["name"]
    WORST["seconds"] = max(WORST["seconds"], time.time() - t0)
    g = F.geometry(c)
    assert not fails and stats["max_ulp"] <= 1.0, "%s: plan %s, byte strides batch %d row %d, view at %d\n  %s" % (c["name"], d, g["bs"], g["rs"], g["base"], "\n  ".join(fails))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the writers, bit for bit at far rows and in far slots
# ---------------------------------------------------------------------------------------------------------------------------------------
WRITERS = [(w, geo, dt) for w in ("flat_vec", "flat_elem", "flat_rope", "flat_fp8", "keep_rows", "keep_rows_fp8") for geo in ("row", "slot") for dt in ("f16", "bf16")]


def _writer_case(w, geo, dt):
    fp8 = w.endswith("fp8")
    lens = [1061] if geo == "row" else [1034, 33, 1033, 97, 1032]
    return F._place(X._xcase("w", "dec", dt, 128, 2, 4, 1, lens, 0, fp8), geo, ())


@pytest.mark.parametrize("w,geo,dt", WRITERS, ids=["%s_%s_%s" % t for t in WRITERS])
def test_far_address_writers(w, geo, dt, bufs):
    from vattention_amd import cache_ops as O
    c = _writer_case(w, geo, dt)
    fp8, dtype, D, Hkv = bool(c.get("fp8")), C.DT[dt], c["D"], c["Hkv"]
    bufs.enter(F.group(c))
    kv, vv = bufs.view(bufs.k, c), bufs.view(bufs.v, c)
    g = F.geometry(c)
    gen = torch.Generator(device=DEV).manual_seed(11)
    # (slot, first row, rows).  Far rows: rows 239 | 240, 495 | 496, 1007 | 1008 straddle the 2, 4 and 8 GiB marks — for each mark one spot whose rows
    # straddle it (keep_rows touches row0 .. row0 + 7: 236.., 492.., 1004..) and one whose FIRST row (keep_rows: row0) lies past it.  Far slots: every zone.
    spots = ([(0, 236, 9), (0, 242, 9), (0, 492, 12), (0, 498, 9), (0, 1004, 17), (0, 1010, 9)] if geo == "row" else
             [(8, 5, 9), (0, 0, 3), (4, 1000, 12), (2, 30, 5), (6, 17, 8)])
    if geo == "row":
        first = [g["base"] + r0 * g["rs"] for _, r0, _ in spots]
        last = [g["base"] + (r0 + min(n, 8) - 1) * g["rs"] for _, r0, n in spots]
        assert all(any(a < m <= z for a, z in zip(first, last)) and any(a >= m and a - m < 8 * g["rs"] for a in first) for m in F.MARKS)
    kf, vf = bufs.fills(F.group(c))
    raw = lambda t: t.view(torch.uint8) if fp8 else t
    for slot, r0, n in spots:
        kd, vd = kv[slot, r0:r0 + n], vv[slot, r0:r0 + n]
        what = "%s %s %s: slot %d rows %d..%d (byte offset %d)" % (w, geo, dt, slot, r0, r0 + n, g["base"] + slot * g["bs"] + r0 * g["rs"])
        if w.startswith("keep_rows"):
            sk = torch.randn(n, Hkv, D, device=DEV, generator=gen)
            sk, sv = (sk.to(torch.float8_e4m3fn), (2 * sk).to(torch.float8_e4m3fn)) if fp8 else (sk.to(dtype), (2 * sk).to(dtype))
            F._bits(kd).copy_(F._bits(sk))
            F._bits(vd).copy_(F._bits(sv))
            keep = [i for i in range(min(n, 8)) if i % 3 != 1]
            idx = torch.tensor([keep + [0] * (8 - len(keep))], dtype=torch.int32, device=DEV)
            i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
            O.keep_rows(kv, vv, i32([r0]), idx, i32([len(keep)]), cache_batch_idx=i32([slot]))
            wk, wv = sk.clone(), sv.clone()
            wk[:len(keep)], wv[:len(keep)] = sk[keep], sv[keep]
        else:
            key = torch.randn(n, Hkv, D, device=DEV, dtype=dtype, generator=gen)
            val = torch.randn(n, Hkv, D, device=DEV, dtype=dtype, generator=gen)
            if w == "flat_elem":          # sources one element off a 16-byte boundary: the 2-byte element path
                key, val = (torch.cat((t.flatten()[:1], t.flatten()))[1:].view(n, Hkv, D) for t in (key, val))
                assert key.data_ptr() % 16 == 2
            if w in ("flat_vec", "flat_elem"):
                O.cache_flat(key, val, kd, vd, "auto")
                wk, wv = key, val
            elif w == "flat_rope":          # (what the rotation computes is tests/test_gpu_rope_*.py's subject: here, the same call into a small dense cache)
                cs = torch.randn(64, D, device=DEV, dtype=dtype, generator=gen)
                wk, wv = torch.zeros_like(key), torch.zeros_like(val)
                O.cache_flat_rope(key, val, wk, wv, cs, 7)
                O.cache_flat_rope(key, val, kd, vd, cs, 7)
                assert torch.equal(wv, val) and not torch.equal(wk, key)
            else:                           # (the bytes are tests/test_gpu_fp8kv.py's subject: here, the same call into a small dense cache)
                ks, vs = (torch.tensor(x, dtype=torch.float32, device=DEV) for x in X.case_scales(c))
                wk, wv = (torch.zeros(n, Hkv, D, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(2))
                O.cache_flat_fp8(key, val, wk, wv, ks, vs)
                O.cache_flat_fp8(key, val, kd, vd, ks, vs)
                assert bool((wk.view(torch.uint8) != 0).any())
        torch.cuda.synchronize()
        bk, bv = F._bits(kd) != F._bits(wk), F._bits(vd) != F._bits(wv)
        raw(kd).fill_(kf)          # (the fill goes back first: a failing spot must not fail the whole-buffer checks behind it)
        raw(vd).fill_(vf)
        assert not bool(bk.any()) and not bool(bv.any()), "%s: %d K and %d V elements differ; first rows %s" % (what, int(bk.sum()), int(bv.sum()), (bk | bv).flatten(1).any(1).nonzero().flatten()[:4].tolist())
    assert bufs.dirty() == 0, "%s %s %s: with the fill put back over the written rows, the buffers differ from the fill elsewhere" % (w, geo, dt)


def test_far_address_plans_reached():
    """The union of (geometry, form, path, tiling, merge launch, queue, windowed, entry point) the table ran on, and the worst figures, printed once.
    When every case ran in this process, the union must hold every plan of tests/far_address.py `needed_plans`, nothing missing."""
    print("\nfar-address census: plans reached (geometry, form, path, tiling, merge_launch, queue, windowed, entry): cases")
    for k in sorted(REACHED, key=str):
        print("  %s: %d" % (k, REACHED[k]))
    took = time.time() - WORST["t0"] if WORST["t0"] else 0.0
    print("far-address census: %d cases, %.1f s for the module so far, slowest case %.2f s; worst element error %.3f ulp; worst |lse - ln n| n = %.4f (%s)"
          % (sum(REACHED.values()), took, WORST["seconds"], WORST["max_ulp"], WORST["lse_worst_times_n"], WORST["lse_case"]))
    if sum(REACHED.values()) != len(CASES):
        print("partial run: %d of %d table cases ran here, the coverage list is not checked" % (sum(REACHED.values()), len(CASES)))
        return
    missing = sorted(F.needed_plans() - set(REACHED), key=str)
    assert not missing, "plans the far-address table no longer reaches: %s" % missing
