"""The fused rotary embedding on the GPU, probed by twin calls on the same build (tests/rope_twin.py; proved on the CPU by
tests/test_rope_twin_model.py): call A rotates in the kernel with a table of random finite values, call B gets operands rotated by the oracle
and the identity table.  Both take the same gate, plan and kernel build — asserted through the plan description of the two launched
parameter blocks — so out, LSE and every byte of the cache allocations must be BIT-IDENTICAL; A is anchored to the f64 oracle with the
project's own tolerance.  A wrong table row for one query row or one new key, an un-rotated second head block or a piece rotated at its
piece-relative row moves every element of the rotated operand: no tolerance is involved in seeing it.  The tables sit between NaN guard rows.

Then the cache writers bit for bit against the oracle over the whole allocation (cache_flat_rope: d 16 / 64 / 128, strided rows, past the
8192-block grid clamp; rotary_embedding: rot_dim < head size, both pairings, q / k as column slices of a qkv tensor) and the drop-in's
rotary_cos / rotary_sin argument."""
import pytest
import torch

from oracle.attn import rotary_embedding_ref
from tests import census as C
from tests import rope_twin as RT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = RT.cases()
REACHED = {}


def run_twin(c):
    t = RT.build(c)
    outA, lseA, kA, vA, pA, dA, lstA = RT.launch(c, t, "A", DEV)
    outB, lseB, kB, vB, pB, dB, lstB = RT.launch(c, t, "B", DEV)
    # 1. the two launched blocks describe alike, and as the case names
    assert dA == dB, "%s: A %s, B %s" % (c["name"], dA, dB)
    what = RT.check_plan(c, pA, dA, lstA)
    RT.check_plan(c, pB, dB, lstB)
    REACHED[RT.union_key(c, dA)] = REACHED.get(RT.union_key(c, dA), 0) + 1
    # 2. out and LSE bit for bit
    fails = RT.bit_diff(outA, outB, "out, A against B")
    if lseA is not None:
        fails += RT.bit_diff(lseA, lseB, "LSE, A against B", "bhs")
    # 3. the whole cache allocations: the appended rows hold the oracle-rotated keys and the un-rotated values, nothing else changed
    for got, exp, name in ((kA, t["k_after"], "k cache after A"), (vA, t["v_after"], "v cache after A"), (kB, t["k_after"], "k cache after B"), (vB, t["v_after"], "v cache after B")):
        fails += RT.bit_diff(got, exp, name, "cache")
    assert not fails, what + "\n  " + "\n  ".join(fails)
    # 4. A against the f64 oracle on the pre-rotated operands: the project's own check
    ref64, lse64 = RT.oracle(c, t, "f64")
    ref32, _ = RT.oracle(c, t, "f32")
    C.check(outA, ref64, ref32, C.DT[c["dt"]], what)
    if lseA is not None:
        C.check_lse(lseA, lse64, what + ": LSE")


@pytest.mark.parametrize("case", [pytest.param(c, marks=pytest.mark.lab) if c["lab"] else c for c in CASES], ids=[c["name"] for c in CASES])
def test_rope_twin(case):
    run_twin(case)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_rotary_cos_sin_arguments_equal_the_table_and_follow_in_place_updates(dt):
    """rotary_cos / rotary_sin [positions, d / 2] with rotary_interleaved=False equal the `_rotary_cos_sin` call bit for bit; after an in-place
    change of rotary_cos the next call follows the new values (the cached cat is keyed on the tensors' versions)."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    dtype, D, Hkv, G, B = C.DT[dt], 128, 2, 4, 3
    g = torch.Generator().manual_seed(77)
    lens = [1, 33, 200]
    q = torch.randn(B, 1, Hkv * G, D, generator=g).to(dtype).to(DEV)
    kn, vn = torch.randn(B, 1, Hkv, D, generator=g).to(dtype).to(DEV), torch.randn(B, 1, Hkv, D, generator=g).to(dtype).to(DEV)
    k0, v0 = torch.randn(B, 208, Hkv, D, generator=g).to(dtype).to(DEV), torch.randn(B, 208, Hkv, D, generator=g).to(dtype).to(DEV)
    cl = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device=DEV)
    tabs = [(torch.rand(200, D, generator=g) * 2 - 1).to(dtype).to(DEV) for _ in range(2)]

    def call(**rot):
        kc, vc = k0.clone(), v0.clone()
        out, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=cl, causal=True, return_softmax_lse=True, **rot)
        torch.cuda.synchronize()
        return out.cpu(), lse.cpu(), kc.cpu(), vc.cpu()
    cos, sin = tabs[0][:, :D // 2].contiguous(), tabs[0][:, D // 2:].contiguous()
    for step in range(2):
        got = call(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False)
        again = call(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False)        # (the cached cat)
        exp = call(_rotary_cos_sin=tabs[step])
        for a, b, e, name in zip(got, again, exp, ("out", "lse", "k cache", "v cache")):
            lay = "bhs" if name == "lse" else "bshd"
            assert not RT.bit_diff(a, e, "%s, step %d" % (name, step), lay) and not RT.bit_diff(b, e, "%s (cached), step %d" % (name, step), lay)
        cos.copy_(tabs[1][:, :D // 2])          # in place: the same tensor objects, new versions
        sin.copy_(tabs[1][:, D // 2:])
    assert not torch.equal(call(_rotary_cos_sin=tabs[0])[0], call(_rotary_cos_sin=tabs[1])[0])
    with pytest.raises(NotImplementedError):
        call(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=True)


def _guarded(shape, dtype, fill=float("nan")):
    """a [rows, width] view with `shape` inside a poisoned allocation two rows and 8 columns larger on each side: (allocation, view)"""
    alloc = torch.full((shape[0] + 4, shape[1] + 16), fill, dtype=dtype)
    return alloc, alloc[2:2 + shape[0], 8:8 + shape[1]]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("D,n,heads,strided", [(16, 70, 3, True), (64, 301, 3, True), (128, 301, 3, False), (128, 130, 3, True), (128, 33000, 8, False)],
                         ids=["d16", "d64", "d128_dense", "d128", "d128_past_the_grid_clamp"])
def test_cache_flat_rope_is_bit_exact_over_the_whole_allocation(dt, D, n, heads, strided):
    """k_cache[t] = rope(key[t], pos0 + t), v_cache[t] = value[t], nothing else written; source and cache rows strided (views of wider
    allocations); 33 000 x 8 x 128 is 2 112 000 threads of work for a grid clamped to 8192 x 256 = 2 097 152: the grid-stride loop's second trip"""
    from vattention_amd.cache_ops import cache_flat_rope
    dtype, pos0 = C.DT[dt], 5
    g = torch.Generator().manual_seed(D + n)
    assert n * heads * (D // 16) > 8192 * 256 or n < 1000
    P = pos0 + n
    talloc = torch.full((RT.GUARD + P + RT.GUARD, 2 * D), float("nan"), dtype=dtype)
    talloc[RT.GUARD:RT.GUARD + P, :D] = (torch.rand(P, D, generator=g) * 2 - 1).to(dtype)
    W = heads * D
    if strided:
        (ka, kv_), (va, vv_), (kca, kcv), (vca, vcv) = (_guarded((n, W), dtype) for _ in range(4))
    else:
        ka, va, kca, vca = (torch.full((n, W), float("nan"), dtype=dtype) for _ in range(4))
        kv_, vv_, kcv, vcv = ka, va, kca, vca
    kv_.copy_(torch.randn(n, W, generator=g).to(dtype))
    vv_.copy_(torch.randn(n, W, generator=g).to(dtype))
    kg, vg, kcg, vcg, tg = ka.to(DEV), va.to(DEV), kca.to(DEV), vca.to(DEV), talloc.to(DEV)
    view = (lambda a: a[2:2 + n, 8:8 + W]) if strided else (lambda a: a)
    cache_flat_rope(view(kg).unflatten(1, (heads, D)), view(vg).unflatten(1, (heads, D)),
                    view(kcg).unflatten(1, (heads, D)), view(vcg).unflatten(1, (heads, D)), tg[RT.GUARD:RT.GUARD + P, :D], pos0)
    torch.cuda.synchronize()
    kr = kv_.clone().contiguous()
    rotary_embedding_ref(torch.arange(pos0, pos0 + n), torch.zeros(n, D, dtype=dtype), kr, D, talloc[RT.GUARD:RT.GUARD + P, :D])
    kcv.copy_(kr)
    vcv.copy_(vv_)
    for got, exp, name in ((kcg, kca, "k cache"), (vcg, vca, "v cache"), (kg, ka, "key (source)"), (vg, va, "value (source)")):
        assert not RT.bit_diff(got.cpu()[None, :, None, :], exp[None, :, None, :], name, "cache")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("hs,rot", [(64, 64), (64, 32), (128, 128), (128, 64)])
@pytest.mark.parametrize("neox", [True, False], ids=["neox", "gptj"])
def test_rotary_embedding_partial_dim_and_qkv_slices(dt, hs, rot, neox):
    """the stand-alone kernel with rot_dim <= head size, both pairings, q and k as column slices of one qkv tensor: elements outside rot_dim
    and outside the slices (the v columns, a pad column block) untouched"""
    from vattention_amd.cache_ops import rotary_embedding
    dtype, T, Hq, Hkv = C.DT[dt], 77, 5, 3
    g = torch.Generator().manual_seed(hs + rot)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * hs + 8, generator=g).to(dtype)
    pos = torch.randint(0, 500, (T,), generator=g, dtype=torch.int64)
    talloc = torch.full((RT.GUARD + 500 + RT.GUARD, 2 * rot), float("nan"), dtype=dtype)
    talloc[RT.GUARD:RT.GUARD + 500, :rot] = (torch.rand(500, rot, generator=g) * 2 - 1).to(dtype)
    qg, tg = qkv.to(DEV), talloc.to(DEV)
    rotary_embedding(pos.to(DEV), qg[:, :Hq * hs], qg[:, Hq * hs:(Hq + Hkv) * hs], hs, tg[RT.GUARD:RT.GUARD + 500, :rot], neox)
    torch.cuda.synchronize()
    exp = qkv.clone()
    qe, ke = exp[:, :Hq * hs].contiguous(), exp[:, Hq * hs:(Hq + Hkv) * hs].contiguous()
    rotary_embedding_ref(pos, qe, ke, hs, talloc[RT.GUARD:RT.GUARD + 500, :rot], neox)
    exp[:, :Hq * hs], exp[:, Hq * hs:(Hq + Hkv) * hs] = qe, ke
    assert torch.equal(exp[:, (Hq + Hkv) * hs:], qkv[:, (Hq + Hkv) * hs:])
    if rot < hs:
        assert torch.equal(exp[:, :Hq * hs].view(T, Hq, hs)[..., rot:], qkv[:, :Hq * hs].view(T, Hq, hs)[..., rot:])
    assert not RT.bit_diff(qg.cpu()[None, :, None, :], exp[None, :, None, :], "qkv", "cache")


def test_rope_twin_plans_reached():
    """The union of (form, path, tiling, merge launch, head blocks, groups, window, D, dtype) the table ran on, printed once.  When every
    case of the table ran in this process the union must hold every combination of rope_twin.NEED; a partial run (-k, `not lab`, a worker
    of a split run) says so and concludes nothing."""
    print("\nrope twin: plans reached (form, path, tiling, merge_launch, head blocks, groups, windowed, D, dtype): calls")
    for k in sorted(REACHED, key=str):
        print("  %s: %d" % (k, REACHED[k]))
    if sum(REACHED.values()) != len(CASES):
        print("partial run: %d of %d table cases ran here, the coverage list is not checked" % (sum(REACHED.values()), len(CASES)))
        return
    miss = RT.missing(REACHED)
    assert not miss, "combinations the twin table no longer reaches: %s" % miss
