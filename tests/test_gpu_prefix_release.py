"""GPU: windowed attention over sequences whose dead prefix is REALLY unmapped (HIP VMM backend, vattention.release_prefix), with small
pages so that a few thousand tokens span many of them.

Every case runs its shape twice.  First in the POISON form of tests/test_gpu_window.py: everything stays mapped, and instead of releasing,
K rows are set to NaN and V rows to Inf below the no-read contract line (align_down(first visible key, T), T = 32 decode / 64 prefill —
at or above everything the release rule would let go).  Outputs must be finite and torch.equal to a twin that holds ordinary data there:
a load below the line shows up as a wrong number.  Only when that has passed, in the same test function, does the same shape run over
the unmapped prefix, where such a load would be a page fault.

The twin: slots [n, 2n) of the same manager hold the same K/V bits as slots [0, n), stay fully mapped and receive the same calls.
After every step vattention.slot_ranges() equals the plain-Python model (tests/prefix_release_ref.py) driven with the same calls."""
import pytest
import torch

from oracle.attn import flash_attn_with_kvcache_ref
from tests.prefix_release_ref import PrefixReleaseOracle
from vattention_amd.window_release import keep_from_decode, keep_from_prompt, pages_below

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Caches:
    """One manager, 2n slots: [0, n) are released (or poisoned), [n, 2n) are their fully mapped twins."""

    def __init__(self, n, Hkv, D, dtype, ctx=4096, groups=1200):
        from vattention_amd import vattention as va
        self.va, self.n, self.Hkv, self.D, self.dtype = va, n, Hkv, D, dtype
        torch.zeros(1, device=DEV)
        va.enable_layered_async(False)
        self.page = max(va.granularity(0)[0], 16 << 10)
        itemsize = 2
        self.k, self.v = va.init_kvcache(1, Hkv, D, 2 * n, ctx, 0, dtype, self.page, False)
        assert va.reserve_physical_pages(groups * 2 * self.page) == groups * 2
        self.row_bytes = Hkv * D * itemsize
        self.model = PrefixReleaseOracle(1, Hkv, D, 2 * n, ctx, itemsize, self.page, False)
        self.model.reserve_physical_pages(groups * 2 * self.page)
        self.lens = [0] * (2 * n)
        self.dead = [0] * n                   # poison form: rows already poisoned per slot

    def alloc_all(self, lengths):
        for i, n_tok in enumerate(list(lengths) + list(lengths)):
            assert self.va.alloc_new_batch_idx(n_tok) == i == self.model.alloc_new_batch_idx(n_tok)
            self.lens[i] = n_tok

    def step(self):
        self.va.step_async(self.lens)
        self.model.step_async(self.lens)

    def release(self, slot, keep):
        """The engine's rule: call only when a whole page would go."""
        if pages_below(keep, self.row_bytes, self.page) > self.model.head[slot]:
            n = self.va.release_prefix(slot, keep)
            assert n == self.model.release_prefix(slot, keep) and n > 0

    def poison(self, slot, first_visible, tile):
        """The poison form: what the no-read contract says no kernel reads (T = `tile`) becomes NaN / Inf instead of being released."""
        line = max(0, first_visible) // tile * tile
        if line > self.dead[slot]:
            self.k[slot, self.dead[slot]:line] = float("nan")
            self.v[slot, self.dead[slot]:line] = float("inf")
            self.dead[slot] = line

    def check_ranges(self):
        assert self.va.slot_ranges() == self.model.ranges()

    def fill(self, slot, lo, hi, gen):
        """The same random rows into a slot and its twin."""
        kr = torch.randn(hi - lo, self.Hkv, self.D, generator=gen).to(self.dtype).to(DEV)
        vr = torch.randn(hi - lo, self.Hkv, self.D, generator=gen).to(self.dtype).to(DEV)
        for s in (slot, slot + self.n):
            self.k[s, lo:hi].copy_(kr)
            self.v[s, lo:hi].copy_(vr)

    def close(self):
        self.va.cleanup()


def _decode_run(dtype, left, unmapped, steps=150):
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    Hq, Hkv, D = 8, 2, 128
    start = [700, 40, 333, 1290]                                  # ragged; 32 tokens per 16 KiB page at 512 B per row
    n = len(start)
    c = Caches(n, Hkv, D, dtype)
    outs = []
    try:
        gen = torch.Generator().manual_seed(7)
        c.alloc_all(start)
        c.step()
        for s in range(n):
            c.fill(s, 0, start[s], gen)
        idx_a = torch.arange(0, n, dtype=torch.int32, device=DEV)
        idx_b = torch.arange(n, 2 * n, dtype=torch.int32, device=DEV)
        cur = list(start)
        for it in range(steps):
            for s in range(n):
                c.lens[s] = c.lens[s + n] = cur[s] + 1            # the step appends one token
            c.step()
            for s in range(n):
                if unmapped:
                    c.release(s, keep_from_decode(cur[s] + 1, left))
                else:
                    c.poison(s, cur[s] - left, 32)
            c.check_ranges()
            q = torch.randn(n, 1, Hq, D, generator=gen).to(dtype).to(DEV)
            kn = torch.randn(n, 1, Hkv, D, generator=gen).to(dtype).to(DEV)
            vn = torch.randn(n, 1, Hkv, D, generator=gen).to(dtype).to(DEV)
            cl = torch.tensor(cur, dtype=torch.int32, device=DEV)
            rows = max(cur) + 1
            a = flash_attn_with_kvcache(q, c.k[:, :rows], c.v[:, :rows], kn, vn, cache_seqlens=cl, cache_batch_idx=idx_a, causal=True,
                                        window_size=(left, 0))
            b = flash_attn_with_kvcache(q, c.k[:, :rows], c.v[:, :rows], kn, vn, cache_seqlens=cl, cache_batch_idx=idx_b, causal=True,
                                        window_size=(left, 0))
            if it % 16 == 15 or it == steps - 1:
                torch.cuda.synchronize()
                assert bool(torch.isfinite(a).all()) and torch.equal(a, b), "decode step %d left %d unmapped %s" % (it, left, unmapped)
            outs.append(a)
            cur = [x + 1 for x in cur]
        torch.cuda.synchronize()
        if unmapped:
            st = c.va.stats()
            assert st["prefix_pages_released"] == sum(h for h, _ in c.model.ranges()) and st["prefix_pages_released"] > 0
            c.va.wait()
            mapped_groups = sum(e - h for h, e in c.model.ranges())
            assert c.va.stats()["pages_mapped_now"] == 2 * mapped_groups
        return [o.cpu() for o in outs]
    finally:
        c.close()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("left", [0, 31, 1000, 200])
def test_decode_over_an_unmapped_prefix(left, dtype):
    """Ragged batch growing token by token across several page boundaries, the in-kernel one-row append, release rule every step.
    left = 200 spans six pages; left = 1000 keeps the short sequences whole while the long ones release."""
    poison = _decode_run(dtype, left, unmapped=False)
    real = _decode_run(dtype, left, unmapped=True)
    assert all(torch.equal(x, y) for x, y in zip(poison, real))


def _prefill_run(D, Hkv, varlen, unmapped, left=300):
    from vattention_amd.flash_attn import flash_attn_varlen_with_kvcache, flash_attn_with_kvcache
    dtype, Hq = torch.float16, 8
    prompts = [3000, 2200] if varlen else [3000]
    chunks = [512, 300, 700, 64, 1000, 424]                       # cut to each prompt's remainder
    n = len(prompts)
    c = Caches(n, Hkv, D, dtype)
    outs = []
    try:
        gen = torch.Generator().manual_seed(11)
        done = [0] * n
        c.alloc_all([min(chunks[0], p) for p in prompts])
        ci = 0
        while any(d < p for d, p in zip(done, prompts)):
            qls = [min(chunks[ci % len(chunks)], p - d) for d, p in zip(done, prompts)]
            ci += 1
            for s in range(n):
                c.lens[s] = c.lens[s + n] = done[s] + qls[s] if qls[s] else c.lens[s]
            c.step()
            for s in range(n):
                if not qls[s]:
                    continue
                if unmapped:
                    c.release(s, keep_from_prompt(done[s], left))
                else:
                    c.poison(s, done[s] - left, 64)
                c.fill(s, done[s], done[s] + qls[s], gen)
            c.check_ranges()
            live = [s for s in range(n) if qls[s]]
            res = []
            for off in (0, n):
                if varlen:
                    q = torch.randn(sum(qls), Hq, D, generator=torch.Generator().manual_seed(ci)).to(dtype).to(DEV)
                    starts = [sum(qls[i] for i in live[:j]) for j in range(len(live))]
                    t32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
                    o = flash_attn_varlen_with_kvcache(q, c.k, c.v, t32(starts), t32([qls[s] for s in live]), max(qls),
                                                       t32([done[s] + qls[s] for s in live]), t32([s + off for s in live]), causal=True,
                                                       window_size=(left, 0))
                else:
                    s = live[0] + off
                    q = torch.randn(1, qls[0], Hq, D, generator=torch.Generator().manual_seed(ci)).to(dtype).to(DEV)
                    o = flash_attn_with_kvcache(q, c.k[s:s + 1, :done[0] + qls[0]], c.v[s:s + 1, :done[0] + qls[0]], cache_seqlens=done[0] + qls[0],
                                                causal=True, window_size=(left, 0))
                res.append(o)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(res[0]).all()) and torch.equal(res[0], res[1]), "chunk %d unmapped %s" % (ci, unmapped)
            outs.append(res[0].cpu())
            done = [d + x for d, x in zip(done, qls)]
        if unmapped:
            assert c.va.stats()["prefix_pages_released"] > 0 and c.model.head[0] > 0
        return outs
    finally:
        c.close()


@pytest.mark.parametrize("D,Hkv", [(128, 2), (64, 4)], ids=["d128", "d64"])
@pytest.mark.parametrize("varlen", [False, True], ids=["kvcache", "varlen"])
def test_chunked_prefill_over_an_unmapped_prefix(varlen, D, Hkv):
    poison = _prefill_run(D, Hkv, varlen, unmapped=False)
    real = _prefill_run(D, Hkv, varlen, unmapped=True)
    assert all(torch.equal(x, y) for x, y in zip(poison, real))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_slot_reuse_after_a_hole_maps_other_pages_at_the_same_addresses(dtype):
    """Free a slot with a hole; the next request takes it with NO window from position 0: unmap + map of another handle at the same
    virtual address, the case the TLB step exists for.  Against the oracle at the project's tolerances."""
    from vattention_amd.flash_attn import flash_attn_with_kvcache
    Hq, Hkv, D, left = 8, 2, 128, 100
    c = Caches(1, Hkv, D, dtype)
    try:
        gen = torch.Generator().manual_seed(3)
        c.alloc_all([2000])
        c.step()
        c.fill(0, 0, 2000, gen)
        # poison form first, then the release
        q = torch.randn(1, 1, Hq, D, generator=gen).to(dtype).to(DEV)
        c.poison(0, 1999 - left, 32)
        a = flash_attn_with_kvcache(q, c.k[0:1, :2000], c.v[0:1, :2000], cache_seqlens=2000, causal=True, window_size=(left, 0))
        b = flash_attn_with_kvcache(q, c.k[1:2, :2000], c.v[1:2, :2000], cache_seqlens=2000, causal=True, window_size=(left, 0))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        c.release(0, keep_from_decode(2000, left))
        a2 = flash_attn_with_kvcache(q, c.k[0:1, :2000], c.v[0:1, :2000], cache_seqlens=2000, causal=True, window_size=(left, 0))
        torch.cuda.synchronize()
        assert torch.equal(a2, b)
        assert c.va.slot_ranges()[0][0] > 0
        c.va.free_batch_idx(0)
        c.model.free_batch_idx(0)
        c.check_ranges()
        assert c.va.slot_ranges()[0] == (0, 0)
        assert c.va.alloc_new_batch_idx(1500) == 0 == c.model.alloc_new_batch_idx(1500)
        c.lens[0] = 1501
        c.step()
        c.check_ranges()
        assert c.va.slot_ranges()[0][0] == 0
        hk = torch.randn(1, 1501, Hkv, D, generator=gen).to(dtype)
        hv = torch.randn(1, 1501, Hkv, D, generator=gen).to(dtype)
        c.k[0, :1500].copy_(hk[0, :1500].to(DEV))
        c.v[0, :1500].copy_(hv[0, :1500].to(DEV))
        q = torch.randn(1, 1, Hq, D, generator=gen).to(dtype)
        kn, vn = hk[:, 1500:1501].clone(), hv[:, 1500:1501].clone()
        cl = torch.tensor([1500], dtype=torch.int32)
        out = flash_attn_with_kvcache(q.to(DEV), c.k[0:1, :1501], c.v[0:1, :1501], kn.to(DEV), vn.to(DEV), cache_seqlens=cl.to(DEV), causal=True)
        torch.cuda.synchronize()
        ref = flash_attn_with_kvcache_ref(q, hk.clone(), hv.clone(), kn, vn, cache_seqlens=cl, causal=True)
        tol = 2e-3 if dtype == torch.float16 else 1.6e-2
        err = (out.double().cpu() - ref).abs()
        assert bool((err <= tol + tol * ref.abs()).all()), "max err %.3e" % err.max().item()
        assert torch.equal(c.k[0, :1501].cpu(), hk[0]) and torch.equal(c.v[0, :1501].cpu(), hv[0])      # the new occupant's rows, all of them
    finally:
        c.close()


# ---- engine level ----

class _Mirror:
    """Forwards the page manager's calls of one replay to the model, call for call."""

    def __init__(self, pm, model):
        self.pm, self.model = pm, model
        for name in ("alloc_new_batch_idx", "step_async", "step", "release_prefix", "release_prefixes", "free_batch_idx"):
            setattr(pm, name, self._wrap(name, getattr(pm, name)))

    def _wrap(self, name, real):
        def call(*a, **kw):
            ret = real(*a, **kw)
            args = a[:2] if name == "release_prefix" else a[:1] if name in ("free_batch_idx", "release_prefixes") else a
            want = getattr(self.model, name)(*args)
            if name in ("alloc_new_batch_idx", "release_prefix", "release_prefixes"):
                assert ret == want, name
            assert self.pm.ranges() == self.model.ranges(), name
            return ret
        return call


def _engine_run(left, mode):
    """mode: "plain" = windowed kernels over fully mapped, ordinary data; "poison" = the same, with NaN K rows / Inf V rows below the
    no-read contract line of every scheduled slot (T = 64 for a prompt chunk, 32 for a decode token), written after the engine's step and
    before the iteration's kernels; "release" = the engine releases the pages in front of the window."""
    from vattention_amd import vattention as va
    from vattention_amd.replay import CacheConfig, HotPathRunner, ModelConfig, ParallelConfig
    page = max(va.granularity(0)[0], 16 << 10)
    L, Hq, Hkv, D, B, ctx = 2, 8, 2, 128, 4, 4096
    model = ModelConfig(name="tiny", num_layers=L, num_q_heads=Hq, num_kv_heads=Hkv, head_size=D, dtype=torch.float16, max_model_len=ctx)
    groups = 600
    cache = CacheConfig(page_size=page, max_batch_size=B, memory_for_gpu=groups * 2 * L * page, vattn_keep_layout=True)
    r = HotPathRunner(model, ParallelConfig(1, 1), cache, device=DEV, seed=5, sliding_window=left, release_prefix=mode == "release")
    try:
        assert r.engine.page_size == page and not r.engine.vattn_mega_cache
        ref = PrefixReleaseOracle(L, Hkv, D, B, ctx, 2, page, False)
        ref.reserve_physical_pages(groups * 2 * L * page)
        _Mirror(va._pm, ref)
        r.admission_lookahead = False            # (premap is not part of the model)
        r.sample_kv_util = False
        outs, peaks, dead, now = [], [0, 0], {}, []
        run_iteration = r.run_iteration

        def after_step(_runner):                 # right after engine.step, on the compute stream, before the iteration's kernels
            va.wait()
            peaks[0] = max(peaks[0], va.stats()["pages_mapped_now"])
            peaks[1] = max(peaks[1], len(ref.mapped_ranges()))
            if mode != "poison":
                return
            for md in now:
                slot = r.engine.seq_to_batch_idx[md.seq.seq_id]
                if md.is_prompt:
                    first_visible, tile = md.seq.prompt_processed - left, 64
                    if md.seq.prompt_processed == 0:
                        dead[slot] = 0               # a new occupant
                else:
                    first_visible, tile = md.seq.get_len() - 1 - left, 32
                line = max(0, first_visible) // tile * tile
                if line > dead.get(slot, 0):
                    for k_l, v_l in r.engine.gpu_cache:
                        k_l[slot, dead.get(slot, 0):line] = float("nan")
                        v_l[slot, dead.get(slot, 0):line] = float("inf")
                    dead[slot] = line

        def recording(mds):
            now[:] = mds
            out = run_iteration(mds)
            outs.append(out.clone())
            return out
        r.iter_hook = after_step
        r.run_iteration = recording
        r.run_static_trace(num_requests=6, total_len=1400, pd_ratio=20.0, chunk_size=256)      # prompt chunks with piggy-backed decodes, then decode batches
        torch.cuda.synchronize()
        if mode == "poison":
            assert max(dead.values()) > 1000
        return [o.cpu() for o in outs], peaks, va.stats()
    finally:
        r.close()


def test_engine_replay_poisoned_then_released_equals_the_fully_mapped_replay_and_holds_fewer_pages():
    """The engine's shapes — mixed prompt-chunk + decode batches through the wrapper, 256-token chunks under left = 128, two layers,
    layer-ordered mapping — first in the poison form against the fully mapped twin run, and only then over released pages."""
    left = 128
    plain, peak_plain, st_plain = _engine_run(left, "plain")
    poison, _, st_poison = _engine_run(left, "poison")
    assert len(poison) == len(plain)
    assert all(bool(torch.isfinite(x).all()) and torch.equal(x, y) for x, y in zip(poison, plain)), "a load below the no-read contract line"
    assert st_plain["prefix_pages_released"] == 0 == st_poison["prefix_pages_released"]
    real, peak_real, st_real = _engine_run(left, "release")
    assert len(real) == len(plain) and all(torch.equal(x, y) for x, y in zip(real, plain))
    assert st_real["prefix_pages_released"] > 0
    assert peak_plain[0] == peak_plain[1] and peak_real[0] == peak_real[1]
    assert peak_real[0] < peak_plain[0]


def test_a_wider_attention_window_than_the_engines_is_refused():
    """No kernel is launched over released pages here: the engine's step alone is what raises (or, for a narrower window, releases)."""
    from vattention_amd.attention import get_attention_wrapper
    from vattention_amd.replay import CacheConfig, HotPathRunner, ModelConfig, ParallelConfig, Sequence, SequenceMetadata
    from vattention_amd import vattention as va
    page = max(va.granularity(0)[0], 16 << 10)
    model = ModelConfig(name="tiny", num_layers=1, num_q_heads=8, num_kv_heads=2, head_size=128, dtype=torch.float16, max_model_len=2048)
    cache = CacheConfig(page_size=page, max_batch_size=2, memory_for_gpu=200 * 2 * page, vattn_keep_layout=True)
    r = HotPathRunner(model, ParallelConfig(1, 1), cache, device=DEV, sliding_window=100)
    try:
        seq = Sequence(0, 600, 700)
        r.run_iteration([SequenceMetadata(seq, 300, True)])          # processed = 0: nothing to release yet
        torch.cuda.synchronize()
        assert va.stats()["prefix_pages_released"] == 0
        for wider in (None, 101):
            get_attention_wrapper().set_sliding_window(wider)
            with pytest.raises(ValueError, match="sliding window"):
                r.engine.step([SequenceMetadata(seq, 300, True)])
            assert va.stats()["prefix_pages_released"] == 0
        get_attention_wrapper().set_sliding_window(64)          # narrower is fine: it reads less than the engine keeps
        r.engine.step([SequenceMetadata(seq, 300, True)])
        assert va.stats()["prefix_pages_released"] == (300 - 100) // 64 * 64 * 512 // page
        with pytest.raises(ValueError):
            r.engine.set_sliding_window(-1)
        with pytest.raises(ValueError):
            r.engine.set_sliding_window(200)                    # cannot be widened over a prefix that is already gone
    finally:
        get_attention_wrapper().set_sliding_window(None)
        r.close()
