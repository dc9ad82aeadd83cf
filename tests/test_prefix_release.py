"""vattn_release_prefix / vattn_slot_ranges: libvattn_amd.so on the fake physical backend against the plain-Python model
(tests/prefix_release_ref.py).  After EVERY call the product's dumps, ranges, free-block count and the backend's mapped VA set
equal the model's; the fake backend counts contract violations (double map, unmap of a hole, access on a hole)."""
import random

import pytest

from oracle.pagemgr import PageManagerOracle
from tests.impls import ProductImpl, fake, fake_counters
from tests.prefix_release_ref import PrefixReleaseOracle
from vattention_amd import _lib as L
from vattention_amd.window_release import keep_from_decode, keep_from_prompt, pages_below

assert hasattr(L.lib(), "vattn_release_prefix") and hasattr(L.lib(), "vattn_slot_ranges")

STREAM = 0x5151          # any non-zero "hipStream_t": the fake backend only records that a fence exists

PAGE = 4096
PLAIN = dict(num_layers=2, num_kv_heads=2, head_size=128, max_batch_size=4, max_context_length=1024, itemsize=2,
             page_size=PAGE, megacache=False)                     # row 512 B: 8 tokens per page
MEGA = dict(PLAIN, megacache=True)                                # row 1024 B (layers inside): 4 tokens per page
STRADDLE = dict(PLAIN, num_kv_heads=3)                            # row 768 B: 5.33 rows per page, a row straddles two pages
DEEP = dict(PLAIN, num_layers=4)                                  # more layers than sync_layers (2): layer-ordered steps engage
CONFIGS = {"plain": PLAIN, "megacache": MEGA, "kvh3": STRADDLE, "layers4": DEEP}
# "layered": the cache engine's default — a new prompt's layers [0, 2) are mapped before step_async returns, the rest by the mapper
MODES = {"inline": L.FLAG_NO_MAPPER_THREAD, "mapper_thread": 0, "layered": L.FLAG_LAYERED_ASYNC}


def row_bytes(cfg):
    return cfg["num_kv_heads"] * cfg["head_size"] * cfg["itemsize"] * (cfg["num_layers"] if cfg["megacache"] else 1)


def make_model(cls, cfg, **kw):
    return cls(cfg["num_layers"], cfg["num_kv_heads"], cfg["head_size"], cfg["max_batch_size"], cfg["max_context_length"],
               cfg["itemsize"], cfg["page_size"], cfg["megacache"], **kw)


class Pair:
    """The product and a model, driven call for call."""

    def __init__(self, cfg, flags, model=None):
        self.cfg = cfg
        self.p = ProductImpl(cfg, flags=flags)
        self.m = model if model is not None else make_model(PrefixReleaseOracle, cfg)
        self.peak_product = self.peak_model = 0

    def call(self, name, *args, stream=STREAM):
        got = []
        for side in ("model", "product"):
            a = args
            if side == "model":
                fn = getattr(self.m, name)
            else:
                fn = getattr(self.p.pm, name)
                if name in ("release_prefix", "release_prefixes", "free_batch_idx"):
                    a = args + (stream,)
            try:
                got.append(("ok", fn(*a)))
            except (ValueError, RuntimeError) as e:
                got.append((type(e).__name__, None))
        assert got[0] == got[1], "%s%r: model %r, product %r" % (name, args, got[0], got[1])
        self.check()
        return got[1]

    def check(self):
        snap = self.p.snapshot(full=True)
        st = self.m.state()
        assert snap["mapped"] == st["mapped_pages"]
        assert snap["lens"] == st["curr_seq_lengths"]
        assert snap["pool_handles"] == st["pool"]
        assert snap["pagemap"] == [list(t) for t in st["pagemap"]]
        ranges = self.p.pm.ranges()
        if hasattr(self.m, "ranges"):
            assert ranges == self.m.ranges()
            assert self.p.pm.counts()["mapped_groups"] == self.m.mapped_groups()
        else:
            assert [f for f, _ in ranges] == [0] * len(ranges)
        assert self.p.pm.num_free_kvblocks() == self.m.num_free_kvblocks()
        assert self.p.mapped_ranges() == self.m.mapped_ranges()          # joins the mapper first
        c = fake_counters()
        assert c["violations"] == 0 and c["stale_vas"] == 0
        now = self.p.pm.stats()["pages_mapped_now"]
        assert now == c["mapped_pages"] == len(self.m.mapped_ranges())
        self.peak_product = max(self.peak_product, now)
        self.peak_model = max(self.peak_model, len(self.m.mapped_ranges()))

    def finish(self):
        self.call("cleanup")
        c = fake_counters()
        assert c["violations"] == 0 and c["mapped_pages"] == 0 and c["live_handles"] == 0 and c["reserved_ranges"] == 0
        self.p.pm.close()


def reserve(pair, groups):
    L2 = 2 * pair.cfg["num_layers"]
    pair.call("reserve_physical_pages", groups * L2 * pair.cfg["page_size"])


# ---------------------------------------------------------------------------------------------------------------------
# which pages go
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CONFIGS)
def test_pages_wholly_below_the_kept_token_go_and_no_byte_above(name, mode):
    cfg = CONFIGS[name]
    t = Pair(cfg, MODES[mode])
    reserve(t, 120)
    assert t.call("alloc_new_batch_idx", 300) == ("ok", 0)
    t.call("step_async", [300, 0, 0, 0])
    rb = row_bytes(cfg)
    bases = [t.p.pm.tensor_base(i) for i in range(t.p.pm.num_tensors)]
    for keep in (0, 1, 5, 6, 63, 64, 65, 127, 128, 201, 299, 300):
        before = t.p.pm.ranges()[0]
        P = keep * rb // PAGE
        want = max(0, P - before[0])
        assert t.call("release_prefix", 0, keep) == ("ok", want)
        first, end = t.p.pm.ranges()[0]
        assert first == max(before[0], P) and end == before[1]
        # every byte of rows [keep, 300) is still mapped, in every tensor
        mapped = t.p.mapped_ranges()
        for page in range(keep * rb // PAGE, (300 * rb - 1) // PAGE + 1):
            for i in range(len(bases)):
                assert (i, page * PAGE) in mapped
        # ... and nothing below the first position is
        assert all(off >= first * PAGE for _, off in mapped)
    if name == "kvh3":
        # tokens_per_page = floor(4096 / 768) = 5 would have released floor(201 / 5) = 40 positions: 3 more than the bytes allow
        assert 201 // (PAGE // rb) == 40 and 201 * rb // PAGE == 37
    st = t.p.pm.stats()
    assert st["prefix_releases"] == t.m.prefix_releases and st["prefix_pages_released"] == t.m.prefix_pages_released
    assert st["prefix_pages_released"] == t.p.pm.ranges()[0][0]
    t.finish()


# ---------------------------------------------------------------------------------------------------------------------
# arguments, fence, no-op
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_argument_rules_and_noop_calls_touch_nothing(mode):
    t = Pair(PLAIN, MODES[mode])
    reserve(t, 60)
    t.call("alloc_new_batch_idx", 100)
    t.call("step_async", [100, 0, 0, 0])
    t.p.pm.wait()
    c0, f0, q0 = fake_counters(), fake().vattn_fake_fence_wait_count(), fake().vattn_fake_quiesce_count()
    for slot, keep in ((-1, 0), (4, 0), (1, 0), (0, 101), (0, 1 << 40)):
        assert t.call("release_prefix", slot, keep)[0] == "ValueError"
    assert t.call("release_prefix", 0, 7) == ("ok", 0)                # 7 tokens: no whole page
    assert t.call("release_prefix", 0, 0) == ("ok", 0)
    c1 = fake_counters()
    assert c1["n_unmap"] == c0["n_unmap"] and c1["n_flush"] == c0["n_flush"]
    assert fake().vattn_fake_fence_wait_count() == f0 and fake().vattn_fake_quiesce_count() == q0
    assert t.p.pm.stats()["prefix_releases"] == 0
    # released once, the same keep_from_token is a no-op
    assert t.call("release_prefix", 0, 64) == ("ok", 8)
    assert t.call("release_prefix", 0, 64) == ("ok", 0)
    assert t.call("release_prefix", 0, 10) == ("ok", 0)               # below the head
    assert t.p.pm.stats()["prefix_releases"] == 1 and t.p.pm.stats()["prefix_pages_released"] == 8
    # a slot reserved by premap is not active (product only: the model has no premap)
    assert t.p.pm.premap(50) == 1
    with pytest.raises(ValueError):
        t.p.pm.release_prefix(1, 0, STREAM)
    assert t.p.pm.ranges()[1][0] == 0
    t.p.pm.close()


@pytest.mark.parametrize("mode", MODES)
def test_every_releasing_call_waits_for_its_fence_or_for_the_device(mode):
    t = Pair(PLAIN, MODES[mode])
    reserve(t, 60)
    t.call("alloc_new_batch_idx", 400)
    t.call("step_async", [400, 0, 0, 0])
    for i, keep in enumerate((64, 128, 192)):                          # on a stream: the slot's fence
        t.p.pm.wait()
        f0, q0 = fake().vattn_fake_fence_wait_count(), fake().vattn_fake_quiesce_count()
        assert t.call("release_prefix", 0, keep) == ("ok", 8)
        t.p.pm.wait()
        assert fake().vattn_fake_fence_wait_count() == f0 + 1 and fake().vattn_fake_quiesce_count() == q0
    f0, q0 = fake().vattn_fake_fence_wait_count(), fake().vattn_fake_quiesce_count()
    assert t.call("release_prefix", 0, 256, stream=None) == ("ok", 8)  # no stream: the device drains
    t.p.pm.wait()
    assert fake().vattn_fake_fence_wait_count() == f0 and fake().vattn_fake_quiesce_count() == q0 + 1
    # the free of a slot with a hole: everything else goes, behind the fence the free records
    f0 = fake().vattn_fake_fence_wait_count()
    t.call("free_batch_idx", 0)
    t.p.pm.wait()
    assert fake().vattn_fake_fence_wait_count() == f0 + 1
    st = t.p.pm.stats()
    assert st["fence_waits"] == 4 and st["quiesce_calls"] == 1
    t.finish()


# ---------------------------------------------------------------------------------------------------------------------
# a hole never outlives its occupant; shrinking
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "eager"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", ["free", "step_async_zero", "step_zero"])
def test_a_hole_never_outlives_its_occupant(how, mode, deferred):
    t = Pair(PLAIN, MODES[mode])
    t.call("set_deferred_reclamation", deferred)
    reserve(t, 80)
    pool0 = t.p.pm.state()["pool"]
    t.call("alloc_new_batch_idx", 200)
    t.call("alloc_new_batch_idx", 64)
    t.call("step_async", [200, 64, 0, 0])
    assert t.call("release_prefix", 0, 128) == ("ok", 16)
    if how == "free":
        t.call("free_batch_idx", 0)
    elif how == "step_async_zero":
        q0 = fake().vattn_fake_quiesce_count()
        t.call("step_async", [0, 65, 0, 0])
        assert fake().vattn_fake_quiesce_count() == q0 + 1      # nobody recorded a fence after the last launch: the device drains
    else:
        t.call("step", [0, 65, 0, 0], False)
    assert t.p.pm.ranges()[0] == (0, 0)
    assert not any(r[0] == 0 for r in t.p.pm.pagemap())
    used_by_1 = t.p.pm.ranges()[1][1] * 2 * PLAIN["num_layers"]
    assert t.p.pm.state()["pool"] == pool0 - used_by_1           # every page of slot 0 is back in the pool
    # the next occupant maps from position 0
    t.call("free_batch_idx", 1) if how == "free" else None
    lens = [0, 0 if how == "free" else 65, 0, 0]
    s = t.call("alloc_new_batch_idx", 40)[1]
    lens[s] = 40
    t.call("step_async", lens)
    first, end = t.p.pm.ranges()[s]
    assert first == 0 and end >= 5
    assert (s, s * t.p.pm.layout.virt_bytes_per_req, 0) in {(r[0], r[1], r[2]) for r in t.p.pm.pagemap()}
    t.finish()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CONFIGS)
def test_shrinking_into_the_hole_is_refused_before_anything_changes(name, mode):
    cfg = CONFIGS[name]
    t = Pair(cfg, MODES[mode])
    reserve(t, 120)
    t.call("alloc_new_batch_idx", 300)
    t.call("alloc_new_batch_idx", 100)
    t.call("step_async", [300, 100, 0, 0])
    t.call("release_prefix", 0, 130)
    head = t.p.pm.ranges()[0][0]
    first_tok = -(-head * PAGE // row_bytes(cfg))             # first token wholly in mapped positions
    assert 0 < first_tok <= 130
    before = (t.p.snapshot(full=True), t.p.pm.ranges())
    assert t.call("step_async", [first_tok - 1, 180, 0, 0])[0] == "ValueError"
    assert t.call("step", [1, 180, 0, 0], True)[0] == "ValueError"
    assert (t.p.snapshot(full=True), t.p.pm.ranges()) == before     # slot 1 did not grow either
    t.call("step_async", [first_tok, 100, 0, 0])                    # the boundary itself is a legal length
    t.call("step", [300, 100, 0, 0], True)
    t.finish()


@pytest.mark.parametrize("mode", MODES)
def test_tail_reclamation_stops_at_the_head(mode):
    """reclaim_on_demand takes over-mapped tail pages of other slots; a slot with a hole keeps [head, needed) and its head."""
    t = Pair(PLAIN, MODES[mode])
    reserve(t, 40)
    t.call("alloc_new_batch_idx", 200)
    t.call("step_async", [200, 0, 0, 0])                     # 25 groups + look-ahead
    t.call("release_prefix", 0, 160)                          # head = 20
    t.call("step_async", [161, 0, 0, 0])                      # shrink to just above the head: tail pages become reclaimable
    t.call("alloc_new_batch_idx", 300)
    t.call("step_async", [161, 300, 0, 0])                    # 38 groups: needs slot 0's tail
    first, end = t.p.pm.ranges()[0]
    assert first == 20 and end == 21
    t.finish()


# ---------------------------------------------------------------------------------------------------------------------
# shared prefixes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_released_shared_positions_leave_their_group_and_the_pair_returns_with_its_last_mapping(mode):
    t = Pair(PLAIN, MODES[mode])
    reserve(t, 60)
    t.call("map_common_pages", 24)                            # 3 groups aliased into the 4 slots
    pool_after_common = t.p.pm.state()["pool"]
    lens = [0, 0, 0, 0]
    for r in range(4):
        assert t.call("alloc_new_batch_idx", 100)[1] == r
        lens[r] = 100
    t.call("step_async", list(lens))
    for r in range(3):
        p0 = t.p.pm.state()["pool"]
        assert t.call("release_prefix", r, 32) == ("ok", 4)   # 3 shared positions + 1 private one
        assert t.p.pm.state()["pool"] == p0 + 4               # only the private group's 4 pages came back
    p0 = t.p.pm.state()["pool"]
    assert t.call("release_prefix", 3, 32) == ("ok", 4)       # the last holder
    assert t.p.pm.state()["pool"] == p0 + 4 + 3 * 4
    assert pool_after_common + 12 > p0
    t.finish()


# ---------------------------------------------------------------------------------------------------------------------
# traces
# ---------------------------------------------------------------------------------------------------------------------
def run_trace(cfg, flags, seed, release, deferred=True, common=0, iters=70, left=40, chunk=48, pool_groups=150):
    """Engine-shaped workload: admissions, chunked prefill, decode growth, the engine's release rule after every step, random
    extra release_prefix calls (legal and illegal), completions.  release=False: the same calls without release_prefix, against
    the restated reference itself."""
    rng = random.Random(seed)
    B, ctx = cfg["max_batch_size"], cfg["max_context_length"]
    model = None if release else make_model(PageManagerOracle, cfg, shared_page_refcount=True)
    t = Pair(cfg, flags, model)
    t.call("set_deferred_reclamation", deferred)
    reserve(t, pool_groups)
    if common:
        t.call("map_common_pages", common)
    lens = [0] * B
    seqs = {}            # slot -> dict(prompt, total, done = keys cached before this iteration)
    rb = row_bytes(cfg)
    released = dropped = 0
    for it in range(iters):
        for _ in range(rng.randrange(3)):
            if len(seqs) + dropped >= B:
                break
            prompt = rng.randrange(1, 400)
            total = min(ctx, prompt + rng.randrange(1, 80))
            first = min(prompt, chunk)
            r = t.call("alloc_new_batch_idx", first)[1]
            assert r >= 0 and r not in seqs
            seqs[r] = dict(prompt=prompt, total=total, done=0, now=first)
            lens[r] = first
        use_async = rng.random() < 0.7
        # (a small pool may answer "OOM on demand": the model must then say so too, and the state after it is compared like any other)
        t.call("step_async", list(lens)) if use_async else t.call("step", list(lens), rng.random() < 0.5)
        dropped = 0
        if release:
            due = []
            for r, s in sorted(seqs.items()):
                keep = keep_from_prompt(s["done"], left) if s["done"] < s["prompt"] else keep_from_decode(s["now"], left)
                if pages_below(keep, rb, cfg["page_size"]) > t.p.pm.ranges()[r][0]:
                    due.append((r, keep))
            if due and rng.random() < 0.5:                       # the engine's form: one call for the iteration
                n = t.call("release_prefixes", due)[1]
                assert n >= len(due)
                released += n
            else:
                for r, keep in due:
                    n = t.call("release_prefix", r, keep, stream=STREAM if rng.random() < 0.8 else None)[1]
                    assert n > 0
                    released += n
            if rng.random() < 0.3:                              # anything at all: errors and no-ops must agree too
                t.call("release_prefix", rng.randrange(-1, B + 1), rng.randrange(0, 64))
        for r in sorted(seqs):
            s = seqs[r]
            s["done"] = s["now"]
            if s["done"] >= s["total"] or rng.random() < 0.04:
                t.call("free_batch_idx", r, stream=STREAM if rng.random() < 0.7 else None)
                lens[r] = 0
                del seqs[r]
                continue
            s["now"] = min(s["prompt"], s["done"] + chunk) if s["done"] < s["prompt"] else s["done"] + 1
            lens[r] = s["now"]
        if rng.random() < 0.1 and seqs:                          # a slot dropped by the step alone (no free)
            r = rng.choice(sorted(seqs))
            lens[r] = 0
            del seqs[r]
            dropped = 1                                          # still active in the manager until the next step
    t.finish()
    return released


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CONFIGS)
def test_random_traces_equal_the_model_after_every_call(name, mode, seed):
    released = run_trace(CONFIGS[name], MODES[mode], 1000 + seed, release=True, deferred=seed % 2 == 0,
                         common=16 if seed == 3 else 0, pool_groups=150 if seed < 2 else 520)
    assert released > 0


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CONFIGS)
def test_without_the_new_call_the_traces_equal_the_restated_reference(name, mode, seed):
    """Untouched behaviour: the same workloads with release_prefix never called — dumps equal oracle.pagemgr.PageManagerOracle's
    after every call and every slot's first mapped position stays 0 (Pair.check)."""
    run_trace(CONFIGS[name], MODES[mode], 1000 + seed, release=False, deferred=seed % 2 == 0, common=16 if seed == 3 else 0,
              pool_groups=150 if seed < 2 else 520)


def test_scripted_trace_with_every_kind_of_call():
    for mode in MODES:
        t = Pair(STRADDLE, MODES[mode])
        t.call("set_deferred_reclamation", False)
        reserve(t, 100)
        t.call("map_common_pages", 10)
        t.call("alloc_new_batch_idx", 90)
        t.call("alloc_new_batch_idx", 30)
        t.call("step_async", [90, 30, 0, 0])
        t.call("release_prefix", 0, 64)
        t.call("step", [91, 31, 0, 0], True)
        t.call("release_prefix", 1, 30)
        t.call("release_prefix", 0, 91)
        t.call("step_async", [150, 31, 0, 0])
        t.call("free_batch_idx", 1)
        t.call("alloc_new_batch_idx", 20)
        t.call("step_async", [151, 20, 0, 0])
        t.call("release_prefix", 1, 20, stream=None)
        t.call("step_async", [0, 21, 0, 0])
        t.call("free_batch_idx", 1)
        t.call("step", [0, 0, 0, 0], True)
        t.finish()


# ---------------------------------------------------------------------------------------------------------------------
# capacity: the point of it
# ---------------------------------------------------------------------------------------------------------------------
CAP_B, CAP_N, CAP_LEFT, CAP_CHUNK, CAP_POOL = 4, 1024, 128, 32, 200


def capacity_run(mode, release):
    """4 sequences grow to 1024 tokens, 32 per iteration as prompt chunks up to 768 and token by token from there, under a window
    of 128 tokens.  8 tokens per page-group: holding them whole takes 4 * ceil(1024 / 8) = 512 page-groups; the pool has 200, so
    without release the step that takes the sequences past 200 / 4 * 8 = 400 tokens must fail.  With the engine's release rule a
    sequence holds the window, one alignment unit, its chunk and the look-ahead: at most (128 + 64 + 32 + 10) / 8 + 2 < 32 groups,
    128 for the four."""
    assert CAP_B * -(-CAP_N // 8) == 512 > CAP_POOL and CAP_B * 32 < CAP_POOL
    t = Pair(PLAIN, MODES[mode])
    reserve(t, CAP_POOL)
    lens = [0] * CAP_B
    for r in range(CAP_B):
        assert t.call("alloc_new_batch_idx", CAP_CHUNK)[1] == r
    done = 0
    rb = row_bytes(PLAIN)
    while done < CAP_N:
        prompt = done < 768
        now = done + CAP_CHUNK if prompt else done + 1
        lens = [now] * CAP_B
        res = t.call("step_async", lens)
        if res[0] != "ok":
            msg = t.p.pm._lib.vattn_last_error(t.p.pm._h).decode()
            t.p.pm.close()
            return res[0], msg, done
        if release:
            keep = keep_from_prompt(done, CAP_LEFT) if prompt else keep_from_decode(now, CAP_LEFT)
            for r in range(CAP_B):
                if pages_below(keep, rb, PAGE) > t.p.pm.ranges()[r][0]:
                    t.call("release_prefix", r, keep)
        done = now
    peaks = (t.peak_product, t.peak_model)
    for r in range(CAP_B):
        t.call("free_batch_idx", r)
    t.finish()
    return "ok", peaks, done


@pytest.mark.parametrize("mode", MODES)
def test_capacity_a_windowed_batch_that_cannot_be_held_whole_runs_to_the_end(mode):
    kind, msg, at = capacity_run(mode, release=False)
    assert kind == "RuntimeError" and "OOM on demand" in msg and 384 <= at <= 416
    kind, peaks, at = capacity_run(mode, release=True)
    assert kind == "ok" and at == CAP_N
    assert peaks[0] == peaks[1]
    assert peaks[0] <= CAP_B * 32 * 2 * PLAIN["num_layers"]              # physical pages: 4 per page-group


# ---------------------------------------------------------------------------------------------------------------------
# one batch per iteration; layer-ordered steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_release_prefixes_is_one_batch_one_tlb_step_and_all_or_nothing_on_arguments(mode):
    t = Pair(PLAIN, MODES[mode])
    reserve(t, 120)
    for r in range(3):
        t.call("alloc_new_batch_idx", 200)
    t.call("step_async", [200, 200, 200, 0])
    t.p.pm.wait()
    before = (t.p.snapshot(full=True), t.p.pm.ranges())
    c0 = fake_counters()
    assert t.call("release_prefixes", [(0, 64), (3, 0), (1, 64)])[0] == "ValueError"       # slot 3 is inactive: nothing changes
    assert t.call("release_prefixes", [(0, 64), (1, 201)])[0] == "ValueError"
    assert (t.p.snapshot(full=True), t.p.pm.ranges()) == before and fake_counters()["n_unmap"] == c0["n_unmap"]
    f0 = fake().vattn_fake_fence_wait_count()
    assert t.call("release_prefixes", [(0, 64), (1, 128), (2, 7)]) == ("ok", 8 + 16)
    t.p.pm.wait()
    c1 = fake_counters()
    assert c1["n_flush"] == c0["n_flush"] + 1                                               # ONE TLB step for the three slots
    assert c1["n_unmap"] == c0["n_unmap"] + 24 * 2 * PLAIN["num_layers"]
    assert fake().vattn_fake_fence_wait_count() == f0 + 2                                   # one wait per slot that released
    assert t.call("release_prefixes", []) == ("ok", 0)
    assert t.p.pm.stats()["prefix_releases"] == 2
    t.finish()


def test_release_reaching_positions_whose_later_layers_are_still_queued():
    """Layer-ordered step: layers [2, 4) of the new prompt's pages are mapped by the mapper thread after step_async has returned.  A
    release up to the slot's length reaches those positions: it must come after their maps (it joins), never before."""
    t = Pair(DEEP, MODES["layered"])
    reserve(t, 120)
    t.call("alloc_new_batch_idx", 300)
    t.call("step_async", [300, 0, 0, 0])
    assert t.p.pm.stats()["layered_batches"] == 1
    assert t.call("release_prefix", 0, 300) == ("ok", 300 * 512 // PAGE)
    t.call("step_async", [301, 0, 0, 0])
    t.finish()


@pytest.mark.parametrize("drop_hole_slot", [False, True], ids=["no_hole_dropped", "hole_slot_dropped"])
@pytest.mark.parametrize("fail_after", [10, 150], ids=["fails_in_sync_layers", "fails_on_the_mapper"])
def test_failed_map_in_a_layer_ordered_step_is_rolled_back_with_and_without_a_dropped_hole(fail_after, drop_hole_slot):
    """A hipMemMap that fails in a layer-ordered step_async: the whole step's page-groups are taken back, the unmaps of a slot
    with a hole that the same step dropped still run, and driver state equals bookkeeping equals the model."""
    t = Pair(DEEP, MODES["layered"])
    reserve(t, 200)
    t.call("alloc_new_batch_idx", 200)
    t.call("alloc_new_batch_idx", 100)
    t.call("step_async", [200, 100, 0, 0])
    assert t.call("release_prefix", 0, 128) == ("ok", 16)
    assert t.call("alloc_new_batch_idx", 240) == ("ok", 2)
    t.p.pm.wait()
    lens = [0 if drop_hole_slot else 200, 100, 240, 0]              # slot 2: 30 groups x 4 layers x 2 = 240 maps, 120 of them synchronous
    fake().vattn_fake_fail_map_after(fail_after)
    failed = False
    try:
        t.p.pm.step_async(lens)
        t.p.pm.wait()
    except RuntimeError:
        failed = True
    fake().vattn_fake_fail_map_after((1 << 64) - 1)
    try:
        t.p.pm.wait()
    except RuntimeError:
        failed = True
    assert failed
    # the model: the step took the lengths over and closed the dropped slot's hole, and mapped nothing for slot 2
    m = t.m
    m._before_step(lens)
    m.curr_seq_lengths = list(lens)

    def consistent():
        st = t.p.pm.state()
        assert st["lens"] == m.curr_seq_lengths
        assert t.p.pm.ranges() == m.ranges()
        assert t.p.mapped_ranges() == m.mapped_ranges()                 # driver state == model
        rows = t.p.pm.pagemap()
        assert {(r[0], r[1], r[2]) for r in rows} == set(m.pagemap)
        in_use = [x for r in rows for x in r[3:5]]
        assert len(st["pool_ids"]) == len(set(st["pool_ids"])) == len(m.pool)      # no page twice in the pool
        assert not set(st["pool_ids"]) & set(in_use) and len(in_use) == len(set(in_use))
        c = fake_counters()
        assert c["violations"] == 0 and c["stale_vas"] == 0
        assert c["mapped_pages"] == t.p.pm.stats()["pages_mapped_now"] == len(m.mapped_ranges())
    consistent()
    assert t.p.pm.ranges()[2] == (0, 0)
    if drop_hole_slot:
        assert t.p.pm.ranges()[0] == (0, 0)
    # the manager stays usable: the same step now succeeds
    t.p.pm.step_async(lens)
    m.step_async(lens)
    consistent()
    t.p.pm.cleanup()
    c = fake_counters()
    assert c["violations"] == 0 and c["mapped_pages"] == 0 and c["live_handles"] == 0
    t.p.pm.close()
