#!/usr/bin/env python3
"""Kernel microbenchmark (GPU): times the attention kernels through the C ABI with HIP events
(vattn_time_attn) on the shapes of BASELINE.md §3 and prints TFLOP/s / GB/s against the rooflines.
usage: python tools/kbench.py [prefill] [decode] [--variant N]
       python tools/kbench.py multitoken --mt B,sq,Hq,Hkv,ctx[,ragged] [--mt ...] [--base LIB] [--bf16] [--tree]   (the multi-token decode form;
                                                                          --tree: the tree-masked entry with a chain mask beside the causal call)
       python tools/kbench.py decode --kv-fp8 [--only NAMES] / multitoken --kv-fp8 --mt ...   (the same call over an fp8 (e4m3) cache —
                                                                          vattn_fp8kv_attn_with_kvcache — beside the 2-byte call, alternating, over rotating caches)
       python tools/kbench.py prefill --kv-fp8 [--only NAMES] [--bf16]   (a chunk on a prefix through vattn_fp8kv_prefill_with_kvcache beside the 2-byte call
                                                                          forced to the same tiling and split, and the 2-byte call under its default plan)
       python tools/kbench.py decode --softcap X [--only NAMES] / multitoken --softcap X --mt ... / prefill --softcap X [--only NAMES]   (the call with logit
                                                                          soft-capping — vattn_softcap_attn_with_kvcache — beside the plain call, alternating, over rotating
                                                                          caches; prefill: beside the plain call on the SAME tiling and split, and under its default plan)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vattention_amd import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")


def params(q, kc, vc, cl, idx=None, kn=None, vn=None, causal=True, splits=0, variant=0, ws=None):
    out = torch.empty_like(q)
    p = K.AttnParams()
    p.q, p.out = q.data_ptr(), out.data_ptr()
    p.q_batch_stride, p.q_row_stride, p.q_head_stride = q.stride(0), q.stride(1), q.stride(2)
    p.o_batch_stride, p.o_row_stride, p.o_head_stride = out.stride(0), out.stride(1), out.stride(2)
    p.k_cache, p.v_cache = kc.data_ptr(), vc.data_ptr()
    p.k_batch_stride, p.k_row_stride, p.k_head_stride = kc.stride(0), kc.stride(1), kc.stride(2)
    p.v_batch_stride, p.v_row_stride, p.v_head_stride = vc.stride(0), vc.stride(1), vc.stride(2)
    if kn is not None:
        p.k_new, p.v_new = kn.data_ptr(), vn.data_ptr()
        p.knew_batch_stride, p.knew_row_stride, p.knew_head_stride = kn.stride(0), kn.stride(1), kn.stride(2)
        p.vnew_batch_stride, p.vnew_row_stride, p.vnew_head_stride = vn.stride(0), vn.stride(1), vn.stride(2)
        p.seqlen_knew = kn.shape[1]
    p.cache_seqlens = cl.data_ptr()
    p.cache_batch_idx = idx.data_ptr() if idx is not None else None
    p.b, p.seqlen_q, p.h, p.d = q.shape[0], q.shape[1], q.shape[2], q.shape[3]
    p.seqlen_k, p.h_k = kc.shape[1], kc.shape[2]
    p.is_causal, p.dtype, p.num_splits, p.softmax_scale, p.variant = int(causal), (1 if q.dtype == torch.bfloat16 else 0), splits, q.shape[3] ** -0.5, variant
    p.max_seqlen_k_hint = kc.shape[1]        # the benchmark caches are exactly as long as the sequences
    p.split_reserved = int(os.environ.get("KBENCH_SWITCH_TILES", "-1")) + 1      # stream decode: switch allowance override (tuning)
    p.split_reserved |= int(os.environ.get("KBENCH_LAB_SUB", "0")) << 16         # lab builds: sub-selector (prefill64 round-6 price list)
    keep = [out, q, kc, vc, cl, idx, kn, vn]
    need = K.klib_for(p.variant).vattn_attn_workspace_bytes(C.byref(p))
    if need:
        w = torch.empty(need // 4 + 1, dtype=torch.float32, device=DEV)
        p.workspace = w.data_ptr()
        keep.append(w)
    return p, keep


def time_ms(p, warmup=2, iters=5):
    lib = K.klib_for(p.variant)       # product library unless the variant names a lab build
    ms = lib.vattn_time_attn(C.byref(p), torch.cuda.current_stream().cuda_stream, warmup, iters)
    if ms < 0:
        raise RuntimeError(K.last_error(lib))
    return ms


def prefill(variant):
    print("== prefill (causal chunk n against c cached), %s, D=128 ==" % ("bf16" if DTYPE == torch.bfloat16 else "fp16"))
    for name, Hq, Hkv, n, c in [("yi6b whole", 32, 4, 32702, 0), ("yi6b chunk4k@28k", 32, 4, 4096, 28672), ("yi6b chunk4k@0", 32, 4, 4096, 0),
                                ("llama8b 16k", 32, 8, 16384, 0), ("yi34b/tp2 chunk16k@112k", 28, 4, 16384, 114688),
                                ("llama70b/tp8 8k", 8, 1, 8192, 0), ("small 2k", 32, 4, 2048, 0),
                                ("llama70b/tp8 chunk2k@30k", 8, 1, 2048, 30720), ("llama70b/tp8 chunk512@16k", 8, 1, 512, 15872),
                                ("yi34b/tp2 chunk1k@64k", 28, 4, 1024, 64512), ("llama70b/tp8 4k", 8, 1, 4096, 0),
                                ("llama70b/tp8 2k", 8, 1, 2048, 0), ("llama8b chunk512@8k", 32, 8, 512, 7680)]:
        if ONLY and not any(o in name for o in ONLY.split(",")):
            continue
        torch.manual_seed(0)
        q = torch.randn(1, n, Hq, 128, device=DEV, dtype=DTYPE)
        kc = torch.randn(1, c + n, Hkv, 128, device=DEV, dtype=DTYPE)
        vc = torch.randn(1, c + n, Hkv, 128, device=DEV, dtype=DTYPE)
        scale = float(os.environ.get("KBENCH_DATA_SCALE", "1"))     # 0 = zero-filled inputs (data-dependent power: clocks rise)
        if scale != 1.0:
            q, kc, vc = q * scale, kc * scale, vc * scale
        if os.environ.get("KBENCH_DATA_STYLE") == "same_token":
            # what the reference's own benchmark feeds its kernels: prompt ids [1]*n through random-init weights
            # (scripts/benchmark_e2e_static_trace.py) -> every position carries the SAME hidden state, so v rows are identical and
            # q / k rows are RoPE rotations of one vector per head
            def rope(x, pos0):
                T, H, Dh = x.shape[1], x.shape[2], x.shape[3]
                pos = torch.arange(pos0, pos0 + T, device=DEV, dtype=torch.float32)[:, None]
                inv = 10000.0 ** (-torch.arange(0, Dh, 2, device=DEV, dtype=torch.float32) / Dh)
                ang = pos * inv[None, :]
                cos, sin = ang.cos()[None, :, None, :], ang.sin()[None, :, None, :]
                x = x.float()
                x1, x2 = x[..., 0::2], x[..., 1::2]
                o = torch.empty_like(x)
                o[..., 0::2] = x1 * cos - x2 * sin
                o[..., 1::2] = x1 * sin + x2 * cos
                return o.to(DTYPE)
            q = rope(q[:, :1].expand(-1, n, -1, -1).contiguous(), c)
            kc = rope(kc[:, :1].expand(-1, c + n, -1, -1).contiguous(), 0)
            vc = vc[:, :1].expand(-1, c + n, -1, -1).contiguous()
        cl = torch.tensor([c + n], dtype=torch.int32, device=DEV)
        p, keep = params(q, kc, vc, cl, variant=variant, splits=PF_SPLITS)
        tag = ""
        if WORKLIST:          # host-planned work list (vattn_prefill_plan) where the planner wants one
            from vattention_amd import flash_attn as FA
            pl = FA.prefill_plan(p, [n], [c + n], DEV, force_tiles=WL_TILES, persistent=PERSIST, drawn=DRAWN)
            if pl.t is not None:
                pl.attach(p)
                need = K.klib().vattn_attn_workspace_bytes(C.byref(p))
                w = torch.empty(need // 4 + 1, dtype=torch.float32, device=DEV)
                p.workspace = w.data_ptr()
                keep += [pl, w]
                tag = "  [work list: %d pieces, %d split blocks%s]" % (pl.n_items, pl.n_blocks, ", %d persistent workgroups" % pl.n_wg if pl.n_wg else ", one workgroup per piece")
        ms = time_ms(p, 1, 3 if n > 10000 else 10)
        fl = 4.0 * Hq * 128 * (n * c + n * (n + 1) / 2)
        print("  %-26s n=%6d c=%6d Hq=%2d Hkv=%d : %9.3f ms  %8.1f TFLOP/s  (%.1f%% of 2500)%s" % (name, n, c, Hq, Hkv, ms, fl / ms / 1e9, fl / ms / 1e9 / 25, tag))
        del keep


def decode(variant):
    print("== decode (Sq=1, append + split-KV + combine), %s, D=128 ==" % ("bf16" if DTYPE == torch.bfloat16 else "fp16"))
    for name, Hq, Hkv, B, ctx, slots in [("yi6b B16@32k", 32, 4, 16, 32768, 16), ("yi6b B1@32k", 32, 4, 1, 32768, 4), ("yi6b B4@32k", 32, 4, 4, 32768, 4),
                                         ("yi6b B2@32k", 32, 4, 2, 32768, 4), ("yi6b B8@32k", 32, 4, 8, 32768, 8),
                                         ("yi6b B1@8k", 32, 4, 1, 8192, 4), ("yi6b B1@2k", 32, 4, 1, 2048, 4), ("yi6b B16@2k", 32, 4, 16, 2048, 16),
                                         ("llama8b B64@8k", 32, 8, 64, 8192, 64), ("llama8b B256@2k", 32, 8, 256, 2048, 256),
                                         ("llama70b/tp8 B64@32k", 8, 1, 64, 32768, 64), ("yi34b/tp2 B8@128k", 28, 4, 8, 131072, 8),
                                         ("yi34b/tp2 B1@128k", 28, 4, 1, 131072, 2), ("yi34b/tp4 B1@128k", 14, 2, 1, 131072, 2),
                                         ("mqa G32 B16@16k", 32, 1, 16, 16384, 16), ("gqa G32x4 B8@16k", 128, 4, 8, 16384, 8),
                                         ("mqa G64 B16@8k", 64, 1, 16, 8192, 16)]:
        if ONLY and not any(o.strip() in name for o in ONLY.split(",")):
            continue
        torch.manual_seed(0)
        q = torch.randn(B, 1, Hq, 128, device=DEV, dtype=DTYPE)
        if MEGA > 1:      # megacache layout [slots, ctx, L, Hkv, D]: one layer's view has a row stride of L x Hkv x D elements
            kc = torch.randn(slots, ctx, MEGA, Hkv, 128, device=DEV, dtype=DTYPE)[:, :, MEGA // 2]
            vc = torch.randn(slots, ctx, MEGA, Hkv, 128, device=DEV, dtype=DTYPE)[:, :, MEGA // 2]
        else:
            kc = torch.randn(slots, ctx, Hkv, 128, device=DEV, dtype=DTYPE)
            vc = torch.randn(slots, ctx, Hkv, 128, device=DEV, dtype=DTYPE)
        kn = torch.randn(B, 1, Hkv, 128, device=DEV, dtype=DTYPE)
        vn = torch.randn(B, 1, Hkv, 128, device=DEV, dtype=DTYPE)
        cl = torch.full((B,), ctx - 1, dtype=torch.int32, device=DEV)
        idx = torch.arange(B, dtype=torch.int32, device=DEV) % slots
        for splits in SPLITS:
            p, keep = params(q, kc, vc, cl, idx, kn, vn, splits=splits, variant=variant)
            if ROTATE:
                # launches of one shape over R different caches in turn, R x bytes >= 1.5 GB: nothing is served from the 256 MiB
                # Infinity Cache (a small launch repeated on ONE cache is: B1 @ 128 k reads 52 us that way and 63 us in a real model,
                # whose 60 layers each own their K/V)
                by1 = B * 2.0 * ctx * Hkv * 128 * 2
                R = max(2, int(1.5e9 // by1) + 1)
                ps = [(p, keep)]
                for _ in range(R - 1):
                    kc2, vc2 = torch.randn_like(kc), torch.randn_like(vc)
                    ps.append(params(q, kc2, vc2, cl, idx, kn, vn, splits=splits, variant=variant))
                lib = K.klib_for(p.variant)
                st = torch.cuda.current_stream().cuda_stream
                for pp, _k in ps:
                    lib.vattn_flash_attn_with_kvcache(C.byref(pp), st)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                iters = max(2, 40 // R + 1)
                e0.record()
                for _ in range(iters):
                    for pp, _k in ps:
                        lib.vattn_flash_attn_with_kvcache(C.byref(pp), st)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / (iters * R)
                del ps
            else:
                ms = time_ms(p, 3, 20)
            by = B * 2.0 * ctx * Hkv * 128 * 2 + B * Hq * 128 * 2 * 2
            print("  %-22s B=%3d ctx=%6d Hq=%2d Hkv=%d splits=%d : %8.4f ms  %7.1f GB/s  (%.1f%% of 8000, %.1f%% of 6290)" % (
                name, B, ctx, Hq, Hkv, splits, ms, by / ms / 1e6, by / ms / 1e6 / 80, by / ms / 1e6 / 62.9))
        del keep, kc, vc


def fp8_ab(name, B, sq, Hq, Hkv, ctx, slots, ragged=False):
    """--kv-fp8: the call (q [B, sq, Hq, 128], sq new rows appended at ctx - sq) over a 2-byte cache and over an fp8 (e4m3) cache of the same
    values (quantised with per-head amax scales by vattn_cache_flat_fp8), ALTERNATING in one process, each over R caches in turn with
    R x bytes >= 1.5 GB of the 2-byte caches (nothing is served from the 256 MiB Infinity Cache; the same R for both), warmed up, five
    windows each; HIP events around each window.  Bytes = the K/V rows read + q and out, per cache dtype."""
    from vattention_amd.cache_ops import cache_flat_fp8
    torch.manual_seed(0)
    lib, st = K.klib(), torch.cuda.current_stream().cuda_stream
    by16 = B * 2.0 * ctx * Hkv * 128 * 2
    R = max(2, int(1.5e9 // by16) + 1)
    lens = [ctx - sq - (i * 7919 % (ctx - ctx // 8)) for i in range(B)] if ragged else [ctx - sq] * B
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    idx = torch.arange(B, dtype=torch.int32, device=DEV) % slots
    q = torch.randn(B, sq, Hq, 128, device=DEV, dtype=DTYPE)
    kn, vn = torch.randn(B, sq, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(B, sq, Hkv, 128, device=DEV, dtype=DTYPE)
    ks = torch.full((Hkv,), 6.0 / 448.0, dtype=torch.float32, device=DEV)       # N(0,1) data: amax over 10^8 samples is below 6
    vs = ks.clone()
    p16, p8 = [], []
    for _ in range(R):
        kc, vc = torch.randn(slots, ctx, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(slots, ctx, Hkv, 128, device=DEV, dtype=DTYPE)
        k8, v8 = torch.empty(slots, ctx, Hkv, 128, device=DEV, dtype=torch.float8_e4m3fn), torch.empty(slots, ctx, Hkv, 128, device=DEV, dtype=torch.float8_e4m3fn)
        cache_flat_fp8(kc.view(-1, Hkv, 128), vc.view(-1, Hkv, 128), k8.view(-1, Hkv, 128), v8.view(-1, Hkv, 128), ks, vs)
        p16.append(params(q, kc, vc, cl, idx, kn, vn))
        p8.append(params(q, k8, v8, cl, idx, kn, vn))          # (the workspace need is the 2-byte call's: the same planners)
    d = K.describe_fp8kv(p8[0][0])
    assert d == K.describe(p16[0][0])
    call16 = lambda pp: lib.vattn_flash_attn_with_kvcache(C.byref(pp), st)
    call8 = lambda pp: lib.vattn_fp8kv_attn_with_kvcache(C.byref(pp), ks.data_ptr(), vs.data_ptr(), st)
    iters = max(2, 60 // R + 1)

    def window(call, ps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            for pp, _k in ps:
                if call(pp) != 0:
                    raise RuntimeError(K.last_error(lib))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (iters * len(ps)) * 1e3
    for call, ps in ((call16, p16), (call8, p8)):              # warm-up: every cache of both
        window(call, ps)
    t16, t8 = [], []
    for _rep in range(5):                                       # alternating windows
        t16.append(window(call16, p16))
        t8.append(window(call8, p8))
    vis = sum(n + sq for n in lens)
    b16 = vis * 2.0 * Hkv * 128 * 2 + 2.0 * B * sq * Hq * 128 * 2
    b8 = vis * 2.0 * Hkv * 128 * 1 + 2.0 * B * sq * Hq * 128 * 2
    m16, m8 = sorted(t16)[2], sorted(t8)[2]
    print("  %-22s B=%3d sq=%d ctx=%6d Hq=%2d Hkv=%d  path %d tiling %d wg %d, %d rotating caches" % (name, B, sq, ctx, Hq, Hkv, d["path"], d["tiling"], d["workgroups"], R))
    print("    2-byte cache : median %8.1f us  (5 windows: %s)  %7.1f GB/s = %.1f%% of 8000, %.1f%% of the 6290 GB/s read stream" % (
        m16, " ".join("%.1f" % x for x in t16), b16 / m16 / 1e3, b16 / m16 / 1e3 / 80, b16 / m16 / 1e3 / 62.9))
    print("    fp8 cache    : median %8.1f us  (5 windows: %s)  %7.1f GB/s = %.1f%% of 8000, %.1f%% of the 6290 GB/s read stream" % (
        m8, " ".join("%.1f" % x for x in t8), b8 / m8 / 1e3, b8 / m8 / 1e3 / 80, b8 / m8 / 1e3 / 62.9))
    print("    ratio 2-byte / fp8 : %.2fx" % (m16 / m8), flush=True)


def fp8_tree_ab(B, sq, Hq, Hkv, ctx, ragged=False):
    """multitoken --kv-fp8 --tree: ONE block (q [B, sq, Hq, 128], the sq draft rows appended at ctx - sq) through four entry points, ALTERNATING
    in one process over the same R rotating caches (R x the 2-byte K/V bytes >= 1.5 GB), warmed up, five windows each, HIP events around each
    window: (a) vattn_fp8kv_tree_attn_with_kvcache with a CHAIN mask, (b) vattn_fp8kv_attn_with_kvcache, causal — the same visibility: what the
    mask costs on fp8; (c) vattn_tree_attn_with_kvcache with the chain mask over the 2-byte caches — what fp8 saves on a tree; (d) the causal
    2-byte multi-token call.  sq = 7: also the 7-node, 3-leaf tree 0-1-{3,4}, 0-2-5-6 through both tree entries."""
    from vattention_amd.cache_ops import cache_flat_fp8
    torch.manual_seed(0)
    lib, st = K.klib(), torch.cuda.current_stream().cuda_stream
    by16 = B * 2.0 * ctx * Hkv * 128 * 2
    R = max(2, int(1.5e9 // by16) + 1)
    lens = [ctx - sq - (i * 7919 % (ctx - ctx // 8)) for i in range(B)] if ragged else [ctx - sq] * B
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    q = torch.randn(B, sq, Hq, 128, device=DEV, dtype=DTYPE)
    kn, vn = torch.randn(B, sq, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(B, sq, Hkv, 128, device=DEV, dtype=DTYPE)
    ks = torch.full((Hkv,), 6.0 / 448.0, dtype=torch.float32, device=DEV)       # N(0,1) data: amax over 10^8 samples is below 6
    vs = ks.clone()
    words = lambda w: torch.tensor(w, dtype=torch.int32, device=DEV).expand(B, sq).contiguous()
    chain = words([(2 << t) - 1 for t in range(sq)])
    p16, p8 = [], []
    for _ in range(R):
        kc, vc = torch.randn(B, ctx, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(B, ctx, Hkv, 128, device=DEV, dtype=DTYPE)
        k8, v8 = torch.empty(B, ctx, Hkv, 128, device=DEV, dtype=torch.float8_e4m3fn), torch.empty(B, ctx, Hkv, 128, device=DEV, dtype=torch.float8_e4m3fn)
        cache_flat_fp8(kc.view(-1, Hkv, 128), vc.view(-1, Hkv, 128), k8.view(-1, Hkv, 128), v8.view(-1, Hkv, 128), ks, vs)
        p16.append(params(q, kc, vc, cl, idx, kn, vn))
        p8.append(params(q, k8, v8, cl, idx, kn, vn))          # (the workspace need is the 2-byte call's: the same planners)
    d = K.describe_fp8kv_tree(p8[0][0])
    assert d == K.describe_tree(p16[0][0]) == K.describe(p16[0][0]) and d["form"] == 1, d
    ksp, vsp = ks.data_ptr(), vs.data_ptr()
    runs = [("(a) fp8 tree entry, chain mask ", lambda pp: lib.vattn_fp8kv_tree_attn_with_kvcache(C.byref(pp), chain.data_ptr(), ksp, vsp, st), p8, 1),
            ("(b) fp8 causal multi-token call", lambda pp: lib.vattn_fp8kv_attn_with_kvcache(C.byref(pp), ksp, vsp, st), p8, 1),
            ("(c) 2-byte tree entry, chain   ", lambda pp: lib.vattn_tree_attn_with_kvcache(C.byref(pp), chain.data_ptr(), st), p16, 2),
            ("(d) 2-byte causal multi-token  ", lambda pp: lib.vattn_flash_attn_with_kvcache(C.byref(pp), st), p16, 2)]
    if sq == 7:
        leaf3 = words([0b1, 0b11, 0b101, 0b1011, 0b10011, 0b100101, 0b1100101])
        runs += [("(e) fp8 tree entry, 3-leaf tree", lambda pp: lib.vattn_fp8kv_tree_attn_with_kvcache(C.byref(pp), leaf3.data_ptr(), ksp, vsp, st), p8, 1),
                 ("(f) 2-byte tree entry, 3-leaf  ", lambda pp: lib.vattn_tree_attn_with_kvcache(C.byref(pp), leaf3.data_ptr(), st), p16, 2)]
    runs.append(("(b') the call of (b) again     ", runs[1][1], p8, 1))      # the same code twice: what two lines of this table differ by on their own
    iters = max(2, 400 // R + 1)                                # (windows of ~0.1 s)

    def window(call, ps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            for pp, _k in ps:
                if call(pp) != 0:
                    raise RuntimeError(K.last_error(lib))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (iters * len(ps)) * 1e3
    for _n, call, ps, _e in runs:                               # warm-up: every cache of every run
        window(call, ps)
    t = [[] for _ in runs]
    for _rep in range(5):                                       # alternating windows
        for i, (_n, call, ps, _e) in enumerate(runs):
            t[i].append(window(call, ps))
    med = [sorted(x)[2] for x in t]
    vis = sum(n + sq for n in lens)
    print("  B=%3d sq=%d ctx=%6d%s Hq=%2d Hkv=%d %s  path %d tiling %d wg %d, %d rotating caches" % (
        B, sq, ctx, " ragged" if ragged else "", Hq, Hkv, "bf16" if DTYPE == torch.bfloat16 else "fp16", d["path"], d["tiling"], d["workgroups"], R))
    for (name, _c, _p, esz), m, x in zip(runs, med, t):
        by = vis * 2.0 * Hkv * 128 * esz + 2.0 * B * sq * Hq * 128 * 2
        print("    %s : median %8.1f us  (5 windows: %s; spread %.1f%%)  %7.1f GB/s = %.1f%% of the 6290 GB/s read stream" % (
            name, m, " ".join("%.1f" % y for y in x), 100.0 * (max(x) - min(x)) / m, by / m / 1e3, by / m / 1e3 / 62.9))
    print("    ratios: (a) / (b) = %.3f [the mask on fp8]   (b') / (b) = %.3f [the same call twice]   (c) / (a) = %.2fx [fp8 on a tree]   (d) / (b) = %.2fx [fp8 on the causal call]   (c) / (d) = %.3f%s" % (
        med[0] / med[1], med[-1] / med[1], med[2] / med[0], med[3] / med[1], med[2] / med[3],
        "   (e) / (a) = %.3f   (f) / (e) = %.2fx" % (med[4] / med[0], med[5] / med[4]) if sq == 7 else ""), flush=True)


def fp8_prefill_ab(name, Hq, Hkv, n, c):
    """prefill --kv-fp8: ONE block — a causal chunk of n rows whose keys [0, c + n) are in the cache — timed three ways, ALTERNATING in one
    process over R rotating caches (R x the 2-byte K/V bytes beyond the 256 MiB Infinity Cache, at most 24), warmed up, five windows each:
    (a) vattn_fp8kv_prefill_with_kvcache over an fp8 (e4m3) cache of the same values; (b) the 2-byte call FORCED to (a)'s tiling and split
    count — the yardstick of the fp8 builds: the same grid, the same kernel but for the staging; (c) the 2-byte call under its default plan
    (prefill64 where the planner takes it): what a caller pays for prefill64 having no fp8 build."""
    from vattention_amd.cache_ops import cache_flat_fp8
    torch.manual_seed(0)
    lib, st = K.klib(), torch.cuda.current_stream().cuda_stream
    rows = c + n
    by16 = 2.0 * rows * Hkv * 128 * 2
    R = min(24, max(2, int(1.5e9 // by16) + 1))
    cl = torch.tensor([rows], dtype=torch.int32, device=DEV)
    q = torch.randn(1, n, Hq, 128, device=DEV, dtype=DTYPE)
    ks = torch.full((Hkv,), 6.0 / 448.0, dtype=torch.float32, device=DEV)       # N(0,1) data: amax over 10^8 samples is below 6
    vs = ks.clone()
    pa, pb, pc = [], [], []
    for _ in range(R):
        kc, vc = torch.randn(1, rows, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(1, rows, Hkv, 128, device=DEV, dtype=DTYPE)
        k8, v8 = torch.empty(1, rows, Hkv, 128, device=DEV, dtype=torch.float8_e4m3fn), torch.empty(1, rows, Hkv, 128, device=DEV, dtype=torch.float8_e4m3fn)
        cache_flat_fp8(kc.view(-1, Hkv, 128), vc.view(-1, Hkv, 128), k8.view(-1, Hkv, 128), v8.view(-1, Hkv, 128), ks, vs)
        p8, keep = params(q, k8, v8, cl)
        da = K.describe_fp8kv_prefill(p8)
        w = torch.empty(da["workspace_bytes"] // 4 + 1, dtype=torch.float32, device=DEV)      # (this call's own need: its plan has no prefill64)
        p8.workspace = w.data_ptr()
        pa.append((p8, keep + [w]))
        pb.append(params(q, kc, vc, cl, splits=da["nsplit"], variant=da["tiling"] << 1))
        pc.append(params(q, kc, vc, cl))
    db, dc = K.describe(pb[0][0]), K.describe(pc[0][0])
    assert (db["tiling"], db["nsplit"], db["workgroups"]) == (da["tiling"], da["nsplit"], da["workgroups"]), (da, db)
    call16 = lambda pp: lib.vattn_flash_attn_with_kvcache(C.byref(pp), st)
    call8 = lambda pp: lib.vattn_fp8kv_prefill_with_kvcache(C.byref(pp), ks.data_ptr(), vs.data_ptr(), st)
    iters = max(1, 24 // R)

    def window(call, ps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            for pp, _k in ps:
                if call(pp) != 0:
                    raise RuntimeError(K.last_error(lib))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (iters * len(ps)) * 1e3
    runs = ((call8, pa), (call16, pb), (call16, pc))
    for call, ps in runs:                                       # warm-up: every cache of all three
        window(call, ps)
    t = [[], [], []]
    for _rep in range(5):                                       # alternating windows
        for i, (call, ps) in enumerate(runs):
            t[i].append(window(call, ps))
    med = [sorted(x)[2] for x in t]
    fl = 4.0 * Hq * 128 * (n * c + n * (n + 1) / 2)
    print("  %-26s n=%d c=%d Hq=%2d Hkv=%d, %s, %d rotating caches" % (name, n, c, Hq, Hkv, "bf16" if DTYPE == torch.bfloat16 else "fp16", R))
    for tag, d, m, x in (("(a) fp8 cache            ", da, med[0], t[0]), ("(b) 2-byte, (a)'s plan   ", db, med[1], t[1]), ("(c) 2-byte, default plan ", dc, med[2], t[2])):
        print("    %s tiling %d nsplit %d wg %4d : median %8.1f us  (5 windows: %s; spread %.1f%%)  %7.1f TFLOP/s" % (
            tag, d["tiling"], d["nsplit"], d["workgroups"], m, " ".join("%.1f" % y for y in x), 100.0 * (max(x) - min(x)) / m, fl / m / 1e6))
    print("    ratios: (a) / (b) = %.3f   (a) / (c) = %.3f   (b) / (c) = %.3f" % (med[0] / med[1], med[0] / med[2], med[1] / med[2]), flush=True)


def _ab_windows(runs, iters, lib):
    """median and the five alternating windows (us per call) of every (call, blocks) pair of `runs`, after one warm-up window each"""
    def window(call, ps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            for pp, _k in ps:
                if call(pp) != 0:
                    raise RuntimeError(K.last_error(lib))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (iters * len(ps)) * 1e3
    for call, ps in runs:
        window(call, ps)
    t = [[] for _ in runs]
    for _rep in range(5):
        for i, (call, ps) in enumerate(runs):
            t[i].append(window(call, ps))
    return [sorted(x)[2] for x in t], t


def softcap_ab(name, B, sq, Hq, Hkv, ctx, cap, ragged=False):
    """--softcap X (decode, multitoken): ONE block (q [B, sq, Hq, 128], sq new rows appended at ctx - sq) through vattn_flash_attn_with_kvcache
    and through vattn_softcap_attn_with_kvcache(softcap = X), ALTERNATING in one process over the same R rotating caches (R x bytes >= 1.5 GB:
    nothing is served from the 256 MiB Infinity Cache), warmed up, five windows each.  The plan is the same by construction (asserted)."""
    torch.manual_seed(0)
    lib, st = K.klib(), torch.cuda.current_stream().cuda_stream
    by16 = B * 2.0 * ctx * Hkv * 128 * 2
    R = max(2, int(1.5e9 // by16) + 1)
    lens = [ctx - sq - (i * 7919 % (ctx - ctx // 8)) for i in range(B)] if ragged else [ctx - sq] * B
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    q = torch.randn(B, sq, Hq, 128, device=DEV, dtype=DTYPE)
    kn, vn = torch.randn(B, sq, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(B, sq, Hkv, 128, device=DEV, dtype=DTYPE)
    ps = []
    for _ in range(R):
        kc, vc = torch.randn(B, ctx, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(B, ctx, Hkv, 128, device=DEV, dtype=DTYPE)
        ps.append(params(q, kc, vc, cl, idx, kn, vn))
    d = K.describe_softcap(ps[0][0], cap)
    assert d == K.describe(ps[0][0])
    plain = lambda pp: lib.vattn_flash_attn_with_kvcache(C.byref(pp), st)
    capped = lambda pp: lib.vattn_softcap_attn_with_kvcache(C.byref(pp), cap, st)
    med, t = _ab_windows(((plain, ps), (capped, ps)), max(2, 60 // R + 1), lib)
    by = sum(n + sq for n in lens) * 2.0 * Hkv * 128 * 2 + 2.0 * B * sq * Hq * 128 * 2
    print("  %-22s B=%3d sq=%d ctx=%6d Hq=%2d Hkv=%d%s  path %d tiling %d wg %d, %d rotating caches" % (name, B, sq, ctx, Hq, Hkv, " ragged" if ragged else "", d["path"], d["tiling"], d["workgroups"], R))
    for tag, m, x in (("plain        ", med[0], t[0]), ("softcap %-5g" % cap, med[1], t[1])):
        print("    %s: median %8.1f us  (5 windows: %s; spread %.1f%%)  %7.1f GB/s = %.1f%% of 8000" % (
            tag, m, " ".join("%.1f" % y for y in x), 100.0 * (max(x) - min(x)) / m, by / m / 1e3, by / m / 1e3 / 80))
    print("    ratio softcap / plain : %.3f" % (med[1] / med[0]), flush=True)


def softcap_prefill_ab(name, Hq, Hkv, n, c, cap):
    """prefill --softcap X: ONE block — a causal chunk of n rows whose keys [0, c + n) are in the cache — timed three ways, ALTERNATING in one
    process over R rotating caches, warmed up, five windows each: (a) vattn_softcap_attn_with_kvcache; (b) the plain call FORCED to (a)'s
    tiling and split count — the yardstick of the softcap builds: the same grid, the same kernel but for the tanh; (c) the plain call under
    its default plan (prefill64 where the planner takes it): what a caller pays for prefill64 having no softcap build."""
    torch.manual_seed(0)
    lib, st = K.klib(), torch.cuda.current_stream().cuda_stream
    rows = c + n
    R = min(24, max(2, int(1.5e9 // (2.0 * rows * Hkv * 128 * 2)) + 1))
    cl = torch.tensor([rows], dtype=torch.int32, device=DEV)
    q = torch.randn(1, n, Hq, 128, device=DEV, dtype=DTYPE)
    pa, pb, pc = [], [], []
    for _ in range(R):
        kc, vc = torch.randn(1, rows, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(1, rows, Hkv, 128, device=DEV, dtype=DTYPE)
        p, keep = params(q, kc, vc, cl)
        da = K.describe_softcap(p, cap)
        w = torch.empty(da["workspace_bytes"] // 4 + 1, dtype=torch.float32, device=DEV)      # (this call's own need: its plan has no prefill64)
        p.workspace = w.data_ptr()
        pa.append((p, keep + [w]))
        pb.append(params(q, kc, vc, cl, splits=da["nsplit"], variant=da["tiling"] << 1))
        pc.append(params(q, kc, vc, cl))
    db, dc = K.describe(pb[0][0]), K.describe(pc[0][0])
    assert (db["tiling"], db["nsplit"], db["workgroups"]) == (da["tiling"], da["nsplit"], da["workgroups"]), (da, db)
    plain = lambda pp: lib.vattn_flash_attn_with_kvcache(C.byref(pp), st)
    capped = lambda pp: lib.vattn_softcap_attn_with_kvcache(C.byref(pp), cap, st)
    med, t = _ab_windows(((capped, pa), (plain, pb), (plain, pc)), max(1, 24 // R), lib)
    fl = 4.0 * Hq * 128 * (n * c + n * (n + 1) / 2)
    print("  %-26s n=%d c=%d Hq=%2d Hkv=%d, %s, %d rotating caches" % (name, n, c, Hq, Hkv, "bf16" if DTYPE == torch.bfloat16 else "fp16", R))
    for tag, d, m, x in (("(a) softcap %-5g         " % cap, da, med[0], t[0]), ("(b) plain, (a)'s plan    ", db, med[1], t[1]), ("(c) plain, default plan  ", dc, med[2], t[2])):
        print("    %s tiling %d nsplit %d wg %4d : median %8.1f us  (5 windows: %s; spread %.1f%%)  %7.1f TFLOP/s" % (
            tag, d["tiling"], d["nsplit"], d["workgroups"], m, " ".join("%.1f" % y for y in x), 100.0 * (max(x) - min(x)) / m, fl / m / 1e6))
    print("    ratios: (a) / (b) = %.3f   (a) / (c) = %.3f   (b) / (c) = %.3f" % (med[0] / med[1], med[0] / med[2], med[1] / med[2]), flush=True)


def multitoken(B, sq, Hq, Hkv, ctx, ragged, base_path):
    """The multi-token decode call (q [B, sq, Hq, 128] against `ctx` cached tokens, the sq new rows appended) on caches that ROTATE (as
    --rotate: the Infinity Cache serves no repeat): this tree, the one-token decode step of the same batch, the prefill form of the same
    call (variant 8: what answered it before the form existed), the call and the one-token step WITHOUT k / v (same visible lengths, no
    append) and — with --base PATH, a library built from another commit (tools/build_base.py) — that library's default launch of the same block.  ragged: lengths spread over [ctx / 8, ctx].
    --tree (TREE): only the causal call and, beside it, the same block through vattn_tree_attn_with_kvcache with a CHAIN mask (the same visibility: what
    the mask costs); for sq = 7 also the 7-node, 3-leaf tree 0-1-{3,4}, 0-2-5-6 in ONE call against the three per-path causal calls (3, 3 and
    4 rows) that verify it without the tree form."""
    torch.manual_seed(0)
    slots = B
    by1 = B * 2.0 * ctx * Hkv * 128 * 2
    R = max(2, int(1.5e9 // by1) + 1)
    caches = [(torch.randn(slots, ctx + sq, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(slots, ctx + sq, Hkv, 128, device=DEV, dtype=DTYPE)) for _ in range(R)]
    lens = [ctx - (i * 7919 % (ctx - ctx // 8)) for i in range(B)] if ragged else [ctx] * B
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    libs = [("this tree", K.klib())] + ([("base", K._bind(C.CDLL(base_path)))] if base_path else [])

    def run(label, lib, n, variant, append=True, mask_words=None):
        q = torch.randn(B, n, Hq, 128, device=DEV, dtype=DTYPE)
        kn, vn = torch.randn(B, n, Hkv, 128, device=DEV, dtype=DTYPE), torch.randn(B, n, Hkv, 128, device=DEV, dtype=DTYPE)
        ps = []
        for kc, vc in caches:
            # (without k / v the rows are taken as already in the cache: the same visible length, no append)
            p, keep = params(q, kc, vc, cl, idx, kn, vn, variant=variant) if append else params(q, kc, vc, cl + n, idx, variant=variant)
            p.max_seqlen_k_hint = 0
            need = lib.vattn_attn_workspace_bytes(C.byref(p))          # (the library that runs the call sizes its workspace)
            w = torch.empty(need // 4 + 1, dtype=torch.float32, device=DEV)
            p.workspace = w.data_ptr()
            ps.append((p, keep, w))
        d = K.describe(ps[0][0], lib)
        call = lib.vattn_flash_attn_with_kvcache
        if mask_words is not None:          # the tree-masked entry point: the same block, the mask beside it
            mask = torch.tensor(mask_words, dtype=torch.int32, device=DEV).expand(B, n).contiguous()
            call = lambda pp, st_: lib.vattn_tree_attn_with_kvcache(pp, mask.data_ptr(), st_)
        best = []
        for _rep in range(3):
            for pp, _k, _w in ps:
                if call(C.byref(pp), st) != 0:
                    raise RuntimeError(K.last_error(lib))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            iters = max(2, 40 // R + 1)
            e0.record()
            for _ in range(iters):
                for pp, _k, _w in ps:
                    call(C.byref(pp), st)
            e1.record()
            torch.cuda.synchronize()
            best.append(e0.elapsed_time(e1) / (iters * R) * 1e3)
        print("  %-34s form %d path %d tiling %d wg %5d : %8.1f us  (3 runs: %s)" % (label, d["form"], d["path"], d["tiling"], d["workgroups"], min(best),
                                                                                  " ".join("%.1f" % x for x in best)), flush=True)
        return min(best)
    print("== multi-token decode B=%d sq=%d %d/%d heads ctx=%d%s, %s, D=128, %d rotating caches ==" % (
        B, sq, Hq, Hkv, ctx, " ragged" if ragged else "", "bf16" if DTYPE == torch.bfloat16 else "fp16", R), flush=True)
    if TREE:
        run("this tree: the call (causal)", K.klib(), sq, 0)
        run("this tree: tree entry, chain mask", K.klib(), sq, 0, mask_words=[(2 << t) - 1 for t in range(sq)])
        if sq == 7:
            one = run("this tree: tree entry, 3-leaf tree", K.klib(), 7, 0, mask_words=[0b1, 0b11, 0b101, 0b1011, 0b10011, 0b100101, 0b1100101])
            t3, t4 = run("this tree: causal call, 3-node path", K.klib(), 3, 0), run("this tree: causal call, 4-node path", K.klib(), 4, 0)
            print("  one tree call %.1f us vs the three per-path calls (3 + 3 + 4 rows) %.1f us: %.2fx" % (one, 2 * t3 + t4, (2 * t3 + t4) / one), flush=True)
        return
    for name, lib in libs:
        run("%s: the call (default plan)" % name, lib, sq, 0)
    run("this tree: prefill form (variant 8)", K.klib(), sq, 8)
    run("this tree: one-token decode step", K.klib(), 1, 0)
    # the same two launches without k / v: what the append costs in each form (a launch of its own in front of the multi-token call, fused
    # into the one-token step), apart from what the attention launches themselves cost
    run("this tree: the call, no k/v", K.klib(), sq, 0, append=False)
    run("this tree: one-token step, no k/v", K.klib(), 1, 0, append=False)


ONLY = None
ROTATE = False
WORKLIST = False
DRAWN = False
PERSIST = True       # work lists walked by persistent workgroups (prefill64p_kernel); --per-piece: one workgroup per piece (prefill64_kernel)
WL_TILES = 0
MEGA = 1
DTYPE = torch.float16
SPLITS = (0,)
PF_SPLITS = 0
TREE = False
SOFTCAP = 0.0
# the shapes of the A/B switches (--kv-fp8, --softcap): prefill (name, Hq, Hkv, chunk rows, cached rows), decode (name, Hq, Hkv, B, context);
# --softcap adds the model family that caps its logits
PF_AB_SHAPES = [("yi6b chunk2k@30k", 32, 4, 2048, 30720), ("llama70b/tp8 chunk2k@30k", 8, 1, 2048, 30720), ("yi6b chunk4k@28k", 32, 4, 4096, 28672),
                ("llama8b chunk512@8k", 32, 8, 512, 7680)]
DC_AB_SHAPES = [("llama8b B16@32k", 32, 8, 16, 32768), ("llama8b B1@128k", 32, 8, 1, 131072), ("yi6b B16@32k", 32, 4, 16, 32768),
                ("llama8b B64@8k", 32, 8, 64, 8192), ("llama70b/tp8 B64@32k", 8, 1, 64, 32768), ("mqa G32 B16@16k", 32, 1, 16, 16384)]
GEMMA2_PF_SHAPE, GEMMA2_DC_SHAPE = ("gemma2-27b chunk2k@30k", 32, 16, 2048, 30720), ("gemma2-27b B16@32k", 32, 16, 16, 32768)

if __name__ == "__main__":
    variant = 0
    if "--splits" in sys.argv:
        SPLITS = tuple(int(x) for x in sys.argv[sys.argv.index("--splits") + 1].split(","))
    WORKLIST = "--worklist" in sys.argv
    PERSIST = "--per-piece" not in sys.argv
    DRAWN = "--drawn" in sys.argv        # persistent workgroups draw their pieces (default: host-assigned queues)
    if os.environ.get("KBENCH_PERSIST_MAX_BLOCKS"):      # A/B: let the big balanced grids take a persistent list too
        from vattention_amd import flash_attn as _FA
        _FA.PERSISTENT_MAX_BLOCKS = int(os.environ["KBENCH_PERSIST_MAX_BLOCKS"])
    ROTATE = "--rotate" in sys.argv      # decode: rotate over enough caches that the Infinity Cache cannot serve repeated launches
    WL_TILES = int(sys.argv[sys.argv.index("--wl-tiles") + 1]) if "--wl-tiles" in sys.argv else 0
    if "--mega" in sys.argv:      # decode only: K/V as one layer's view of a megacache tensor with this many layers
        MEGA = int(sys.argv[sys.argv.index("--mega") + 1])
    if "--bf16" in sys.argv:
        DTYPE = torch.bfloat16
    if "--pf-splits" in sys.argv:
        PF_SPLITS = int(sys.argv[sys.argv.index("--pf-splits") + 1])
    if "--only" in sys.argv:
        ONLY = sys.argv[sys.argv.index("--only") + 1]
    if "--variant" in sys.argv:
        variant = int(sys.argv[sys.argv.index("--variant") + 1])
    if "--softcap" in sys.argv:
        SOFTCAP = float(sys.argv[sys.argv.index("--softcap") + 1])
        if not SOFTCAP > 0:
            sys.exit("kbench: --softcap takes a cap > 0")
    VARIANTS = [variant] if "--variant" in sys.argv else [0, 8, 12]
    if "--variants" in sys.argv:
        VARIANTS = [int(x) for x in sys.argv[sys.argv.index("--variants") + 1].split(",")]
    if "multitoken" in sys.argv:
        # multitoken --mt B,sq,Hq,Hkv,ctx[,ragged] [--mt ...] [--base build/base/libvattn_amd.so] [--bf16] [--tree] [--kv-fp8 [--tree]]
        base = sys.argv[sys.argv.index("--base") + 1] if "--base" in sys.argv else None
        TREE = "--tree" in sys.argv
        shapes = []
        for i, a in enumerate(sys.argv):
            if a == "--mt":
                f = sys.argv[i + 1].split(",") if i + 1 < len(sys.argv) else []
                if len(f) not in (5, 6) or not all(x.isdigit() for x in f[:5]) or (len(f) == 6 and f[5] != "ragged"):
                    sys.exit("kbench multitoken: --mt takes B,sq,Hq,Hkv,ctx[,ragged] (five integers), got %r" % ",".join(f))
                shapes.append(([int(x) for x in f[:5]], len(f) == 6))
        if not shapes:
            sys.exit("kbench multitoken: give at least one --mt B,sq,Hq,Hkv,ctx[,ragged]")
        torch.zeros(1, device=DEV)
        for dims, ragged in shapes:
            if SOFTCAP:
                B_, sq_, Hq_, Hkv_, ctx_ = dims
                softcap_ab("multi-token", B_, sq_, Hq_, Hkv_, ctx_ + sq_, SOFTCAP, ragged)
            elif "--kv-fp8" in sys.argv and TREE:          # the fp8 tree entry beside the fp8 causal call and the 2-byte tree call
                B_, sq_, Hq_, Hkv_, ctx_ = dims
                fp8_tree_ab(B_, sq_, Hq_, Hkv_, ctx_ + sq_, ragged)
            elif "--kv-fp8" in sys.argv:
                B_, sq_, Hq_, Hkv_, ctx_ = dims
                fp8_ab("multi-token", B_, sq_, Hq_, Hkv_, ctx_ + sq_, B_, ragged)
            else:
                multitoken(*dims, ragged=ragged, base_path=base)
        sys.exit(0)
    what = [a for a in sys.argv[1:] if a in ("prefill", "decode")] or ["prefill", "decode"]
    torch.zeros(1, device=DEV)
    if SOFTCAP:
        if "prefill" in what:
            print("== prefill (causal chunk n against c cached) with and without logit soft-capping (cap %g), D=128 ==" % SOFTCAP)
            for name, Hq, Hkv, n, c in PF_AB_SHAPES + [GEMMA2_PF_SHAPE]:
                if (ONLY and not any(o.strip() in name for o in ONLY.split(","))) or (not ONLY and "chunk2k@30k" not in name):
                    continue
                softcap_prefill_ab(name, Hq, Hkv, n, c, SOFTCAP)
        if "decode" in what:
            print("== decode (Sq=1, append + split-KV + combine) with and without logit soft-capping (cap %g), %s, D=128 ==" % (SOFTCAP, "bf16" if DTYPE == torch.bfloat16 else "fp16"))
            for name, Hq, Hkv, B, ctx in DC_AB_SHAPES + [GEMMA2_DC_SHAPE]:
                if (ONLY and not any(o.strip() in name for o in ONLY.split(","))) or (not ONLY and "B16@32k" not in name):
                    continue
                softcap_ab(name, B, 1, Hq, Hkv, ctx, SOFTCAP)
        sys.exit(0)
    if "prefill" in what and "--kv-fp8" in sys.argv:
        print("== prefill (causal chunk n against c cached) over an fp8 (e4m3) cache and a 2-byte cache, D=128 ==")
        for name, Hq, Hkv, n, c in PF_AB_SHAPES:
            if (ONLY and not any(o.strip() in name for o in ONLY.split(","))) or (not ONLY and "chunk2k@30k" not in name):
                continue
            fp8_prefill_ab(name, Hq, Hkv, n, c)
    elif "prefill" in what:
        for v in VARIANTS:
            print("-- prefill variant %d (order %s, tiling %s) --" % (v, ["XCD-grouped (default)", "block-major per head", "heaviest-first across heads", "XCD-grouped"][(v >> 5) & 3] + (", prefill64 build %d" % ((v >> 8) & 15) if (v >> 8) & 15 else ""), {0: "default plan", 1: "8 waves x 32 rows", 2: "4 waves x 64 rows", 3: "8 waves x 32 rows, LDS-DMA ring, in-wave software pipeline (prefill32)", 4: "4 waves x 32 rows", 6: "8 waves, hand-interleaved MFMA/VALU groups", 7: "4 waves x 64 rows, LDS-DMA ring, in-wave software pipeline (prefill64)"}[(v >> 1) & 7]))
            prefill(v)
    if "decode" in what and "--kv-fp8" in sys.argv:
        print("== decode (Sq=1, append + split-KV + combine) over a 2-byte and an fp8 (e4m3) cache, %s, D=128 ==" % ("bf16" if DTYPE == torch.bfloat16 else "fp16"))
        for name, Hq, Hkv, B, ctx in DC_AB_SHAPES:
            if ONLY and not any(o.strip() in name for o in ONLY.split(",")):
                continue
            fp8_ab(name, B, 1, Hq, Hkv, ctx, B)
    elif "decode" in what:
        dvs = [variant]
        if "--dvariants" in sys.argv:
            dvs = [int(x) for x in sys.argv[sys.argv.index("--dvariants") + 1].split(",")]
        for v in dvs:
            print("-- decode variant %d (%s%s) --" % (v, "512-thread workgroups" if v & 65536 else "1024-thread workgroups" if v & 131072 else "256 threads, two K/V register sets per wave" if v & 262144 else "256-thread workgroups (default)",
                                                   ", grid heuristics of rounds 1-3" if v & (1 << 19) else ", device-planned stream, in-launch merge (lab)" if v & (1 << 20) else ", device-planned stream"))
            decode(v)
