#!/usr/bin/env python3
"""Sliding-window timings, same box, against the PARENT commit's library (tools/build_base.py -> build/base/libvattn_amd.so).

The parent's parameter block is the current one without its last 8 bytes (the window words sit at the END of vattn_attn_params) and
carries ABI 5: one ctypes struct serves both libraries, the base library is handed struct_size - 8 / abi 5 and never a window.
Launches go through vattn_time_attn (HIP events around `iters` back-to-back launches); arms alternate A B A B ..., REPS times each, the
median per arm is printed.  Decode launches rotate over enough caches that the 256 MiB Infinity Cache cannot serve a repeated launch.

usage: python tools/window_bench.py [--base build/base/libvattn_amd.so] [--reps 5]
Output: one line per (shape, arm), then the ratios profiles/*_window.md quotes."""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vattention_amd import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
BASE = sys.argv[sys.argv.index("--base") + 1] if "--base" in sys.argv else os.path.join(ROOT, "build", "base", "libvattn_amd.so")


def block(q, out, kc, vc, cl, causal, left=None, kn=None, vn=None):
    p = K.AttnParams()
    B, Sq, Hq, D = q.shape
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
    p.cache_seqlens = cl.data_ptr()
    p.b, p.seqlen_q, p.seqlen_k, p.seqlen_knew, p.h, p.h_k, p.d = B, Sq, kc.shape[1], (1 if kn is not None else 0), Hq, kc.shape[2], D
    p.is_causal, p.dtype, p.softmax_scale = causal, 0, D ** -0.5
    if Sq > 1:
        p.max_seqlen_k_hint = kc.shape[1]
    if left is not None:
        p.window_left_plus1 = left + 1
    return p


def as_base(p):
    assert p.window_left_plus1 == 0
    p.struct_size, p.abi_version = C.sizeof(K.AttnParams) - 8, 5
    return p


def time_ms(lib, blocks, iters):
    """blocks: the same launch on several cache copies (rotation); returns ms per launch"""
    st = torch.cuda.current_stream(DEV).cuda_stream
    keep = []
    for p in blocks:
        need = lib.vattn_attn_workspace_bytes(C.byref(p))
        if need:
            ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=DEV)
            keep.append(ws)
            p.workspace = ws.data_ptr()
    tot = 0.0
    for p in blocks:
        ms = lib.vattn_time_attn(C.byref(p), st, 2, iters)
        if ms < 0:
            raise RuntimeError(K.last_error(lib))
        tot += ms
    return tot / len(blocks)


def ab(name, arms, iters):
    """arms: [(label, lib, blocks)]; alternating, REPS rounds"""
    res = {lab: [] for lab, _, _ in arms}
    for _ in range(REPS):
        for lab, lib, blocks in arms:
            res[lab].append(time_ms(lib, blocks, iters))
    med = {lab: statistics.median(v) for lab, v in res.items()}
    for lab in res:
        print("%-34s %-44s median %.4f ms  (min %.4f max %.4f, %d reps)" % (name, lab, med[lab], min(res[lab]), max(res[lab]), REPS), flush=True)
    return med


def main():
    new = K.klib()
    base = K._bind(C.CDLL(BASE))
    torch.manual_seed(0)
    Hq, Hkv, D, B = 32, 4, 128, 16          # Yi-6B
    # ---- decode: B16 @ 32 k with left = 4 095 (this tree) vs the parent at B16 @ 4 096 (same visible keys) and at B16 @ 32 k ----
    NCOPY = 3                                # 3 x 2.1 GiB of K/V at 32 k: nothing of a launch survives in the Infinity Cache
    L = 32768
    caches = [(torch.randn(B, L, Hkv, D, device=DEV, dtype=torch.float16), torch.randn(B, L, Hkv, D, device=DEV, dtype=torch.float16)) for _ in range(NCOPY)]
    q = torch.randn(B, 1, Hq, D, device=DEV, dtype=torch.float16)
    out = torch.empty_like(q)
    kn, vn = torch.randn(B, 1, Hkv, D, device=DEV, dtype=torch.float16), torch.randn(B, 1, Hkv, D, device=DEV, dtype=torch.float16)
    cl32 = torch.full((B,), L - 1, dtype=torch.int32, device=DEV)
    cl4 = torch.full((B,), 4095, dtype=torch.int32, device=DEV)
    win = [block(q, out, kc, vc, cl32, 1, left=4095, kn=kn, vn=vn) for kc, vc in caches]
    new32 = [block(q, out, kc, vc, cl32, 1, kn=kn, vn=vn) for kc, vc in caches]
    base32 = [as_base(block(q, out, kc, vc, cl32, 1, kn=kn, vn=vn)) for kc, vc in caches]
    # B16 @ 4 096: a [:, :4096] view of the same tensors (the wrapper's call), and 24 further row ranges of them for the rotation
    views = [(kc[:, o:o + 4096], vc[:, o:o + 4096]) for kc, vc in caches for o in range(0, L, 4096)]
    base4 = [as_base(block(q, out, kc, vc, cl4, 1, kn=kn, vn=vn)) for kc, vc in views]
    new4 = [block(q, out, kc, vc, cl4, 1, kn=kn, vn=vn) for kc, vc in views]
    m = ab("decode yi6b B16", [("this tree  @32k left=4095", new, win), ("parent     @4096 no window", base, base4), ("this tree  @4096 no window", new, new4),
                               ("parent     @32k no window", base, base32), ("this tree  @32k no window", new, new32)], 20)
    print("decode: windowed @32k / parent @4096 = %.3f ; parent @32k / windowed @32k = %.2fx ; window-less this tree / parent @32k = %.3f, @4096 = %.3f" % (
        m["this tree  @32k left=4095"] / m["parent     @4096 no window"], m["parent     @32k no window"] / m["this tree  @32k left=4095"],
        m["this tree  @32k no window"] / m["parent     @32k no window"], m["this tree  @4096 no window"] / m["parent     @4096 no window"]), flush=True)
    del caches, views, win, new32, base32, base4, new4
    torch.cuda.empty_cache()
    # ---- one sequence (decode_kernel): the two window-less instantiations whose register allocation moved with the block's size ----
    for dt, code in ((torch.float16, 0), (torch.bfloat16, 1)):
        cs = [(torch.randn(1, 131072, Hkv, D, device=DEV, dtype=dt), torch.randn(1, 131072, Hkv, D, device=DEV, dtype=dt)) for _ in range(6)]
        q1 = torch.randn(1, 1, Hq, D, device=DEV, dtype=dt)
        o1 = torch.empty_like(q1)
        k1, v1 = torch.randn(1, 1, Hkv, D, device=DEV, dtype=dt), torch.randn(1, 1, Hkv, D, device=DEV, dtype=dt)
        c1 = torch.full((1,), 131071, dtype=torch.int32, device=DEV)
        nb, bb = [block(q1, o1, kc, vc, c1, 1, kn=k1, vn=v1) for kc, vc in cs], [as_base(block(q1, o1, kc, vc, c1, 1, kn=k1, vn=v1)) for kc, vc in cs]
        for p in nb + bb:
            p.dtype = code
        m = ab("decode yi6b B1 @128k %s" % ("f16" if code == 0 else "bf16"), [("this tree", new, nb), ("parent", base, bb)], 20)
        print("decode_kernel %s: this tree / parent = %.3f" % ("f16" if code == 0 else "bf16", m["this tree"] / m["parent"]), flush=True)
        del cs, nb, bb
        torch.cuda.empty_cache()
    # ---- prefill: the 32 702-token prompt, left = 4 095, vs the parent's full causal launch ----
    n, left = 32702, 4095
    kc, vc = torch.randn(1, n, Hkv, D, device=DEV, dtype=torch.float16), torch.randn(1, n, Hkv, D, device=DEV, dtype=torch.float16)
    qp = torch.randn(1, n, Hq, D, device=DEV, dtype=torch.float16)
    op = torch.empty_like(qp)
    cln = torch.full((1,), n, dtype=torch.int32, device=DEV)
    m = ab("prefill yi6b n=32702", [("this tree  left=4095", new, [block(qp, op, kc, vc, cln, 1, left=left)]), ("parent     full causal", base, [as_base(block(qp, op, kc, vc, cln, 1))]),
                                    ("this tree  full causal", new, [block(qp, op, kc, vc, cln, 1)])], 5)
    pairs_full = n * (n + 1) / 2
    pairs_win = sum(min(i, left) + 1 for i in range(n))
    fl = lambda pairs: 4.0 * Hq * D * pairs
    print("prefill: visible (row, key) pairs windowed / full = %.4f ; time windowed / parent full = %.4f ; windowed %.0f TFLOP/s, parent full %.0f TFLOP/s, "
          "window-less this tree / parent = %.3f" % (pairs_win / pairs_full, m["this tree  left=4095"] / m["parent     full causal"],
                                                     fl(pairs_win) / m["this tree  left=4095"] / 1e9, fl(pairs_full) / m["parent     full causal"] / 1e9,
                                                     m["this tree  full causal"] / m["parent     full causal"]), flush=True)


if __name__ == "__main__":
    main()
