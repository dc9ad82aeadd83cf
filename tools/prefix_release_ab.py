#!/usr/bin/env python3
"""Same-box A/B/C of the windowed decode replay: what releasing the pages in front of a sliding window costs per step.

  (a) the parent commit's library (build/base/libvattn_amd.so, tools/build_base.py), window on, nothing released
  (b) this tree's library, window on, release off
  (c) this tree's library, window on, release on (cache_engine.set_sliding_window(left))

(b) against (a) is the regression check on untouched behaviour, (c) against (a) the price of the feature.  Every leg is a child process
of its own (one manager, one HIP context each); legs are interleaved a b c a b c and the best of the rounds is reported.

usage: python tools/prefix_release_ab.py [--rounds 3] [--out profiles/prefix_release_ab.txt]
       python tools/prefix_release_ab.py --leg b --batch 16 --page 65536          (one leg, one JSON line)

Shape: 4 layers of Yi-6B heads (32 / 4 x 128, fp16; 1 KiB per token and tensor), prompts of 6 144 tokens prefilled whole, then 2 200 decode
steps under left = 2 047: a 2 MiB page (2 048 tokens) is crossed once per sequence, a 64 KiB page (64 tokens) 34 times.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L, HQ, HKV, D, PROMPT, STEPS, LEFT = 4, 32, 4, 128, 6144, 2200, 2047


def one_leg(leg, batch, page):
    from vattention_amd import _lib
    if leg == "a":
        # (the loader accepts a library built before the release entry points existed: vattention_amd/_lib.py)
        _lib.LIB_PATH = os.path.join(ROOT, "build", "base", "libvattn_amd.so")
    import torch
    from vattention_amd import vattention as va
    from vattention_amd.replay import CacheConfig, HotPathRunner, ModelConfig, ParallelConfig, Sequence, SequenceMetadata
    model = ModelConfig(name="yi6b-4l", num_layers=L, num_q_heads=HQ, num_kv_heads=HKV, head_size=D, dtype=torch.float16, max_model_len=16384)
    cache = CacheConfig(page_size=page, max_batch_size=batch, memory_for_gpu=3 << 29, vattn_keep_layout=True)
    r = HotPathRunner(model, ParallelConfig(1, 1), cache, sliding_window=LEFT, release_prefix=leg == "c")
    r.sample_kv_util = False
    seqs = [Sequence(i, PROMPT, PROMPT + STEPS + 1024) for i in range(batch)]      # nobody finishes inside the run
    for s in seqs:
        r.run_iteration([SequenceMetadata(s, PROMPT, True)])
    for _ in range(20):                                  # warm-up decode steps
        r.run_iteration([SequenceMetadata(s, 0, False) for s in seqs])
    torch.cuda.synchronize()
    va.wait()
    s0 = va.stats()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        r.run_iteration([SequenceMetadata(s, 0, False) for s in seqs])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    va.wait()
    s1 = va.stats()
    d = lambda k: s1.get(k, 0) - s0.get(k, 0)
    out = {"leg": leg, "batch": batch, "page_kib": page >> 10, "ms_per_step": round(dt / STEPS * 1e3, 4),
           "join_wait_us_per_step": round(d("join_wait_ns") / STEPS / 1e3, 2), "fence_wait_ms": round(d("fence_wait_ns") / 1e6, 2),
           "fence_waits": d("fence_waits"), "quiesce_calls": d("quiesce_calls"), "unmap_calls": d("unmap_calls"),
           "tlb_flushes": d("tlb_flushes"), "tlb_flush_ms": round(d("tlb_flush_ns") / 1e6, 2),
           "prefix_pages_released": d("prefix_pages_released"), "pages_mapped_end": s1["pages_mapped_now"]}
    r.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["a", "b", "c"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--page", type=int, default=2 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        return one_leg(a.leg, a.batch, a.page)
    lines = ["windowed decode replay, %d layers %d/%d x %d fp16, prompt %d, %d decode steps, left %d; best of %d interleaved rounds" % (
        L, HQ, HKV, D, PROMPT, STEPS, LEFT, a.rounds),
        "leg a = parent library, b = this tree release off, c = this tree release on",
        "%-6s %-8s %-4s %10s %9s %13s %11s %8s %7s %10s %9s %10s" % ("batch", "page", "leg", "ms/step", "vs a", "join us/step", "fence ms", "unmaps", "flush", "flush ms", "released", "mapped@end")]
    for batch in (1, 16):
        for page in (2 << 20, 64 << 10):
            best = {}
            for _ in range(a.rounds):
                for leg in "abc":
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(batch), "--page", str(page)],
                                       capture_output=True, text=True, timeout=280)
                    if p.returncode != 0:          # a leg that failed ends the measurement: nothing more is started on the GPU
                        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                        sys.exit(p.returncode or 1)
                    rec = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
                    if leg not in best or rec["ms_per_step"] < best[leg]["ms_per_step"]:
                        best[leg] = rec
            for leg in "abc":
                b = best[leg]
                lines.append("%-6d %-8s %-4s %10.4f %8.2f%% %13.2f %11.2f %8d %7d %10.2f %9d %10d" % (
                    batch, "%d KiB" % b["page_kib"], leg, b["ms_per_step"], (b["ms_per_step"] / best["a"]["ms_per_step"] - 1) * 100,
                    b["join_wait_us_per_step"], b["fence_wait_ms"], b["unmap_calls"], b["tlb_flushes"], b["tlb_flush_ms"],
                    b["prefix_pages_released"], b["pages_mapped_end"]))
            print("\n".join(lines[-3:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
