"""CPU reference of the FP8 (e4m3) KV cache (include/vattn_kernels.h, "FP8 KV cache"): the quantiser, restated in torch, and attention over a
quantised cache as the oracle (oracle/attn.py) on the dequantised values.  Shared by tests/test_fp8kv_ref.py and tests/test_gpu_fp8kv.py."""
import torch

from oracle.attn import flash_attn_with_kvcache_ref

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize_ref(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x [..., heads, d] (fp16 / bf16 / fp32), scale float32 [heads] -> float8_e4m3fn of x's shape: inv = 1.0f / scale (IEEE fp32, once per
    head), y = float(x) * inv in fp32, clamp to +-448, round-to-nearest-even; a NaN stays the NaN byte."""
    inv = (torch.ones((), dtype=torch.float32) / scale.to(torch.float32)).view(-1, 1)
    return (x.float() * inv).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def dequantize_ref(x8: torch.Tensor, scale: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """value = stored * scale[head]; x8 [..., heads, d]"""
    return x8.to(dtype) * scale.to(dtype).view(-1, 1)


def amax_scales(x: torch.Tensor) -> torch.Tensor:
    """per-head scales amax / 448 over every row of x [..., heads, d] (float32 [heads]; 1 for an all-zero head)"""
    a = x.float().abs().amax(dim=tuple(i for i in range(x.dim()) if i != x.dim() - 2))
    return torch.where(a > 0, a / FP8_MAX, torch.ones_like(a)).to(torch.float32)


def fp8kv_attn_ref(q, k8, v8, k_scale, v_scale, k=None, v=None, cache_seqlens=None, cache_batch_idx=None, softmax_scale=None, causal=False,
                   math="f64", return_lse=False):
    """flash_attn_fp8kv_with_kvcache on the CPU: `k` / `v` (if given) are quantised into k8 / v8 IN PLACE at cache_seqlens, then the oracle
    attends over k8 * k_scale[h], v8 * v_scale[h] — in float64, or (math="f32") in the oracle's fp32 numerics (P and the output rounded to
    q's dtype)."""
    B = q.shape[0]
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((B,), cache_seqlens, dtype=torch.int32)
    elif cache_seqlens is not None and not isinstance(cache_seqlens, torch.Tensor):
        cache_seqlens = torch.tensor(list(cache_seqlens), dtype=torch.int32)
    if k is not None:
        idx = list(range(B)) if cache_batch_idx is None else [int(i) for i in cache_batch_idx.tolist()]
        Sn = k.shape[1]
        for b in range(B):
            n0 = int(cache_seqlens[b])
            k8[idx[b], n0:n0 + Sn] = quantize_ref(k[b], k_scale)
            v8[idx[b], n0:n0 + Sn] = quantize_ref(v[b], v_scale)
        cache_seqlens = cache_seqlens + Sn
    wt = torch.float64 if math == "f64" else torch.float32
    Sk = k8.shape[1]
    lens = [Sk] * B if cache_seqlens is None else [min(int(n), Sk) for n in cache_seqlens.tolist()]
    idx = list(range(B)) if cache_batch_idx is None else [int(i) for i in cache_batch_idx.tolist()]
    outs, lses = [], []
    for b in range(B):          # entry by entry: only the visible rows of the entry's slot are dequantised
        kb = dequantize_ref(k8[idx[b], :lens[b]], k_scale, wt).unsqueeze(0)
        vb = dequantize_ref(v8[idx[b], :lens[b]], v_scale, wt).unsqueeze(0)
        o, l = flash_attn_with_kvcache_ref(q[b:b + 1], kb, vb, cache_seqlens=lens[b], softmax_scale=softmax_scale, causal=causal, math=math, return_lse=True)
        outs.append(o)
        lses.append(l)
    out, lse = torch.cat(outs), torch.cat(lses)
    return (out, lse) if return_lse else out
