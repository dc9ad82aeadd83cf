"""CPU statement of TREE-MASKED multi-token attention over an FP8 (e4m3) KV cache (include/vattn_kernels.h, vattn_fp8kv_tree_attn_with_kvcache):
the two existing references composed, neither restated — `k` / `v` (if given) are quantised IN PLACE into k8 / v8 at cache_seqlens by
tests/fp8kv_ref.quantize_ref, then tests/tree_ref.tree_attn_ref's visibility rule is applied to stored * scale.  The same math switch as
fp8kv_attn_ref: "f64" = exact arithmetic on the dequantised values, "f32" = the kernels' numerics (P and the output rounded to q's dtype).
Shared by tests/test_fp8kv_tree_plan.py and tests/test_gpu_fp8kv_tree.py."""
import torch

from tests.fp8kv_ref import dequantize_ref, quantize_ref
from tests.tree_ref import tree_attn_ref


def fp8kv_tree_ref(q, k8, v8, k_scale, v_scale, mask, k=None, v=None, cache_seqlens=None, cache_batch_idx=None, softmax_scale=None,
                   math="f64", return_lse=False):
    """q [B,Sq,Hq,D] fp16 / bf16; k8 / v8 [Bc,rows,Hkv,D] float8_e4m3fn; k_scale / v_scale float32 [Hkv]; mask int [B,Sq] bit words (or [Sq])."""
    B = q.shape[0]
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((B,), cache_seqlens, dtype=torch.int32)
    elif cache_seqlens is not None and not isinstance(cache_seqlens, torch.Tensor):
        cache_seqlens = torch.tensor(list(cache_seqlens), dtype=torch.int32)
    idx = list(range(B)) if cache_batch_idx is None else [int(i) for i in cache_batch_idx.tolist()]
    if k is not None:
        Sn, Sk = k.shape[1], k8.shape[1]
        for b in range(B):          # (rows beyond the cache view are dropped, as the append launch drops them)
            n0 = int(cache_seqlens[b])
            n1 = min(n0 + Sn, Sk)
            if n1 > n0:
                k8[idx[b], n0:n1] = quantize_ref(k[b, :n1 - n0], k_scale)
                v8[idx[b], n0:n1] = quantize_ref(v[b, :n1 - n0], v_scale)
        cache_seqlens = cache_seqlens + Sn
    wt = torch.float64 if math == "f64" else torch.float32
    Sk = k8.shape[1]
    lens = [Sk] * B if cache_seqlens is None else [min(int(n), Sk) for n in cache_seqlens.tolist()]
    words = mask.expand(B, q.shape[1])
    outs, lses = [], []
    for b in range(B):          # entry by entry: only the visible rows of the entry's slot are dequantised (rows beyond may hold the NaN byte)
        kb = dequantize_ref(k8[idx[b], :lens[b]], k_scale, wt).unsqueeze(0)
        vb = dequantize_ref(v8[idx[b], :lens[b]], v_scale, wt).unsqueeze(0)
        o, l = tree_attn_ref(q[b:b + 1], kb, vb, words[b:b + 1], cache_seqlens=lens[b], softmax_scale=softmax_scale, math=math, return_lse=True)
        outs.append(o)
        lses.append(l)
    out, lse = torch.cat(outs), torch.cat(lses)
    return (out, lse) if return_lse else out
