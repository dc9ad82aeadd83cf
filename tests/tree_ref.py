"""CPU statement of TREE-MASKED multi-token attention (include/vattn_kernels.h, vattn_tree_attn_with_kvcache), for the tree tests — a plain
dense masked softmax; the oracle (oracle/attn.py) has no tree mask and needs none: tests/test_tree_ref.py checks this helper against it.

With Lk visible keys of entry b (after the append of k / v, clamped to the view) and base = Lk - Sq, query token t sees every key
j < base and draft key base + s iff bit s of mask[b, t] is set and base + s >= 0.  No causal flag.  A row that sees no key gives 0 and LSE
+inf.  GQA: query head h uses kv head h // (Hq // Hkv).

``math="f64"``: exact arithmetic on the fp16 / bf16 inputs (what tests compare to); ``math="f32"``: fp32 accumulate, P rounded to the I/O
dtype before PV, output rounded to the I/O dtype — the kernels' numerics, like the oracle's ``math="f32"``.  k / v are appended IN PLACE
at row cache_seqlens[b] of slot cache_batch_idx[b], as the oracle does."""
from typing import Optional, Union

import torch


def pack_mask(vis: torch.Tensor) -> torch.Tensor:
    """bool [.., Sq, Sq] (vis[.., t, s]: token t sees draft key s) -> int32 [.., Sq] bit words"""
    sq = vis.shape[-1]
    return (vis.to(torch.int64) << torch.arange(sq)).sum(-1).to(torch.int32)


def chain_mask(sq: int) -> torch.Tensor:
    """the causal multi-token call as mask words: token t sees draft keys 0..t"""
    return torch.tensor([(2 << t) - 1 for t in range(sq)], dtype=torch.int32)


def tree_attn_ref(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, mask: torch.Tensor,
                  k: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None,
                  cache_seqlens: Optional[Union[int, torch.Tensor, list]] = None, cache_batch_idx: Optional[torch.Tensor] = None,
                  softmax_scale: Optional[float] = None, math: str = "f64", return_lse: bool = False):
    """q [B,Sq,Hq,D]; caches [Bc,Sk,Hkv,D]; mask int [B,Sq] bit words (or [Sq]: every entry).  Returns [B,Sq,Hq,D] in float64 (f64) or the
    input dtype (f32), and the LSE [B,Hq,Sq] when asked."""
    assert math in ("f64", "f32")
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k_cache.shape[1], k_cache.shape[2]
    G = Hq // Hkv
    assert G * Hkv == Hq
    scale = D ** -0.5 if softmax_scale is None else softmax_scale
    if cache_seqlens is None:
        lens = [Sk] * B
    elif isinstance(cache_seqlens, int):
        lens = [cache_seqlens] * B
    else:
        lens = [int(x) for x in (cache_seqlens.tolist() if isinstance(cache_seqlens, torch.Tensor) else cache_seqlens)]
    idx = list(range(B)) if cache_batch_idx is None else [int(x) for x in cache_batch_idx.tolist()]
    words = mask.to(torch.int64).expand(B, Sq) & 0xFFFFFFFF
    Sn = 0
    if k is not None:
        Sn = k.shape[1]
        for b in range(B):
            k_cache[idx[b], lens[b]:lens[b] + Sn] = k[b]
            v_cache[idx[b], lens[b]:lens[b] + Sn] = v[b]
    wt = torch.float64 if math == "f64" else torch.float32
    out = torch.zeros(B, Sq, Hq, D, dtype=wt)
    lse = torch.full((B, Hq, Sq), float("inf"), dtype=wt)
    for b in range(B):
        Lk = min(lens[b] + Sn, Sk)
        if Lk <= 0:
            continue
        base = Lk - Sq
        j = torch.arange(Lk).view(1, Lk)
        s = (j - base).clamp(min=0, max=31)
        keep = (j < base) | (((words[b].view(Sq, 1) >> s) & 1).bool() & (j >= base))      # [Sq,Lk]
        Kh = k_cache[idx[b], :Lk].to(wt).permute(1, 0, 2)          # [Hkv,Lk,D]
        Vh = v_cache[idx[b], :Lk].to(wt).permute(1, 0, 2)
        Qb = q[b].to(wt).reshape(Sq, Hkv, G, D).permute(1, 2, 0, 3).reshape(Hkv, G * Sq, D)      # row r of the stack: token r % Sq
        S = torch.matmul(Qb, Kh.transpose(1, 2)) * scale
        S = S.masked_fill(~keep.repeat(G, 1).unsqueeze(0), float("-inf"))
        m = S.max(dim=-1, keepdim=True).values
        dead = torch.isinf(m) & (m < 0)
        m = torch.where(dead, torch.zeros_like(m), m)
        P = torch.exp(S - m)
        l = P.sum(dim=-1, keepdim=True)
        if math == "f32":
            P = P.to(q.dtype).to(wt)
        O = torch.matmul(P, Vh) / torch.where(dead, torch.ones_like(l), l)
        O = torch.where(dead, torch.zeros_like(O), O)
        out[b] = O.view(Hkv, G, Sq, D).permute(2, 0, 1, 3).reshape(Sq, Hq, D)
        row_lse = (m + torch.log(l)).squeeze(-1)
        row_lse = torch.where(dead.squeeze(-1), torch.full_like(row_lse, float("inf")), row_lse)
        lse[b] = row_lse.view(Hq, Sq)
    if math == "f32":
        out = out.to(q.dtype)
    return (out, lse) if return_lse else out
