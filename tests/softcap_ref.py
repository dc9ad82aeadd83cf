"""CPU statement of attention with logit soft-capping, for the softcap tests (the oracle, oracle/attn.py, has no cap and needs none:
tests/test_softcap_ref.py checks this helper against the oracle and against tests/window_ref.py with a cap so large that it does nothing).

    scores = softcap * tanh(q.k * softmax_scale / softcap)          (flash_api.cpp:105-113, flash_fwd_kernel.h:26-30 apply_softcap)

taken BEFORE the mask: a masked score is -inf whatever the cap.  softcap = 0: no cap.  Masks, bottom-right aligned as everywhere: query row
i of Sq rows over Lk visible keys attends keys j <= i + Lk - Sq when `causal` (all j < Lk otherwise) and, with `left` (needs causal),
j >= i + Lk - Sq - left.  A row that sees no key gives 0 (LSE +inf).  GQA: query head h uses kv head h // (Hq // Hkv).

``math="f64"``: exact arithmetic on the fp16 / bf16 inputs (what tests compare to); ``math="f32"``: fp32 accumulate, P rounded to the
I/O dtype before PV, output rounded to the I/O dtype — the reference kernel's numerics.  Dense over the keys (the softcap tests are small).
Nothing is appended here: the caches hold what the call sees AFTER its append.
"""
from typing import Optional, Union

import torch


def softcap_attn_ref(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, softcap: float, left: Optional[int] = None,
                     causal: bool = True, cache_seqlens: Optional[Union[int, torch.Tensor, list]] = None,
                     cache_batch_idx: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None, math: str = "f64",
                     return_lse: bool = False, q_lens: Optional[list] = None):
    """q [B,Sq,Hq,D]; caches [Bc,Sk,Hkv,D]; cache_seqlens = VISIBLE keys per entry (None: the whole cache).  q_lens: per-entry number of
    valid query rows (entries shorter than Sq; the rows beyond stay 0, LSE +inf).  Returns [B,Sq,Hq,D] in float64 (f64) or the input dtype
    (f32), and the LSE [B,Hq,Sq] when asked."""
    assert math in ("f64", "f32") and softcap >= 0 and (left is None or (left >= 0 and causal))
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
    wt = torch.float64 if math == "f64" else torch.float32
    out = torch.zeros(B, Sq, Hq, D, dtype=wt)
    lse = torch.full((B, Hq, Sq), float("inf"), dtype=wt)
    for b in range(B):
        Lk = min(lens[b], Sk)
        n = Sq if q_lens is None else int(q_lens[b])
        if n <= 0 or Lk <= 0:
            continue
        off = Lk - n
        K = k_cache[idx[b], :Lk].to(wt).permute(1, 0, 2)                                  # [Hkv,Lk,D]
        V = v_cache[idx[b], :Lk].to(wt).permute(1, 0, 2)
        Q = q[b, :n].to(wt).reshape(n, Hkv, G, D).permute(1, 2, 0, 3).reshape(Hkv, G * n, D)
        S = torch.matmul(Q, K.transpose(1, 2)) * scale                                    # [Hkv,G*n,Lk]
        if softcap > 0:
            S = softcap * torch.tanh(S / softcap)
        i, j = torch.arange(n).view(-1, 1), torch.arange(Lk).view(1, -1)
        keep = torch.ones(n, Lk, dtype=torch.bool)
        if causal:
            keep &= j <= i + off
        if left is not None:
            keep &= j >= i + off - left
        S = S.masked_fill(~keep.repeat(G, 1).unsqueeze(0), float("-inf"))
        m = S.max(dim=-1, keepdim=True).values
        dead = torch.isinf(m) & (m < 0)
        m = torch.where(dead, torch.zeros_like(m), m)
        P = torch.exp(S - m)
        l = P.sum(dim=-1, keepdim=True)
        if math == "f32":
            P = P.to(q.dtype).to(wt)
        O = torch.matmul(P, V) / torch.where(dead, torch.ones_like(l), l)
        O = torch.where(dead, torch.zeros_like(O), O)
        out[b, :n] = O.view(Hkv, G, n, D).permute(2, 0, 1, 3).reshape(n, Hq, D)
        row_lse = (m + torch.log(l)).squeeze(-1)
        row_lse = torch.where(dead.squeeze(-1), torch.full_like(row_lse, float("inf")), row_lse)
        lse[b, :, :n] = row_lse.view(Hq, n)
    if math == "f32":
        out = out.to(q.dtype)
    return (out, lse) if return_lse else out
