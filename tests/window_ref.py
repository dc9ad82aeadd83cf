"""CPU statement of causal sliding-window attention, for the window tests (the oracle, oracle/attn.py, has no window and needs none:
tests/test_window_ref.py checks this helper against the oracle's one-row calls on key slices).

flash_attn_interface.py:1204-1206, bottom-right aligned: query row i of Sq rows over Lk visible keys attends keys j with
    max(0, i + Lk - Sq - left) <= j <= i + Lk - Sq.
A row that sees no key gives 0 (LSE +inf), as in the oracle.  GQA: query head h uses kv head h // (Hq // Hkv).

``math="f64"``: exact arithmetic on the fp16 / bf16 inputs (what tests compare to); ``math="f32"``: fp32 accumulate, P rounded to the
I/O dtype before PV, output rounded to the I/O dtype — the reference kernel's numerics, like the oracle's ``math="f32"``.

Vectorised over heads and over blocks of query rows, and only the keys a block of rows can see are touched: a 32 k-token prompt with
left = 4 095 costs what its visible (row, key) pairs cost.  ``rows``: compute these query rows only (sorted 1-D index tensor; the result
then has len(rows) rows) — sampled full-size checks.  Nothing is appended here: the caches hold what the call sees AFTER its append.
"""
from typing import Optional, Union

import torch


def window_attn_ref(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, left: int,
                    cache_seqlens: Optional[Union[int, torch.Tensor, list]] = None, cache_batch_idx: Optional[torch.Tensor] = None,
                    softmax_scale: Optional[float] = None, math: str = "f64", return_lse: bool = False,
                    rows: Optional[torch.Tensor] = None, q_lens: Optional[list] = None):
    """q [B,Sq,Hq,D]; caches [Bc,Sk,Hkv,D]; cache_seqlens = VISIBLE keys per entry (None: the whole cache).  q_lens: per-entry number of
    valid query rows (entries shorter than Sq; the rows beyond stay 0).  Returns [B,R,Hq,D] (R = Sq or len(rows)) in float64 (f64) or
    the input dtype (f32), and the LSE [B,Hq,R] when asked."""
    assert left >= 0 and math in ("f64", "f32")
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
    sel = torch.arange(Sq) if rows is None else rows.to(torch.long)
    R = sel.numel()
    out = torch.zeros(B, R, Hq, D, dtype=wt)
    lse = torch.full((B, Hq, R), float("inf"), dtype=wt)
    for b in range(B):
        Lk = min(lens[b], Sk)
        sq_b = Sq if q_lens is None else int(q_lens[b])
        off = Lk - sq_b
        r0 = 0
        while r0 < R:
            # a chunk of selected rows that lie within 256 positions of each other: one key slice serves them all
            r1 = r0 + 1
            while r1 < R and r1 - r0 < 256 and int(sel[r1]) - int(sel[r0]) < 256:
                r1 += 1
            i = sel[r0:r1]
            keep_rows = i < sq_b
            hi = i + off                                   # last visible key of each row
            lo = (hi - left).clamp(min=0)
            k_lo, k_hi = int(lo.min()), min(int(hi.max()), Lk - 1)
            if k_hi >= k_lo and bool(keep_rows.any()):
                n = r1 - r0
                Kh = k_cache[idx[b], k_lo:k_hi + 1].to(wt).permute(1, 0, 2)            # [Hkv,L,D]
                Vh = v_cache[idx[b], k_lo:k_hi + 1].to(wt).permute(1, 0, 2)
                Qb = q[b, i].to(wt).reshape(n, Hkv, G, D).permute(1, 2, 0, 3).reshape(Hkv, G * n, D)
                S = torch.matmul(Qb, Kh.transpose(1, 2)) * scale                       # [Hkv,G*n,L]
                j = torch.arange(k_lo, k_hi + 1).view(1, -1)
                keep = (j >= lo.view(-1, 1)) & (j <= hi.view(-1, 1)) & keep_rows.view(-1, 1)   # [n,L]
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
                out[b, r0:r1] = O.view(Hkv, G, n, D).permute(2, 0, 1, 3).reshape(n, Hq, D)
                row_lse = (m + torch.log(l)).squeeze(-1)
                row_lse = torch.where(dead.squeeze(-1), torch.full_like(row_lse, float("inf")), row_lse)
                lse[b, :, r0:r1] = row_lse.view(Hq, n)
            r0 = r1
    if math == "f32":
        out = out.to(q.dtype)
    return (out, lse) if return_lse else out


def first_visible_key(Sq: int, Lk: int, left: int) -> int:
    """First key the FIRST query row of an entry sees (what the no-read contract aligns down to the kernel's key tile)."""
    return max(0, Lk - Sq - left)
