"""Drop-in for `sarathi.cache_ops.cache_flat` (/root/reference/sarathi-lean/csrc/cache.cpp:40-46,69-72;
kernel /root/reference/sarathi-lean/csrc/cache_kernels.cu:482-570): append n new tokens of K and V
([n, kvh, D]) to caller-sliced contiguous cache rows, in place, on the current stream."""
from __future__ import annotations

import torch

from . import kernels as K


def cache_flat(key: torch.Tensor, value: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
               kv_cache_dtype: str) -> None:
    if kv_cache_dtype != "auto":
        raise RuntimeError("Unsupported data type of kv cache: " + str(kv_cache_dtype))       # cache_kernels.cu:532-534
    if not (key.is_cuda and value.is_cuda and k_cache.is_cuda and v_cache.is_cuda):
        raise RuntimeError("vattention_amd.cache_ops: tensors must live on the GPU (there is no CPU path)")
    if k_cache.stride(0) != v_cache.stride(0):
        raise RuntimeError("k_cache.stride(0) == v_cache.stride(0)")                          # TORCH_CHECK at :543
    n, nh, hs = key.shape[0], key.shape[1], key.shape[2]
    if n == 0:
        return
    for t in (key, value, k_cache, v_cache):
        if t.stride(-1) != 1 or t.stride(-2) != hs:
            raise RuntimeError("cache_flat expects [tokens, heads, head_size] with contiguous (heads, head_size)")
    rc = K.klib().vattn_cache_flat(key.data_ptr(), value.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), n, nh, hs,
                                   key.stride(0), value.stride(0), k_cache.stride(0), v_cache.stride(0),
                                   key.element_size(), K.current_stream_ptr(key.device))
    if rc != 0:
        raise RuntimeError(K.last_error())


def cache_flat_fp8(key: torch.Tensor, value: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                   k_scale: torch.Tensor, v_scale: torch.Tensor) -> None:
    """MI355X extension (include/vattn_kernels.h, "FP8 KV cache"): cache_flat into a float8_e4m3fn cache — n new tokens of K and V
    ([n, kvh, D], fp16 / bf16) are quantised with one scale per kv head (k_scale / v_scale: float32 [kvh] GPU tensors, value = stored *
    scale) into caller-sliced cache rows, in place, on the current stream.  The bytes are those of
    (x.float() * (1.0 / scale)).clamp(-448, 448).to(torch.float8_e4m3fn); nothing but rows [0, n) is written."""
    ts = (key, value, k_cache, v_cache, k_scale, v_scale)
    if not all(t.is_cuda for t in ts):
        raise RuntimeError("vattention_amd.cache_ops: tensors must live on the GPU (there is no CPU path)")
    if k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn:
        raise RuntimeError("cache_flat_fp8 writes float8_e4m3fn caches")
    if value.dtype != key.dtype:
        raise RuntimeError("key and value must have the same dtype")
    n, nh, hs = key.shape[0], key.shape[1], key.shape[2]
    for s in (k_scale, v_scale):
        if s.dtype != torch.float32 or s.shape != (nh,) or not s.is_contiguous():
            raise RuntimeError("k_scale / v_scale must be contiguous float32 [num_kv_heads] tensors")
    if n == 0:
        return
    for t in (key, value, k_cache, v_cache):
        if t.stride(-1) != 1 or t.stride(-2) != hs:
            raise RuntimeError("cache_flat_fp8 expects [tokens, heads, head_size] with contiguous (heads, head_size)")
    rc = K.klib().vattn_cache_flat_fp8(key.data_ptr(), value.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), n, nh, hs,
                                       key.stride(0), value.stride(0), k_cache.stride(0), v_cache.stride(0), K.dtype_code(key.dtype),
                                       k_scale.data_ptr(), v_scale.data_ptr(), K.current_stream_ptr(key.device))
    if rc != 0:
        raise (NotImplementedError if rc == -10 else RuntimeError)(K.last_error())


def cache_flat_rope(key: torch.Tensor, value: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                    cos_sin_cache: torch.Tensor, pos0: int) -> None:
    """MI355X extension: cache_flat with the rotary embedding of the KEY rows fused in — k_cache[t] = rope(key[t]) at
    position pos0 + t, v_cache[t] = value[t] — one pass over the new K/V instead of the reference's rotary kernel followed by
    cache_flat (models/yi.py:172-173 + vattention_flashattention_wrapper.py:151-156).  `cos_sin_cache` is the model's
    [max_position, rotary_dim] table (rotary_embedding.py:75-84); NeoX pairing, rotary_dim == head size."""
    if not (key.is_cuda and value.is_cuda and k_cache.is_cuda and v_cache.is_cuda and cos_sin_cache.is_cuda):
        raise RuntimeError("vattention_amd.cache_ops: tensors must live on the GPU (there is no CPU path)")
    n, nh, hs = key.shape[0], key.shape[1], key.shape[2]
    if n == 0:
        return
    if cos_sin_cache.dtype != key.dtype or cos_sin_cache.shape[1] != hs or cos_sin_cache.stride(1) != 1:
        raise RuntimeError("cos_sin_cache must be [positions, head_size] in the key's dtype")
    if pos0 + n > cos_sin_cache.shape[0]:
        raise RuntimeError("positions exceed the cos/sin table")
    for t in (key, value, k_cache, v_cache):
        if t.stride(-1) != 1 or t.stride(-2) != hs:
            raise RuntimeError("cache_flat_rope expects [tokens, heads, head_size] with contiguous (heads, head_size)")
    rc = K.klib().vattn_cache_flat_rope(key.data_ptr(), value.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), n, nh, hs,
                                        key.stride(0), value.stride(0), k_cache.stride(0), v_cache.stride(0), K.dtype_code(key.dtype),
                                        cos_sin_cache.data_ptr(), cos_sin_cache.stride(0), int(pos0), K.current_stream_ptr(key.device))
    if rc != 0:
        raise RuntimeError(K.last_error())


def rotary_embedding(positions: torch.Tensor, query: torch.Tensor, key: torch.Tensor, head_size: int,
                     cos_sin_cache: torch.Tensor, is_neox: bool) -> None:
    """Drop-in for sarathi's pos_encoding_ops.rotary_embedding (csrc/pos_encoding_kernels.cu:80-129): in place on query
    [T, Hq*hs] and key [T, Hkv*hs].  The UNFUSED path — what the fused launches are measured against."""
    if not (query.is_cuda and key.is_cuda and positions.is_cuda and cos_sin_cache.is_cuda):
        raise RuntimeError("vattention_amd.cache_ops: tensors must live on the GPU (there is no CPU path)")
    if positions.dtype != torch.int64:
        raise RuntimeError("positions must be int64")
    T = query.shape[0]
    rc = K.klib().vattn_rotary_embedding(positions.data_ptr(), query.data_ptr(), key.data_ptr(), T, query.shape[1] // head_size,
                                         key.shape[1] // head_size, head_size, query.stride(0), key.stride(0), K.dtype_code(query.dtype),
                                         cos_sin_cache.data_ptr(), cos_sin_cache.stride(0), cos_sin_cache.shape[1], 1 if is_neox else 0,
                                         K.current_stream_ptr(query.device))
    if rc != 0:
        raise RuntimeError(K.last_error())


def keep_rows(k_cache: torch.Tensor, v_cache: torch.Tensor, row0: torch.Tensor, keep_idx: torch.Tensor, keep_cnt: torch.Tensor,
              cache_batch_idx=None) -> None:
    """MI355X extension (include/vattn_kernels.h, vattn_cache_keep_rows): compaction of the accepted draft rows behind a tree-masked verify
    call (flash_attn.flash_attn_tree_with_kvcache), in place, on the current stream.  Caches [Bc, rows, Hkv, D] (any strided view with a
    contiguous last dimension); row0 int32 [B]: first draft row of each entry (the cache_seqlens of the verify call); keep_idx int32
    [B, n_draft <= 8]: the draft rows to keep, strictly ascending per entry; keep_cnt int32 [B]: how many of them.  Row row0 + i of slot
    cache_batch_idx[b] receives row row0 + keep_idx[b, i] for i < keep_cnt[b]; nothing else is written.  No host synchronisation.
    float8_e4m3fn caches (behind flash_attn.flash_attn_fp8kv_tree_with_kvcache) go to vattn_cache_keep_rows_fp8: the same contract over bytes."""
    ts = (k_cache, v_cache, row0, keep_idx, keep_cnt, cache_batch_idx)
    if not all(t.is_cuda for t in ts if t is not None):
        raise RuntimeError("vattention_amd.cache_ops: tensors must live on the GPU (there is no CPU path)")
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.dtype != v_cache.dtype or k_cache.stride(-1) != 1 or v_cache.stride(-1) != 1:
        raise RuntimeError("keep_rows expects k_cache and v_cache [slots, rows, kv heads, head_size] of one shape and dtype, last dimension contiguous")
    if keep_idx.dim() != 2:
        raise RuntimeError("keep_idx must be [batch, n_draft]")
    B, n_draft = keep_idx.shape
    for t, name in ((row0, "row0"), (keep_idx, "keep_idx"), (keep_cnt, "keep_cnt"), (cache_batch_idx, "cache_batch_idx")):
        if t is not None and t.dtype != torch.int32:
            raise RuntimeError(name + " must have dtype int32")
    if row0.shape != (B,) or keep_cnt.shape != (B,) or (cache_batch_idx is not None and cache_batch_idx.shape != (B,)):
        raise RuntimeError("row0, keep_cnt and cache_batch_idx must have one entry per row of keep_idx")
    if cache_batch_idx is None and k_cache.shape[0] < B:
        raise RuntimeError("batch size of the cache is smaller than the batch size of keep_idx")
    if B == 0:
        return
    row0, keep_idx, keep_cnt = row0.contiguous(), keep_idx.contiguous(), keep_cnt.contiguous()
    cbi = cache_batch_idx.contiguous() if cache_batch_idx is not None else None
    args = (k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2),
            v_cache.stride(0), v_cache.stride(1), v_cache.stride(2), row0.data_ptr(),
            cbi.data_ptr() if cbi is not None else None, keep_idx.data_ptr(), keep_cnt.data_ptr(), B, n_draft, k_cache.shape[2], k_cache.shape[3])
    if k_cache.dtype == torch.float8_e4m3fn:      # (elements = bytes: the strides already are byte counts)
        rc = K.klib().vattn_cache_keep_rows_fp8(*args, K.current_stream_ptr(k_cache.device))
    else:
        rc = K.klib().vattn_cache_keep_rows(*args, K.dtype_code(k_cache.dtype), K.current_stream_ptr(k_cache.device))
    if rc != 0:
        raise (NotImplementedError if rc == -10 else RuntimeError)(K.last_error())
