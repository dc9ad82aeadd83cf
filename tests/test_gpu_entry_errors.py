"""flash_attn_with_kvcache and flash_attn_tree_with_kvcache share one argument normaliser and block builder (vattention_amd/flash_attn.py,
_build_block): for every bad argument the two entry points have in common they raise the same exception type with the same message — the
kvcache entry's wording, which mirrors the reference's flash_api.cpp — and nothing reaches a launcher."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, SQ, HQ, HKV, D, ROWS = 2, 2, 4, 2, 64, 64


def _good():
    torch.manual_seed(7)
    r = lambda *s: torch.randn(*s, dtype=torch.float16, device=DEV)
    return dict(q=r(B, SQ, HQ, D), k_cache=r(B, ROWS, HKV, D), v_cache=r(B, ROWS, HKV, D), k=r(B, SQ, HKV, D), v=r(B, SQ, HKV, D),
                cache_seqlens=torch.tensor([10, 20], dtype=torch.int32, device=DEV))


def _cpu_tensor(a):
    a["q"] = a["q"].cpu()


def _v_cache_dtype(a):
    a["v_cache"] = a["v_cache"].to(torch.bfloat16)


def _seqlens_int64(a):
    a["cache_seqlens"] = a["cache_seqlens"].long()


def _batch_idx_int64(a):
    a["cache_batch_idx"] = torch.tensor([1, 0], dtype=torch.int64, device=DEV)


def _k_without_v(a):
    a["v"] = None


def _k_without_seqlens(a):
    a["cache_seqlens"] = None


def _k_longer_than_the_cache(a):
    a["k"], a["v"] = (torch.zeros(B, ROWS + 1, HKV, D, dtype=torch.float16, device=DEV) for _ in range(2))


def _out_shape(a):
    a["out"] = torch.empty(B, SQ, HQ + 1, D, dtype=torch.float16, device=DEV)


def _cache_batch_too_small(a):
    a["k_cache"], a["v_cache"] = a["k_cache"][:1], a["v_cache"][:1]


BAD = [_cpu_tensor, _v_cache_dtype, _seqlens_int64, _batch_idx_int64, _k_without_v, _k_without_seqlens, _k_longer_than_the_cache, _out_shape,
       _cache_batch_too_small]


@pytest.mark.parametrize("spoil", BAD, ids=[f.__name__[1:] for f in BAD])
def test_shared_bad_arguments_raise_alike_on_both_entry_points_and_launch_nothing(spoil):
    from vattention_amd import flash_attn as FA
    args = _good()
    spoil(args)
    q, k_cache, v_cache = args.pop("q"), args.pop("k_cache"), args.pop("v_cache")
    mask = torch.ones(SQ, SQ, dtype=torch.bool, device=DEV).tril()
    launched, real = [], (FA._launch, FA._launch_tree)
    FA._launch = lambda p, dev, keep=(): launched.append(p)
    FA._launch_tree = lambda p, mask, dev, keep=(): launched.append(p)
    try:
        with pytest.raises(Exception) as plain:
            FA.flash_attn_with_kvcache(q, k_cache, v_cache, **args)
        with pytest.raises(Exception) as tree:
            FA.flash_attn_tree_with_kvcache(q, k_cache, v_cache, mask, **args)
    finally:
        FA._launch, FA._launch_tree = real
    print("%s: %s(%r)" % (spoil.__name__, plain.type.__name__, str(plain.value)))
    assert plain.type is RuntimeError and str(plain.value)
    assert tree.type is plain.type and str(tree.value) == str(plain.value)
    assert not launched
