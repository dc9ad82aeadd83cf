"""The engine's release rule for a causal sliding window: which token a slot may be released up to before an iteration's
kernels are launched (include/vattn.h, vattn_release_prefix; include/vattn_kernels.h, no-read contract).

Pure integer arithmetic, shared by the cache engine, the trace replay and the tests.
"""
from __future__ import annotations

RELEASE_ALIGN = 64      # the prefill kernels' key tile (the decode kernels' is 32): a windowed call loads no K/V row below
                        # align_down(first key visible to the entry's first query row, tile)


def keep_from_prompt(processed: int, left: int) -> int:
    """A prompt chunk whose first query row sits at position `processed` (the keys already cached): that row sees keys
    [processed - left, processed]."""
    return max(0, processed - left) // RELEASE_ALIGN * RELEASE_ALIGN


def keep_from_decode(ctx: int, left: int) -> int:
    """A decode token at position ctx - 1 (`ctx` = the slot's length of the iteration, the new token included)."""
    return max(0, ctx - 1 - left) // RELEASE_ALIGN * RELEASE_ALIGN


def pages_below(keep_from_token: int, row_bytes: int, page_size: int) -> int:
    """Page positions that lie wholly below token `keep_from_token` — in bytes, as the manager counts them."""
    return keep_from_token * row_bytes // page_size
