"""Model of `vattn_release_prefix` (include/vattn.h) in plain Python.  TEST INFRASTRUCTURE ONLY.

The reference allocator only grows and shrinks a slot at its tail, so there is nothing to restate: this file IS the
specification of the sliding-window half of the page manager, written on top of the restated reference
(oracle.pagemgr.PageManagerOracle, with the product's refcounted shared pages).  Slot r's mapped page positions are
[head[r], mapped_pages[r]); head is 0 until release_prefix is called, and every routine of the base class sees the prefix it
was written for.

Rules (each pinned by tests/test_prefix_release.py against libvattn_amd.so):
  1. release_prefix(slot, keep) unmaps positions [head, P), P = floor(keep * row_bytes / page_size) — in BYTES, so that no byte
     of row `keep` or above loses its mapping where a row straddles two pages; pages return to the pool K then V, layers in
     order, positions ascending; a shared group forgets the holder.
  2. slot out of range / inactive / keep > length: ValueError, nothing changed.  P <= head: 0.
  3. tail reclamation never goes below head.
  4. a hole never outlives its occupant: free_batch_idx, or a step that passes length 0, unmaps all the slot still holds
     (tail first, like release_kvcache_pages_some) and head returns to 0.
  5. a step with a non-zero length below the first token that lies wholly in mapped positions is a ValueError before any change.
"""
from __future__ import annotations

from typing import List, Tuple

from oracle.pagemgr import PageManagerOracle


class PrefixReleaseOracle(PageManagerOracle):
    def __init__(self, *a, **kw):
        kw["shared_page_refcount"] = True
        super().__init__(*a, **kw)
        self.head: List[int] = [0] * self.max_batch_size
        self.prefix_releases = 0
        self.prefix_pages_released = 0

    # ---- rule 1, 2
    def release_prefix(self, r: int, keep_from_token: int) -> int:
        self._check_release(r, keep_from_token)
        first = self.head[r]
        P = min(keep_from_token * self.virt_buff_size_per_token // self.page_size, self.mapped_pages[r])
        if P <= first:
            return 0
        for pos in range(first, P):
            off = r * self.virt_buff_size_per_req + pos * self.page_size
            for layer in ([0] if self.megacache else range(self.num_layers)):
                self._unmap_pages(r, layer, off)
            for g in self.shared:
                if (r, pos) in g:
                    g.remove((r, pos))
                    break
            self.shared = [g for g in self.shared if g]
        self.head[r] = P
        self.prefix_releases += 1
        self.prefix_pages_released += P - first
        return P - first

    def _check_release(self, r: int, keep_from_token: int) -> None:
        if not (0 <= r < self.max_batch_size):
            raise ValueError("slot out of range")
        if not self.is_active_req(r):
            raise ValueError("release_prefix: the slot is not active")
        if keep_from_token > self.curr_seq_lengths[r]:
            raise ValueError("release_prefix: keep_from_token exceeds the slot's length")

    def release_prefixes(self, pairs) -> int:
        """Several slots in one call: every pair is checked before anything changes, then each is released in order."""
        for r, keep in pairs:
            self._check_release(r, keep)
        return sum(self.release_prefix(r, keep) for r, keep in pairs)

    # ---- rule 3
    def release_kvcache_pages_some(self, r: int, retain: int) -> None:
        super().release_kvcache_pages_some(r, max(retain, self.head[r]))

    # ---- rule 4
    def _close_hole(self, r: int) -> None:
        super().release_kvcache_pages_some(r, self.head[r])
        self.mapped_pages[r] = self.head[r] = 0

    def free_batch_idx(self, r: int) -> None:
        super().free_batch_idx(r)
        if self.head[r]:
            self._close_hole(r)

    # ---- rule 5 (then rule 4 for the slots the step drops)
    def first_token_of_head(self, r: int) -> int:
        return -(-self.head[r] * self.page_size // self.virt_buff_size_per_token)

    def _before_step(self, seq_lens: List[int]) -> None:
        self._check_lens(seq_lens)
        for r in range(self.max_batch_size):
            if self.head[r] and seq_lens[r] and seq_lens[r] < self.first_token_of_head(r):
                raise ValueError("length lies in the released prefix")
        for r in range(self.max_batch_size):
            if self.head[r] and seq_lens[r] == 0:
                self.curr_seq_lengths[r] = 0
                self._close_hole(r)

    def step(self, seq_lens: List[int], eager_reclaim: bool) -> None:
        self._before_step(seq_lens)
        super().step(seq_lens, eager_reclaim)

    def step_async(self, seq_lens: List[int]) -> None:
        self._before_step(seq_lens)
        super().step_async(seq_lens)

    def cleanup(self) -> None:
        super().cleanup()                        # (stops at head: rule 3)
        self.mapped_pages = [0] * self.max_batch_size
        self.head = [0] * self.max_batch_size

    # ---- observable
    def ranges(self) -> List[Tuple[int, int]]:
        return [(self.head[r], self.mapped_pages[r]) for r in range(self.max_batch_size)]

    def mapped_groups(self) -> int:
        return sum(m - h for h, m in self.ranges())
