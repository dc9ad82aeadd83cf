"""The reference's OWN fa_vattn wrapper and cache-engine files import against the drop-ins (vattention / flash_attn /
sarathi.cache_ops) with inert stubs for the rest of sarathi's import closure, and bind to the MI355X-native symbols.  The files
are loaded as build() left them under oracle/_ref/pyref (tests/ref_loader.py); nothing is copied."""
import pytest

from tests import ref_loader


@pytest.mark.skipif(not ref_loader.available(), reason="reference wrapper/engine not built (oracle/_ref/pyref)")
def test_reference_wrapper_imports_against_dropins():
    with ref_loader.loaded() as ref:
        mod = ref.wrapper_mod
        import vattention_amd.cache_ops as co
        import vattention_amd.flash_attn as fa
        import vattention_amd.vattention as va
        assert mod.flash_attn_with_kvcache is fa.flash_attn_with_kvcache
        assert mod.cache_flat is co.cache_flat
        assert mod.vattention is va
        w = mod.VAttentionFlashAttentionWrapper.get_instance()
        for meth in ("init", "begin_forward", "set_batch_idx", "forward", "end_forward"):
            assert callable(getattr(w, meth))
        # the 13 functions the reference module exports (vattention.cu:614-637) all exist on the drop-in
        for fn in ("reserve_physical_pages", "init_kvcache", "cleanup", "set_verbose", "set_deferred_reclamation",
                   "show_kvcache_config", "show_allocator_state", "step", "map_common_pages", "step_async",
                   "alloc_new_batch_idx", "free_batch_idx", "num_free_kvblocks"):
            assert callable(getattr(va, fn))


def test_backend_registry_resolves_native_and_hybrid_backends():
    """attention/__init__.py:36-201 mirror: the fa_vattn family resolves to the native wrapper, fa_streams / fa_pod to the
    two-stream hybrid wrapper, CUDA-library backends fail by name (no silent substitution)."""
    import pytest
    from vattention_amd import attention as A
    prev = A.ATTENTION_BACKEND
    try:
        for name in ("fa_vattn", "FA_VATTN_SYNC", "fa_vattn_megacache"):
            A.set_attention_backend(name)
            assert type(A.get_attention_wrapper()).__name__ == "VAttentionFlashAttentionWrapper"
            assert A.is_vattention_backend() and not A.is_vLLM_backend()
        for name, cls in (("fa_streams", "VAttentionFlashAttentionStreamsWrapper"), ("fa_pod", "VAttentionFlashAttentionPodWrapper"),
                          ("fa_pod_megacache", "VAttentionFlashAttentionPodWrapper")):
            A.set_attention_backend(name)
            assert type(A.get_attention_wrapper()).__name__ == cls
            assert A.is_vattention_backend()
        for name in ("fi_vattn", "fa3_vattn", "fa_paged"):
            A.set_attention_backend(name)
            with pytest.raises(NotImplementedError):
                A.get_attention_wrapper()
        with pytest.raises(ValueError):
            A.set_attention_backend("no_such_backend")
    finally:
        A.ATTENTION_BACKEND = prev
