/*
 * vattn_kernels.h — C ABI of the gfx950 attention / KV-append kernels in libvattn_amd.so.
 *
 * These entry points are what the reference's FFI for this path binds:
 *   - vattn_flash_attn_with_kvcache  replaces flash_attn_cuda.fwd_kvcache
 *       (call sites /root/reference/sarathi-lean/sarathi/model_executor/attention/
 *        vattention_flashattention_wrapper.py:159-166 (prefill) and :194-205 (decode);
 *        semantics /root/reference/pod_attn/pod_attn/flash_attn_interface.py:1146-1291,
 *        argument rules /root/reference/pod_attn/pod_attn/flash_api.cpp:1291-1578;
 *        the parameter block is the plain-C analogue of Flash_fwd_params,
 *        /root/reference/pod_attn/pod_attn/flash.h:24-154)
 *   - vattn_cache_flat               replaces sarathi.cache_ops.cache_flat
 *       (/root/reference/sarathi-lean/csrc/cache_kernels.cu:482-570, cache.cpp:40-46)
 *
 * All pointers are DEVICE pointers; strides are in ELEMENTS; `stream` is a hipStream_t.
 * Every function returns 0 on success, a negative VATTN_K_* code otherwise, and never touches
 * key/value rows at or beyond a sequence's visible length (those virtual pages may be unmapped).
 */
#ifndef VATTN_KERNELS_H_
#define VATTN_KERNELS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VATTN_K_OK 0
#define VATTN_K_ERR_UNSUPPORTED (-10)   /* dtype / head_dim / layout not supported */
#define VATTN_K_ERR_INVALID (-11)       /* argument rule violated (message via vattn_kernels_last_error) */
#define VATTN_K_ERR_LAUNCH (-12)        /* HIP launch failure */

#define VATTN_DTYPE_F16 0
#define VATTN_DTYPE_BF16 1

#define VATTN_KERNELS_ABI 6u            /* bumped whenever vattn_attn_params changes */

/* ROW-STRIDE CEILING of the K/V caches, in BYTES (k_row_stride / v_row_stride x 2, x 1 for an fp8 cache): 2^24 - 16.  The kernels rebase a
 * 64-bit address per key tile and keep 32-bit byte offsets inside the tile; with S = the row's byte stride they form, in 32 bits,
 *   decode (32-row tiles)                  31 S + row bytes per lane, 16 S steps, num_records 32 S             -> S <  2^27
 *   register-staged prefill (64-row tiles) 63 S + row bytes per lane, num_records 64 S                          -> S <  2^26
 *   prefill64 / prefill64p (64-row tiles)  the same, 64 S per tile step, and the persistent kernel's piece offsets
 *                                          rows x S with a 24-BIT multiply (v_mad_u32_u24)                      -> S <  2^24
 *   append / cache_flat / keep_rows        64-bit throughout                                                    -> no limit
 * The host enforces the smallest for every call (strides are multiples of 16 bytes, hence - 16) and refuses a negative row stride: a
 * wrapped offset would also wrap the bound that keeps the loads off unmapped pages. */
#define VATTN_MAX_KV_ROW_STRIDE_BYTES ((int64_t)((1 << 24) - 16))

typedef struct vattn_attn_params {
    /* sizeof(vattn_attn_params) and VATTN_KERNELS_ABI of the header the CALLER was built against.  The block grows between releases
     * (the plan fields below are extensions) and the kernels branch on pointers inside it: a caller built against an older header, or
     * one that does not zero the block, would have the library read past its object.  Every entry point that takes the block checks
     * both words first and refuses a mismatch (VATTN_K_ERR_INVALID).  ZERO the block (memset) before filling it in. */
    uint32_t struct_size;
    uint32_t abi_version;
    /* q / out: [b, seqlen_q, h, d] */
    const void* q;
    void* out;
    int64_t q_batch_stride, q_row_stride, q_head_stride;
    int64_t o_batch_stride, o_row_stride, o_head_stride;
    /* caches: [batch_cache, seqlen_k, h_k, d]; last dim contiguous; batch and head strides any multiple of 8 elements (they enter
     * 64-bit address arithmetic only: slots and rows may lie any number of GiB into the view); ROW-STRIDE CEILING: 0 <= k_row_stride,
     * v_row_stride and row stride x bytes per cache element <= VATTN_MAX_KV_ROW_STRIDE_BYTES (below), else VATTN_K_ERR_UNSUPPORTED from
     * every call, 0 from every _workspace_bytes entry and the error from every _plan_describe entry
     * (the decode call passes a [:, :max_cache_len] strided view) */
    void* k_cache;
    void* v_cache;
    int64_t k_batch_stride, k_row_stride, k_head_stride;
    int64_t v_batch_stride, v_row_stride, v_head_stride;
    /* optional new keys/values [b, seqlen_knew, h_k, d], appended at row cache_seqlens[b] */
    const void* k_new;
    const void* v_new;
    int64_t knew_batch_stride, knew_row_stride, knew_head_stride;
    int64_t vnew_batch_stride, vnew_row_stride, vnew_head_stride;
    const int32_t* cache_seqlens;     /* int32[b] on device, or NULL: every sequence uses seqlen_k      */
    const int32_t* cache_batch_idx;   /* int32[b] on device, or NULL: identity                          */
    float* softmax_lse;               /* optional float[b, h, seqlen_q] (natural log), or NULL          */
    /* split-KV workspace; sized by vattn_attn_workspace_bytes, may be NULL if that returns 0.  Its contents on entry are arbitrary, the call
     * writes only inside [workspace, workspace + workspace_bytes), and the results do not depend on the prior contents
     * (tests/test_gpu_workspace.py; vattn_hybrid_attn's zeroed workspace is the one exception). */
    void* workspace;
    /* batched prefill of several sequences with DIFFERENT chunk lengths (MI355X extension; both NULL otherwise): q / out are
     * then [total_tokens, h, d] (q_batch_stride / o_batch_stride ignored), batch entry i owns rows
     * [q_start[i], q_start[i] + q_lens[i]) and seqlen_q is the maximum of q_lens (it sizes the grid) */
    const int32_t* q_start;           /* int32[b] on device */
    const int32_t* q_lens;            /* int32[b] on device */
    int32_t b, seqlen_q, seqlen_k, seqlen_knew, h, h_k, d;
    int32_t is_causal;                /* bottom-right aligned; ignored when seqlen_q == 1               */
    int32_t dtype;                    /* VATTN_DTYPE_*                                                  */
    int32_t num_splits;               /* 0 = heuristic                                                  */
    float softmax_scale;
    int32_t variant;                  /* 0 = default; debug variants select alternative operand paths   */
    int32_t max_seqlen_k_hint;        /* host-side upper bound of cache_seqlens[b] + seqlen_knew, or 0: unknown (seqlen_k is
                                         only the cache tensor's row count); used to size the prefill KV split            */
    /* Fused rotary position embedding (MI355X extension): when rotary_cos_sin != NULL the launch rotates q — and
     * k_new before it is appended / attended — in registers, NeoX style, with the arithmetic of the reference's stand-alone
     * kernel (/root/reference/sarathi-lean/csrc/pos_encoding_kernels.cu:9-77, every product and the sum rounded to the I/O
     * dtype).  Layout = the reference's cos_sin_cache: row `pos` holds cos[0 .. rotary_dim/2) then sin[0 .. rotary_dim/2), I/O
     * dtype, rows rotary_row_stride elements apart.  Token i of batch entry b sits at position cache_seqlens[b] + i (new keys)
     * resp. (visible keys - seqlen_q) + i (queries), i.e. the call-site convention of the wrapper.  rotary_dim must equal d.
     * A query row whose position is NEGATIVE (an entry without a visible key; seqlen_q > visible keys) has no table row: it is left
     * un-rotated and no table row is read for it.  With is_causal or a window such a row sees no key (output 0, LSE +inf); in a non-causal
     * call it attends to every key with its un-rotated q — a caller that wants those rows rotated passes at most as many rows as keys. */
    const void* rotary_cos_sin;
    int64_t rotary_row_stride;
    int32_t rotary_dim;
    int32_t rotary_reserved;
    /* Length-balanced split-KV of a RAGGED decode batch (MI355X extension; all three zero otherwise).  The reference's heuristic
     * (flash_api.cpp:258-323) gives every sequence of a batch the same number of splits, so a launch lasts as long as the longest
     * sequence's split (a 30 k-token sequence beside 4 k-token ones: 3 x the average).  A caller that knows the lengths on the host
     * (the attention wrapper does) asks vattn_decode_plan for work items of near-equal length — sequence b is cut into
     * ceil(tiles_b / T) pieces of T 32-key tiles — copies the two tables to the device once per iteration and passes them with every
     * layer's call.  decode form only; results equal the uniform split's up to the order of the fp32 merge. */
    const struct vattn_decode_item* split_items;   /* device: num_split_items entries                         */
    const int32_t* split_seq;                      /* device: int32[2 * b] = (first item, item count) per sequence */
    int32_t num_split_items;
    int32_t split_reserved;
    /* Work list of an underfilled / unbalanced PREFILL launch (MI355X extension; all zero otherwise; d = 128).  A causal prompt on a
     * tensor-parallel shard has few heads and query blocks whose key walk grows linearly: the launch lasts as long as its longest
     * block, and cutting EVERY block's key range in n shares multiplies the fp32 partial traffic by n.  vattn_prefill_plan lists the
     * (entry, head, 256-row query block, key-tile range) pieces longest first and cuts only the blocks longer than the per-CU average:
     * short blocks write their output directly, long ones write partials that vattn merges (one wave per row) in a second launch.  The
     * caller copies the tables to the device — once per iteration, the plan depends on the lengths only — and passes them with every
     * layer's call.  Results equal the default launch's up to the order of the fp32 merge. */
    const struct vattn_prefill_item* pf_items;     /* device: num_pf_items pieces, longest first                                */
    const struct vattn_prefill_item* pf_blocks;    /* device: num_pf_blocks SPLIT query blocks (what the merge pass walks)      */
    int32_t num_pf_items, num_pf_blocks;
    int32_t pf_part_rows;                          /* fp32 partial rows of all split blocks (sizes the workspace)               */
    /* PERSISTENT form of the work list (round 5; both zero: one workgroup per piece, in list order).  vattn_prefill_plan_wg also
     * ASSIGNS the pieces: pf_items is grouped by workgroup, workgroup w owns pieces [pf_wg_first[w], pf_wg_first[w + 1]) and walks them
     * in that order without stopping its K / V tile stream between them (csrc/prefill64p_kernels.hip: the next piece's Q block and
     * first tiles are fetched under the current piece's last tiles; one workgroup per CU).  pf_wg_first has pf_num_wg + 1 entries.
     * pf_num_wg > 0 with pf_wg_first == NULL: DRAWN queues — pf_items stays in longest-first order, workgroup w starts with piece w and
     * draws further pieces of its XCD's sub-sequence from a library-owned counter, which balances what a static assignment cannot (the
     * workgroups differ in speed by a few per cent).  What vattn_prefill_plan_wg(wg_first_out = NULL) prepares. */
    int32_t pf_num_wg;
    const int32_t* pf_wg_first;                    /* device: int32[pf_num_wg + 1]                                              */
    /* Causal SLIDING WINDOW (flash_attn_interface.py:1204-1206, mask.h:36-60; both zero: no window — a zeroed block attends as before).
     * window_left_plus1 = left + 1 > 0: query row i of a call with Sq query rows and Lk visible keys attends keys j with
     * max(0, i + Lk - Sq - left) <= j <= i + Lk - Sq (bottom-right aligned; left = 0: the own position only).  seqlen_q > 1 needs is_causal
     * (non-causal / right-sided windows: VATTN_K_ERR_UNSUPPORTED); the decode form ignores is_causal as it does without a window.  Not
     * together with split_items / pf_items (VATTN_K_ERR_INVALID): a windowed key walk is bounded by left + 256 rows per query block, there
     * is no imbalance for a host plan to remove, and the three planners return 0 ("default launch") for a block that carries a window.
     * NO-READ CONTRACT: a windowed call issues no K or V load for a row below align_down(first key visible to the FIRST query row of
     * batch entry b, T), T = the kernel's key tile: 32 for the decode kernels (decode_kernel, decode_stream_kernel), 64 for the prefill
     * kernels (prefill_kernel, prefill64_kernel).  Rows inside that first tile but left of a row's limit may be loaded; they are masked
     * before the softmax.  (What releasing the physical pages in front of the window will rest on.) */
    int32_t window_left_plus1;
    int32_t window_reserved;                       /* must be 0 */
} vattn_attn_params;

typedef struct vattn_prefill_item {
    int32_t b, h, qb;     /* batch entry, query head, 256-row query block                                                    */
    int32_t tile_begin;   /* first 64-key tile of the piece (pf_blocks: unused)                                              */
    int32_t tile_end;     /* one past its last tile; INT32_MAX for the block's last share: "to the last tile the block sees" —
                             the kernel clamps every range to what the DEVICE-side lengths give, so a list built from stale
                             host lengths costs balance, never keys                                                          */
    int32_t nshares;      /* pieces the query block was cut into; 1 = this piece writes the output rows itself               */
    int32_t part_row;     /* nshares > 1: first of this piece's 256 partial rows (pf_blocks: of the block's share 0; share s
                             sits 256 * s rows further)                                                                      */
    int32_t reserved;     /* 1 on the block's last share                                                                     */
} vattn_prefill_item;

typedef struct vattn_decode_item {
    int32_t b;            /* batch entry                                            */
    int32_t tile_begin;   /* first 32-key tile of the piece                         */
    int32_t tile_end;     /* one past its last tile; INT32_MAX on the sequence's last piece (open-ended, see vattn_prefill_item) */
    int32_t index_in_seq; /* 0 .. count-1 within the sequence                       */
} vattn_decode_item;

/* Bytes of split-KV workspace the call will need: the decode form's partials, or the prefill form's when its grid
 * would underfill the chip and the key range is split across workgroups (0 otherwise). */
size_t vattn_attn_workspace_bytes(const vattn_attn_params* p);

/* Host-side planner of the length-balanced decode split (see vattn_attn_params.split_items).  `p` describes the call (b, h, h_k, d,
 * seqlen_knew, variant; pointers are not read), cache_seqlens_host[b] are the values the device array will hold.  Writes at most
 * `cap` items and 2 * b ints of (first item, count); returns the number of items, 0 when the uniform split is at least as good
 * (equal lengths, one sequence, batches whose uniform split is already balanced; a block that carries a sliding window: the device
 * plan balances by VISIBLE length, host items are refused with one) or the tables would not fit, < 0 on bad arguments.
 * p->num_splits = -T forces pieces of T tiles (tests, A/B measurements); the call itself is then made with num_splits = 0.
 * Pure host arithmetic (no device access): usable, and tested, without a GPU. */
int32_t vattn_decode_plan(const vattn_attn_params* p, const int32_t* cache_seqlens_host, vattn_decode_item* items_out, int32_t cap,
                          int32_t* seq_out);

/* Host-side planner of the prefill work list (see vattn_attn_params.pf_items).  `p` describes the call (b, seqlen_q, h, h_k, d,
 * is_causal; pointers are not read); q_lens_host[b] are the chunk lengths (NULL: every entry has seqlen_q rows), k_lens_host[b] the
 * visible keys of each entry (cache length + new tokens).  Writes at most cap_items / cap_blocks entries and counts_out[3] =
 * {items, split blocks, partial rows}; returns the number of items, 0 when the default launch is at least as good (grids that fill
 * the chip with balanced work, short key walks, head dimensions other than 128; a block that carries a sliding window: every query
 * block's key walk is then bounded by left + 256 rows, nothing grows down the prompt) or a table would not fit, < 0 on bad arguments.
 * p->num_splits = -T forces pieces of at most T tiles (tests, A/B measurements).  Pure host arithmetic. */
int32_t vattn_prefill_plan(const vattn_attn_params* p, const int32_t* q_lens_host, const int32_t* k_lens_host, vattn_prefill_item* items_out,
                           int32_t cap_items, vattn_prefill_item* blocks_out, int32_t cap_blocks, int32_t* counts_out);

/* The same plan for PERSISTENT workgroups (vattn_attn_params.pf_num_wg / pf_wg_first): pieces are priced with the chained overhead
 * (a piece that follows another in a workgroup's queue pays its epilogue and a fragment of a tile, not a cold prologue), so finer cuts
 * pay off, and are assigned to at most `max_wg` workgroups (<= 0: one per CU, 256) longest first, each to the least loaded one among
 * the workgroups of its kv head's XCD class (workgroup w runs on XCD w % 8; class = kv head modulo the classes that divide 8, so that an
 * XCD's L2 keeps seeing one kv head).  items_out comes back GROUPED by workgroup; wg_first_out receives num_wg + 1 offsets — THE
 * CALLER PROVIDES ROOM FOR (max_wg > 0 ? max_wg : 256) + 1 = at most 257 int32 VALUES (the function has no capacity argument for it);
 * counts_out[4] = {items, split blocks, partial rows, num_wg}.  wg_first_out == NULL: no assignment (drawn queues, see pf_num_wg):
 * items_out stays longest first, only num_wg is chosen.  Returns the number of items (0: default launch, as above — always for a block
 * that carries a sliding window: the persistent kernel is not built for one). */
int32_t vattn_prefill_plan_wg(const vattn_attn_params* p, const int32_t* q_lens_host, const int32_t* k_lens_host, vattn_prefill_item* items_out,
                              int32_t cap_items, vattn_prefill_item* blocks_out, int32_t cap_blocks, int32_t* wg_first_out, int32_t max_wg,
                              int32_t* counts_out);

/* What vattn_flash_attn_with_kvcache will launch for `p` — pure host arithmetic on the shapes (pointers are only tested for NULL), so a
 * test can pin the launch plans without a GPU and without a stopwatch (tests/test_plan_table.py; the reference's equivalents are the
 * launch heuristics of flash_api.cpp:258-323 and flash_fwd_launch_template.h:100-162).  Returns 0, or VATTN_K_ERR_INVALID. */
typedef struct vattn_plan_desc {
    int32_t form;          /* 0 = prefill (seqlen_q > 1), 1 = the decode kernels: seqlen_q == 1, or the multi-token form           */
    int32_t path;          /* prefill: 0 = grid order, 1 = work list (pf_items).  decode: 0 = uniform split of every sequence (grid
                              heuristics), 1 = host item plan (split_items), 2 = device-planned stream decomposition               */
    int32_t tiling;        /* prefill: 1 = 8 waves x 32 rows, 4 = 4 waves x 32 rows, 7 = prefill64 (4 waves x 64 rows).
                              decode: 16-head blocks per workgroup (1 or 2; multi-token form: 16-column blocks)                   */
    int32_t nsplit;        /* key-range shares per work item of the grid paths (1 = none); 0 on the list / item / stream paths      */
    int32_t workgroups;    /* workgroups of the main launch that hold work (grid padding excluded)                                 */
    int32_t merge_launch;  /* 1 = a second launch merges fp32 partials                                                             */
    int64_t workspace_bytes;
} vattn_plan_desc;
int vattn_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out);

/* flash_attn_with_kvcache: appends k_new/v_new (if given) and attends; prefill form (seqlen_q > 1,
 * causal chunk against the growing cache) and decode form (seqlen_q == 1, split-KV + combine).
 *
 * MULTI-TOKEN FORM (the verify step of speculative decoding / multi-token prediction: a few query rows per entry against a long
 * cache).  The split-KV decode kernels run the call — the MFMA columns that hold a kv head's G = h / h_k query heads hold
 * seqlen_q * G (token, head) pairs, every K/V row is read once per kv head — instead of the prefill kernels' 128- / 256-row query
 * blocks.  GATE, all of: 2 <= seqlen_q <= 8 and seqlen_q * G <= 64; q_lens, pf_items, split_items and rotary_cos_sin NULL; `variant`
 * tiling bits 1-3 zero; num_splits <= 0 (< 0 keeps its decode meaning: forced workgroups per kv head / pieces); the product library (a
 * -DVATTN_LAB build has no such kernels).  Every other block behaves as before: an explicit prefill tiling or num_splits > 0 keeps the
 * prefill kernels for the same call (the A/B selector), as do fused-rotary calls; split_items and vattn_hybrid_attn's decode block stay
 * seqlen_q == 1.  vattn_attn_workspace_bytes and vattn_attn_plan_describe (form 1) answer for the form the call will take.
 * VISIBILITY: with Lk = cache_seqlens[b] + seqlen_knew visible keys, query row t sees keys j <= Lk - seqlen_q + t when is_causal and
 * all j < Lk otherwise; with window_left_plus1 > 0 (needs is_causal) also j >= max(0, Lk - seqlen_q + t - left).  A row without a
 * visible key (Lk - seqlen_q + t < 0) gives 0 and LSE +inf.  out[b, t, h, :] through o_row_stride; softmax_lse [b, h, seqlen_q].
 * APPEND: k_new / v_new (seqlen_knew rows, any count) land at rows cache_seqlens[b] .. before the attention launch on the same stream,
 * bit-exact, nothing else in the cache is touched.  CONTRACT: as everywhere — no K/V load at or beyond Lk; in a windowed call none
 * below align_down(first key visible to the entry's FIRST query row, 32). */
int vattn_flash_attn_with_kvcache(const vattn_attn_params* p, void* stream);

/* TREE-MASKED MULTI-TOKEN FORM (verifying a draft TREE — Medusa, EAGLE, SpecInfer — in one pass over the cache: a node sees its ancestors,
 * not its siblings).  The multi-token form above with the causal rule among the draft rows replaced by a caller-given bit mask.  The mask
 * travels BESIDE the parameter block — vattn_attn_params and VATTN_KERNELS_ABI are unchanged — as an extra argument of builds of the decode
 * kernels of their own; every other kernel is what it was.
 * MASK: tree_mask is DEVICE memory, uint32[b * seqlen_q], one word per (entry, query token); only the low seqlen_q bits are read; the
 * host never dereferences it.  VISIBILITY: with Lk = cache_seqlens[b] + seqlen_knew visible keys (clamped to the view as everywhere) and
 * base = Lk - seqlen_q, query token t of entry b sees every key j < base (the committed context) and draft key base + s iff bit s of
 * tree_mask[b * seqlen_q + t] is set and base + s >= 0.  is_causal is ignored.  Any bit pattern is legal: no topological order and no self
 * bit are required; a row without a visible key gives 0 and LSE +inf.  out, softmax_lse, strides and cache_batch_idx as in the multi-token
 * form; k_new / v_new are appended by the same launch in front of the attention launch, bit-exact.  A chain is mask word t =
 * (2 << t) - 1 (the causal multi-token call), all ones the non-causal one — equal to those calls up to the order of the fp32 sums.
 * GATE: tree_mask == NULL delegates to vattn_flash_attn_with_kvcache(p, stream), unchanged.  Otherwise the block must take the multi-token
 * form (its gate above: 2 <= seqlen_q <= 8, seqlen_q * G <= 64, no q_lens / pf_items / split_items / rotary_cos_sin, tiling bits zero,
 * num_splits <= 0, the product library), else VATTN_K_ERR_UNSUPPORTED with a message that names the rule; window_left_plus1 > 0 beside a
 * mask is VATTN_K_ERR_INVALID (a tree node's position is its depth, not its index: an index-based window would be wrong).
 * vattn_tree_attn_workspace_bytes and vattn_tree_attn_plan_describe (form 1) answer what the multi-token call of the same block gets: the
 * same planners, grids and workspace, nothing is tuned apart.  CONTRACT: no K/V load at or beyond Lk.  Draft keys a row must not see ARE
 * loaded (they are other rows' keys) and masked before the softmax: they must hold finite-or-not data like any visible row, never sit on
 * unmapped pages.  The keys that columns disagree about lie in at most two 32-key tiles at the tail; only those take the masked path. */
int vattn_tree_attn_with_kvcache(const vattn_attn_params* p, const uint32_t* tree_mask, void* stream);
size_t vattn_tree_attn_workspace_bytes(const vattn_attn_params* p);
int vattn_tree_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out);

/* Compaction of the ACCEPTED path behind a tree-masked verify call, so that the virtually contiguous cache is contiguous again: for entry
 * b (cache slot cache_batch_idx[b], identity if NULL) and i < keep_cnt[b], row row0[b] + i receives row row0[b] + keep_idx[b * n_draft + i],
 * for K and V and all h_k kv heads.  keep_idx is strictly ascending per entry (so keep_idx[i] >= i; an index that is not is skipped).  In
 * place and race-free: a thread owns one 16-byte chunk column, reads that chunk of all kept rows into registers, then stores them.  No
 * other byte of the cache is written; rows at or past row0 + keep_cnt keep their contents.  The caller guarantees that rows
 * [row0, row0 + n_draft) lie inside the cache view.  All index arrays are DEVICE int32.  Limits: n_draft <= 8, 2-byte dtypes
 * (VATTN_DTYPE_*; an fp8 cache: vattn_cache_keep_rows_fp8 below), d 64 / 128, strides multiples of 8 elements — anything else is
 * VATTN_K_ERR_UNSUPPORTED. */
int vattn_cache_keep_rows(void* k_cache, void* v_cache, int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                          int64_t v_batch_stride, int64_t v_row_stride, int64_t v_head_stride,
                          const int32_t* row0,            /* device int32[b]: first draft row of each entry */
                          const int32_t* cache_batch_idx, /* or NULL */
                          const int32_t* keep_idx,        /* device int32[b * n_draft], strictly ascending per entry */
                          const int32_t* keep_cnt,        /* device int32[b], 0..n_draft */
                          int32_t b, int32_t n_draft, int32_t h_k, int32_t d, int32_t dtype, void* stream);

/* vattn_cache_keep_rows over an fp8 (e4m3) cache — the compaction behind vattn_fp8kv_tree_attn_with_kvcache below.  The arguments of
 * vattn_cache_keep_rows without `dtype`: elements are single bytes, strides are in bytes.  The same contract: in place and race-free (a thread
 * owns one 16-byte chunk column — 16 elements — and reads that chunk of all kept rows before it stores them), no other byte of the cache is
 * written, rows at or past row0 + keep_cnt keep their contents, bytes are moved as they are (no scale is read: a row keeps its kv heads'
 * scales).  Limits: n_draft <= 8, d 64 / 128 (4 / 8 chunks per row and head), row / head / batch strides multiples of 16, 16-byte aligned
 * bases — anything else is VATTN_K_ERR_UNSUPPORTED. */
int vattn_cache_keep_rows_fp8(void* k_cache, void* v_cache, int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                              int64_t v_batch_stride, int64_t v_row_stride, int64_t v_head_stride,
                              const int32_t* row0,            /* device int32[b]: first draft row of each entry */
                              const int32_t* cache_batch_idx, /* or NULL */
                              const int32_t* keep_idx,        /* device int32[b * n_draft], strictly ascending per entry */
                              const int32_t* keep_cnt,        /* device int32[b], 0..n_draft */
                              int32_t b, int32_t n_draft, int32_t h_k, int32_t d, void* stream);

/* FP8 KV CACHE (OCP e4m3): halves the K/V bytes a decode step reads, doubles the tokens per physical page.  Additive: vattn_attn_params and
 * VATTN_KERNELS_ABI are unchanged, the scale pointers travel BESIDE the parameter block as extra arguments of builds of the decode kernels
 * — and of the register-staged prefill kernels: "Prefill over an fp8 cache" below — of their own; every other kernel and entry point is what it was.
 * STORAGE: OCP float8_e4m3fn, one byte per element, caches of the usual shape [batch_cache, rows, h_k, d]; last dimension contiguous, the
 * other strides multiples of 16 elements (16-byte chunks).  SCALES: k_scale, v_scale are DEVICE float32[h_k], positive and finite; the host
 * never dereferences them (calls stay graph-capturable).  value = stored * scale.
 * QUANTISER (one answer for every input): (1) inv = 1.0f / scale by IEEE fp32 division, once per head; (2) y = float(x) * inv in fp32;
 * (3) y is clamped to +-448 explicitly (v_med3), no conversion mode is relied on; (4) fp32 -> e4m3 with round-to-nearest-even; (5) a NaN
 * input stores the NaN byte (0x7f, with the input's sign bit).  Bit-for-bit
 * (x.float() * (1.0 / scale)).clamp(-448, 448).to(torch.float8_e4m3fn) on the CPU.
 * READING: the decode kernels widen the bytes to the I/O dtype in registers — exact, e4m3 has 3 mantissa bits and |x| <= 448 — and run the
 * f16 / bf16 MFMAs; q and P are not quantised.  The scales never touch an element: k_scale[hk] folds into the workgroup's softmax scale,
 * v_scale[hk] into the final 1 / l normalisation (fp32, wave-uniform), so against the 2-byte kernels run on the dequantised values no
 * rounding step is added. */

/* cache_flat into an fp8 cache: k_cache[t*k_cache_stride + i] = quantise(key[t*key_stride + i], k_scale[i / head_size]), same for value,
 * t < num_tokens, i < num_heads*head_size; nothing else is written (vattn_cache_flat's contract).  key / value are src_dtype
 * (VATTN_DTYPE_F16 / _BF16), source strides in source elements, cache strides in bytes.  Whole 16-byte chunks are stored where head_size,
 * the strides and the pointers allow (head_size % 16 == 0, source strides % 8 == 0, cache strides % 16 == 0, 16-byte aligned pointers). */
int vattn_cache_flat_fp8(const void* key, const void* value, void* k_cache, void* v_cache, int64_t num_tokens, int32_t num_heads,
                         int32_t head_size, int64_t key_stride, int64_t value_stride, int64_t k_cache_stride, int64_t v_cache_stride,
                         int32_t src_dtype, const float* k_scale, const float* v_scale, void* stream);

/* Decode over an fp8 cache.  p->dtype is the dtype of q / out / k_new / v_new (f16 or bf16); k_cache / v_cache point at fp8 bytes and their
 * strides are in elements = bytes.  k_new / v_new (any count) are quantised into rows cache_seqlens[b] .. by an append launch in front of
 * the attention launch on the same stream (no fused in-kernel append, no fused rotary in these builds).
 * GATE: the one-token decode form (seqlen_q == 1) and the causal / non-causal multi-token form (its gate above).  Refused with
 * VATTN_K_ERR_UNSUPPORTED and a message that names the rule: window_left_plus1 > 0, rotary_cos_sin, split_items, q_lens / pf_items, the
 * prefill form, a -DVATTN_LAB build.  A tree mask has an entry point of its own (vattn_fp8kv_tree_attn_with_kvcache below); vattn_hybrid_attn
 * has no fp8 entry point: its caches are 2-byte.  NULL scales: VATTN_K_ERR_INVALID.
 * PLAN: planners, grids, stream decomposition, record layouts, merge / combine kernels and workspace sizes are those of
 * vattn_flash_attn_with_kvcache for the same block — nothing is tuned apart; partials are fp32, published already scaled by v_scale, and do
 * not know the cache dtype.  vattn_fp8kv_attn_workspace_bytes / _plan_describe answer what that call gets (0 / an error outside the gate).
 * CONTRACT: as everywhere — no K/V load at or beyond Lk = cache_seqlens[b] + seqlen_knew. */
int vattn_fp8kv_attn_with_kvcache(const vattn_attn_params* p, const float* k_scale, const float* v_scale, void* stream);
size_t vattn_fp8kv_attn_workspace_bytes(const vattn_attn_params* p);
int vattn_fp8kv_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out);

/* TREE-MASKED MULTI-TOKEN FORM over an fp8 cache: verifying a draft tree against e4m3 K/V — the tree-masked form and the fp8 decode call above,
 * multiplied: builds of the decode kernels of their own whose last argument carries the mask words AND the scale pointers; every other
 * kernel, entry point and refusal is what it was (vattn_tree_attn_with_kvcache still takes 2-byte caches only, vattn_fp8kv_attn_with_kvcache
 * still refuses a window).  Conventions of the fp8 decode call: p->dtype is the dtype of q / out / k_new / v_new, cache strides in bytes,
 * device scales the host never dereferences; of the tree call: tree_mask is device uint32[b * seqlen_q], only the low seqlen_q bits of a
 * word are read, never by the host — calls stay graph-capturable.
 * VISIBILITY: the tree call's, on the stored values — with Lk = cache_seqlens[b] + seqlen_knew (clamped to the view) and base = Lk -
 * seqlen_q, query token t sees every key j < base and draft key base + s iff bit s of tree_mask[b * seqlen_q + t] is set and base + s >= 0;
 * is_causal is ignored; any bit pattern is legal; a row without a visible key gives 0 and LSE +inf.  value = stored * scale: k_scale[hk]
 * folds into the softmax scale, v_scale[hk] into the final 1 / l and into published partials; the bytes are widened in registers (exact) and
 * the mask is a select on the scores of the at most two tail tiles: no rounding step is added over either parent.  A chain (word t =
 * (2 << t) - 1) equals the causal multi-token fp8 call, all ones the non-causal one, up to the order of the fp32 sums.  k_new / v_new are
 * quantised into rows cache_seqlens[b] .. by the append launch in front of the attention launch (vattn_cache_flat_fp8's bytes).
 * GATE: tree_mask == NULL delegates to vattn_fp8kv_attn_with_kvcache(p, k_scale, v_scale, stream), unchanged.  Otherwise the block must take
 * the multi-token form (its gate above: 2 <= seqlen_q <= 8, seqlen_q * G <= 64, no q_lens / pf_items / split_items / rotary_cos_sin, tiling
 * bits zero, num_splits <= 0, the product library) and carry nothing the fp8 decode gate refuses, else VATTN_K_ERR_UNSUPPORTED with a message
 * that names the rule; window_left_plus1 > 0 beside a mask is VATTN_K_ERR_INVALID as in the 2-byte tree call; NULL scales are
 * VATTN_K_ERR_INVALID, and the fp8 stride / alignment rules hold (cache strides multiples of 16, k_new / v_new 16-byte aligned).
 * PLAN: planners, grids, stream decomposition, record layout, merges and workspace are those of the multi-token call on the same block —
 * vattn_fp8kv_tree_attn_workspace_bytes / _plan_describe answer exactly what vattn_tree_attn_workspace_bytes / _plan_describe answer (0 / an
 * error outside the gate); nothing is tuned apart.
 * CONTRACT: no K/V load at or beyond Lk.  Draft keys a row must not see ARE loaded (they are other rows' keys) and masked before the softmax:
 * they must hold data like any visible row, never sit on unmapped pages.  vattn_cache_keep_rows_fp8 compacts the accepted path afterwards. */
int vattn_fp8kv_tree_attn_with_kvcache(const vattn_attn_params* p, const uint32_t* tree_mask, const float* k_scale, const float* v_scale,
                                       void* stream);
size_t vattn_fp8kv_tree_attn_workspace_bytes(const vattn_attn_params* p);
int vattn_fp8kv_tree_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out);

/* Prefill over an fp8 cache: chunk n of a prompt attends to chunks 0 .. n-1 as the fp8 bytes they were stored as.  Same conventions as the
 * decode call above (p->dtype, strides in bytes, device scales, stride / alignment rules).  Builds of their own of the register-staged
 * prefill kernels (8 / 4 waves x 32 rows, d = 64 / 128, f16 / bf16): a 16-byte load is 16 consecutive d of one key, widened on its way
 * into LDS — the LDS image is the 2-byte kernel's for the unscaled values, everything behind it is that kernel; k_scale[hk] folds into the
 * softmax scale and the LSE, v_scale[hk] into the final 1 / l, also of the published fp32 partials (the merge does not know the dtype).
 * APPEND: k_new / v_new are quantised into rows cache_seqlens[b] .. by an append launch in front of the attention launch on the same
 * stream, so the chunk attends to its OWN keys AS STORED — exactly what a later decode step reads, not the 2-byte values it was given.
 * GATE: the prefill form — every block the decode gate above does not take — causal or not, with or without cache_batch_idx, softmax_lse,
 * batched chunks (q_start / q_lens; k_new then stays refused as everywhere: append with vattn_cache_flat_fp8 first).  Refused with
 * VATTN_K_ERR_UNSUPPORTED and a message that names the rule: a decode-form block (call vattn_fp8kv_attn_with_kvcache), window_left_plus1 > 0,
 * rotary_cos_sin, pf_items / pf_num_wg, split_items, explicit tiling 7 (prefill64 moves its tiles by LDS-DMA and has no fp8 build), d other
 * than 64 / 128, a -DVATTN_LAB build.  NULL scales: VATTN_K_ERR_INVALID.
 * PLAN: that of vattn_flash_attn_with_kvcache for the same block with its prefill64 branch skipped — tiling 1 or 4 and the split count
 * those rules give, the same grid, workgroup order and workspace layout; nothing is tuned apart.  _workspace_bytes / _plan_describe answer
 * what this call gets (0 / an error outside the gate).
 * CONTRACT: as everywhere — no K/V load at or beyond Lk = cache_seqlens[b] + seqlen_knew. */
int vattn_fp8kv_prefill_with_kvcache(const vattn_attn_params* p, const float* k_scale, const float* v_scale, void* stream);
size_t vattn_fp8kv_prefill_workspace_bytes(const vattn_attn_params* p);
int vattn_fp8kv_prefill_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out);

/* LOGIT SOFT-CAPPING (Gemma-2 / Gemma-3: attn_logit_softcapping): scores = softcap * tanh(q.k * softmax_scale / softcap), the `softcap` of the
 * reference's operator (flash_api.cpp:105-113, apply_softcap in flash_fwd_kernel.h:26-30).  Additive: vattn_attn_params and VATTN_KERNELS_ABI
 * are unchanged, the cap travels BESIDE the parameter block as an extra argument of builds of the decode kernels and of the register-staged
 * prefill kernels of their own; every other kernel, entry point and refusal is what it was.
 * ARITHMETIC (one answer for every input, the reference's order of operations): (1) the host forms pre = softmax_scale / softcap by IEEE fp32
 * division; (2) in the kernel t = tanh(s * pre) is taken on the fp32 MFMA accumulator s = q.k BEFORE any mask is applied — a masked score stays
 * -inf (tanh(-inf) = -1 would unmask it); (3) tanh(x) = 1 - 2 / (1 + exp2(2 log2e x)) on the hardware exp2 and reciprocal, evaluated as
 * fma(-2, rcp(1 + exp2(s * k2)), 1) with k2 = pre * 2 log2e formed once per kernel in fp32: branch-free, and +-1 at the limits without a select;
 * (4) the online softmax runs on t with softcap as its scale (sc = softcap * log2e where the plain kernels use softmax_scale * log2e): running
 * max, rescaling, the cross-wave merge and published partials follow from that; (5) softmax_lse is the natural log of sum exp(softcap * t); a
 * row without a visible key gives 0 and LSE +inf, as everywhere.  ERROR: that tanh expression in IEEE fp32 has absolute error 1.9e-7 on
 * [-12, 12]; a capped logit is off by about softcap * 2e-7 — 1e-5 at softcap 50 — and the error GROWS WITH THE CAP: a huge cap is not a way
 * to spell "no cap" (pass 0).  The hardware exp2 / reciprocal are 1-ulp approximations; the single-key
 * probe of tests/test_gpu_census_softcap.py (a row with one visible key has LSE = softcap * tanh(s * pre) and nothing else) measures them: worst
 * |lse - softcap * tanh(x)| / softcap = 2.6e-7 over x in [-40, 40] at softcap 1.5 / 30 / 50 on an MI355X, held to 6e-7 + one fp32 ulp of the LSE.
 * softcap == 0.0f delegates to vattn_flash_attn_with_kvcache(p, stream), unchanged and bit-identical; negative, NaN or infinite softcap is
 * VATTN_K_ERR_INVALID, and so is one so small (a denormal) that pre = softmax_scale / softcap is no finite fp32 number.
 * GATE (softcap > 0): the one-token decode form; the multi-token form (its gate above), causal or not; the prefill form on the register-staged
 * kernels (8 / 4 waves x 32 rows, d 64 / 128, f16 / bf16): causal or not, cache_batch_idx, softmax_lse, KV split, batched chunks (q_start /
 * q_lens) — each WITH OR WITHOUT window_left_plus1 under the window's rules and no-read contract above; k_new / v_new behave as in the plain
 * call for the same block (one decode row inside the attention kernel, otherwise an append launch in front of it).  Refused with
 * VATTN_K_ERR_UNSUPPORTED and a message that names the rule: rotary_cos_sin (rotate first: vattn_rotary_embedding / vattn_cache_flat_rope),
 * split_items, pf_items / pf_num_wg, explicit tiling 7 (prefill64 has no softcap build), d other than 64 / 128, a -DVATTN_LAB build.  There is
 * no tree-masked, fp8 or hybrid entry point with a cap.
 * PLAN: that of vattn_flash_attn_with_kvcache for the same block with its prefill64 branch skipped (the rule of vattn_fp8kv_prefill_*): grids,
 * stream decomposition, record layouts, merge / combine kernels and workspace sizes are the plain call's; partials are fp32 and do not know
 * about the cap.  _workspace_bytes / _plan_describe answer what this call gets (0 / an error outside the gate; softcap == 0: the plain call's). */
int vattn_softcap_attn_with_kvcache(const vattn_attn_params* p, float softcap, void* stream);
size_t vattn_softcap_attn_workspace_bytes(const vattn_attn_params* p, float softcap);
int vattn_softcap_attn_plan_describe(const vattn_attn_params* p, float softcap, vattn_plan_desc* out);

/* Fused prefill || decode for a hybrid batch (replaces the reference's POD-Attention entry point
 * /root/reference/pod_attn/pod_attn/flash_attn_interface.py true_fused_attn_with_kvcache, call site
 * /root/reference/sarathi-lean/sarathi/model_executor/attention/vattention_flashattention_pod_wrapper.py:121-203): ONE launch of
 * persistent workgroups, two per CU, typed prefill / decode by a per-CU arrival counter, fed from two device-side work queues;
 * the decode part's split-KV merge happens in the same launch.  `prefill` is a prefill-form parameter block (seqlen_q > 1 or the
 * batched-chunk form, k_new == NULL: append with vattn_cache_flat first), `decode` a decode-form block (seqlen_q == 1, optional
 * one-row append); both d == 128 and the same dtype; their `workspace` fields are ignored.  `workspace` is
 * vattn_hybrid_workspace_bytes() bytes of device memory that must be ZERO before the first launch; the launch leaves its control
 * words and merge counters zero (they sit in a fixed-size region ahead of the split partials, whatever the batch), so it can be
 * reused by the next launch on the same stream — of any batch size it is large enough for — without a memset.  Results are those of the two
 * stand-alone launches (same device functions). */
size_t vattn_hybrid_workspace_bytes(const vattn_attn_params* prefill, const vattn_attn_params* decode);
int vattn_hybrid_attn(const vattn_attn_params* prefill, const vattn_attn_params* decode, void* workspace, void* stream);

/* cache_flat: k_cache[t*k_cache_stride + i] = key[t*key_stride + i], same for value,
 * t < num_tokens, i < num_heads*head_size (cache_kernels.cu:483-520). */
int vattn_cache_flat(const void* key, const void* value, void* k_cache, void* v_cache,
                     int64_t num_tokens, int32_t num_heads, int32_t head_size,
                     int64_t key_stride, int64_t value_stride, int64_t k_cache_stride, int64_t v_cache_stride,
                     int32_t itemsize, void* stream);

/* cache_flat with the rotary embedding of the KEY rows fused in: k_cache[t] = rope(key[t], position pos0 + t),
 * v_cache[t] = value[t]; one pass over the new K/V instead of the reference's rotary kernel + cache_flat.  2-byte dtypes, NeoX
 * style, rotary_dim == head_size.  dtype = VATTN_DTYPE_*. */
int vattn_cache_flat_rope(const void* key, const void* value, void* k_cache, void* v_cache, int64_t num_tokens,
                          int32_t num_heads, int32_t head_size, int64_t key_stride, int64_t value_stride, int64_t k_cache_stride,
                          int64_t v_cache_stride, int32_t dtype, const void* cos_sin, int64_t cos_sin_row_stride, int64_t pos0,
                          void* stream);

/* The reference's stand-alone rotary kernel (pos_encoding_kernels.cu:39-77, rotary_embedding): in place on query [T, Hq*hs]
 * and key [T, Hkv*hs], positions int64[T].  Provided for the UNFUSED path (what the fused launches are measured against). */
int vattn_rotary_embedding(const int64_t* positions, void* query, void* key, int64_t num_tokens, int32_t num_q_heads,
                           int32_t num_kv_heads, int32_t head_size, int64_t query_stride, int64_t key_stride, int32_t dtype,
                           const void* cos_sin, int64_t cos_sin_row_stride, int32_t rot_dim, int32_t is_neox, void* stream);

/* Device-side self-tests of the hardware layout assumptions (MFMA fragment maps, LDS transpose read, LDS-DMA lane
 * mapping); 0 = all assumptions hold.  detail_out[0..5] are per-assumption failure flags, detail_out[6] reports what
 * an out-of-range LDS-DMA lane does to its LDS bytes (0 zeros, 1 untouched).  Used by tests/test_gpu_hw_and_vmm.py. */
int vattn_selftest_layouts(void* stream, int32_t* detail_out /* int32[8] host buffer */);

/* Times `iters` launches of the kernel family last used by vattn_flash_attn_with_kvcache with HIP
 * events on `stream`; returns average milliseconds per call (negative on error). */
float vattn_time_attn(const vattn_attn_params* p, void* stream, int32_t warmup, int32_t iters);

const char* vattn_kernels_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* VATTN_KERNELS_H_ */
