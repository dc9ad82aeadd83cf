// Prefill form of flash_attn_with_kvcache, second-generation kernel for head dimension 128 (gfx950):
//   * a workgroup is 4 waves = one 256-row query block; every wave owns 64 query rows (two 32-row blocks) and a whole SIMD
//     (one wave per SIMD, 512 registers): each K fragment and each V^T fragment read from LDS feeds TWO MFMAs, halving the
//     LDS fragment traffic per flop of the 8 x 32-row kernel (prefill_kernels.hip);
//   * K / V tiles (64 keys) travel HBM/L2 -> LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`, one 1-KiB piece per wave
//     instruction), no staging registers: the LDS image of a tile is shaped on the GLOBAL side (lane i fetches the 16 bytes that
//     belong at LDS position M0 + 16*i) — K as 16 padded 4-row pieces whose fragment addresses are lane + immediate (product;
//     the first version's row-major image with the chunk index XOR-swizzled by the row is build 3), V as [d/32][key][32 d]
//     sub-tiles for `ds_read_b64_tr_b16`; a K ring of 2 and a V ring of 3 slots (K runs one tile ahead of V), one barrier per
//     tile, counted `vmcnt` (the DMA is issued by inline asm, the compiler's wait-count pass never sees it);
//   * software pipeline inside the wave: phase A  S(t+1) = K(t+1).Q^T  ||  P(t) = exp2(S(t)), row sums;
//                                        phase B  O += V(t)^T.P(t)^T   ||  row max of S(t+1), f16 packing of P(t);
//     so the softmax VALU work of a tile is issued between the MFMAs of its neighbours by the same wave; the scalar bookkeeping of
//     the DMA stream (running descriptors in fixed SGPR quads, slot rotation) and the row-max reduction sit inside MFMA gaps as
//     well — one instruction before a step's first MFMA, two behind its last (round 3);
//   * softmax exactly as the reference states it (softmax.h:69-94): P = exp2(s*scale*log2e - m*scale*log2e) in fp32, one v_fma
//     + one v_exp per score; the running maximum is only moved when a tile's maximum exceeds it by more than 2^kDeferLog2
//     (deferred rescale, cdna guide T13) — O and l are rescaled exactly once in that (rare) branch, the pending S(t+1) is still
//     raw and needs nothing.  [Measured and dropped: pre-scaling Q (rounds q once more: 2.2x the reference-numerics error on
//     short contexts) and carrying -m in the accumulators (64 extra moves per tile) — with one wave per SIMD the kernel is bound
//     by instruction ISSUE (about 8 slots per MFMA), so the instruction count per tile is what matters.]
// Semantics as prefill_kernels.hip: /root/reference/pod_attn/pod_attn/flash_attn_interface.py:1146-1291, mask.h:164-196
// (bottom-right causal), softmax.h:69-157 (fp32 max/sum via exp2, P rounded to the I/O dtype before PV),
// flash_fwd_kernel.h:57-499 (the operator's non-split kernel), :1116-1297 (split combine, here combine_rows_kernel).
// Every K/V access is bounded by a buffer descriptor that ends at the sequence's visible length.
#include "prefill64_common.h"

namespace vattn_k {


// The schedule of the tile step (tile_step in prefill64_common.h; its compile-time constants below): 24 of the tile's 32 exp2 pairs start in phase A, a fragment ring of 4
// (three fragments ahead of their MFMA), the row-max chain in phase-B groups 8-23, the per-tile wait + barrier in front of group 8, one
// LDS-DMA piece in groups 9, 12, ... 30.  Every alternative that was measured — other placements, the XOR-swizzled K image, timing
// ablations, per-group clock stamps, the issue-price list of round 6 — lives in the LAB copy of this kernel, tools/lab/csrc/prefill64_lab.hip
// (built into tools/lab/libvattn_lab.so only).
// Round 6 (profiles/r06_p64_price_list.txt, r06_p64_issue_ablation_pmc.txt): the step is bound by what ONE wave can issue to the vector
// ALU — a VALU instruction beside the MFMAs costs 7.3 cycles (v_exp 10.7, packed-f32 43), a scalar instruction, an s_nop or an
// s_waitcnt that does not wait 0.3, and the matrix pipe idles a third of the time.  Hence: (1) nothing per-lane that a scalar
// register can carry stays in the VALU (the scale of the exp2 argument; the distance of an LDS-DMA piece from piece 0 travels in the
// load's scalar offset instead of a v_mad per piece); (2) the first V^T fragments of phase B are read during the LAST groups of phase A
// (the first P.V MFMA used to wait a whole LDS round trip with the matrix pipe idle); (3) the row-max chain starts from its first link.
// What is left per tile is the algorithm's own 64 v_fma + 64 v_exp + 64 v_add + 32 v_cvt_pk + 32 v_max3 and ~20 others against 64 MFMAs.
// WIN: causal sliding window (p.window_left_plus1 = left + 1 > 0, is_causal set, no work list; include/vattn_kernels.h) — a build of its own, the
// window-less kernel is untouched and tile_step is shared as it is.  Query row i sees keys [i + off - left, i + off].  The workgroup's key walk
// starts at the 64-key tile that holds the first key its FIRST row sees (no-read contract, T = 64: tiles below it are never fetched) and ends
// where it ends without a window; key-range shares divide that walk.  The few tiles at the front that lie left of, or straddle, the left limit of
// some row of a wave are masked where the causal diagonal is (needs_mask / mask_tile, wave-uniform).  A row whose first visible key lies in a
// LATER tile than the walk's first has seen only -inf so far and holds a zero reference: it takes its first visible tile's maximum as its
// running maximum (nothing is accumulated yet, so nothing is rescaled) — without that, scores far below zero would underflow against the zero reference.
// The kernel's text lives in prefill64_kernel.inc and is compiled twice: prefill64_kernel<T> (no window) and prefill64w_kernel<T> (WIN).
#define P64_KERNEL_NAME prefill64_kernel
#define P64_WIN false
#include "prefill64_kernel.inc"
#undef P64_KERNEL_NAME
#undef P64_WIN
#define P64_KERNEL_NAME prefill64w_kernel
#define P64_WIN true
#include "prefill64_kernel.inc"
#undef P64_KERNEL_NAME
#undef P64_WIN

// host side: grid as prefill_kernels.hip's 1-D / 3-D orders (prefill_grid) with 256-row query blocks
constexpr int kSmem64 = 36864 + 3 * PfSmem<128>::kTileBytes;      // K ring (2 x 17 408, rounded up) + V ring
template <typename T, bool WIN> static void launch64_t(const vattn_attn_params* p, hipStream_t st, int nsplit) {
    const int nqb = (p->seqlen_q + 255) / 256;
    int order;
    dim3 grid = prefill_grid(p, nqb, p->pf_items ? 1 : nsplit, &order);
    if (p->pf_items) grid = dim3((unsigned)p->num_pf_items);      // one workgroup per listed piece
    constexpr auto kern = WIN ? prefill64w_kernel<T> : prefill64_kernel<T>;
    static const bool once = [] {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem64 + 16);
        return true;
    }();
    (void)once;
    hipLaunchKernelGGL(kern, grid, dim3(256), kSmem64 + 16, st, *p, order, nqb, nsplit);
}

// ONE build per dtype, and one more for blocks that carry a sliding window (validate() keeps those off the work list); key-range shares are
// merged by combine_rows_kernel / combine_blocks_kernel in a second launch (prefill_kernels.hip).
void launch_prefill64(const vattn_attn_params* p, hipStream_t st, int nsplit) {
    const bool win = p->window_left_plus1 > 0 && !p->pf_items, bf = p->dtype == VATTN_DTYPE_BF16;
    (bf ? (win ? launch64_t<__bf16, true> : launch64_t<__bf16, false>) : (win ? launch64_t<_Float16, true> : launch64_t<_Float16, false>))(p, st, nsplit);
}

}  // namespace vattn_k
