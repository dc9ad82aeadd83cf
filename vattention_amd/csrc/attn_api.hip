// C ABI of the gfx950 attention kernels over virtually-contiguous KV tensors (include/vattn_kernels.h).
//   prefill_kernels.hip : seqlen_q > 1   (chunked causal prefill, KV split, batched variable-length chunks)
//   decode_kernels.hip  : seqlen_q == 1  (split-KV decode with in-kernel append, combine), and the multi-token form: 2..8 query rows
//                         per entry as (token, head) columns of the same kernels (multitoken_form, attn_common.h)
//   cache_kernels.hip   : cache_flat / append
// Semantics follow the operator the reference calls (flash_attn_with_kvcache):
//   /root/reference/pod_attn/pod_attn/flash_attn_interface.py:1146-1291, flash_api.cpp:1291-1578,
//   mask.h:164-196 (bottom-right causal), softmax.h:69-157 (fp32 max/sum, exp2, P rounded to the
//   I/O dtype before PV), flash_fwd_kernel.h:1116-1297 (split combine).
// Every K/V access is predicated on the sequence's visible length: rows at or beyond it may sit
// on unmapped virtual pages (SURVEY §7 "never touch unmapped VA").
#include <map>
#include <mutex>
#include <utility>
#include "attn_common.h"

namespace vattn_k {

// ============================================================================================
// hardware-layout self test
// ============================================================================================

// Checks, against plain integer arithmetic, the three layout facts the kernels rely on:
//  [0] 32x32x16 C/D map: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
//  [1] 16x16x32 C/D map: col = lane&15, row = 4*(lane>>4) + r
//  [2] ds_read_b64_tr_b16: lane i of a 16-lane group receives element (i&3) of the 8-byte chunks
//      addressed by lanes 4*j + (i>>2), j = 0..3, of the same group
//  [3] A/B operands: lane (x = lane&31, g = lane>>5) contributes row/col x with k-slots (g, 0..7) (32x32x16)
//  [4] same for 16x16x32 with g = lane>>4
//  [5] LDS-DMA (`buffer_load_dwordx4 ... lds`, prefill64_kernels.hip): lane i's 16 bytes land at LDS address M0 + 16*i, whatever
//      global offset the lane fetched from (the K-tile swizzle is applied on the global side)
//  [6] (informational, not a failure) what a lane beyond the descriptor's bound does to its 16 LDS bytes:
//      0 = writes zeros, 1 = leaves them untouched, 2 = something else
__global__ void selftest_kernel(int* res, const unsigned* gsrc) {
    __shared__ __attribute__((aligned(16))) short lds[64 * 4];
    const int lane = threadIdx.x;
    // [0],[3]: A = one-hot rows, B = one-hot cols with distinct values -> C[m][n] = sum_k A[m][k]B[k][n]
    {
        // A[m][slot] = (m + 1) if slot == (m & 15) else 0 ; B[slot][n] = (n + 1) * 64 + ... keep small ints
        f16x8 a, bq;
        const int x = lane & 31, g = lane >> 5;
        for (int j = 0; j < 8; j++) {
            const int slot = 8 * g + j;                 // logical k index shared by A and B
            a[j] = (_Float16)((slot == (x & 15)) ? (float)(x + 1) : 0.f);      // A[m=x][k]
            bq[j] = (_Float16)((slot == 3) ? 0.f : 0.f);
        }
        // B[k][n=x] = 1 for every k -> C[m][n] = sum_k A[m][k] = m + 1 for every n
        for (int j = 0; j < 8; j++) bq[j] = (_Float16)1.f;
        f32x16 c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq, c, 0, 0, 0);
        int bad = 0;
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * g;
            if (c[r] != (float)(row + 1)) bad = 1;
        }
        // columns: A[m][k] = 1 for all, B[k][n] = (n+1) if k-slot == (n & 15) -> C[m][n] = n + 1
        for (int j = 0; j < 8; j++) {
            a[j] = (_Float16)1.f;
            bq[j] = (_Float16)(((8 * g + j) == (x & 15)) ? (float)(x + 1) : 0.f);
        }
        f32x16 c2 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        c2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq, c2, 0, 0, 0);
        int bad3 = 0;
        for (int r = 0; r < 16; r++)
            if (c2[r] != (float)(x + 1)) bad3 = 1;
        if (bad) atomicOr(&res[0], 1);
        if (bad3) atomicOr(&res[3], 1);
    }
    {
        f16x8 a, bq;
        const int x = lane & 15, g = lane >> 4;
        for (int j = 0; j < 8; j++) {
            a[j] = (_Float16)(((8 * g + j) == x) ? (float)(x + 1) : 0.f);
            bq[j] = (_Float16)1.f;
        }
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bq, c, 0, 0, 0);
        int bad = 0;
        for (int r = 0; r < 4; r++)
            if (c[r] != (float)(4 * g + r + 1)) bad = 1;
        for (int j = 0; j < 8; j++) {
            a[j] = (_Float16)1.f;
            bq[j] = (_Float16)(((8 * g + j) == x) ? (float)(x + 1) : 0.f);
        }
        f32x4 c2 = {0.f, 0.f, 0.f, 0.f};
        c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bq, c2, 0, 0, 0);
        int bad4 = 0;
        for (int r = 0; r < 4; r++)
            if (c2[r] != (float)(x + 1)) bad4 = 1;
        if (bad) atomicOr(&res[1], 1);
        if (bad4) atomicOr(&res[4], 1);
    }
    {
        // each lane owns the 8-byte chunk at lds[lane*4 .. lane*4+3]; value encodes (lane, element)
        for (int e = 0; e < 4; e++) lds[lane * 4 + e] = (short)(lane * 4 + e);
        __syncthreads();
        const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, &lds[lane * 4]));
        const int grp = lane >> 4, i = lane & 15;
        int bad = 0;
        for (int j = 0; j < 4; j++) {
            const int src_lane = grp * 16 + 4 * j + (i >> 2);
            if (t[j] != (short)(src_lane * 4 + (i & 3))) bad = 1;
        }
        if (bad) atomicOr(&res[2], 1);
    }
    {
        __shared__ __attribute__((aligned(16))) unsigned dst[2 * 256];      // two 1-KiB pieces
        for (int e = 0; e < 8; e++) dst[lane * 8 + e] = 0xABABABABu;
        __syncthreads();
        // gsrc[w] = w for 512 dwords (2 KiB).  piece 0: lane i fetches 16-byte chunk (i ^ 5); piece 1: descriptor bounded at 512
        // bytes, lane i fetches chunk i (lanes >= 32 are out of range)
        const unsigned long long a = (unsigned long long)gsrc;
        u32x4 r0, r1;
        r0[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
        r0[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) & 0xffffu;
        r0[2] = 2048u;
        r0[3] = 0x00020000u;
        r1 = r0;
        r1[2] = 512u;
        const unsigned l0 = (unsigned)(size_t)LDS_PTR(unsigned, dst), l1 = l0 + 1024u;
        const unsigned v0 = (unsigned)((lane ^ 5) * 16), v1 = (unsigned)(lane * 16);
        asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %1, 0 offen lds" : : "s"(l0), "s"(r0), "v"(v0) : "memory", "m0");
        asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %1, 0 offen lds" : : "s"(l1), "s"(r1), "v"(v1) : "memory", "m0");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int bad = 0;
        for (int e = 0; e < 4; e++)
            if (dst[lane * 4 + e] != (unsigned)((lane ^ 5) * 4 + e)) bad = 1;
        if (lane < 32)
            for (int e = 0; e < 4; e++)
                if (dst[256 + lane * 4 + e] != (unsigned)(lane * 4 + e)) bad = 1;
        if (bad) atomicOr(&res[5], 1);
        if (lane >= 32) {
            int code = 0;
            for (int e = 0; e < 4; e++) {
                const unsigned x = dst[256 + lane * 4 + e];
                if (x == 0xABABABABu) code |= 1;
                else if (x != 0u) code |= 2;
            }
            if (code) atomicOr(&res[6], code);
        }
    }
}

// [7] (informational) LDS-DMA into an LDS address beyond 64 KiB (the destination base travels in M0): 1 KiB is sent to byte offset
// 72 KiB of a 96-KiB dynamic allocation; reports 1 + the KiB offset the data is found at (73 = where it was sent), 0 = nowhere
__global__ void selftest_dma_high_kernel(int* res, const unsigned* gsrc) {
    extern __shared__ __attribute__((aligned(16))) unsigned big[];
    const int lane = threadIdx.x;
    for (int i = lane; i < (96 << 10) / 4; i += 64) big[i] = 0xCDCDCDCDu;
    __syncthreads();
    const unsigned long long a = (unsigned long long)gsrc;
    u32x4 r0;
    r0[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
    r0[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) & 0xffffu;
    r0[2] = 2048u;
    r0[3] = 0x00020000u;
    const unsigned l0 = (unsigned)(size_t)LDS_PTR(unsigned, big) + (72u << 10);
    const unsigned v0 = (unsigned)(lane * 16);
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %1, 0 offen lds" : : "s"(l0), "s"(r0), "v"(v0) : "memory", "m0");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (lane == 0) {
        int found = 0;
        for (int kib = 0; kib < 96; kib++) {
            bool ok = true;
            for (int w = 0; w < 256 && ok; w++) ok = big[kib * 256 + w] == (unsigned)w;
            if (ok) { found = kib + 1; break; }
        }
        res[7] = found;
    }
}

// Counters of the single-launch merges (split-KV decode, KV-split prefill) for launches on stream `st`: created (and zeroed, stream-ordered) on first use, never while
// the stream is being captured into a graph (then the caller takes the two-launch form; a warm-up call before capture creates it).
int* merge_counters(hipStream_t st, size_t n_ints) {
    if (!kLab) return nullptr;        // the in-launch merges of the stand-alone launches are measurement scaffolding (measured slower)
    struct Buf { int* p; size_t n; };
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, Buf> bufs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> l(mu);
    Buf& b = bufs[std::make_pair(dev, st)];
    if (b.p && b.n >= n_ints) return b.p;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    const size_t n = n_ints < 16384 ? 16384 : n_ints;
    int* np = nullptr;
    if (hipMalloc((void**)&np, n * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipMemsetAsync(np, 0, n * sizeof(int), st) != hipSuccess) { (void)hipFree(np); return nullptr; }
    // an older, smaller buffer may still be in use by launches queued on the stream: it is leaked on purpose (a few KiB, at most
    // once per growth step)
    b.p = np;
    b.n = n;
    return np;
}


// Counters of the DRAWN queues of the persistent prefill launch (csrc/prefill64p_kernels.hip): 8 ints per (device, stream), zeroed by the
// caller in front of every drawn launch (launch_prefill_t; the last draw of a queue also resets its counter).  Created on first use; never
// while the stream is being captured into a graph (NULL then: the caller launches one workgroup per piece; a warm-up call before capture
// creates them).
int* queue_counters(hipStream_t st) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, int*> bufs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> l(mu);
    auto it = bufs.find(std::make_pair(dev, st));
    if (it != bufs.end()) return it->second;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    int* np = nullptr;
    if (hipMalloc((void**)&np, 16 * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipMemsetAsync(np, 0, 16 * sizeof(int), st) != hipSuccess) { (void)hipFree(np); return nullptr; }
    bufs[std::make_pair(dev, st)] = np;
    return np;
}

thread_local std::string g_err;
int fail(int code, const char* msg) {
    g_err = msg;
    return code;
}

// The post-launch check of every launch sequence (decode_kernels.hip, prefill_kernels.hip).
int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VATTN_K_OK : fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
}

// the caller's header and ours describe the same block (include/vattn_kernels.h)
bool abi_ok(const vattn_attn_params* p) { return p && p->struct_size == (uint32_t)sizeof(vattn_attn_params) && p->abi_version == VATTN_KERNELS_ABI; }

// The row-stride ceiling of the caches (include/vattn_kernels.h, "ROW-STRIDE CEILING"): inside one key tile the kernels keep 32-bit byte offsets
// against a per-tile 64-bit base — row x stride per lane, 16 x stride and 64 x stride steps, rows x stride as the descriptor's num_records —
// and prefill64p forms its piece offsets with a 24-bit multiply of the row's byte stride (prefill64_common.h, piece_off).  kv_bytes: bytes per
// cache element (2; an fp8 cache: 1).  A stride of 0 (one row broadcast) stays legal.
static const char* kRowStride = "row-stride ceiling: k_row_stride / v_row_stride must be >= 0 and at most 2^24 - 16 BYTES (the kernels keep 32-bit byte "
                                "offsets inside a key tile; prefill64 multiplies the row's byte stride in 24 bits)";
static bool row_strides_ok(const vattn_attn_params* p, int kv_bytes) {
    const int64_t lim = VATTN_MAX_KV_ROW_STRIDE_BYTES / kv_bytes;
    return p->k_row_stride >= 0 && p->k_row_stride <= lim && p->v_row_stride >= 0 && p->v_row_stride <= lim;
}

int validate(const vattn_attn_params* p, int kv_bytes = 2) {
    if (!p) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library (zero the block, then set both from include/vattn_kernels.h)");
    if (!p->q || !p->out || !p->k_cache || !p->v_cache) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    if (p->dtype != VATTN_DTYPE_F16 && p->dtype != VATTN_DTYPE_BF16)
        return fail(VATTN_K_ERR_UNSUPPORTED, "FlashAttention only support fp16 and bf16 data type");      // flash_api.cpp:1325-1326
    // d = 256 instantiates but spills (O^T alone is 128 accumulator registers per wave): not shipped until it has its own tiling
    if (p->d != 64 && p->d != 128) return fail(VATTN_K_ERR_UNSUPPORTED, "this build supports head dimensions 64 and 128");
    if (p->b <= 0) return fail(VATTN_K_ERR_INVALID, "batch size must be postive");                       // flash_api.cpp:1353
    if (p->h_k <= 0 || p->h % p->h_k != 0)
        return fail(VATTN_K_ERR_INVALID, "Number of heads in key/value must divide number of heads in query");   // :1355
    if ((p->k_new == nullptr) != (p->v_new == nullptr))
        return fail(VATTN_K_ERR_INVALID, "If key is supplied, value must also be passed in");            // :1452
    if (p->k_new && !p->cache_seqlens)
        return fail(VATTN_K_ERR_INVALID, "If key is supplied, seqlens_k must also be passed in");        // :1453
    if (p->seqlen_q <= 0 || p->seqlen_k < 0) return fail(VATTN_K_ERR_INVALID, "bad sequence lengths");
    if ((p->q_start == nullptr) != (p->q_lens == nullptr)) return fail(VATTN_K_ERR_INVALID, "q_start and q_lens must be given together");
    if (p->q_lens && p->seqlen_q == 1) return fail(VATTN_K_ERR_UNSUPPORTED, "batched chunks need max(q_lens) > 1 (the decode form is already batched)");
    if (p->q_lens && p->k_new) return fail(VATTN_K_ERR_UNSUPPORTED, "batched chunks: append the new keys/values with cache_flat first");
    // 16-byte vector access requirements
    const int64_t strides[] = {p->q_batch_stride, p->q_row_stride, p->q_head_stride, p->k_batch_stride, p->k_row_stride,
                               p->k_head_stride, p->v_batch_stride, p->v_row_stride, p->v_head_stride};
    for (int64_t s : strides)
        if (s % 8 != 0) return fail(VATTN_K_ERR_UNSUPPORTED, "strides must be multiples of 8 elements (16-byte vector access)");
    if (!row_strides_ok(p, kv_bytes)) return fail(VATTN_K_ERR_UNSUPPORTED, kRowStride);
    if (((uintptr_t)p->q | (uintptr_t)p->k_cache | (uintptr_t)p->v_cache | (uintptr_t)p->out) & 15)
        return fail(VATTN_K_ERR_UNSUPPORTED, "tensor base pointers must be 16-byte aligned");
    if (p->rotary_cos_sin) {
        if (p->rotary_dim != p->d) return fail(VATTN_K_ERR_UNSUPPORTED, "fused rotary embedding needs rotary_dim == head dimension");
        if ((p->rotary_row_stride & 7) || ((uintptr_t)p->rotary_cos_sin & 15))
            return fail(VATTN_K_ERR_UNSUPPORTED, "rotary cos/sin rows must be 16-byte aligned");
    }
    if (p->o_row_stride % 4 != 0 || p->o_head_stride % 4 != 0 || p->o_batch_stride % 4 != 0)
        return fail(VATTN_K_ERR_UNSUPPORTED, "output strides must be multiples of 4 elements");
    if (p->pf_items && (p->seqlen_q == 1 || p->d != 128)) return fail(VATTN_K_ERR_INVALID, "pf_items (prefill work list) applies to the prefill form with head dimension 128");
    if (p->pf_num_wg < 0 || (p->pf_wg_first && !p->pf_num_wg) || (p->pf_num_wg && (!p->pf_items || p->pf_num_wg > p->num_pf_items)))
        return fail(VATTN_K_ERR_INVALID, "pf_num_wg (persistent work list) needs pf_items and at most one workgroup per piece; pf_wg_first needs pf_num_wg");
    if (p->split_items && p->seqlen_q != 1) return fail(VATTN_K_ERR_INVALID, "split_items (length-balanced plan) applies to the decode form only");
    // sliding window (include/vattn_kernels.h): causal, left-sided; its key walks are short and equal, so the host plans are refused with it
    if (p->window_left_plus1 < 0 || p->window_reserved != 0) return fail(VATTN_K_ERR_INVALID, "window_left_plus1 must be left + 1 >= 0 (0: no window) and window_reserved 0");
    if (p->window_left_plus1 > 0) {
        if (kLab) return fail(VATTN_K_ERR_UNSUPPORTED, "the measurement build has no sliding-window kernels (use libvattn_amd.so)");
        if (p->seqlen_q > 1 && !p->is_causal)
            return fail(VATTN_K_ERR_UNSUPPORTED, "a sliding window needs is_causal when seqlen_q > 1 (supported: causal windows, (left >= 0, right = 0))");
        if (p->split_items || p->pf_items)
            return fail(VATTN_K_ERR_INVALID, "a sliding window cannot be combined with split_items / pf_items (the planners return 0 for it: take the default launch)");
    }
    if (!kLab) {
        const int til = (p->variant >> 1) & 7;
        if ((p->variant & ~kProductVariantMask) || !(til == 0 || til == 1 || til == 4 || til == 7))
            return fail(VATTN_K_ERR_INVALID, "variant selects a measurement build that this library does not contain (tools/lab/libvattn_lab.so, -DVATTN_LAB)");
    }
    return VATTN_K_OK;
}

// the prefill planners' answer for a block that carries a sliding window: no list, the default launch (key walks bounded by left + 256 rows)
static int32_t window_plan_none(int32_t* counts_out, int n) {
    for (int i = 0; counts_out && i < n; i++) counts_out[i] = 0;
    return 0;
}

// Why a block is outside the gate of the tree-masked form — multitoken_form (attn_common.h) rule by rule — or NULL when it passes
static const char* tree_gate_reason(const vattn_attn_params* p) {
    if (kLab) return "the measurement build has no tree-masked kernels (use libvattn_amd.so)";
    if (p->seqlen_q < 2 || p->seqlen_q > 8) return "a tree mask needs 2 <= seqlen_q <= 8 (one mask word of 8 bits per query token)";
    if (p->h_k <= 0 || p->h < p->h_k || (long)p->seqlen_q * (p->h / p->h_k) > 64) return "a tree mask needs seqlen_q * (h / h_k) <= 64 (token, head) columns per kv head";
    if (p->q_lens || p->pf_items || p->split_items) return "a tree mask cannot be combined with q_lens / pf_items / split_items";
    if (p->rotary_cos_sin) return "a tree mask cannot be combined with fused rotary embedding (rotary_cos_sin): rotate q and k first";
    if ((p->variant >> 1) & 7) return "a tree mask needs the default tiling (variant bits 1-3 zero)";
    if (p->num_splits > 0) return "a tree mask needs num_splits <= 0";
    return multitoken_form(p) ? nullptr : "the block does not take the multi-token form";
}
static const char* kTreeWindow = "a tree mask cannot be combined with a sliding window (window_left_plus1 > 0): a node's position is its depth, not its index";


// Why a block is outside the gate of the call over an fp8 (e4m3) cache (include/vattn_kernels.h) — rule by rule — or NULL when it passes
static const char* fp8kv_gate_reason(const vattn_attn_params* p) {
    if (kLab) return "the measurement build has no fp8 KV cache kernels (use libvattn_amd.so)";
    if (p->window_left_plus1 > 0) return "an fp8 KV cache cannot be combined with a sliding window (window_left_plus1 > 0)";
    if (p->rotary_cos_sin) return "an fp8 KV cache cannot be combined with fused rotary embedding (rotary_cos_sin): rotate q and k first";
    if (p->split_items) return "an fp8 KV cache cannot be combined with split_items (host item plan)";
    if (p->q_lens || p->pf_items) return "an fp8 KV cache cannot be combined with q_lens / pf_items (batched chunks, prefill work lists)";
    if (!decode_form(p)) return "an fp8 KV cache is read by the decode kernels only: seqlen_q == 1 or the multi-token form, not the prefill form";
    return nullptr;
}

// ... of the tree-masked call over an fp8 cache (vattn_fp8kv_tree_attn_with_kvcache): the multi-token form's gate, rule by rule as the 2-byte tree
// call names it, then whatever the fp8 decode gate refuses (the window is refused before either, as an INVALID argument: kTreeWindow)
static const char* fp8kv_tree_gate_reason(const vattn_attn_params* p) {
    if (const char* why = tree_gate_reason(p)) return why;
    return fp8kv_gate_reason(p);
}

// ... and of the PREFILL form over an fp8 cache (vattn_fp8kv_prefill_with_kvcache): every block that decode_form() rejects, on the register-staged
// prefill kernels (prefill_body.h, FP8) under the default launch — no window, rotation, host plan or prefill64 there
static const char* fp8kv_prefill_gate_reason(const vattn_attn_params* p) {
    if (kLab) return "the measurement build has no fp8 KV cache kernels (use libvattn_amd.so)";
    if (p->window_left_plus1 > 0) return "an fp8 KV cache cannot be combined with a sliding window (window_left_plus1 > 0)";
    if (p->rotary_cos_sin) return "an fp8 KV cache cannot be combined with fused rotary embedding (rotary_cos_sin): rotate q and k first";
    if (p->split_items) return "an fp8 KV cache cannot be combined with split_items (host item plan)";
    if (p->pf_items || p->pf_num_wg) return "fp8 prefill cannot be combined with pf_items / pf_num_wg (prefill work lists run on prefill64, which has no fp8 build)";
    if (((p->variant >> 1) & 7) == 7) return "fp8 prefill: explicit tiling 7 is refused — prefill64 has no fp8 build (its tiles move by LDS-DMA and cannot be widened in flight)";
    if (p->d != 64 && p->d != 128) return "fp8 prefill supports head dimensions 64 and 128";
    if (decode_form(p)) return "fp8 prefill: this block takes the decode form (seqlen_q == 1 or the multi-token form) — call vattn_fp8kv_attn_with_kvcache";
    return nullptr;
}

// Why a block is outside the gate of the soft-capped call (vattn_softcap_attn_with_kvcache, include/vattn_kernels.h) — rule by rule — or NULL when it
// passes: every form the plain call takes, window or not, minus what has no softcap build
static const char* softcap_gate_reason(const vattn_attn_params* p) {
    if (kLab) return "the measurement build has no softcap kernels (use libvattn_amd.so)";
    if (p->rotary_cos_sin) return "softcap cannot be combined with fused rotary embedding (rotary_cos_sin): rotate q and k first (vattn_rotary_embedding / vattn_cache_flat_rope)";
    if (p->split_items) return "softcap cannot be combined with split_items (host item plan)";
    if (p->pf_items || p->pf_num_wg) return "softcap cannot be combined with pf_items / pf_num_wg (prefill work lists run on prefill64, which has no softcap build)";
    if (((p->variant >> 1) & 7) == 7) return "softcap: explicit tiling 7 is refused — prefill64 has no softcap build (its tile step is scheduled around the uncapped softmax)";
    if (p->d != 64 && p->d != 128) return "softcap supports head dimensions 64 and 128";
    return nullptr;
}
// softcap is a finite number > 0 (0 delegates before this is asked) ...
static bool softcap_ok(float softcap) { return softcap > 0.f && softcap <= 3.402823466e+38f; }
static const char* kSoftcapValue = "softcap must be finite and >= 0 (0: no cap)";
// ... and large enough for pre = softmax_scale / softcap, which the kernels multiply every score by, to be a finite fp32 number (a denormal cap)
static bool softcap_pre_ok(const vattn_attn_params* p, float softcap) { return fabsf(p->softmax_scale / softcap) <= 3.402823466e+38f; }
static const char* kSoftcapPre = "softcap is too small: softmax_scale / softcap overflows fp32";

// The argument rules both calls over an fp8 cache add to validate(): the scales, whole 16-byte chunks of BYTES in the caches, aligned new rows
static int fp8kv_check_args(const vattn_attn_params* p, const float* k_scale, const float* v_scale) {
    if (!k_scale || !v_scale) return fail(VATTN_K_ERR_INVALID, "an fp8 KV cache needs k_scale and v_scale (device float32[h_k])");
    const int64_t strides[] = {p->k_batch_stride, p->k_row_stride, p->k_head_stride, p->v_batch_stride, p->v_row_stride, p->v_head_stride};
    for (int64_t s : strides)
        if (s % 16 != 0) return fail(VATTN_K_ERR_UNSUPPORTED, "fp8 cache strides must be multiples of 16 elements (16-byte vector access)");
    if (p->k_new && (((p->knew_batch_stride | p->knew_row_stride | p->knew_head_stride | p->vnew_batch_stride | p->vnew_row_stride | p->vnew_head_stride) & 7) ||
                     ((((uintptr_t)p->k_new) | ((uintptr_t)p->v_new)) & 15)))
        return fail(VATTN_K_ERR_UNSUPPORTED, "k_new / v_new must be 16-byte aligned (strides of 8 elements)");
    if (p->k_new && p->seqlen_knew > 0 && !p->cache_seqlens) return fail(VATTN_K_ERR_INVALID, "If key is supplied, seqlens_k must also be passed in");
    return VATTN_K_OK;
}

}  // namespace vattn_k

using namespace vattn_k;

extern "C" {

const char* vattn_kernels_last_error(void) { return g_err.c_str(); }

// the plain call's workspace need / plan of a block whose row strides the caller has checked for ITS cache element size (row_strides_ok)
static size_t plain_workspace_bytes(const vattn_attn_params* p) {
    if (!abi_ok(p)) return 0;
    if (!p || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || p->seqlen_q <= 0) return 0;
    return decode_form(p) ? decode_workspace_bytes(p) : prefill_workspace_bytes(p);
}
static int plain_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out) {
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library");
    if (!p || !out || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || p->seqlen_q <= 0 || (p->d != 64 && p->d != 128)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_plan_describe: bad shape");
    memset(out, 0, sizeof *out);
    if (decode_form(p)) decode_describe(p, out);
    else prefill_describe(p, out);
    out->workspace_bytes = (int64_t)plain_workspace_bytes(p);
    return VATTN_K_OK;
}

size_t vattn_attn_workspace_bytes(const vattn_attn_params* p) {
    if (!abi_ok(p) || !row_strides_ok(p, 2)) return 0;
    return plain_workspace_bytes(p);
}

int vattn_flash_attn_with_kvcache(const vattn_attn_params* p, void* stream) {
    int rc = validate(p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->k_new && p->seqlen_knew > 0 && !p->cache_seqlens) return fail(VATTN_K_ERR_INVALID, "If key is supplied, seqlens_k must also be passed in");
    return decode_form(p) ? launch_decode_form(p, st) : launch_prefill_form(p, st);
}

int vattn_tree_attn_with_kvcache(const vattn_attn_params* p, const uint32_t* tree_mask, void* stream) {
    if (!tree_mask) return vattn_flash_attn_with_kvcache(p, stream);
    if (!abi_ok(p)) return validate(p);
    if (p->window_left_plus1 > 0) return fail(VATTN_K_ERR_INVALID, kTreeWindow);      // (before validate: is_causal is ignored in this form)
    int rc = validate(p);
    if (rc) return rc;
    if (const char* why = tree_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);
    if (p->k_new && p->seqlen_knew > 0 && !p->cache_seqlens) return fail(VATTN_K_ERR_INVALID, "If key is supplied, seqlens_k must also be passed in");
#ifndef VATTN_LAB
    return launch_tree_form(p, tree_mask, (hipStream_t)stream);
#else
    return VATTN_K_ERR_UNSUPPORTED;
#endif
}

// The tree-masked call runs the multi-token launch of the same block on other builds of the same kernels: same planners, same answers.
size_t vattn_tree_attn_workspace_bytes(const vattn_attn_params* p) {
    if (!abi_ok(p) || p->window_left_plus1 > 0 || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || tree_gate_reason(p)) return 0;
    return vattn_attn_workspace_bytes(p);      // (checks the row strides)
}

int vattn_tree_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out) {
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library");
    if (p->window_left_plus1 > 0) return fail(VATTN_K_ERR_INVALID, kTreeWindow);
    if (const char* why = tree_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);
    return vattn_attn_plan_describe(p, out);      // (checks the row strides)
}

int vattn_fp8kv_attn_with_kvcache(const vattn_attn_params* p, const float* k_scale, const float* v_scale, void* stream) {
    if (!abi_ok(p)) return validate(p);
    if (const char* why = fp8kv_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);      // (before validate: the refusal names the fp8 rule)
    int rc = validate(p, 1);      // (fp8: strides in bytes)
    if (rc) return rc;
    if ((rc = fp8kv_check_args(p, k_scale, v_scale))) return rc;
#ifndef VATTN_LAB
    return launch_fp8kv_form(p, k_scale, v_scale, (hipStream_t)stream);
#else
    return VATTN_K_ERR_UNSUPPORTED;
#endif
}

// The call over an fp8 cache runs the launch of the same block on other builds of the same kernels: same planners, same answers.
size_t vattn_fp8kv_attn_workspace_bytes(const vattn_attn_params* p) {
    if (!abi_ok(p) || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || fp8kv_gate_reason(p) || !row_strides_ok(p, 1)) return 0;
    return plain_workspace_bytes(p);
}

int vattn_fp8kv_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out) {
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library");
    if (const char* why = fp8kv_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);
    if (!row_strides_ok(p, 1)) return fail(VATTN_K_ERR_UNSUPPORTED, kRowStride);
    return plain_plan_describe(p, out);
}

int vattn_fp8kv_tree_attn_with_kvcache(const vattn_attn_params* p, const uint32_t* tree_mask, const float* k_scale, const float* v_scale, void* stream) {
    if (!tree_mask) return vattn_fp8kv_attn_with_kvcache(p, k_scale, v_scale, stream);
    if (!abi_ok(p)) return validate(p);
    if (p->window_left_plus1 > 0) return fail(VATTN_K_ERR_INVALID, kTreeWindow);      // (as in the 2-byte tree call; before the gates: the fp8 gate would call it unsupported)
    if (const char* why = fp8kv_tree_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);      // (before validate: the refusal names the rule)
    int rc = validate(p, 1);      // (fp8: strides in bytes)
    if (rc) return rc;
    if ((rc = fp8kv_check_args(p, k_scale, v_scale))) return rc;
#ifndef VATTN_LAB
    return launch_fp8kv_tree_form(p, tree_mask, k_scale, v_scale, (hipStream_t)stream);
#else
    return VATTN_K_ERR_UNSUPPORTED;
#endif
}

// The tree-masked call over an fp8 cache runs the multi-token launch of the same block on other builds of the same kernels: what
// vattn_tree_attn_workspace_bytes / _plan_describe answer.
size_t vattn_fp8kv_tree_attn_workspace_bytes(const vattn_attn_params* p) {
    if (!abi_ok(p) || p->window_left_plus1 > 0 || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || fp8kv_tree_gate_reason(p) || !row_strides_ok(p, 1)) return 0;
    return plain_workspace_bytes(p);
}

int vattn_fp8kv_tree_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out) {
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library");
    if (p->window_left_plus1 > 0) return fail(VATTN_K_ERR_INVALID, kTreeWindow);
    if (const char* why = fp8kv_tree_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);
    if (!row_strides_ok(p, 1)) return fail(VATTN_K_ERR_UNSUPPORTED, kRowStride);
    return plain_plan_describe(p, out);
}

int vattn_fp8kv_prefill_with_kvcache(const vattn_attn_params* p, const float* k_scale, const float* v_scale, void* stream) {
    if (!abi_ok(p)) return validate(p);
    if (const char* why = fp8kv_prefill_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);      // (before validate: the refusal names the fp8 rule)
    int rc = validate(p, 1);      // (fp8: strides in bytes)
    if (rc) return rc;
    if ((rc = fp8kv_check_args(p, k_scale, v_scale))) return rc;
#ifndef VATTN_LAB
    return launch_fp8kv_prefill_form(p, k_scale, v_scale, (hipStream_t)stream);
#else
    return VATTN_K_ERR_UNSUPPORTED;
#endif
}

// The prefill call over an fp8 cache takes the 2-byte call's plan without its prefill64 branch (prefill_kernels.hip, plan_prefill): tiling 1 or 4
size_t vattn_fp8kv_prefill_workspace_bytes(const vattn_attn_params* p) {
    if (!abi_ok(p) || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || p->seqlen_q <= 0 || fp8kv_prefill_gate_reason(p) || !row_strides_ok(p, 1)) return 0;
#ifndef VATTN_LAB
    return fp8kv_prefill_workspace_bytes(p);
#else
    return 0;
#endif
}

int vattn_fp8kv_prefill_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out) {
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library");
    if (const char* why = fp8kv_prefill_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);
    if (!row_strides_ok(p, 1)) return fail(VATTN_K_ERR_UNSUPPORTED, kRowStride);
    if (!out || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || p->seqlen_q <= 0) return fail(VATTN_K_ERR_INVALID, "vattn_fp8kv_prefill_plan_describe: bad shape");
#ifndef VATTN_LAB
    memset(out, 0, sizeof *out);
    fp8kv_prefill_describe(p, out);
    out->workspace_bytes = (int64_t)fp8kv_prefill_workspace_bytes(p);
    return VATTN_K_OK;
#else
    return VATTN_K_ERR_UNSUPPORTED;
#endif
}

int vattn_softcap_attn_with_kvcache(const vattn_attn_params* p, float softcap, void* stream) {
    if (softcap == 0.0f) return vattn_flash_attn_with_kvcache(p, stream);
    if (!softcap_ok(softcap)) return fail(VATTN_K_ERR_INVALID, kSoftcapValue);
    if (!abi_ok(p)) return validate(p);
    if (!softcap_pre_ok(p, softcap)) return fail(VATTN_K_ERR_INVALID, kSoftcapPre);
    if (const char* why = softcap_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);      // (before validate: the refusal names the softcap rule)
    int rc = validate(p);
    if (rc) return rc;
    if (p->k_new && p->seqlen_knew > 0 && !p->cache_seqlens) return fail(VATTN_K_ERR_INVALID, "If key is supplied, seqlens_k must also be passed in");
#ifndef VATTN_LAB
    return decode_form(p) ? launch_softcap_decode_form(p, softcap, (hipStream_t)stream) : launch_softcap_prefill_form(p, softcap, (hipStream_t)stream);
#else
    return VATTN_K_ERR_UNSUPPORTED;
#endif
}

// The soft-capped call runs the plain call's plan for the same block — its prefill form without the prefill64 branch, the rule of the prefill call
// over an fp8 cache (prefill_kernels.hip, plan_prefill): same planners, same answers, nothing tuned apart.
size_t vattn_softcap_attn_workspace_bytes(const vattn_attn_params* p, float softcap) {
    if (softcap == 0.0f) return vattn_attn_workspace_bytes(p);
    if (!softcap_ok(softcap) || !abi_ok(p) || !softcap_pre_ok(p, softcap) || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || p->seqlen_q <= 0 || softcap_gate_reason(p) || !row_strides_ok(p, 2)) return 0;
#ifndef VATTN_LAB
    return decode_form(p) ? decode_workspace_bytes(p) : fp8kv_prefill_workspace_bytes(p);
#else
    return 0;
#endif
}

int vattn_softcap_attn_plan_describe(const vattn_attn_params* p, float softcap, vattn_plan_desc* out) {
    if (softcap == 0.0f) return vattn_attn_plan_describe(p, out);
    if (!softcap_ok(softcap)) return fail(VATTN_K_ERR_INVALID, kSoftcapValue);
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library");
    if (!softcap_pre_ok(p, softcap)) return fail(VATTN_K_ERR_INVALID, kSoftcapPre);
    if (const char* why = softcap_gate_reason(p)) return fail(VATTN_K_ERR_UNSUPPORTED, why);
    if (!row_strides_ok(p, 2)) return fail(VATTN_K_ERR_UNSUPPORTED, kRowStride);
    if (!out || p->h_k <= 0 || p->h <= 0 || p->b <= 0 || p->seqlen_q <= 0) return fail(VATTN_K_ERR_INVALID, "vattn_softcap_attn_plan_describe: bad shape");
#ifndef VATTN_LAB
    memset(out, 0, sizeof *out);
    if (decode_form(p)) decode_describe(p, out);
    else fp8kv_prefill_describe(p, out);
    out->workspace_bytes = (int64_t)vattn_softcap_attn_workspace_bytes(p, softcap);
    return VATTN_K_OK;
#else
    return VATTN_K_ERR_UNSUPPORTED;
#endif
}

int vattn_attn_plan_describe(const vattn_attn_params* p, vattn_plan_desc* out) {
    if (!abi_ok(p)) return fail(VATTN_K_ERR_INVALID, "vattn_attn_params: struct_size / abi_version do not match this library");
    if (!row_strides_ok(p, 2)) return fail(VATTN_K_ERR_UNSUPPORTED, kRowStride);
    return plain_plan_describe(p, out);
}

int32_t vattn_decode_plan(const vattn_attn_params* p, const int32_t* cache_seqlens_host, vattn_decode_item* items_out, int32_t cap, int32_t* seq_out) {
    if (!abi_ok(p)) return VATTN_K_ERR_INVALID;
    if (p->window_left_plus1 > 0) return 0;      // windowed: the device-planned launch balances by visible length
    return decode_plan(p, cache_seqlens_host, items_out, cap, seq_out);
}

int32_t vattn_prefill_plan(const vattn_attn_params* p, const int32_t* q_lens_host, const int32_t* k_lens_host, vattn_prefill_item* items_out,
                           int32_t cap_items, vattn_prefill_item* blocks_out, int32_t cap_blocks, int32_t* counts_out) {
    if (!abi_ok(p)) return VATTN_K_ERR_INVALID;
    if (p->window_left_plus1 > 0) return window_plan_none(counts_out, 3);
    return prefill_worklist(p, q_lens_host, k_lens_host, items_out, cap_items, blocks_out, cap_blocks, counts_out);
}

int32_t vattn_prefill_plan_wg(const vattn_attn_params* p, const int32_t* q_lens_host, const int32_t* k_lens_host, vattn_prefill_item* items_out,
                              int32_t cap_items, vattn_prefill_item* blocks_out, int32_t cap_blocks, int32_t* wg_first_out, int32_t max_wg,
                              int32_t* counts_out) {
    if (!abi_ok(p)) return VATTN_K_ERR_INVALID;
    if (p->window_left_plus1 > 0) return window_plan_none(counts_out, 4);
    return prefill_worklist(p, q_lens_host, k_lens_host, items_out, cap_items, blocks_out, cap_blocks, counts_out, wg_first_out, max_wg, wg_first_out ? 1 : 2);
}

size_t vattn_hybrid_workspace_bytes(const vattn_attn_params* prefill, const vattn_attn_params* decode) {
    if (!abi_ok(prefill) || !abi_ok(decode)) return 0;
    if (!prefill || !decode || decode->h_k <= 0 || decode->h <= 0 || decode->b <= 0) return 0;
    return hybrid_workspace_bytes(prefill, decode);
}

int vattn_hybrid_attn(const vattn_attn_params* prefill, const vattn_attn_params* decode, void* workspace, void* stream) {
    int rc = validate(prefill);
    if (rc) return rc;
    rc = validate(decode);
    if (rc) return rc;
    return launch_hybrid(prefill, decode, workspace, (hipStream_t)stream);
}

int vattn_selftest_layouts(void* stream, int32_t* detail_out) {
    hipStream_t st = (hipStream_t)stream;
    int* d = nullptr;
    if (hipMalloc(&d, 8 * sizeof(int)) != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, "hipMalloc failed");
    (void)hipMemsetAsync(d, 0, 8 * sizeof(int), st);      // (a failure of any of these surfaces in the synchronising copy below)
    unsigned* gsrc = nullptr;
    unsigned hsrc[512];
    for (int i = 0; i < 512; i++) hsrc[i] = (unsigned)i;
    if (hipMalloc(&gsrc, sizeof(hsrc)) != hipSuccess) { (void)hipFree(d); return fail(VATTN_K_ERR_LAUNCH, "hipMalloc failed"); }
    (void)hipMemcpyAsync(gsrc, hsrc, sizeof(hsrc), hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, st, d, (const unsigned*)gsrc);
    (void)hipFuncSetAttribute((const void*)selftest_dma_high_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 << 10);
    hipLaunchKernelGGL(selftest_dma_high_kernel, dim3(1), dim3(64), 96 << 10, st, d, (const unsigned*)gsrc);
    int h[8] = {0};
    hipError_t e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d);
    (void)hipFree(gsrc);
    if (e != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
    int bad = 0;
    for (int i = 0; i < 8; i++) {
        if (detail_out) detail_out[i] = h[i];
        if (i < 6) bad |= h[i];            // [6], [7] report LDS-DMA behaviour (out-of-range lanes, destinations beyond 64 KiB)
    }
    return bad ? fail(VATTN_K_ERR_INVALID, "hardware layout assumption violated") : VATTN_K_OK;
}

float vattn_time_attn(const vattn_attn_params* p, void* stream, int32_t warmup, int32_t iters) {
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < warmup; i++)
        if (vattn_flash_attn_with_kvcache(p, stream) != 0) return -1.f;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return -1.f;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return -1.f; }
    hipError_t e = hipEventRecord(e0, st);
    for (int i = 0; i < iters && e == hipSuccess; i++)
        if (vattn_flash_attn_with_kvcache(p, stream) != 0) e = hipErrorUnknown;
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (e != hipSuccess) return -1.f;
    return ms / (iters > 0 ? iters : 1);
}

}  // extern "C"
