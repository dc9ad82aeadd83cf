// Building blocks shared by the two prefill64 kernels (prefill64_kernels.hip: one workgroup per query block; prefill64p_kernels.hip:
// persistent workgroups that walk a queue of query-block pieces): LDS-DMA pieces, the running buffer descriptors in fixed SGPR quads,
// the matrix instructions with the register file of every operand fixed by the constraint, and the tile step itself (tile_step, with
// its fragment readers, softmax stages and the LDS image they address).
#pragma once
#include "attn_common.h"

namespace vattn_k {

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr float kDeferLog2 = 6.0f;      // P stays below 2^6 between rescales (f16 / bf16 keep their relative precision)

// ---- LDS-DMA: one 1-KiB piece (64 lanes x 16 bytes) of a K or V tile per call ----
// lds_addr: wave-uniform LDS byte address of the piece; rsrc: buffer descriptor of the tile, bounded at the visible rows; voff:
// per-lane byte offset inside the tile.  A lane whose offset lies beyond the descriptor fetches nothing (zeros).  s_nop 0 after
// the M0 write is the M0 -> LDS-DMA hazard; the _first form opens with s_nop 4 for a descriptor whose SGPRs were written by a
// VALU readfirstlane (cdna guide §5.7).  The compiler's wait-count pass does not see these loads: waits are counted by hand.
__device__ __forceinline__ void dma_piece(unsigned lds_addr, u32x4 rsrc, unsigned voff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %1, 0 offen lds" : : "s"(lds_addr), "s"(rsrc), "v"(voff) : "memory", "m0");
}
__device__ __forceinline__ void dma_piece_first(unsigned lds_addr, u32x4 rsrc, unsigned voff) {
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %1, 0 offen lds" : : "s"(lds_addr), "s"(rsrc), "v"(voff) : "memory", "m0");
}
// the same with the piece's LDS address formed in M0 by one SALU add (base register + literal): steady-state form, the descriptor's
// SGPRs are SALU-written (no VALU -> SGPR -> VMEM hazard, no s_nop 4)
template <int OFF> __device__ __forceinline__ void dma_piece_at(unsigned lds_base, u32x4 rsrc, unsigned voff) {
    asm volatile("s_add_u32 m0, %0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %1, 0 offen lds" : : "s"(lds_base), "s"(rsrc), "v"(voff), "i"(OFF) : "memory", "m0", "scc");
}
// the same with the piece's distance from piece 0 in the SCALAR offset operand (ROWS x row_bytes, formed by one s_mul in the wait state
// behind the M0 write): every piece of a tile then takes piece 0's per-lane offset — no v_mad per piece (a VALU instruction beside the
// MFMAs costs 7.3 cycles of this wave, a scalar one 0.3: profiles/r06_p64_price_list.txt).  The scalar offset is part of the descriptor's
// range check on gfx950 (tools/lab/soffset_probe.cpp: a lane with voffset + soffset >= num_records reads zeros), so rows beyond the
// sequence's visible length stay unfetched exactly as before.
template <int OFF, int ROWS> __device__ __forceinline__ void dma_piece_so(unsigned lds_base, u32x4 rsrc, unsigned voff, unsigned row_bytes) {
    unsigned so;
    asm volatile("s_add_u32 m0, %1, %6\n\ts_mul_i32 %0, %4, %5\n\tbuffer_load_dwordx4 %3, %2, %0 offen lds"
                 : "=&s"(so) : "s"(lds_base), "s"(rsrc), "v"(voff), "s"(row_bytes), "n"(ROWS), "i"(OFF) : "memory", "m0", "scc");
}
// base + ROWS x row_bytes per lane (row strides are far below 2^24 bytes)
template <int ROWS> __device__ __forceinline__ unsigned piece_off(unsigned base, unsigned row_bytes) {
    unsigned r;
    asm("v_mad_u32_u24 %0, %1, %3, %2" : "=v"(r) : "s"(row_bytes), "v"(base), "n"(ROWS));
    return r;
}
// The two running buffer descriptors of the steady state live in FIXED scalar registers — K(t+3)'s in s[92:95], V(t+2)'s in s[96:99] —
// so that moving one a tile forward is a handful of SALU instructions on its own words and the DMA reads the quad where it is: no
// copies into an aligned tuple, no second set of registers (the kernel sits at the SGPR limit; an SGPR spill costs a scratch access
// whose wait count the hand-counted DMA waits do not know).  base += tile bytes (with carry); rows left behind the new base -= 64;
// bound = clamp(rows left, 0, 64) x row bytes: past the sequence's end nothing is fetched.  Counting ROWS keeps every quantity far
// from 32 bits whatever the row stride (a layer's view of a megacache tensor has rows of 64 KiB and spans > 4 GiB at 128 k tokens).
// The caller places the call inside an MFMA gap.
__device__ __forceinline__ void k_rsrc_advance(u32x4& r, int& rows_left, unsigned tile_bytes, unsigned row_bytes) {
    asm volatile("s_add_u32 s92, s92, %3\n\ts_addc_u32 s93, s93, 0\n\ts_sub_i32 %1, %1, 64\n\ts_min_i32 s94, %1, 64\n\ts_max_i32 s94, s94, 0\n\ts_mul_i32 s94, s94, %4"
                 : "={s[92:95]}"(r), "+s"(rows_left) : "0"(r), "s"(tile_bytes), "s"(row_bytes) : "scc");
}
__device__ __forceinline__ void v_rsrc_advance(u32x4& r, int& rows_left, unsigned tile_bytes, unsigned row_bytes) {
    asm volatile("s_add_u32 s96, s96, %3\n\ts_addc_u32 s97, s97, 0\n\ts_sub_i32 %1, %1, 64\n\ts_min_i32 s98, %1, 64\n\ts_max_i32 s98, s98, 0\n\ts_mul_i32 s98, s98, %4"
                 : "={s[96:99]}"(r), "+s"(rows_left) : "0"(r), "s"(tile_bytes), "s"(row_bytes) : "scc");
}
__device__ __forceinline__ u32x4 tile_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    u32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) & 0xffffu;     // stride 0, no swizzle
    r[2] = __builtin_amdgcn_readfirstlane(bytes);                             // num_records (bytes): the bound
    r[3] = 0x00020000u;                                                       // raw buffer, 32-bit data format
    return r;
}

// ---- matrix instructions with the register FILE of every operand fixed by the constraint (cdna guide §5.7) ----
// S^T accumulators live in architectural VGPRs (the softmax VALU reads them), O^T accumulators and the Q^T fragments in the
// accumulator half of the 512-entry file; hipcc's own allocation of a 512-register kernel shuttles all of them through
// v_accvgpr_read/write (measured: 2 700 copies and 324 spills in the builtin version of this kernel).
// hipcc does not pad hazards around inline asm: callers keep MFMA results away from VALU readers by program order (an 8-pass
// MFMA result is readable >= 12 states later) and use the _NOP forms when an A/B/C operand was just written by the VALU.
template <typename T> struct Mfma;
#define VATTN_MFMA_STRUCT(TYPE, MNEM)                                                                                                    \
    template <> struct Mfma<TYPE> {                                                                                                \
        using V8 = typename Tr<TYPE>::v8;                                                                                          \
        /* S(vgpr) = A(vgpr) x B(agpr) + 0: the first MFMA of a chain */                                                           \
        static __device__ __forceinline__ void qk_first(f32x16& d, V8 a, V8 b) {                                                   \
            asm volatile(MNEM " %0, %1, %2, 0" : "=&v"(d) : "v"(a), "a"(b));                                                       \
        }                                                                                                                          \
        static __device__ __forceinline__ void qk_acc(f32x16& d, V8 a, V8 b) {                                                     \
            asm volatile(MNEM " %0, %1, %2, %0" : "+v"(d) : "v"(a), "a"(b));                                                       \
        }                                                                                                                          \
        /* the same with the A fragment in the accumulator half (fragments carried from one tile step to the next are read from LDS  \
           straight into accumulator registers: no v_accvgpr_read at the seam) */                                                   \
        static __device__ __forceinline__ void qk_first_a(f32x16& d, V8 a, V8 b) {                                                 \
            asm volatile(MNEM " %0, %1, %2, 0" : "=&v"(d) : "a"(a), "a"(b));                                                       \
        }                                                                                                                          \
        static __device__ __forceinline__ void qk_acc_a(f32x16& d, V8 a, V8 b) {                                                   \
            asm volatile(MNEM " %0, %1, %2, %0" : "+v"(d) : "a"(a), "a"(b));                                                       \
        }                                                                                                                          \
        /* O(agpr) += A(vgpr) x B(vgpr) */                                                                                         \
        static __device__ __forceinline__ void pv(f32x16& o, V8 a, V8 b) {                                                         \
            asm volatile(MNEM " %0, %1, %2, %0" : "+a"(o) : "v"(a), "v"(b));                                                       \
        }                                                                                                                          \
    };
VATTN_MFMA_STRUCT(_Float16, "v_mfma_f32_32x32x16_f16")
VATTN_MFMA_STRUCT(__bf16, "v_mfma_f32_32x32x16_bf16")
#undef VATTN_MFMA_STRUCT
// one scalar f32 add that the SLP vectoriser cannot pack into v_pk_add_f32 (packed f32 VALU beside MFMAs costs more than two
// plain adds, MI355X_MICROARCH "price of one filler")
__device__ __forceinline__ float add1(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// no instruction is scheduled across it: the tile step's groups stay where they are written
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// ---- the tile step of the two kernels (head dimension 128, 64 query rows per wave, 64-key tiles) ----
// The LDS image (address 0): the K ring (2 slots), then the V ring (3 slots of PfSmem<128>::kTileBytes).  A K tile is stored as 16
// pieces of 4 rows, each piece 1088 bytes apart (64 bytes of padding), inside a piece chunk c of row r3 at byte 64*c + 16*r3.
// ds_read_b128's lane groups ({0-3,12-15,20-27}, ...) then hit 16 distinct 16-byte slots of the 256-byte bank row WITHOUT an XOR
// swizzle, so the address of fragment (kk, kb) is one lane-dependent register + the immediate 8704*kb + 128*kk (+ the slot, static
// because slots go by (t - tb) & 1 and the loop is unrolled twice): no per-fragment address arithmetic in the hot loop.  V is stored as
// [d/32][key][32 d] sub-tiles for ds_read_b64_tr_b16.
constexpr int kKPiece = 1088;
constexpr int kKSlot = 16 * 1088;
constexpr int kVBase = 36864;

// LDS fragment reads: the kernel's lane-dependent base (kfrag_lane / vfrag_lane) + immediate offsets
template <typename V8> __device__ __forceinline__ V8 kfrag(const char* ksm, int f, unsigned kfrag_lane) {      // f = 2*kk + kb: K rows 32*kb + l31, d = 16*kk + 8*g ..
    const int kk = f >> 1, kb = f & 1;
    return *(const V8*)(ksm + kb * 8 * kKPiece + kk * 128 + kfrag_lane);
}
template <typename V8> __device__ __forceinline__ V8 vfrag(const char* vsm, int f, unsigned vfrag_lane) {      // f = 4*ks + db: keys 16*ks .. 16*ks+15, d block db
    const int ks = f >> 2, db = f & 3;
    const char* a1 = vsm + db * PfSmem<128>::kVSubBytes + (16 * ks) * 64 + vfrag_lane;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, a1));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, a1 + 8 * 64));
    return join_tr<V8>(lo, hi);
}
__device__ __forceinline__ float row_max(const f32x16 (&s)[2][2], int qc) {
    float m0 = fmaxf(s[0][qc][0], s[1][qc][0]);
#pragma unroll
    for (int r = 1; r < 16; r++) m0 = fmaxf(fmaxf(m0, s[0][qc][r]), s[1][qc][r]);     // v_max3_f32
    return fmaxf(m0, swap_halves(m0));
}
// moves the running maximum of query block qc up by delta >= 0 (log2 units, per lane): everything accumulated at the old scale
// — O and l — is rescaled exactly once (cdna guide T13); scores not yet exponentiated are raw and take the new maximum
template <int DB> __device__ __forceinline__ void raise_max(f32x16 (&o)[DB][2], float (&l_acc)[2][2], float (&nmsub)[2], int qc, float delta) {
    const float alpha = fast_exp2(-delta);
    nmsub[qc] -= delta;
#pragma unroll
    for (int i = 0; i < DB; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[i][qc][r] *= alpha;
#pragma unroll
    for (int a4 = 0; a4 < 2; a4++) l_acc[qc][a4] *= alpha;
}
// P(t) -> the PV B-operand fragment of key slice ks for query block qc: slot (g, j) <-> P registers 8*(ks&1) + j of key block ks>>1
template <typename T> __device__ __forceinline__ typename Tr<T>::v8 pack_p(const f32x16 (&pt)[2][2], int ks, int qc) {
    typename Tr<T>::v8 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = Tr<T>::cvt(pt[ks >> 1][qc][8 * (ks & 1) + j]);
    return r;
}
// clamp(rows, 0, 64) x row bytes by scalar min / max: the compiler's own clamp is a VALU v_med3 (+ a copy back that it cannot do)
__device__ __forceinline__ unsigned bound(int rows, unsigned rs) {
    int r;
    asm("s_min_i32 %0, %1, 64\n\ts_max_i32 %0, %0, 0" : "=s"(r) : "s"(rows) : "scc");
    return (unsigned)r * rs;
}

// ---- software pipeline of the softmax VALU work, in units of PAIRS of scores (pair e: key block e>>4, half (e>>3)&1, query
// block (e>>2)&1, registers 8*half + 2*(e&3), +1 — the order in which the P.V key slices consume them).  Stage E (two
// v_exp) of pair e sits in group GE(e) of the tile's 64 MFMA groups, stage M (two v_fma: s*scale*log2e - m*scale*log2e) one
// group earlier, stage A (two v_add into the two row-sum accumulators) one group later: no instruction waits for the one
// before it (one wave per SIMD: a stalled wave issues no MFMA either).  The exp2 is IN PLACE: the S' register becomes the P register.
template <int NA> __device__ __forceinline__ void softmax_stages(int G, f32x16 (&cur)[2][2], float (&l_acc)[2][2], const float (&nmsub)[2], unsigned escale_s) {
    auto GE = [](int e) { return e < NA ? 1 + (e * 30) / NA : 33 + ((e - NA) * 17) / (32 - NA); };
#define P64_X0(cur, e) cur[(e) >> 4][((e) >> 2) & 1][8 * (((e) >> 3) & 1) + 2 * ((e) & 3)]
#define P64_X1(cur, e) cur[(e) >> 4][((e) >> 2) & 1][8 * (((e) >> 3) & 1) + 2 * ((e) & 3) + 1]
#pragma unroll
    for (int e = 0; e < 32; e++) {
        const int qc = (e >> 2) & 1;
        if (GE(e) - 1 == G)
            asm("v_fma_f32 %0, %0, %2, %3\n\tv_fma_f32 %1, %1, %2, %3" : "+v"(P64_X0(cur, e)), "+v"(P64_X1(cur, e)) : "s"(escale_s), "v"(nmsub[qc]));
        if (GE(e) == G) asm("v_exp_f32 %0, %0\n\tv_exp_f32 %1, %1" : "+v"(P64_X0(cur, e)), "+v"(P64_X1(cur, e)));
        if (GE(e) + 1 == G)      // (v_pk_add_f32: a packed-f32 instruction beside the MFMAs costs 43 cycles, six plain ones)
            asm("v_add_f32 %0, %0, %2\n\tv_add_f32 %1, %1, %3" : "+v"(l_acc[qc][0]), "+v"(l_acc[qc][1]) : "v"(P64_X0(cur, e)), "v"(P64_X1(cur, e)));
    }
#undef P64_X0
#undef P64_X1
}

// S(tb) of a cold start = K(tb).Q^T with K(tb) in K slot 0 (ksm); on return the results are VALU-readable
template <typename T, int KK> __device__ __forceinline__ void first_scores(const char* ksm, f32x16 (&sc)[2][2], const typename Tr<T>::v8 (&qf)[2][KK], unsigned kfrag_lane) {
    using V8 = typename Tr<T>::v8;
    using M = Mfma<T>;
#pragma unroll
    for (int f = 0; f < 2 * KK; f++) {
        const V8 a = kfrag<V8>(ksm, f, kfrag_lane);
#pragma unroll
        for (int qc = 0; qc < 2; qc++) {
            if (f < 2) M::qk_first(sc[f & 1][qc], a, qf[qc][f >> 1]);
            else M::qk_acc(sc[f & 1][qc], a, qf[qc][f >> 1]);
        }
    }
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");     // the last MFMA results are VALU-readable from here
    SCHED_FENCE();
}

// Row maxima of S'(t+1) after a tile step, raw (mx0 / mx1, per query block) and as growth over the running maxima in log2 units (g0 / g1,
// grow = the larger): the caller masks the tile and retakes them where it must, and rescales when grow > kDeferLog2 in some lane.
struct StepMax {
    float mx0, mx1, g0, g1, grow;
};
// The 64 groups of one tile step of the wave: 64 x { MFMA ; fragment read ahead ; a slice of softmax VALU }.  cur holds S(t) on entry
// and P(t) afterwards, nxt receives S(t+1); kf0 / kf1 / kf2 hold the first three K(t+1) fragments on entry (read before the previous step
// ended) and the first three of K(t+2) on exit.  par = (t - tb) & 1, a literal at the call sites: with the padded K image every K fragment
// address folds to lane + immediate.
// The DMA stream's scalars are carried across the steps and advanced INSIDE MFMA gaps (a lone wave pays an issue slot for every SALU
// instruction, and whatever sits between the last MFMA of a step and the first of the next is not hidden at all): rk / rv, descriptors
// of K(t+2) / V(t+1) at step entry (in the fixed SGPR quads of k_rsrc_advance / v_rsrc_advance), are moved one tile on in phase A and fetch K(t+3) / V(t+2)
// in phase B; vs_cur / vs_dma, byte offsets inside the V ring of V(t)'s slot and of the slot V(t+2) goes to (= the one V(t-1) left).
// Invariants at entry: K(t+1) and V(t) have landed and every wave knows it (the barrier of step t-1); K(t+2) and V(t+1) are in flight.
// The barrier of this step opens phase-B group BJ: by then every wave has finished reading K(t+1) (phase A) and V(t-1) (step t-1), so
// K(t+3) -> slot of K(t+1) and V(t+2) -> slot of V(t-1) may be issued behind it — one piece every DS-th group from group D0 on
// (back-to-back pieces in the barrier's own group and the seven after it, round 2's placement, measured 1-2 % slower on boxes that are
// not pinned at their power limit: profiles/r03_p64_schedules.txt).  NA: the first NA of the tile's 32 exp2 pairs start in phase A;
// RING: the K / V^T fragment ring (RING - 1 fragments ahead of their MFMA); MS: the first phase-B group of the row-max chain of S'(t+1).
// hook(i) is called in every phase-A group i, behind the group's own work.
// Every wave runs the SAME straight-line body for every tile of the workgroup (the barrier makes the waves wait for each other anyway):
// a tile that lies wholly beyond a wave's causal limit is masked to -inf by the caller, contributes P = 0, and leaves the running maximum
// alone; past the last tile S'(t+1) is computed from a zero-filled K slot and never used.
template <typename T, int NA, int RING, int MS, int BJ, int D0, int DS, typename Hook>
__device__ __forceinline__ StepMax tile_step(const int par, const char* smem, f32x16 (&cur)[2][2], f32x16 (&nxt)[2][2], typename Tr<T>::v8& kf0,
                                             typename Tr<T>::v8& kf1, typename Tr<T>::v8& kf2, const typename Tr<T>::v8 (&qf)[2][8], f32x16 (&o)[4][2],
                                             float (&l_acc)[2][2], const float (&nmsub)[2], u32x4& rk, u32x4& rv, int& k_rows_left, int& v_rows_left,
                                             unsigned& vs_cur, unsigned& vs_dma, unsigned k_lds_wave, unsigned v_lds_wave, unsigned koff, unsigned voff,
                                             unsigned k_rs_bytes, unsigned v_rs_bytes, unsigned k_tile_b, unsigned v_tile_b, unsigned kfrag_lane,
                                             unsigned vfrag_lane, unsigned escale_s, Hook hook) {
    using V8 = typename Tr<T>::v8;
    using M = Mfma<T>;
    using S = PfSmem<128>;
    constexpr int KK = 8;
    static_assert(D0 >= BJ && D0 + 7 * DS < 32, "DMA pieces behind the barrier, inside phase B");
    static_assert(NA >= 16 && NA < 32, "key slice 0 of P is packed in phase-A groups 13 / 15: its eight pairs must be exponentiated by group 12");
    static_assert(MS >= 4 && MS + 19 < 32, "row-max chain >= 4 MFMAs behind the last S^T MFMA, its reduction inside phase B");
    auto dma_gap = [](int k) { return D0 + DS * k; };
    const int s_cur = par;                                                  // slot of K(t), K(t+2)
    const char* ksm = smem + (s_cur ^ 1) * kKSlot;                          // K(t+1)
    const char* ksm_next = smem + s_cur * kKSlot;                           // K(t+2)
    const char* vsm = smem + kVBase + vs_cur;                               // V(t)
    const unsigned lk0 = k_lds_wave + (unsigned)((s_cur ^ 1) * kKSlot);     // K(t+3) -> the slot K(t+1) leaves
    unsigned lv0 = 0;                                                       // V(t+2)'s pieces of this wave (set in phase A)
    // phase A: S'(t+1) = K(t+1).Q^T - m   (32 MFMAs: k-step kk = i>>2, key block (i>>1)&1, query block i&1)
    V8 pf[2][2];         // P(t) fragments of the key slice being multiplied and of the next one
    V8 kf[RING];         // RING - 1 fragments (twice as many MFMAs) ahead of their use
    V8 vf[RING];         // V(t)^T fragments of phase B
    SCHED_FENCE();
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const int f = i >> 1, qc = i & 1;
        if (f < RING - 1) {
            // the fragments read before the previous step ended sit in accumulator registers
            const V8 a = f == 0 ? kf0 : (f == 1 ? kf1 : kf2);
            if (i < 4) M::qk_first_a(nxt[f & 1][qc], a, qf[qc][f >> 1]);
            else M::qk_acc_a(nxt[f & 1][qc], a, qf[qc][f >> 1]);
        } else if (i < 4) M::qk_first(nxt[f & 1][qc], kf[f % RING], qf[qc][f >> 1]);
        else M::qk_acc(nxt[f & 1][qc], kf[f % RING], qf[qc][f >> 1]);
        if ((i & 1) == 0 && f + RING - 1 < 2 * KK) kf[(f + RING - 1) % RING] = kfrag<V8>(ksm, f + RING - 1, kfrag_lane);
        softmax_stages<NA>(i, cur, l_acc, nmsub, escale_s);
        // key slice 0 of P(t) (pairs 0-7: exponentiated by group GE(7) <= 12 for NA >= 16) is packed HERE, so the first P.V MFMA
        // of phase B does not wait for eight conversions issued right in front of it
        if (i == 13) pf[0][0] = pack_p<T>(cur, 0, 0);
        if (i == 15) pf[0][1] = pack_p<T>(cur, 0, 1);
        // the DMA stream's scalars move one tile on (SALU work, inside gaps)
        if (i == 17) lv0 = v_lds_wave + vs_dma;
        if (i == 19) asm volatile("s_mov_b32 %1, %0\n\ts_add_u32 %0, %0, %2\n\ts_cmp_eq_u32 %0, %3\n\ts_cselect_b32 %0, 0, %0"
                                  : "+s"(vs_cur), "=&s"(vs_dma) : "i"(S::kTileBytes), "i"(3 * S::kTileBytes) : "scc");
        if (i == 21) k_rsrc_advance(rk, k_rows_left, k_tile_b, k_rs_bytes);
        if (i == 23) v_rsrc_advance(rv, v_rows_left, v_tile_b, v_rs_bytes);
        hook(i);
        // V(t) landed a step ago: its first fragments are asked for while the last S' MFMAs run (the K ring has stopped reading at i = 24)
        if (i == 26) vf[0] = vfrag<V8>(vsm, 0, vfrag_lane);
        if (i == 28) vf[1] = vfrag<V8>(vsm, 1, vfrag_lane);
        if (i == 30 && RING > 3) vf[2] = vfrag<V8>(vsm, 2, vfrag_lane);
        SCHED_FENCE();
    }
    // phase B: O^T += V(t)^T.P(t)^T   (32 MFMAs: key slice ks = j>>3, d block (j>>1)&3, query block j&1)
    float mx0 = -INFINITY, mx1 = -INFINITY, g0 = -INFINITY, g1 = -INFINITY, grow = -INFINITY;
    SCHED_FENCE();
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const int f = j >> 1, ks = j >> 3, qc = j & 1;
        if (j == BJ) {
            // this wave's pieces of K(t+2) and V(t+1) (issued one step ago) have landed; behind the barrier everyone's have, and
            // every wave is past its reads of K(t+1) and V(t-1)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        // (a P fragment is packed at least one MFMA group before its first use: no VALU -> MFMA operand hazard to pad)
        M::pv(o[f & 3][qc], vf[f % RING], pf[ks & 1][qc]);
        if ((j & 1) == 0 && f + RING - 1 < 16) vf[(f + RING - 1) % RING] = vfrag<V8>(vsm, f + RING - 1, vfrag_lane);
        softmax_stages<NA>(32 + j, cur, l_acc, nmsub, escale_s);
        // P fragments of key slice ks+1 are packed while slice ks is multiplied (4 cvt_pk per group, groups 4 and 6 of a slice)
        if (ks < 3 && (j & 7) == 4) pf[(ks + 1) & 1][0] = pack_p<T>(cur, ks + 1, 0);
        if (ks < 3 && (j & 7) == 6) pf[(ks + 1) & 1][1] = pack_p<T>(cur, ks + 1, 1);
        // row max of S'(t+1): 2 chains x 16 v_max3, groups MS .. MS+15 (>= 4 MFMAs after the last S^T MFMA was issued); the
        // half-wave exchange and the growth test follow in the next gaps, so that only the branch itself is left behind the
        // step's last MFMA
        if (j >= MS && j < MS + 16) {
            const int r = j - MS;
            if (r == 0) {      // the chain's first link needs no -inf to start from
                asm("v_max_f32_e32 %0, %1, %2" : "=v"(mx0) : "v"(nxt[0][0][0]), "v"(nxt[1][0][0]));
                asm("v_max_f32_e32 %0, %1, %2" : "=v"(mx1) : "v"(nxt[0][1][0]), "v"(nxt[1][1][0]));
            } else {
                asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mx0) : "v"(nxt[0][0][r]), "v"(nxt[1][0][r]));
                asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mx1) : "v"(nxt[0][1][r]), "v"(nxt[1][1][r]));
            }
        }
        if (j == MS + 16) mx0 = max_halves(mx0);
        if (j == MS + 17) mx1 = max_halves(mx1);
        if (j == MS + 18) {
            // growth of the row maxima over the running maxima, log2 units (nmsub = -m*scale*log2e; -inf for rows that see nothing here)
            asm("v_fma_f32 %0, %2, %4, %5\n\tv_fma_f32 %1, %3, %4, %6" : "=&v"(g0), "=&v"(g1) : "v"(mx0), "v"(mx1), "s"(escale_s), "v"(nmsub[0]), "v"(nmsub[1]));
        }
        if (j == MS + 19) asm("v_max_f32 %0, %1, %2" : "=v"(grow) : "v"(g0), "v"(g1));
        // this wave's four pieces of K(t+3) and of V(t+2): every piece takes piece 0's per-lane offset, its distance from piece 0 (4 K rows |
        // 16 V keys per piece) travels in the load's scalar offset (dma_piece_so)
        if (j == dma_gap(0)) dma_piece_at<0>(lk0, rk, koff);
        if (j == dma_gap(1)) dma_piece_so<kKPiece, 4>(lk0, rk, koff, k_rs_bytes);
        if (j == dma_gap(2)) dma_piece_so<2 * kKPiece, 8>(lk0, rk, koff, k_rs_bytes);
        if (j == dma_gap(3)) dma_piece_so<3 * kKPiece, 12>(lk0, rk, koff, k_rs_bytes);
        if (j == dma_gap(4)) dma_piece_at<0>(lv0, rv, voff);
        if (j == dma_gap(5)) dma_piece_so<1024, 16>(lv0, rv, voff, v_rs_bytes);
        if (j == dma_gap(6)) dma_piece_so<2048, 32>(lv0, rv, voff, v_rs_bytes);
        if (j == dma_gap(7)) dma_piece_so<3072, 48>(lv0, rv, voff, v_rs_bytes);
        if (j == 27) kf0 = kfrag<V8>(ksm_next, 0, kfrag_lane);          // the next step's first K fragments: K(t+2) is behind the barrier
        if (j == 28) kf1 = kfrag<V8>(ksm_next, 1, kfrag_lane);
        if (j == 29 && RING > 3) kf2 = kfrag<V8>(ksm_next, 2, kfrag_lane);
        SCHED_FENCE();
    }
    return {mx0, mx1, g0, g1, grow};
}

}  // namespace vattn_k
