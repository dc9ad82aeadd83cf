// cache_flat / append: contiguous KV append (16-byte vector copies).  gfx950.
#include "attn_common.h"

namespace vattn_k {

// ============================================================================================
// cache_flat / append
// ============================================================================================

// One 16-byte chunk per thread; K and V rows copied by the same launch (cache_kernels.cu:483-520).
__global__ void cache_flat_vec_kernel(const uint4* __restrict__ key, const uint4* __restrict__ value,
                                      uint4* __restrict__ k_cache, uint4* __restrict__ v_cache,
                                      int64_t num_tokens, int chunks_per_row, int64_t key_stride, int64_t value_stride,
                                      int64_t k_cache_stride, int64_t v_cache_stride) {
    // strides are in 16-byte chunks here
    const int64_t total = num_tokens * chunks_per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = i / chunks_per_row;
        const int c = (int)(i - t * chunks_per_row);
        const uint4 kv = key[t * key_stride + c];
        const uint4 vv = value[t * value_stride + c];
        k_cache[t * k_cache_stride + c] = kv;
        v_cache[t * v_cache_stride + c] = vv;
    }
}

template <typename E>
__global__ void cache_flat_scalar_kernel(const E* __restrict__ key, const E* __restrict__ value, E* __restrict__ k_cache,
                                         E* __restrict__ v_cache, int64_t num_tokens, int n, int64_t key_stride,
                                         int64_t value_stride, int64_t k_cache_stride, int64_t v_cache_stride) {
    const int64_t total = num_tokens * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = i / n;
        const int c = (int)(i - t * n);
        k_cache[t * k_cache_stride + c] = key[t * key_stride + c];
        v_cache[t * v_cache_stride + c] = value[t * value_stride + c];
    }
}

// cache_flat with the rotary embedding of the key rows fused in (include/vattn_kernels.h): one thread per (token, head, 8-element
// chunk of the FIRST half): it owns the chunk and its NeoX partner chunk (d + hs/2), rotates both and stores both; the V row
// is copied by the same thread (two chunks).
template <typename T>
__global__ void cache_flat_rope_kernel(const T* __restrict__ key, const T* __restrict__ value, T* __restrict__ k_cache, T* __restrict__ v_cache,
                                       int64_t num_tokens, int num_heads, int hs, int64_t key_stride, int64_t value_stride,
                                       int64_t k_cache_stride, int64_t v_cache_stride, const T* __restrict__ cos_sin, int64_t cs_stride, int64_t pos0) {
    using V8 = typename Tr<T>::v8;
    const int half_chunks = hs / 16;
    const int64_t total = num_tokens * num_heads * half_chunks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % half_chunks);
        const int h = (int)((i / half_chunks) % num_heads);
        const int64_t t = i / ((int64_t)half_chunks * num_heads);
        const int d0 = 8 * c;
        const T* krow = key + t * key_stride + (int64_t)h * hs;
        const T* vrow = value + t * value_stride + (int64_t)h * hs;
        V8 x = as_v8<V8>(*(const uint4*)(krow + d0)), y = as_v8<V8>(*(const uint4*)(krow + hs / 2 + d0));
        const T* cs = cos_sin + (pos0 + t) * cs_stride;
        const V8 cc = as_v8<V8>(*(const uint4*)(cs + d0)), ss = as_v8<V8>(*(const uint4*)(cs + hs / 2 + d0));
        rope8<T>(x, y, cc, ss);
        T* kdst = k_cache + t * k_cache_stride + (int64_t)h * hs;
        T* vdst = v_cache + t * v_cache_stride + (int64_t)h * hs;
        uint4 ux, uy;
        __builtin_memcpy(&ux, &x, 16);
        __builtin_memcpy(&uy, &y, 16);
        *(uint4*)(kdst + d0) = ux;
        *(uint4*)(kdst + hs / 2 + d0) = uy;
        *(uint4*)(vdst + d0) = *(const uint4*)(vrow + d0);
        *(uint4*)(vdst + hs / 2 + d0) = *(const uint4*)(vrow + hs / 2 + d0);
    }
}

// The reference's stand-alone rotary kernel (pos_encoding_kernels.cu:39-77): in place on query and key, one thread per
// (token, head, rotation pair).
template <typename T, bool NEOX>
__global__ void rotary_embedding_kernel(const int64_t* __restrict__ positions, T* __restrict__ query, T* __restrict__ key,
                                        const T* __restrict__ cos_sin, int64_t cs_stride, int rot_dim, int64_t query_stride,
                                        int64_t key_stride, int num_heads, int num_kv_heads, int hs, int64_t num_tokens) {
#pragma clang fp contract(off)      // every product is rounded to the I/O dtype before the sum, as scalar_t arithmetic does in the reference
    using X = Tr<T>;
    const int e = rot_dim / 2;
    const int64_t per_tok = (int64_t)(num_heads + num_kv_heads) * e;
    const int64_t total = num_tokens * per_tok;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = i / per_tok;
        const int r = (int)(i % per_tok);
        const int head = r / e, ro = r % e;
        T* arr = head < num_heads ? query + t * query_stride + (int64_t)head * hs : key + t * key_stride + (int64_t)(head - num_heads) * hs;
        const T* cs = cos_sin + positions[t] * cs_stride;
        const int xi = NEOX ? ro : 2 * ro, yi = NEOX ? e + ro : 2 * ro + 1;
        const float cf = (float)cs[ro], sf = (float)cs[e + ro];
        const float xf = (float)arr[xi], yf = (float)arr[yi];
        const float p1 = (float)X::cvt(xf * cf), p2 = (float)X::cvt(yf * sf), q1 = (float)X::cvt(yf * cf), q2 = (float)X::cvt(xf * sf);
        arr[xi] = X::cvt(p1 - p2);
        arr[yi] = X::cvt(q1 + q2);
    }
}

// Append of k_new/v_new [b, sn, h_k, d] at row cache_seqlens[b] of slot cache_batch_idx[b]
// (flash_attn_interface.py:1168-1176).  16-byte chunks; d*itemsize is a multiple of 16.  With fused RoPE the key chunk of the
// first half and its partner chunk are rotated by the thread that owns the first-half chunk.
template <typename T> __device__ __forceinline__ void append_rope_pair(const vattn_attn_params& p, const uint16_t* src, uint16_t* dst, int c, int64_t pos) {
    using V8 = typename Tr<T>::v8;
    V8 x = as_v8<V8>(*(const uint4*)(src + c * 8)), y = as_v8<V8>(*(const uint4*)(src + p.d / 2 + c * 8));
    V8 cc, ss;
    rope_load<T>(p, pos, c * 8, cc, ss);
    rope8<T>(x, y, cc, ss);
    uint4 ux, uy;
    __builtin_memcpy(&ux, &x, 16);
    __builtin_memcpy(&uy, &y, 16);
    *(uint4*)(dst + c * 8) = ux;
    *(uint4*)(dst + p.d / 2 + c * 8) = uy;
}
__global__ void append_kv_kernel(vattn_attn_params p) {
    const int b = blockIdx.y;
    const int slot = p.cache_batch_idx ? p.cache_batch_idx[b] : b;
    const int len = p.cache_seqlens ? p.cache_seqlens[b] : p.seqlen_k;
    const int cpr = p.d / 8;                       // 16-byte chunks per head row
    const int total = p.seqlen_knew * p.h_k * cpr;
    const uint16_t* kn = (const uint16_t*)p.k_new;
    const uint16_t* vn = (const uint16_t*)p.v_new;
    uint16_t* kc = (uint16_t*)p.k_cache;
    uint16_t* vc = (uint16_t*)p.v_cache;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int c = i % cpr;
        const int hk = (i / cpr) % p.h_k;
        const int t = i / (cpr * p.h_k);
        const int row = len + t;
        if (row >= p.seqlen_k) continue;           // never write past the cache view
        const uint16_t* ksrc = kn + b * p.knew_batch_stride + t * p.knew_row_stride + hk * p.knew_head_stride;
        uint16_t* kdst = kc + (int64_t)slot * p.k_batch_stride + (int64_t)row * p.k_row_stride + hk * p.k_head_stride;
        if (p.rotary_cos_sin) {
            if (c < cpr / 2) {
                if (p.dtype == VATTN_DTYPE_F16) append_rope_pair<_Float16>(p, ksrc, kdst, c, (int64_t)row);
                else append_rope_pair<__bf16>(p, ksrc, kdst, c, (int64_t)row);
            }
        } else {
            *(uint4*)(kdst + c * 8) = *(const uint4*)(ksrc + c * 8);
        }
        const uint4 vv = *(const uint4*)(vn + b * p.vnew_batch_stride + t * p.vnew_row_stride + hk * p.vnew_head_stride + c * 8);
        *(uint4*)(vc + (int64_t)slot * p.v_batch_stride + (int64_t)row * p.v_row_stride + hk * p.v_head_stride + c * 8) = vv;
    }
}

// vattn_cache_keep_rows (include/vattn_kernels.h): compaction of the accepted draft rows behind a tree-masked verify call, in place.  One
// thread per (entry, K or V, kv head, 16-byte chunk): it reads ITS chunk of the kept rows (at most 8) into registers, then stores them to
// rows row0 .. row0 + cnt - 1 — every byte is read and written by one thread only, reads before writes: no race, whatever the overlap of
// source and destination rows.  An index outside [i, n_draft) breaks the caller's contract (strictly ascending): that row is left alone.
// E: a cache element — uint16_t (vattn_cache_keep_rows), uint8_t (vattn_cache_keep_rows_fp8: e4m3 bytes, strides in bytes, 16 elements per chunk).
constexpr int KEEP_MAX = 8;
template <typename E>
__global__ void cache_keep_rows_kernel(E* k_cache, E* v_cache, int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                                       int64_t v_batch_stride, int64_t v_row_stride, int64_t v_head_stride, const int32_t* row0,
                                       const int32_t* cache_batch_idx, const int32_t* keep_idx, const int32_t* keep_cnt, int b_total, int n_draft,
                                       int h_k, int cpr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b_total * 2 * h_k * cpr) return;
    const int c = i % cpr;
    const int hk = (i / cpr) % h_k;
    const int is_v = (i / (cpr * h_k)) & 1;
    const int b = i / (cpr * h_k * 2);
    const int slot = cache_batch_idx ? cache_batch_idx[b] : b;
    const int cnt = min(max(keep_cnt[b], 0), n_draft);
    const int64_t row_stride = is_v ? v_row_stride : k_row_stride;
    E* base = is_v ? v_cache + (int64_t)slot * v_batch_stride + (int64_t)hk * v_head_stride
                          : k_cache + (int64_t)slot * k_batch_stride + (int64_t)hk * k_head_stride;
    base += (int64_t)row0[b] * row_stride + c * (int)(16 / sizeof(E));
    uint4 rows[KEEP_MAX];
    bool ok[KEEP_MAX];
#pragma unroll
    for (int j = 0; j < KEEP_MAX; j++) {
        ok[j] = false;
        if (j < cnt) {
            const int src = keep_idx[b * n_draft + j];
            ok[j] = src >= j && src < n_draft;
            if (ok[j]) rows[j] = *(const uint4*)(base + (int64_t)src * row_stride);
        }
    }
#pragma unroll
    for (int j = 0; j < KEEP_MAX; j++)
        if (ok[j]) *(uint4*)(base + (int64_t)j * row_stride) = rows[j];
}

// ---- e4m3 KV cache: the quantiser (include/vattn_kernels.h, "FP8 KV cache") ----
// One byte of the cache: y = float(x) * inv (inv = 1.0f / scale, IEEE division, once per head), clamped to +-448 by an explicit v_med3, converted
// with round-to-nearest-even; a NaN stores the NaN byte (0x7f, with the input's sign: v_med3 would return a bound for it).
__device__ __forceinline__ float fp8_clamp(float y) { return __builtin_amdgcn_fmed3f(y, -448.f, 448.f); }
// 16 source elements (two 16-byte chunks) -> one 16-byte chunk of the cache
template <typename T> __device__ __forceinline__ uint4 fp8_quant16(const T* src, const float inv) {
    using V8 = typename Tr<T>::v8;
    const V8 a = as_v8<V8>(*(const uint4*)src), b = as_v8<V8>(*(const uint4*)(src + 8));
    float y[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        y[j] = (float)a[j] * inv;
        y[8 + j] = (float)b[j] * inv;
    }
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int r = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(y[4 * i]), fp8_clamp(y[4 * i + 1]), 0, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(y[4 * i + 2]), fp8_clamp(y[4 * i + 3]), r, true);
        unsigned u = (unsigned)r;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float v = y[4 * i + e];
            if (v != v) u = (u & ~(0xffu << (8 * e))) | ((0x7fu | ((__builtin_bit_cast(unsigned, v) >> 24) & 0x80u)) << (8 * e));
        }
        w[i] = u;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
template <typename T> __device__ __forceinline__ uint8_t fp8_quant1(const T x, const float inv) {
    const float y = (float)x * inv;
    if (y != y) return (uint8_t)(0x7fu | ((__builtin_bit_cast(unsigned, y) >> 24) & 0x80u));
    return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(fp8_clamp(y), 0.f, 0, false) & 0xff);
}

// vattn_cache_flat_fp8: rows t < num_tokens of key / value [t * stride + head * hs + i] (T) -> cache bytes, one thread per 16 elements of
// a row (VEC: two 16-byte loads, ONE 16-byte store per tensor) or per element (rows that are not 16-byte aligned).  Nothing else is written.
template <typename T, bool VEC>
__global__ void cache_flat_fp8_kernel(const T* __restrict__ key, const T* __restrict__ value, uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
                                      int64_t num_tokens, int n, int hs, int64_t key_stride, int64_t value_stride, int64_t k_cache_stride,
                                      int64_t v_cache_stride, const float* __restrict__ k_scale, const float* __restrict__ v_scale) {
    constexpr int E = VEC ? 16 : 1;
    const int per_row = n / E;
    const int64_t total = num_tokens * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = i / per_row;
        const int c = (int)(i - t * per_row) * E;
        const int h = c / hs;
        const float ik = 1.0f / k_scale[h], iv = 1.0f / v_scale[h];
        if constexpr (VEC) {
            *(uint4*)(k_cache + t * k_cache_stride + c) = fp8_quant16<T>(key + t * key_stride + c, ik);
            *(uint4*)(v_cache + t * v_cache_stride + c) = fp8_quant16<T>(value + t * value_stride + c, iv);
        } else {
            k_cache[t * k_cache_stride + c] = fp8_quant1<T>(key[t * key_stride + c], ik);
            v_cache[t * v_cache_stride + c] = fp8_quant1<T>(value[t * value_stride + c], iv);
        }
    }
}

// append_kv_kernel for an e4m3 cache: k_new / v_new [b, sn, h_k, d] (T) quantised into rows cache_seqlens[b] .. of slot cache_batch_idx[b];
// cache strides are in bytes.  One thread per 16 elements; d is a multiple of 16 and every stride of the cache a multiple of 16 bytes.
template <typename T>
__global__ void append_kv_fp8_kernel(vattn_attn_params p, const float* __restrict__ k_scale, const float* __restrict__ v_scale) {
    const int b = blockIdx.y;
    const int slot = p.cache_batch_idx ? p.cache_batch_idx[b] : b;
    const int len = p.cache_seqlens ? p.cache_seqlens[b] : p.seqlen_k;
    const int cpr = p.d / 16;
    const int total = p.seqlen_knew * p.h_k * cpr;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int c = i % cpr;
        const int hk = (i / cpr) % p.h_k;
        const int t = i / (cpr * p.h_k);
        const int row = len + t;
        if (row < 0 || row >= p.seqlen_k) continue;           // never write outside the cache view
        const T* ksrc = (const T*)p.k_new + b * p.knew_batch_stride + t * p.knew_row_stride + hk * p.knew_head_stride + c * 16;
        const T* vsrc = (const T*)p.v_new + b * p.vnew_batch_stride + t * p.vnew_row_stride + hk * p.vnew_head_stride + c * 16;
        *(uint4*)((uint8_t*)p.k_cache + (int64_t)slot * p.k_batch_stride + (int64_t)row * p.k_row_stride + hk * p.k_head_stride + c * 16) = fp8_quant16<T>(ksrc, 1.0f / k_scale[hk]);
        *(uint4*)((uint8_t*)p.v_cache + (int64_t)slot * p.v_batch_stride + (int64_t)row * p.v_row_stride + hk * p.v_head_stride + c * 16) = fp8_quant16<T>(vsrc, 1.0f / v_scale[hk]);
    }
}

void launch_append_fp8(const vattn_attn_params* p, const float* k_scale, const float* v_scale, hipStream_t st) {
    const int total = p->seqlen_knew * p->h_k * (p->d / 16);
    if (total <= 0) return;
    dim3 grid((total + 255) / 256, p->b), block(256);
    if (p->dtype == VATTN_DTYPE_F16) hipLaunchKernelGGL(append_kv_fp8_kernel<_Float16>, grid, block, 0, st, *p, k_scale, v_scale);
    else hipLaunchKernelGGL(append_kv_fp8_kernel<__bf16>, grid, block, 0, st, *p, k_scale, v_scale);
}

void launch_append(const vattn_attn_params* p, hipStream_t st) {
    const int total = p->seqlen_knew * p->h_k * (p->d / 8);
    dim3 grid((total + 255) / 256, p->b), block(256);
    hipLaunchKernelGGL(append_kv_kernel, grid, block, 0, st, *p);
}

}  // namespace vattn_k

using namespace vattn_k;

extern "C" {

int vattn_cache_flat(const void* key, const void* value, void* k_cache, void* v_cache, int64_t num_tokens,
                     int32_t num_heads, int32_t head_size, int64_t key_stride, int64_t value_stride,
                     int64_t k_cache_stride, int64_t v_cache_stride, int32_t itemsize, void* stream) {
    if (num_tokens <= 0) return VATTN_K_OK;
    if (!key || !value || !k_cache || !v_cache) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)num_heads * head_size;
    const int64_t row_bytes = n * itemsize;
    const bool vec = row_bytes % 16 == 0 && (key_stride * itemsize) % 16 == 0 && (value_stride * itemsize) % 16 == 0 &&
                     (k_cache_stride * itemsize) % 16 == 0 && (v_cache_stride * itemsize) % 16 == 0 &&
                     ((((uintptr_t)key) | ((uintptr_t)value) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15) == 0;
    if (vec) {
        const int cpr = (int)(row_bytes / 16);
        const int64_t total = num_tokens * cpr;
        int64_t blocks = (total + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        const int64_t f = 16 / itemsize;
        hipLaunchKernelGGL(cache_flat_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)key, (const uint4*)value,
                           (uint4*)k_cache, (uint4*)v_cache, num_tokens, cpr, key_stride / f, value_stride / f,
                           k_cache_stride / f, v_cache_stride / f);
    } else {
        const int64_t total = num_tokens * n;
        int64_t blocks = (total + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        if (itemsize == 2)
            hipLaunchKernelGGL(cache_flat_scalar_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const uint16_t*)key,
                               (const uint16_t*)value, (uint16_t*)k_cache, (uint16_t*)v_cache, num_tokens, (int)n, key_stride,
                               value_stride, k_cache_stride, v_cache_stride);
        else if (itemsize == 4)
            hipLaunchKernelGGL(cache_flat_scalar_kernel<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t*)key,
                               (const uint32_t*)value, (uint32_t*)k_cache, (uint32_t*)v_cache, num_tokens, (int)n, key_stride,
                               value_stride, k_cache_stride, v_cache_stride);
        else
            return fail(VATTN_K_ERR_UNSUPPORTED, "cache_flat supports 2- and 4-byte element types");
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
    return VATTN_K_OK;
}

int vattn_cache_flat_fp8(const void* key, const void* value, void* k_cache, void* v_cache, int64_t num_tokens, int32_t num_heads,
                         int32_t head_size, int64_t key_stride, int64_t value_stride, int64_t k_cache_stride, int64_t v_cache_stride,
                         int32_t src_dtype, const float* k_scale, const float* v_scale, void* stream) {
    if (num_tokens <= 0) return VATTN_K_OK;
    if (!key || !value || !k_cache || !v_cache) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    if (!k_scale || !v_scale) return fail(VATTN_K_ERR_INVALID, "cache_flat_fp8 needs k_scale and v_scale (device float32[num_heads])");
    if (src_dtype != VATTN_DTYPE_F16 && src_dtype != VATTN_DTYPE_BF16) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_flat_fp8 quantises fp16 and bf16 sources");
    if (num_heads <= 0 || head_size <= 0) return fail(VATTN_K_ERR_INVALID, "cache_flat_fp8: num_heads and head_size must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)num_heads * head_size;
    const bool vec = head_size % 16 == 0 && ((key_stride | value_stride) & 7) == 0 && ((k_cache_stride | v_cache_stride) & 15) == 0 &&
                     ((((uintptr_t)key) | ((uintptr_t)value) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15) == 0;
    const int64_t total = num_tokens * (vec ? n / 16 : n);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
#define VATTN_FLAT8(TT, VV)                                                                                                                 \
    hipLaunchKernelGGL((cache_flat_fp8_kernel<TT, VV>), dim3((unsigned)blocks), dim3(256), 0, st, (const TT*)key, (const TT*)value,         \
                       (uint8_t*)k_cache, (uint8_t*)v_cache, num_tokens, (int)n, (int)head_size, key_stride, value_stride, k_cache_stride,  \
                       v_cache_stride, k_scale, v_scale)
    if (src_dtype == VATTN_DTYPE_F16) { if (vec) VATTN_FLAT8(_Float16, true); else VATTN_FLAT8(_Float16, false); }
    else { if (vec) VATTN_FLAT8(__bf16, true); else VATTN_FLAT8(__bf16, false); }
#undef VATTN_FLAT8
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
    return VATTN_K_OK;
}

int vattn_cache_keep_rows(void* k_cache, void* v_cache, int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                          int64_t v_batch_stride, int64_t v_row_stride, int64_t v_head_stride, const int32_t* row0,
                          const int32_t* cache_batch_idx, const int32_t* keep_idx, const int32_t* keep_cnt, int32_t b, int32_t n_draft,
                          int32_t h_k, int32_t d, int32_t dtype, void* stream) {
    if (!k_cache || !v_cache || !row0 || !keep_idx || !keep_cnt) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    if (b <= 0 || h_k <= 0 || n_draft <= 0) return fail(VATTN_K_ERR_INVALID, "cache_keep_rows: batch size, kv heads and n_draft must be positive");
    if (dtype != VATTN_DTYPE_F16 && dtype != VATTN_DTYPE_BF16) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows supports fp16 and bf16");
    if (n_draft > KEEP_MAX) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows handles at most 8 draft rows per entry");
    if (d != 64 && d != 128) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows supports head dimensions 64 and 128");
    if (((k_batch_stride | k_row_stride | k_head_stride | v_batch_stride | v_row_stride | v_head_stride) & 7) || ((((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15))
        return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows needs 16-byte aligned rows (strides of 8 elements)");
    const int64_t total = (int64_t)b * 2 * h_k * (d / 8);
    if (total > 0x7fffffff) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows: batch too large");
    hipLaunchKernelGGL(cache_keep_rows_kernel<uint16_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)k_cache, (uint16_t*)v_cache,
                       k_batch_stride, k_row_stride, k_head_stride, v_batch_stride, v_row_stride, v_head_stride, row0, cache_batch_idx, keep_idx,
                       keep_cnt, (int)b, (int)n_draft, (int)h_k, (int)(d / 8));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
    return VATTN_K_OK;
}

int vattn_cache_keep_rows_fp8(void* k_cache, void* v_cache, int64_t k_batch_stride, int64_t k_row_stride, int64_t k_head_stride,
                              int64_t v_batch_stride, int64_t v_row_stride, int64_t v_head_stride, const int32_t* row0,
                              const int32_t* cache_batch_idx, const int32_t* keep_idx, const int32_t* keep_cnt, int32_t b, int32_t n_draft,
                              int32_t h_k, int32_t d, void* stream) {
    if (!k_cache || !v_cache || !row0 || !keep_idx || !keep_cnt) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    if (b <= 0 || h_k <= 0 || n_draft <= 0) return fail(VATTN_K_ERR_INVALID, "cache_keep_rows_fp8: batch size, kv heads and n_draft must be positive");
    if (n_draft > KEEP_MAX) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows_fp8 handles at most 8 draft rows per entry");
    if (d != 64 && d != 128) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows_fp8 supports head dimensions 64 and 128");
    if (((k_batch_stride | k_row_stride | k_head_stride | v_batch_stride | v_row_stride | v_head_stride) & 15) || ((((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15))
        return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows_fp8 needs 16-byte aligned rows (strides of 16 bytes)");
    const int64_t total = (int64_t)b * 2 * h_k * (d / 16);
    if (total > 0x7fffffff) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_keep_rows_fp8: batch too large");
    hipLaunchKernelGGL(cache_keep_rows_kernel<uint8_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint8_t*)k_cache, (uint8_t*)v_cache,
                       k_batch_stride, k_row_stride, k_head_stride, v_batch_stride, v_row_stride, v_head_stride, row0, cache_batch_idx, keep_idx,
                       keep_cnt, (int)b, (int)n_draft, (int)h_k, (int)(d / 16));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
    return VATTN_K_OK;
}

int vattn_cache_flat_rope(const void* key, const void* value, void* k_cache, void* v_cache, int64_t num_tokens, int32_t num_heads,
                          int32_t head_size, int64_t key_stride, int64_t value_stride, int64_t k_cache_stride, int64_t v_cache_stride,
                          int32_t dtype, const void* cos_sin, int64_t cos_sin_row_stride, int64_t pos0, void* stream) {
    if (num_tokens <= 0) return VATTN_K_OK;
    if (!key || !value || !k_cache || !v_cache || !cos_sin) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    if (dtype != VATTN_DTYPE_F16 && dtype != VATTN_DTYPE_BF16) return fail(VATTN_K_ERR_UNSUPPORTED, "cache_flat_rope supports fp16 and bf16");
    if (head_size % 16 != 0 || ((key_stride | value_stride | k_cache_stride | v_cache_stride | cos_sin_row_stride) & 7) ||
        ((((uintptr_t)key) | ((uintptr_t)value) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache) | ((uintptr_t)cos_sin)) & 15))
        return fail(VATTN_K_ERR_UNSUPPORTED, "cache_flat_rope needs 16-byte aligned rows (head_size a multiple of 16, strides of 8 elements)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = num_tokens * num_heads * (head_size / 16);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (dtype == VATTN_DTYPE_F16)
        hipLaunchKernelGGL(cache_flat_rope_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, st, (const _Float16*)key, (const _Float16*)value,
                           (_Float16*)k_cache, (_Float16*)v_cache, num_tokens, num_heads, head_size, key_stride, value_stride, k_cache_stride,
                           v_cache_stride, (const _Float16*)cos_sin, cos_sin_row_stride, pos0);
    else
        hipLaunchKernelGGL(cache_flat_rope_kernel<__bf16>, dim3((unsigned)blocks), dim3(256), 0, st, (const __bf16*)key, (const __bf16*)value,
                           (__bf16*)k_cache, (__bf16*)v_cache, num_tokens, num_heads, head_size, key_stride, value_stride, k_cache_stride,
                           v_cache_stride, (const __bf16*)cos_sin, cos_sin_row_stride, pos0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
    return VATTN_K_OK;
}

int vattn_rotary_embedding(const int64_t* positions, void* query, void* key, int64_t num_tokens, int32_t num_q_heads, int32_t num_kv_heads,
                           int32_t head_size, int64_t query_stride, int64_t key_stride, int32_t dtype, const void* cos_sin,
                           int64_t cos_sin_row_stride, int32_t rot_dim, int32_t is_neox, void* stream) {
    if (num_tokens <= 0) return VATTN_K_OK;
    if (!positions || !query || !key || !cos_sin) return fail(VATTN_K_ERR_INVALID, "null tensor pointer");
    if (dtype != VATTN_DTYPE_F16 && dtype != VATTN_DTYPE_BF16) return fail(VATTN_K_ERR_UNSUPPORTED, "rotary_embedding supports fp16 and bf16");
    if (rot_dim <= 0 || rot_dim > head_size || (rot_dim & 1)) return fail(VATTN_K_ERR_INVALID, "bad rotary dimension");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = num_tokens * (int64_t)(num_q_heads + num_kv_heads) * (rot_dim / 2);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
#define VATTN_ROT(TT, NX)                                                                                                                   \
    hipLaunchKernelGGL((rotary_embedding_kernel<TT, NX>), dim3((unsigned)blocks), dim3(256), 0, st, positions, (TT*)query, (TT*)key,        \
                       (const TT*)cos_sin, cos_sin_row_stride, rot_dim, query_stride, key_stride, num_q_heads, num_kv_heads, head_size, num_tokens)
    if (dtype == VATTN_DTYPE_F16) { if (is_neox) VATTN_ROT(_Float16, true); else VATTN_ROT(_Float16, false); }
    else { if (is_neox) VATTN_ROT(__bf16, true); else VATTN_ROT(__bf16, false); }
#undef VATTN_ROT
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VATTN_K_ERR_LAUNCH, hipGetErrorString(e));
    return VATTN_K_OK;
}

}  // extern "C"
