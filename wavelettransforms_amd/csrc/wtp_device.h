/*
 * wtp_device.h -- device primitives shared by the selection, resident, pruning and level
 * kernels: coherent loads and stores, buffer resources, DPP wave scans and reductions, the
 * chunk loads and ragged stores, and the lab probe macros (empty in the library).
 * Built with -ffp-contract=off: the float32 operation order IS the parity contract.
 */
#ifndef WTP_DEVICE_H
#define WTP_DEVICE_H
#include "wtp_internal.h"

#pragma clang fp contract(off)

namespace wtp {

/* ---------------------------------------------------------------- helpers --- */
__device__ __forceinline__ uint32_t abs_key(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }

/* Loads and stores of bytes handed between workgroups of ONE launch (k_resident): agent-scope
 * relaxed atomics lower to global_load/store ... sc1, which bypass the CU's L1 and write
 * through the XCD's L2 (MI355X_MICROARCH.md, inter-workgroup visibility: sc1 stores + sc1 loads
 * + an agent-scope arrival counter, one workgroup per CU).  COH = false: plain accesses (the
 * data was produced by an earlier launch). */
template <bool COH, class T>
__device__ __forceinline__ T ldc(const T* p) {
    if constexpr (COH) return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <class T>
__device__ __forceinline__ void stc(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
/* a 16-byte write-through (sc1) vector store: MI355X_MICROARCH.md's hand-off form for tens of KB
 * per workgroup (drained by the storer's vmcnt(0) before its arrival, read with sc1 loads).  A
 * buffer store through the builtin (cache policy 16 = sc1), not inline asm: the compiler then
 * knows the store reads its data VGPRs late and keeps the wait state before they are rewritten
 * (an inline-asm dwordx4 store had its data registers overwritten by the next VALU op). */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t region_rsrc(const uint32_t* p, int words) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, words * 4, 0x00020000);
}
__device__ __forceinline__ void st16_sc1(__amdgpu_buffer_rsrc_t r, int word, uint4 v) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    const u4v x = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(x, r, 4 * word, 0, 16);
}

__device__ __forceinline__ int find_seg(const SegTable& t, int b) {
    int s = 0; /* blk_begin[0] == 0; entries past nseg hold INT32_MAX */
#pragma unroll
    for (int i = 1; i < SEG_PER_LAUNCH; ++i) s += b >= t.blk_begin[i];
    return s;
}

/* Cross-lane primitives on DPP (GFX9 wave64: row_shr inside rows of 16 lanes, row_bcast:15/31
 * across rows): a few VALU cycles per step, where __shfl (ds_bpermute) pays an LDS round trip
 * per step.  Every lane of the wave must be active. */
template <int CTRL, int ROWM = 0xf, int BANKM = 0xf>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWM, BANKM, false);
}

/* inclusive prefix sum across the 64 lanes */
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v) {
    v += dpp_u32<0x111>(v); /* row_shr:1 */
    v += dpp_u32<0x112>(v); /* row_shr:2 */
    v += dpp_u32<0x114>(v); /* row_shr:4 */
    v += dpp_u32<0x118>(v); /* row_shr:8 */
    v += dpp_u32<0x142, 0xa>(v); /* row_bcast:15 into rows 1, 3 */
    v += dpp_u32<0x143, 0xc>(v); /* row_bcast:31 into rows 2, 3 */
    return v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_u32(v), 63);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, dpp_u32<0x111>(v));
    v = max(v, dpp_u32<0x112>(v));
    v = max(v, dpp_u32<0x114>(v));
    v = max(v, dpp_u32<0x118>(v));
    v = max(v, dpp_u32<0x142, 0xa>(v));
    v = max(v, dpp_u32<0x143, 0xc>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

/* wave-wide reduction where a lane without a DPP source keeps its own value (old = v): min needs
 * it, the zero a dpp_u32 step reads there would win.  The result is read from lane 63. */
template <int CTRL, int ROWM = 0xf, int BANKM = 0xf>
__device__ __forceinline__ uint32_t dpp_keep_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWM, BANKM, false);
}
template <class Op>
__device__ __forceinline__ uint32_t wave_red_u32(uint32_t v, const Op& op) {
    v = op(v, dpp_keep_u32<0x111>(v));
    v = op(v, dpp_keep_u32<0x112>(v));
    v = op(v, dpp_keep_u32<0x114>(v));
    v = op(v, dpp_keep_u32<0x118>(v));
    v = op(v, dpp_keep_u32<0x142, 0xa>(v));
    v = op(v, dpp_keep_u32<0x143, 0xc>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return wave_red_u32(v, [](uint32_t a, uint32_t b) { return a < b ? a : b; }); }
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v) { return wave_red_u32(v, [](uint32_t a, uint32_t b) { return a | b; }); }

/* exact 64-bit sum (three 32-bit reductions of 16/16/32-bit fields) */
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    const uint32_t lo = wave_sum_u32((uint32_t)v & 0xFFFFu);
    const uint32_t mid = wave_sum_u32((uint32_t)(v >> 16) & 0xFFFFu);
    const uint32_t hi = wave_sum_u32((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) + ((unsigned long long)mid << 16) + lo;
}

/* block sum of an unsigned 64-bit value; result valid in thread 0 */
template <int THREADS>
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v) {
    __shared__ unsigned long long ws[THREADS / 64];
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < THREADS / 64; ++i) t += ws[i];
    return t;
}

/* IT float4 per thread of one chunk (fully populated, 16-byte aligned).  NT: nontemporal loads
 * (the `nt` policy bit) -- k_resident's once-read chunk: measured neutral with warm caches and 7 us
 * shorter behind a 512 MiB write to another buffer (its reads then no longer evict that buffer's
 * dirty Infinity-Cache lines) */
template <int IT, int CT = STREAM_THREADS, bool NT = false>
__device__ __forceinline__ void load_chunk(const float* p, float4 (&v)[IT]) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    typedef float f4v __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        if (NT) {
            const f4v t = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p4 + it * CT + threadIdx.x));
            v[it] = make_float4(t.x, t.y, t.z, t.w);
        } else {
            v[it] = p4[it * CT + threadIdx.x];
        }
    }
}

/* A ragged or unaligned chunk of len elements: element e of slot (it, c) is
 * 4 * (it * STREAM_THREADS + tid) + c, as in load_chunk.  Range-checked buffer loads: every
 * load is issued unconditionally (no per-load branch and wait) and reads 0 past len. */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ragged_rsrc(const float* p, int len) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    void* base = reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, __builtin_amdgcn_readfirstlane(len * 4), 0x00020000);
}
template <int IT, int CT = STREAM_THREADS, bool NT = false>
__device__ __forceinline__ void load_chunk_ragged(const float* p, int len, float4 (&v)[IT]) {
    const __amdgpu_buffer_rsrc_t r = ragged_rsrc(p, len);
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (len & 3) == 0) { /* uniform */
        /* every float4 lies wholly inside or wholly past len: one 16-byte range-checked load
         * each (past len it reads as zeros) instead of four dword loads */
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const u4 q = __builtin_amdgcn_raw_buffer_load_b128(r, 16 * (it * CT + (int)threadIdx.x), 0, NT ? 2 : 0);
            v[it] = make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
        }
        return;
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int e = 4 * (it * CT + (int)threadIdx.x);
        v[it].x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * e, 0, NT ? 2 : 0));
        v[it].y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * e + 4, 0, NT ? 2 : 0));
        v[it].z = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * e + 8, 0, NT ? 2 : 0));
        v[it].w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * e + 12, 0, NT ? 2 : 0));
    }
}
/* range-checked float4 store: the dwords past the buffer's length are dropped */
__device__ __forceinline__ void store4_ragged(const float4& y, __amdgpu_buffer_rsrc_t r, int off) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y.x), r, off, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y.y), r, off + 4, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y.z), r, off + 8, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y.w), r, off + 12, 0, 0);
}
/* a copy the compiler cannot see through: keys derived from it are recomputed where needed
 * instead of being kept live beside the data (k_resident holds 96 floats per thread) */
__device__ __forceinline__ float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}
/* float4 slot j of a partial chunk of len elements: whole float4 stores where the slot is
 * complete and the buffer 16-byte aligned, range-checked dword stores otherwise */
__device__ __forceinline__ void store4_tail(const float4& y, float* q, __amdgpu_buffer_rsrc_t r, int j, int len,
                                            bool aligned) {
    if (aligned && 4 * j + 3 < len) reinterpret_cast<float4*>(q)[j] = y;
    else if (4 * j < len) store4_ragged(y, r, 16 * j);
}
__device__ __forceinline__ float f4_get(const float4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

__device__ __forceinline__ uint64_t wall_ticks() { return __builtin_amdgcn_s_memrealtime(); }

/* --------------------------------------------------------- radix select --- */
/* Find the digit (8 bits) holding rank r in a 256-bin LDS histogram; one wave. */
__device__ __forceinline__ void wave_pick_digit(const uint32_t* hb, int64_t r, int* digit, int64_t* below) {
    const int lane = threadIdx.x & 63;
    const uint32_t c0 = hb[4 * lane], c1 = hb[4 * lane + 1], c2 = hb[4 * lane + 2], c3 = hb[4 * lane + 3];
    const uint32_t s = c0 + c1 + c2 + c3; /* histograms count < 2^32 keys */
    const int64_t incl = wave_scan_u32(s);
    int64_t cum = incl - s;
    if (r >= cum && r < incl) {
        int d = 4 * lane;
        if (r >= cum + c0) { cum += c0; ++d;
            if (r >= cum + c1) { cum += c1; ++d;
                if (r >= cum + c2) { cum += c2; ++d; } } }
        *digit = d;
        *below = cum;
    }
}

/* timing probes for tools/mb/lab.hip (empty in the library) */
#ifndef WTP_PROBE
#define WTP_PROBE(i)
#endif
#ifndef WTP_PROBE_T /* a probe taken by thread t */
#define WTP_PROBE_T(i, t)
#endif
#ifndef WTP_CPROBE
#define WTP_CPROBE(i)
#endif
#ifndef WTP_RPROBE
#define WTP_RPROBE(i)
#endif
#ifndef WTP_WPROBE
#define WTP_WPROBE(i)
#endif
#ifndef WTP_RTAG /* k_resident: the workgroup's segment flags, for the phase lab */
#define WTP_RTAG(tagv)
#endif
#ifndef WTP_GPROBE /* a probe taken by lane 0 of the executing wave */
#define WTP_GPROBE(i)
#endif

}  // namespace wtp
#endif
