// kmer_dev.hpp -- what the k-mer pipelines on the device share (dbgen.hip: the database builder; kcov.hip: the per-group k-mer coverage;
// dbexport.hip: the export of a loaded database, which uses the wave helpers and the host part).
//   device: the wave helpers and the two phases of the text scan -- a wave's 1024 bytes packed into LDS (pack_span), the canonical
//           k-mer of the window that ends at one byte of them (window_kmer) -- and the record of a text position (span_records / record_at);
//   host:   with_temp (rocPRIM's two calls) and LapTimer (HIP-event time per stage); DevBuf and ensure_all come from devbuf.hpp.
// Included by HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "devbuf.hpp"

namespace lmat_dev {

typedef unsigned long long u64;
typedef uint32_t u32;

constexpr int kSpan = 992;        // window ends one wave covers: 62 blocks of 16 bases, behind 2 blocks (32 bases >= k - 1) of lead-in
constexpr int kLead = 32;         // bytes of text in front of a chunk (the k - 1 overlap, rounded up to the 16-byte loads)
constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ u32 lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// the memory of the wave's own LDS / global writes made visible to its other lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <class T, class Op> __device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, (T)__shfl_xor(v, d));
    return v;
}
template <class T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T x, T y) { return x + y; }); }
template <class T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T x, T y) { return x > y ? x : y; }); }

// reverse complement of a k-mer held in the low 2k bits (Encoder::rc): 2-bit groups reversed, complemented
__device__ __forceinline__ u64 revcomp(u64 x, int k) {
    u64 r = __brevll(x);
    r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
    return (~r) >> (64 - 2 * k);
}

// Phase 1 of the text scan, by one wave: lane l packs the 16 bases at p + 16 l (p: the wave's 1024-byte window, 16-byte aligned or not --
// the load is one uint4) into one 32-bit word (first base in the high bits) and a mask of its invalid bytes; an inclusive max-scan over
// the lanes gives, per block, the last invalid byte at or before its end.  The three arrays are the wave's own 64 LDS words each; the
// caller puts a wave_sync() between this and window_kmer.
__device__ __forceinline__ void pack_span(const uint8_t* p, u32 lane, u32* s_word, u32* s_inv, int* s_last) {
    const uint4 q = *reinterpret_cast<const uint4*>(p + 16 * lane);
    const u32 w4[4] = {q.x, q.y, q.z, q.w};
    u32 word = 0, inv = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const u32 c = (w4[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        const u32 up = (c & 0xDFu) - 0x41u;                              // 'A' -> 0, 'C' -> 2, 'G' -> 6, 'T' -> 19
        const bool ok = up < 20u && ((0x80045u >> up) & 1u);
        const u32 code = ((c >> 1) ^ (c >> 2)) & 3u;                     // A 0, C 1, G 2, T 3
        word |= code << (30 - 2 * j);
        inv |= (ok ? 0u : 1u) << j;
    }
    int last = inv ? (int)(16 * lane) + 31 - __clz((int)inv) : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(last, d);
        if ((int)lane >= d) last = max(last, o);
    }
    s_word[lane] = word;
    s_inv[lane] = inv;
    s_last[lane] = last;
}

// Phase 2, by one lane: the window of k bases that ends at byte t (kLead <= t < 1024) of the wave's window.  The run of valid bases that
// ends there is the distance to the last invalid byte (the scan's value of the block before + the own block's mask); the k-mer is 2k bits
// cut from three packed words (48 bases: enough for k <= 32 at any place in the block).  False: no k valid bases end at t.
__device__ __forceinline__ bool window_kmer(const u32* s_word, const u32* s_inv, const int* s_last, u32 t, int k, u64 kmask, u64& canon) {
    const u32 bt = t >> 4, in = t & 15u;
    const u32 m = s_inv[bt] & ((2u << in) - 1u);
    const int last = m ? (int)(16 * bt) + 31 - __clz((int)m) : s_last[bt - 1];
    if ((int)t - last < k) return false;
    const u64 lo = ((u64)s_word[bt - 1] << 32) | s_word[bt];
    const unsigned __int128 x = ((unsigned __int128)s_word[bt - 2] << 64) | lo;
    const u64 fwd = (u64)(x >> (2 * (15 - in))) & kmask;
    const u64 rc = revcomp(fwd, k);
    canon = fwd < rc ? fwd : rc;
    return true;
}

// the records [rlo, rhi) that text positions p0 .. p1 can lie in: rec_start ascends, a record reaches to the start of the next
__device__ __forceinline__ void span_records(const u64* rec_start, u32 n_rec, u64 p0, u64 p1, u32& rlo, u32& rhi) {
    u32 lo = 0, hi = n_rec;
    while (lo < hi) { const u32 m = (lo + hi) >> 1; if (rec_start[m] <= p0) lo = m + 1; else hi = m; }
    rlo = lo ? lo - 1 : 0;
    hi = n_rec;
    while (lo < hi) { const u32 m = (lo + hi) >> 1; if (rec_start[m] <= p1) lo = m + 1; else hi = m; }
    rhi = lo;
}

// the last record of [lo, hi) that starts at or before pos
__device__ __forceinline__ u32 record_at(const u64* rec_start, u32 lo, u32 hi, u64 pos) {
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (rec_start[mid] <= pos) lo = mid; else hi = mid; }
    return lo;
}

// ------------------------------------------------------------------------------------------------------------------ host
// rocPRIM's two calls: without storage it reports the bytes it needs, with them it runs.  call(void* storage, size_t& bytes)
template <class Call> hipError_t with_temp(DevBuf& temp, Call call) {
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess) e = temp.ensure(bytes);
    if (e == hipSuccess) e = call(temp.p, bytes);
    return e;
}

// HIP-event time on the stream, stage by stage: lap() adds the ms since start() or the lap before it
struct LapTimer {
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~LapTimer() { if (ev[0]) hipEventDestroy(ev[0]); if (ev[1]) hipEventDestroy(ev[1]); }
    hipError_t init(hipStream_t s) {
        st = s;
        const hipError_t e = hipEventCreate(&ev[0]);
        return e == hipSuccess ? hipEventCreate(&ev[1]) : e;
    }
    hipError_t start() { return hipEventRecord(ev[0], st); }
    hipError_t lap(float& acc) {
        hipError_t e = hipEventRecord(ev[1], st);
        if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
        acc += ms;
        if (e == hipSuccess) e = hipEventRecord(ev[0], st);
        return e;
    }
};

}  // namespace lmat_dev
