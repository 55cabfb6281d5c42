// kcov.hip -- per-group k-mer coverage of a set of reads on the GPU (the lmat_cov_* family of include/lmat_hip.h).
//
// Replaces the counting of the reference's content_summ (src/content_summ.cpp:113-152 and :538-571): for every read the distinct
// canonical k-mers, for several k at once, counted once per read in a std::set and per called taxid in a map of maps; the report wants,
// per taxid and k, the number of distinct k-mers, the sum of their multiplicities and the histogram multiplicity -> number of k-mers.
// Here a "group" is whatever 32-bit id the caller counts a read under.  Per k and per prefix pass, all on the context's stream:
//   cov_extract_kernel<count>   per wave the number of windows whose canonical k-mer has the pass's prefix; exclusive scan
//   cov_extract_kernel<emit>    (key, read index) per window occurrence, in text order -- no atomic cursor, every wave knows its place
//   rocPRIM radix sort, stable, by (group, k-mer): one packed key, or (k-mer), gather, (group) when both do not fit 64 bits
//   cov_flag / scan / cov_scatter   runs of one (group, k-mer); inside a run the read indices ascend (text order + stable sort), so the
//                               multiplicity is the number of positions whose read index differs from the one before
//   cov_hkey, radix sort, run-length encode    (group, multiplicity, number of k-mers) triples in report order, copied to the host
// Every reported quantity is additive over disjoint k-mer sets: the host adds the triples of the passes.
// The text scan (pack_span, window_kmer), the record lookup, DevBuf, with_temp and LapTimer are kmer_dev.hpp's, shared with dbgen.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <rocprim/rocprim.hpp>
#include <string>
#include <vector>
#include "lmat_internal.hpp"
#include "kmer_dev.hpp"

namespace {

using namespace lmat_dev;

constexpr int kMaxPrefixBits = 24;
constexpr u64 kMaxWindows = 0x7FFFFF00ull;   // occurrences of one pass: 31-bit positions in the packed flags

enum { V_WINDOWS = 0, V_N };   // counters (device, 64-bit words)

struct CovExtractArgs {
    const uint8_t* buf;      // chunk bytes: buf[kLead + i] = text[chunk_lo + i]; every wave's 1024-byte window is allocated and filled
    u64 chunk_lo;            // text position of buf[kLead]
    u32 chunk_len;           // window ends of this chunk: text[chunk_lo .. chunk_lo + chunk_len)
    const u64* rec_start;    // [n_rec] text position of the first base of every read, ascending
    const u32* rec_dgroup;   // [n_rec] dense group index
    u32 n_rec;
    int k, prefix_bits;      // the top prefix_bits (<= 2k) of the canonical k-mer select the pass
    int key_bits;            // 2k - prefix_bits: what is left of the k-mer in the key
    int packed;              // key = dense group << key_bits | k-mer; else key = k-mer alone
    int count_windows;       // count pass: add the valid windows, of any prefix, to counters[V_WINDOWS]
    u32 pass;
    u64* wave_cnt;           // count pass: [first_wave + wave] occurrences of the pass
    const u64* wave_off;     // emit pass: their exclusive scan = where the wave's first occurrence goes
    u64 first_wave;          // of the chunk, in the numbering over the whole text
    u64* keys;
    u32* vals;               // read index of the occurrence
    u64* counters;
};

// Every wave covers kSpan consecutive window ends, as dbgen.hip's extract_kernel does.  The count pass and the emit pass take the same
// decisions, so the emit pass writes exactly wave_cnt occurrences from wave_off on, lanes and steps in text order.
template <bool EMIT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void cov_extract_kernel(CovExtractArgs a) {
    __shared__ u32 s_word[kWavesPerBlock][64];
    __shared__ int s_last[kWavesPerBlock][64];
    __shared__ u32 s_inv[kWavesPerBlock][64];
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u64 wave = (u64)blockIdx.x * kWavesPerBlock + wv;
    const u64 wbase = wave * kSpan;               // first window end of the wave, relative to the chunk
    if (wbase >= a.chunk_len) return;             // whole waves only: no block-wide barrier below
    pack_span(a.buf + wbase, lane, s_word[wv], s_inv[wv], s_last[wv]);
    wave_sync();
    const int k = a.k;
    const u64 kmask = (1ull << (2 * k)) - 1;      // k <= 31
    const u64 lowmask = (1ull << a.key_bits) - 1; // key_bits <= 62
    u32 rlo = 0, rhi = 0;
    if (EMIT) span_records(a.rec_start, a.n_rec, a.chunk_lo + wbase, a.chunk_lo + wbase + kSpan - 1, rlo, rhi);
    u64 at = EMIT ? a.wave_off[a.first_wave + wave] : 0;
    u64 n_windows = 0;
    for (int step = 0; step * 64 < kSpan; ++step) {
        const u32 q = step * 64 + lane;            // window end within the span
        const u32 t = q + kLead;                   // ... as a byte of the wave's window
        bool emit = false;
        u64 canon = 0;
        if (q < (u32)kSpan && wbase + q < a.chunk_len) {
            if (window_kmer(s_word[wv], s_inv[wv], s_last[wv], t, k, kmask, canon)) {
                emit = a.prefix_bits == 0 || (u32)(canon >> a.key_bits) == a.pass;
                n_windows += 1;
            }
        }
        const u64 bal = __ballot(emit);
        if (EMIT && emit) {
            const u32 rd = record_at(a.rec_start, rlo, rhi, a.chunk_lo + wbase + q);
            const u64 dst = at + __popcll(bal & ((1ull << lane) - 1));
            const u64 low = canon & lowmask;
            a.keys[dst] = a.packed ? (((u64)a.rec_dgroup[rd] << a.key_bits) | low) : low;
            a.vals[dst] = rd;
        }
        at += __popcll(bal);
    }
    if (!EMIT) {
        if (lane == 0) a.wave_cnt[a.first_wave + wave] = at;
        if (a.count_windows) {
            n_windows = wave_sum(n_windows);
            if (lane == 0 && n_windows) atomicAdd(&a.counters[V_WINDOWS], n_windows);
        }
    }
}

// two-sort form, between the sorts: the group of every occurrence as the next key, its place as the value
__global__ __launch_bounds__(256) void cov_gather_kernel(const u32* reads, const u32* rec_dgroup, u32 n, u32* gkey, u32* idx) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { gkey[i] = rec_dgroup[reads[i]]; idx[i] = i; }
}

struct CovSorted {   // the sorted occurrences, either form
    const u64* keys;
    const u32* reads;
    const u32* gkey;     // two-sort form: sorted groups and the place of each in keys / reads
    const u32* idx;
    int key_bits, packed;
    __device__ __forceinline__ void get(u32 i, u32& g, u64& km, u32& rd) const {
        if (packed) {
            const u64 x = keys[i];
            g = key_bits ? (u32)(x >> key_bits) : (u32)x;   // key_bits == 0: the key is the group alone
            km = key_bits ? x & ((1ull << key_bits) - 1) : 0;
            rd = reads[i];
        } else {
            const u32 j = idx[i];
            g = gkey[i];
            km = keys[j];
            rd = reads[j];
        }
    }
};

// flag[i] = (head of a run of one (group, k-mer)) << 32 | (first occurrence of a read in its run)
__global__ __launch_bounds__(256) void cov_flag_kernel(CovSorted s, u32 n, u64* flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 g, rd, pg = 0, prd = 0;
    u64 km, pkm = 0;
    s.get(i, g, km, rd);
    if (i) s.get(i - 1, pg, pkm, prd);
    const bool head = i == 0 || g != pg || km != pkm;
    const bool fresh = head || rd != prd;
    flag[i] = ((u64)head << 32) | (u64)fresh;
}

// pos = exclusive scan of flag: run r starts where the low half counted run_first[r] reads-in-runs; run_first[R] = their total
__global__ __launch_bounds__(256) void cov_scatter_kernel(CovSorted s, u32 n, const u64* flag, const u64* pos, u32* run_first, u32* run_group, u64* totals) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 f = flag[i], p = pos[i];
    const u32 r = (u32)(p >> 32);
    if (f >> 32) {
        u32 g, rd;
        u64 km;
        s.get(i, g, km, rd);
        run_first[r] = (u32)p;
        run_group[r] = g;
    }
    if (i == n - 1) {
        const u32 R = r + (u32)(f >> 32);
        run_first[R] = (u32)p + (u32)(f & 1ull);
        totals[0] = R;
    }
}

// one key per run: dense group << 32 | multiplicity
__global__ __launch_bounds__(256) void cov_hkey_kernel(const u32* run_first, const u32* run_group, u32 R, u64* hkey) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) hkey[r] = ((u64)run_group[r] << 32) | (u64)(run_first[r + 1] - run_first[r]);
}

}  // namespace

struct lmat_cov {
    lmat_ctx* ctx = nullptr;
    std::vector<int> ks;
    std::string err;
    // input
    std::vector<uint8_t> text;          // reads, one '\n' behind each
    std::vector<u64> rec_start;
    std::vector<u32> rec_group;
    u64 bases = 0;
    // options
    u64 budget = 0;
    int prefix_bits = -1;
    // result
    bool done = false;
    struct Rep {
        u64 distinct = 0, total = 0;
        std::map<u64, u64> hist;         // multiplicity -> number of k-mers
    };
    std::vector<std::map<u32, Rep>> rep; // [k index][group]
    lmat_cov_stats stats;
};

namespace {

int cov_err(lmat_cov* c, int code, const std::string& msg) {
    c->err = msg;
    return code;
}

#define CHIP(c, call)                                                                            \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) return cov_err(c, e__ == hipErrorOutOfMemory ? LMAT_E_NOMEM : LMAT_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// One run: the dense group numbering, the memory model and the device buffers of the passes.
// Bytes per window occurrence of a pass: key and read index twice for the sort (24), flag and scan (16), run start and run group (8) = 48;
// the two-sort form adds group key and place twice (16); rocPRIM's own scratch is reckoned at 16.  The histogram's keys, their sorted copy,
// the run-length output and its counts reuse flag, scan, the first key buffer and the first read-index buffer.
struct CovRun {
    lmat_cov* c = nullptr;
    hipStream_t st = nullptr;
    u64 T = 0;
    u32 n_rec = 0;
    std::vector<u32> groups;             // dense index -> group id, ascending
    std::vector<u32> rec_dgroup;
    int gb = 0;                          // bits of a dense group index
    u64 budget = 0, fixed = 0;
    u64 chunk = 0, chunk_waves = 0, chunk_alloc = 0, n_chunks = 0, n_waves = 0;
    bool resident = false, uploaded = false;   // the whole text is one chunk and stays on the device
    DevBuf text, rec_start, d_dgroup, wave_cnt, wave_off, counters, totals, keysA, keysB, valsA, valsB, gkeyA, gkeyB, idxA, idxB, flag, pos, run_first,
        run_group, temp;
    uint8_t* stage = nullptr;            // pinned: one chunk of text on its way up
    LapTimer timer;
    ~CovRun() { if (stage) hipHostFree(stage); }

    static u64 per_window(bool packed) { return packed ? 64 : 80; }

    int plan() {
        groups = c->rec_group;
        std::sort(groups.begin(), groups.end());
        groups.erase(std::unique(groups.begin(), groups.end()), groups.end());
        rec_dgroup.resize(n_rec);
        for (u32 r = 0; r < n_rec; ++r) rec_dgroup[r] = (u32)(std::lower_bound(groups.begin(), groups.end(), c->rec_group[r]) - groups.begin());
        while ((1ull << gb) < groups.size()) ++gb;
        budget = c->budget;
        if (!budget) {
            size_t fr = 0, tot = 0;
            CHIP(c, hipMemGetInfo(&fr, &tot));
            budget = fr / 2;
        }
        // the text goes up in chunks of 1/64 of the budget (a window occurrence takes 64 bytes or more), 64 KiB .. 1 GiB; a text of one chunk stays
        chunk = std::min<u64>(T, std::min<u64>(std::max<u64>(budget / 64, 1u << 16), 1u << 30));
        resident = chunk == T;
        chunk_waves = (chunk + kSpan - 1) / kSpan;
        chunk_alloc = chunk_waves * kSpan + kLead + 64;
        n_chunks = (T + chunk - 1) / chunk;
        n_waves = n_chunks * chunk_waves;
        fixed = chunk_alloc + (u64)n_rec * 12 + (n_waves + 1) * 16 + (64u << 10);
        if (budget <= fixed + per_window(false) * 64)
            return cov_err(c, LMAT_E_CAPACITY, "device budget of " + std::to_string(budget) + " bytes is below the " + std::to_string(fixed) + " bytes of the fixed buffers");
        return LMAT_OK;
    }

    bool packed(int k) const { return gb + 2 * k <= 64; }
    u64 cap(int k) const { return std::min<u64>(std::min<u64>((budget - fixed) / per_window(packed(k)), kMaxWindows), T); }

    int alloc() {
        CHIP(c, ensure_all({{&text, chunk_alloc}, {&rec_start, (size_t)n_rec * 8}, {&d_dgroup, (size_t)n_rec * 4}, {&wave_cnt, (n_waves + 1) * 8},
                            {&wave_off, (n_waves + 1) * 8}, {&counters, V_N * 8}, {&totals, 32}}));
        CHIP(c, hipMemcpyAsync(rec_start.p, c->rec_start.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
        CHIP(c, hipMemcpyAsync(d_dgroup.p, rec_dgroup.data(), (size_t)n_rec * 4, hipMemcpyHostToDevice, st));
        CHIP(c, hipMemsetAsync(counters.p, 0, V_N * 8, st));
        CHIP(c, hipStreamSynchronize(st));
        CHIP(c, hipHostMalloc((void**)&stage, chunk_alloc));
        CHIP(c, timer.init(st));
        return LMAT_OK;
    }

    // chunk ci of the text on the device, kLead bytes of the text before it in front; 'N' where there is no text
    int upload(u64 ci, u32& len) {
        const u64 lo = ci * chunk;
        len = (u32)std::min<u64>(chunk, T - lo);
        if (resident && uploaded) return LMAT_OK;
        const u64 waves = ((u64)len + kSpan - 1) / kSpan;
        const u64 bytes = waves * kSpan + kLead;
        const u64 lead = std::min<u64>(lo, kLead);
        memset(stage, 'N', kLead - lead);
        memcpy(stage + kLead - lead, c->text.data() + lo - lead, lead);
        const u64 avail = std::min<u64>(T - lo, bytes - kLead);   // bases behind the chunk's end are read but never end a window of it
        memcpy(stage + kLead, c->text.data() + lo, avail);
        memset(stage + kLead + avail, 'N', bytes - kLead - avail);
        CHIP(c, hipMemcpyAsync(text.p, stage, bytes, hipMemcpyHostToDevice, st));
        CHIP(c, hipStreamSynchronize(st));   // the staging buffer is refilled next
        uploaded = true;
        return LMAT_OK;
    }

    // one pass over the text, count or emit
    template <bool EMIT> int scan_text(int k, int pe, u32 pass, bool count_windows) {
        for (u64 ci = 0; ci < n_chunks; ++ci) {
            u32 len = 0;
            if (const int rc = upload(ci, len)) return rc;
            CovExtractArgs a;
            a.buf = text.as<uint8_t>();
            a.chunk_lo = ci * chunk;
            a.chunk_len = len;
            a.rec_start = rec_start.as<u64>();
            a.rec_dgroup = d_dgroup.as<u32>();
            a.n_rec = n_rec;
            a.k = k;
            a.prefix_bits = pe;
            a.key_bits = 2 * k - pe;
            a.packed = packed(k) ? 1 : 0;
            a.count_windows = count_windows ? 1 : 0;
            a.pass = pass;
            a.wave_cnt = wave_cnt.as<u64>();
            a.wave_off = wave_off.as<u64>();
            a.first_wave = ci * chunk_waves;
            a.keys = keysA.as<u64>();
            a.vals = valsA.as<u32>();
            a.counters = counters.as<u64>();
            const u64 waves = ((u64)len + kSpan - 1) / kSpan;
            const u32 grid = (u32)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
            hipLaunchKernelGGL(cov_extract_kernel<EMIT>, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, a);
            CHIP(c, hipGetLastError());
            if (!resident) CHIP(c, hipStreamSynchronize(st));   // the text buffer is overwritten by the next chunk
        }
        return LMAT_OK;
    }

    // The N occurrences of a pass in keysA / valsA -> the (group, multiplicity, k-mers) triples, added to the report of k index ki.
    int reduce(int ki, int k, int pe, u32 N) {
        lmat_cov_stats& S = c->stats;
        const int key_bits = 2 * k - pe;
        const bool pk = packed(k);
        CovSorted sorted;
        memset(&sorted, 0, sizeof(sorted));
        sorted.key_bits = key_bits;
        sorted.packed = pk ? 1 : 0;
        if (pk) {
            const int bits = std::max(key_bits + gb, 1);
            CHIP(c, with_temp(temp, [&](void* t, size_t& tb) {
                return rocprim::radix_sort_pairs(t, tb, keysA.as<u64>(), keysB.as<u64>(), valsA.as<u32>(), valsB.as<u32>(), N, 0, bits, st);
            }));
        } else {
            CHIP(c, ensure_all({{&gkeyA, (size_t)N * 4}, {&gkeyB, (size_t)N * 4}, {&idxA, (size_t)N * 4}, {&idxB, (size_t)N * 4}}));
            CHIP(c, with_temp(temp, [&](void* t, size_t& tb) {
                return rocprim::radix_sort_pairs(t, tb, keysA.as<u64>(), keysB.as<u64>(), valsA.as<u32>(), valsB.as<u32>(), N, 0, std::max(key_bits, 1), st);
            }));
            hipLaunchKernelGGL(cov_gather_kernel, dim3((N + 255) / 256), dim3(256), 0, st, valsB.as<u32>(), d_dgroup.as<u32>(), N, gkeyA.as<u32>(), idxA.as<u32>());
            CHIP(c, hipGetLastError());
            CHIP(c, with_temp(temp, [&](void* t, size_t& tb) {
                return rocprim::radix_sort_pairs(t, tb, gkeyA.as<u32>(), gkeyB.as<u32>(), idxA.as<u32>(), idxB.as<u32>(), N, 0, std::max(gb, 1), st);
            }));
            sorted.gkey = gkeyB.as<u32>();
            sorted.idx = idxB.as<u32>();
        }
        sorted.keys = keysB.as<u64>();
        sorted.reads = valsB.as<u32>();
        CHIP(c, timer.lap(S.sort_ms));

        // ---- runs of one (group, k-mer) and the reads in each
        const u32 gridN = (N + 255) / 256;
        hipLaunchKernelGGL(cov_flag_kernel, dim3(gridN), dim3(256), 0, st, sorted, N, flag.as<u64>());
        CHIP(c, hipGetLastError());
        CHIP(c, with_temp(temp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, flag.as<u64>(), pos.as<u64>(), 0ull, (size_t)N, rocprim::plus<u64>(), st); }));
        hipLaunchKernelGGL(cov_scatter_kernel, dim3(gridN), dim3(256), 0, st, sorted, N, flag.as<u64>(), pos.as<u64>(), run_first.as<u32>(), run_group.as<u32>(),
                           totals.as<u64>());
        CHIP(c, hipGetLastError());
        u64 tot = 0;
        CHIP(c, hipMemcpyAsync(&tot, totals.p, 8, hipMemcpyDeviceToHost, st));
        CHIP(c, timer.lap(S.segment_ms));
        const u32 R = (u32)tot;
        S.runs += R;

        // ---- histogram: keys into the flag array, sorted into the scan's, run-length encoded into the first key / read-index buffers
        hipLaunchKernelGGL(cov_hkey_kernel, dim3((R + 255) / 256), dim3(256), 0, st, run_first.as<u32>(), run_group.as<u32>(), R, flag.as<u64>());
        CHIP(c, hipGetLastError());
        CHIP(c, with_temp(temp, [&](void* t, size_t& tb) { return rocprim::radix_sort_keys(t, tb, flag.as<u64>(), pos.as<u64>(), R, 0, 32 + std::max(gb, 1), st); }));
        u32* d_h = reinterpret_cast<u32*>(totals.as<u64>() + 2);
        CHIP(c, with_temp(temp, [&](void* t, size_t& tb) { return rocprim::run_length_encode(t, tb, pos.as<u64>(), R, keysA.as<u64>(), valsA.as<u32>(), d_h, st); }));
        u32 H = 0;
        CHIP(c, hipMemcpyAsync(&H, d_h, 4, hipMemcpyDeviceToHost, st));
        CHIP(c, hipStreamSynchronize(st));
        std::vector<u64> h_key(H);
        std::vector<u32> h_cnt(H);
        if (H) {
            CHIP(c, hipMemcpyAsync(h_key.data(), keysA.p, (size_t)H * 8, hipMemcpyDeviceToHost, st));
            CHIP(c, hipMemcpyAsync(h_cnt.data(), valsA.p, (size_t)H * 4, hipMemcpyDeviceToHost, st));
        }
        CHIP(c, timer.lap(S.histogram_ms));
        auto& rep = c->rep[ki];
        for (u32 i = 0; i < H; ++i) {
            const u64 mult = h_key[i] & 0xFFFFFFFFull, n = h_cnt[i];
            lmat_cov::Rep& r = rep[groups[(size_t)(h_key[i] >> 32)]];
            r.distinct += n;
            r.total += mult * n;
            r.hist[mult] += n;
        }
        return LMAT_OK;
    }

    // all passes of one k under the split pe; overflow: a pass holds more occurrences than the budget does (nothing was emitted for it)
    int run_k(int ki, int pe, bool first_try, bool& overflow, u64& over_n, u32& over_pass) {
        const int k = c->ks[ki];
        lmat_cov_stats& S = c->stats;
        const u64 cp = cap(k);
        overflow = false;
        for (u32 pass = 0; pass < (1u << pe); ++pass) {
            CHIP(c, timer.start());
            CHIP(c, hipMemsetAsync(wave_cnt.p, 0, (n_waves + 1) * 8, st));
            if (const int rc = scan_text<false>(k, pe, pass, first_try && pass == 0)) return rc;   // every pass sees every window: counted once
            CHIP(c, with_temp(temp, [&](void* t, size_t& tb) {
                return rocprim::exclusive_scan(t, tb, wave_cnt.as<u64>(), wave_off.as<u64>(), 0ull, (size_t)(n_waves + 1), rocprim::plus<u64>(), st);
            }));
            u64 N = 0;
            CHIP(c, hipMemcpyAsync(&N, wave_off.as<u64>() + n_waves, 8, hipMemcpyDeviceToHost, st));
            CHIP(c, hipStreamSynchronize(st));
            if (N > cp) {
                overflow = true;
                over_n = N;
                over_pass = pass;
                CHIP(c, timer.lap(S.extract_ms));
                return LMAT_OK;
            }
            if (N == 0) { CHIP(c, timer.lap(S.extract_ms)); continue; }
            CHIP(c, ensure_all({{&keysA, (size_t)N * 8}, {&keysB, (size_t)N * 8}, {&valsA, (size_t)N * 4}, {&valsB, (size_t)N * 4}, {&flag, (size_t)N * 8},
                                {&pos, (size_t)N * 8}, {&run_first, ((size_t)N + 1) * 4}, {&run_group, (size_t)N * 4}}));
            if (const int rc = scan_text<true>(k, pe, pass, false)) return rc;
            CHIP(c, timer.lap(S.extract_ms));
            if (const int rc = reduce(ki, k, pe, (u32)N)) return rc;
        }
        return LMAT_OK;
    }
};

int run_cov(lmat_cov* c) {
    lmat_cov_stats& S = c->stats;
    S.reads = c->rec_start.size();
    S.bases = c->bases;
    c->rep.assign(c->ks.size(), std::map<u32, lmat_cov::Rep>());
    if (c->rec_start.empty()) return LMAT_OK;
    CovRun r;
    r.c = c;
    r.st = c->ctx->stream;
    r.T = c->text.size();
    r.n_rec = (u32)c->rec_start.size();
    if (const int rc = r.plan()) return rc;
    if (const int rc = r.alloc()) return rc;
    for (int ki = 0; ki < (int)c->ks.size(); ++ki) {
        const int k = c->ks[ki];
        const int pb_max = std::min(2 * k, kMaxPrefixBits);
        const u64 cp = r.cap(k);
        int pe = std::min(c->prefix_bits, 2 * k);
        if (c->prefix_bits < 0) {   // the smallest split whose even share fits; canonical k-mers crowd the low prefixes: the exact count decides
            pe = 0;
            while (pe < pb_max && r.T > cp && (double)r.T / (double)(1ull << pe) > (double)cp) ++pe;
        }
        for (bool first = true;; first = false) {
            bool overflow = false;
            u64 over_n = 0;
            u32 over_pass = 0;
            c->rep[ki].clear();
            const u64 runs0 = S.runs;
            const u32 passes0 = S.passes;
            S.passes += 1u << pe;
            if (const int rc = r.run_k(ki, pe, first, overflow, over_n, over_pass)) return rc;
            if (!overflow) break;
            if (c->prefix_bits >= 0 || pe >= pb_max)
                return cov_err(c, LMAT_E_CAPACITY, "k = " + std::to_string(k) + ": prefix pass " + std::to_string(over_pass) + " of " + std::to_string(1u << pe) + " holds " +
                                                   std::to_string(over_n) + " window occurrences, the device budget holds " + std::to_string(cp) +
                                                   ": raise the budget" + (pe < pb_max ? " or prefix_bits" : ""));
            S.runs = runs0;       // a derived split proved too coarse for the skew of this input: this k again, one bit finer
            S.passes = passes0;
            ++pe;
        }
        S.prefix_bits = std::max<uint32_t>(S.prefix_bits, (uint32_t)pe);
    }
    u64 w = 0;
    CHIP(c, hipMemcpy(&w, r.counters.p, 8, hipMemcpyDeviceToHost));
    S.windows = w;
    return LMAT_OK;
}

}  // namespace

extern "C" {

int lmat_cov_create(lmat_ctx* ctx, const int* k_sizes, int n_k, lmat_cov** out) {
    if (!out) return LMAT_E_ARG;
    *out = nullptr;
    if (!ctx) return LMAT_E_ARG;
    if (!k_sizes || n_k < 1) return lmat::set_err(ctx, LMAT_E_ARG, "at least one k size is required");
    for (int i = 0; i < n_k; ++i)
        if (k_sizes[i] < 1 || k_sizes[i] > 31) return lmat::set_err(ctx, LMAT_E_ARG, "k sizes must lie in 1..31 (62-bit k-mers)");
    lmat_cov* c = new lmat_cov();
    c->ctx = ctx;
    c->ks.assign(k_sizes, k_sizes + n_k);
    memset(&c->stats, 0, sizeof(c->stats));
    *out = c;
    return LMAT_OK;
}

void lmat_cov_destroy(lmat_cov* c) { delete c; }
const char* lmat_cov_error(const lmat_cov* c) { return c ? c->err.c_str() : "null coverage object"; }

int lmat_cov_set_options(lmat_cov* c, uint64_t device_budget_bytes, int prefix_bits) {
    if (!c) return LMAT_E_ARG;
    if (prefix_bits < -1 || prefix_bits > kMaxPrefixBits) return cov_err(c, LMAT_E_ARG, "prefix_bits must be -1 (derive) or 0 .. 24");
    c->budget = device_budget_bytes;
    c->prefix_bits = prefix_bits;
    return LMAT_OK;
}

int lmat_cov_add_reads(lmat_cov* c, const uint8_t* ascii, const uint64_t* off, uint64_t n_reads, const uint32_t* group) {
    if (!c) return LMAT_E_ARG;
    if (c->done) return cov_err(c, LMAT_E_ARG, "reads cannot be added after lmat_cov_run");
    if (n_reads == 0) return LMAT_OK;
    if (!ascii || !off || !group) return cov_err(c, LMAT_E_ARG, "ascii, off and group are required with n_reads > 0");
    // the count first: it needs none of the arrays
    if (n_reads > 0xFFFFFFFFull || c->rec_start.size() + n_reads > 0xFFFFFFFFull) return cov_err(c, LMAT_E_CAPACITY, "more than 2^32 - 1 reads");
    for (u64 i = 0; i < n_reads; ++i)
        if (off[i + 1] < off[i]) return cov_err(c, LMAT_E_ARG, "off does not ascend at read " + std::to_string(i));
    const u64 bytes = off[n_reads] - off[0];
    const size_t n0 = c->rec_start.size(), t0 = c->text.size();
    try {
        c->text.reserve(t0 + bytes + n_reads);
        c->rec_start.reserve(n0 + n_reads);
        c->rec_group.reserve(n0 + n_reads);
        for (u64 i = 0; i < n_reads; ++i) {
            c->rec_start.push_back(c->text.size());
            c->rec_group.push_back(group[i]);
            c->text.insert(c->text.end(), ascii + off[i], ascii + off[i + 1]);
            c->text.push_back('\n');   // a read boundary is an invalid byte
        }
    } catch (const std::exception&) {   // out of host memory: the call adds nothing
        c->rec_start.resize(std::min(n0, c->rec_start.size()));
        c->rec_group.resize(std::min(n0, c->rec_group.size()));
        c->text.resize(std::min(t0, c->text.size()));
        return cov_err(c, LMAT_E_NOMEM, "out of host memory for " + std::to_string(bytes + n_reads) + " more bytes of read text");
    }
    c->bases += bytes;
    return LMAT_OK;
}

int lmat_cov_run(lmat_cov* c, lmat_cov_stats* out) {
    if (!c) return LMAT_E_ARG;
    if (c->done) return cov_err(c, LMAT_E_ARG, "lmat_cov_run may be called once per object");
    if (hipSetDevice(c->ctx->device) != hipSuccess) return cov_err(c, LMAT_E_DEVICE, "hipSetDevice failed");
    memset(&c->stats, 0, sizeof(c->stats));
    const int rc = run_cov(c);
    if (rc) return rc;
    c->done = true;
    if (out) *out = c->stats;
    return LMAT_OK;
}

int lmat_cov_summary(lmat_cov* c, int k_index, uint32_t* groups, uint64_t* distinct, uint64_t* total, uint64_t cap, uint64_t* n) {
    if (!c || !n) return LMAT_E_ARG;
    if (!c->done) return cov_err(c, LMAT_E_ARG, "lmat_cov_run first");
    if (k_index < 0 || k_index >= (int)c->ks.size()) return cov_err(c, LMAT_E_ARG, "k_index beyond the k sizes of the object");
    const auto& rep = c->rep[k_index];
    *n = rep.size();
    if (rep.size() > cap) return cov_err(c, LMAT_E_CAPACITY, "cap below the " + std::to_string(rep.size()) + " groups with a k-mer");
    if (rep.size() && (!groups || !distinct || !total)) return LMAT_E_ARG;
    u64 j = 0;
    for (const auto& g : rep) { groups[j] = g.first; distinct[j] = g.second.distinct; total[j++] = g.second.total; }
    return LMAT_OK;
}

int lmat_cov_histogram(lmat_cov* c, int k_index, uint32_t group, uint64_t* multiplicity, uint64_t* n_kmers, uint64_t cap, uint64_t* n) {
    if (!c || !n) return LMAT_E_ARG;
    if (!c->done) return cov_err(c, LMAT_E_ARG, "lmat_cov_run first");
    if (k_index < 0 || k_index >= (int)c->ks.size()) return cov_err(c, LMAT_E_ARG, "k_index beyond the k sizes of the object");
    *n = 0;
    const auto it = c->rep[k_index].find(group);
    if (it == c->rep[k_index].end()) return LMAT_OK;
    const auto& h = it->second.hist;
    *n = h.size();
    if (h.size() > cap) return cov_err(c, LMAT_E_CAPACITY, "cap below the " + std::to_string(h.size()) + " multiplicities of the group");
    if (!multiplicity || !n_kmers) return LMAT_E_ARG;
    u64 j = 0;
    for (const auto& m : h) { multiplicity[j] = m.first; n_kmers[j++] = m.second; }
    return LMAT_OK;
}

}  // extern "C"
