// dbexport.hip -- a loaded k-mer database back out as tax_histo records, on the GPU (the lmat_export_* family of include/lmat_hip.h,
// DESIGN section 12).  The inverse of every way into the table: whatever built it (files, either image, genomes, a merge), the export
// is the sorted list of its k-mers with their taxid lists in stored order, in the file format lmat_db_add_taxhisto reads.
//
// Per prefix pass (pass p = the k-mers whose top prefix_bits bits equal p), all on the context's stream:
//   scan_cpt_kernel    the compact bucket array: 16 buckets per wave load, empty loads skipped, a lane per occupied slot,
//                      cpt_unaddress (lmat_common.hpp) gives the k-mer back, (k-mer, 24-bit payload) pairs compacted by ballot + mbcnt
//   scan_wide_kernel   the same for 8 x u64 slot buckets: the overflow table of a compact table, or the whole table in the wide layout
//   rocPRIM radix_sort_pairs on bits [0, 2k)
//   dup_kernel         two equal neighbours = the table holds a key twice: reported, never de-duplicated
//   with a filter (lmat_export_set_filter): slice_kernel, exclusive scan, scatter_kernel -- the kept pairs, still ascending
//   len_kernel, exclusive scan, write_kernel   CSR of 32-bit ids in stored order (the three decodings of lookup_kernel, kernels.hip)
//   radix_sort_keys + run_length_encode of the pass's ids    per-taxid counts (frequency_counter), merged on the host
// The host fetches the pass and appends it to the result or streams it to the file, so neither memory bounds the table's size.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <rocprim/rocprim.hpp>
#include <string>
#include <vector>
#include "lmat_internal.hpp"
#include "kmer_dev.hpp"

namespace {

using namespace lmat_dev;
using namespace lmat;

// counters of one pass (device, 64-bit words)
enum { X_CURSOR = 0, X_OVERFLOW, X_FROM_BUCKETS, X_FROM_WIDE, X_DUP, X_DUP_KMER, X_ENTRIES, X_SINGLETONS, X_N };

constexpr u32 kShortList = 8;       // lists up to this length are written by their lane, longer ones by the wave
constexpr u64 kPairBytes = 40;      // device bytes per (k-mer, payload) pair of a pass: keys and payloads twice for the sort, length, offset
constexpr u64 kEntryBytes = 20;     // ... per list entry: the CSR, its sorted copy, the distinct ids and their counts
constexpr u32 kScanBlocks = 2048;   // grid of the scans: waves stride over the wave loads

struct ScanArgs {
    const uint4* table;      // 64-byte buckets
    u64 n_buckets;
    CptGeom cpt;             // scan_cpt_kernel only
    int k, prefix_bits;
    u32 pass;
    u64* keys;
    u32* pays;
    u64 cap;
    u64* counters;
};

// one compaction step of a wave: the lanes with `emit` append (kmer, pay); false when the pass's arrays are full (flagged, nothing written)
__device__ __forceinline__ void emit_pairs(const ScanArgs& a, u32 lane, bool emit, u64 kmer, u32 pay) {
    const u64 bal = __ballot(emit);
    if (!bal) return;
    const u32 cnt = __popcll(bal);
    u64 base = 0;
    if (lane == 0) base = atomicAdd(&a.counters[X_CURSOR], (u64)cnt);
    base = __shfl(base, 0);
    if (base + cnt > a.cap) {
        if (lane == 0) atomicMax(&a.counters[X_OVERFLOW], 1ull);   // the pass is repeated under a finer split or refused by the host, never cut short
    } else if (emit) {
        const u64 dst = base + __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
        a.keys[dst] = kmer;
        a.pays[dst] = pay;
    }
}

// Compact buckets (lmat_common.hpp): tag u16[12] | payload low u16[12] | payload high u8[12] | header.  A wave load is 16 buckets, four
// lanes of 16 bytes each; a load without a tag is left at once.  Otherwise the 1024 bytes go through the wave's LDS and the 192 slots
// are taken in three steps of 64 lanes.
__global__ __launch_bounds__(64 * kWavesPerBlock) void scan_cpt_kernel(ScanArgs a) {
    __shared__ uint4 s_buf[kWavesPerBlock][64];
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u64 n_loads = (a.n_buckets + 15) / 16, n_waves = (u64)gridDim.x * kWavesPerBlock;
    const int shift = 2 * a.k - a.prefix_bits;
    u64 found = 0;
    for (u64 ld = (u64)blockIdx.x * kWavesPerBlock + wv; ld < n_loads; ld += n_waves) {
        const u64 b = ld * 16 + (lane >> 2);
        uint4 q = make_uint4(0, 0, 0, 0);
        if (b < a.n_buckets) q = a.table[b * 4 + (lane & 3)];
        const u32 part = lane & 3;
        const bool tags = part == 0 ? (q.x | q.y | q.z | q.w) != 0 : (part == 1 && (q.x | q.y) != 0);
        if (!__ballot(tags)) continue;
        wave_sync();                 // the steps of the load before are through with the buffer
        s_buf[wv][lane] = q;
        wave_sync();
        const uint16_t* h = reinterpret_cast<const uint16_t*>(&s_buf[wv][0]);
        const uint8_t* c = reinterpret_cast<const uint8_t*>(&s_buf[wv][0]);
#pragma unroll
        for (u32 step = 0; step < 3; ++step) {
            const u32 g = step * 64 + lane, bi = g / kCptSlots, i = g - bi * kCptSlots;   // bi < 16
            const u32 tag = h[bi * 32 + i];
            bool emit = false;
            u64 kmer = 0;
            u32 pay = 0;
            if (tag) {
                kmer = cpt_unaddress(a.cpt, (u32)(ld * 16 + bi), tag);
                pay = (u32)h[bi * 32 + 12 + i] | ((u32)c[bi * 64 + 48 + i] << 16);
                emit = a.prefix_bits == 0 || (u32)(kmer >> shift) == a.pass;
            }
            found += emit ? 1 : 0;
            emit_pairs(a, lane, emit, kmer, pay);
        }
    }
    found = wave_sum(found);
    if (lane == 0 && found) atomicAdd(&a.counters[X_FROM_BUCKETS], found);
}

// 8 x u64 slot buckets (slot = k-mer << 24 | payload, 0 = empty): a lane loads two slots, a wave load is 16 buckets
__global__ __launch_bounds__(64 * kWavesPerBlock) void scan_wide_kernel(ScanArgs a) {
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u64 n_quads = a.n_buckets * 4, n_loads = (n_quads + 63) / 64, n_waves = (u64)gridDim.x * kWavesPerBlock;
    const int shift = 2 * a.k - a.prefix_bits;
    u64 found = 0;
    for (u64 ld = (u64)blockIdx.x * kWavesPerBlock + wv; ld < n_loads; ld += n_waves) {
        const u64 qi = ld * 64 + lane;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (qi < n_quads) q = a.table[qi];
        const u64 v[2] = {((u64)q.y << 32) | q.x, ((u64)q.w << 32) | q.z};
        if (!__ballot((v[0] | v[1]) != 0)) continue;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u64 kmer = v[s] >> kPayloadBits;
            const bool emit = v[s] != 0 && (a.prefix_bits == 0 || (u32)(kmer >> shift) == a.pass);
            found += emit ? 1 : 0;
            emit_pairs(a, lane, emit, kmer, (u32)v[s] & kPayloadMask);
        }
    }
    found = wave_sum(found);
    if (lane == 0 && found) atomicAdd(&a.counters[X_FROM_WIDE], found);
}

__global__ __launch_bounds__(256) void dup_kernel(const u64* keys, u64 n, u64* counters) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 || i >= n || keys[i] != keys[i - 1]) return;
    if (atomicAdd(&counters[X_DUP], 1ull) == 0) counters[X_DUP_KMER] = keys[i];
}

// the stored list of a payload: 1 entry for a plain singleton, else n_raw of the list record (n of a gene record)
__device__ __forceinline__ u32 list_len(const DeviceTables& tb, u32 pay) {
    if (pay < kListBase) return 1;
    const size_t eoff = LMAT_LIST_OFF(pay, tb.list_shift);
    return (tb.arena[eoff] & 0x8000u) ? tb.arena[eoff + 1] : tb.arena[eoff + 2];
}

__global__ __launch_bounds__(256) void len_kernel(DeviceTables tb, const u32* pays, u64 n, u64* len, u64* counters) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    u64 l = 0;
    if (i < n) { l = list_len(tb, pays[i]); len[i] = l; }
    const u64 ones = __popcll(__ballot(l == 1));
    const u64 sum = wave_sum(l);
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(&counters[X_ENTRIES], sum);
        if (ones) atomicAdd(&counters[X_SINGLETONS], ones);
    }
}

// entry j of the list behind a list payload, as a 32-bit id: a gene record's pair, a wide database's (low, high) pair, or conv[16-bit code]
struct ListRef {
    const uint16_t* raw;
    int kind;   // 0: 16-bit codes through conv, 1: pairs
};
__device__ __forceinline__ ListRef list_ref(const DeviceTables& tb, u32 pay) {
    const size_t eoff = LMAT_LIST_OFF(pay, tb.list_shift);
    if (tb.arena[eoff] & 0x8000u) return ListRef{tb.arena + eoff + kListHdr, 1};
    const u32 nk = tb.arena[eoff + 1];
    if (tb.wide) return ListRef{tb.arena + eoff + kListHdr + 4 * (size_t)nk, 1};
    return ListRef{tb.arena + eoff + kListHdr + 2 * (size_t)nk, 0};
}
__device__ __forceinline__ u32 list_entry(const DeviceTables& tb, const ListRef& r, u32 j) {
    return r.kind ? (u32)r.raw[2 * j] | ((u32)r.raw[2 * j + 1] << 16) : tb.conv[r.raw[j]];
}

// A lane per record: singletons and lists of up to kShortList entries are written by their lane, the others by the whole wave in turn
__global__ __launch_bounds__(64 * kWavesPerBlock) void write_kernel(DeviceTables tb, const u32* pays, const u64* off, u64 n, u32* tids) {
    const u32 lane = lane_id();
    const u64 i = ((u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * 64 + lane;
    u32 pay = 0, len = 0;
    u64 o = 0;
    if (i < n) {
        pay = pays[i];
        o = off[i];
        len = (u32)(off[i + 1] - o);
        if (pay < kListBase) tids[o] = tb.tid32[pay];
        else if (len <= kShortList) {
            const ListRef r = list_ref(tb, pay);
            for (u32 j = 0; j < len; ++j) tids[o + j] = list_entry(tb, r, j);
        }
    }
    u64 longs = __ballot(pay >= kListBase && len > kShortList);
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const u32 lp = __shfl(pay, src), ln = __shfl(len, src);
        const u64 lo = ((u64)__shfl((u32)(o >> 32), src) << 32) | __shfl((u32)o, src);
        const ListRef r = list_ref(tb, lp);
        for (u32 j = lane; j < ln; j += 64) tids[lo + j] = list_entry(tb, r, j);
    }
}

// ---- the taxonomic slice (lmat_export_set_filter): between dup_kernel and len_kernel, so that everything behind it
// sees kept records only.  facts_kernel (once per run) -> slice_kernel (keep flag per record) -> exclusive scan -> scatter_kernel.
enum { F_KEPT = 0, F_DROP_TAXON, F_DROP_DEPTH, F_DROP_LEN, F_WAVE_LISTS, F_N };

constexpr u32 kInS = 0x80000000u;   // fact word of a list entry: this bit when it lies in S, its tree depth below it; 0 for an id the taxonomy does not hold
constexpr u64 kFilterPairBytes = 8; // device bytes a filter adds per scanned pair: keep flag and position

struct SliceArgs {
    const u32* id_fact;      // [n_ids] by internal id: singleton payloads, pair entries once found
    const u32* code_fact;    // [65536] by stored 16-bit code
    u32 n_ids;               // nodes + 1
    int mode;
    u32 min_depth, max_entries;
};

// the internal id of a 32-bit taxid (tid32[1 .. n_ids) ascends), 0 when the taxonomy does not hold it
__device__ __forceinline__ u32 find_id(const u32* tid32, u32 n_ids, u32 tid) {
    u32 lo = 1, hi = n_ids;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (tid32[mid] < tid) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_ids && tid32[lo] == tid ? lo : 0;
}

// iv: the merged Euler intervals of S, n_iv pairs (first tick, last tick), ascending and disjoint
__device__ __forceinline__ u32 node_fact(const u32* tin, const u32* depth, const u32* iv, u32 n_iv, u32 id) {
    const u32 t = tin[id];
    u32 lo = 0, hi = n_iv;
    while (lo < hi) {   // the intervals that start at or before t
        const u32 mid = (lo + hi) >> 1;
        if (iv[2 * mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return (lo && t <= iv[2 * lo - 1] ? kInS : 0u) | depth[id];
}

// a thread per internal id, then per 16-bit code
__global__ __launch_bounds__(256) void facts_kernel(const u32* tid32, const u32* conv, const u32* tin, const u32* depth, const u32* iv, u32 n_iv, u32 n_ids,
                                                    u32* id_fact, u32* code_fact) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g < n_ids) id_fact[g] = g ? node_fact(tin, depth, iv, n_iv, g) : 0u;
    else if (g - n_ids < 65536u) {
        const u32 t = conv[g - n_ids];
        const u32 id = t ? find_id(tid32, n_ids, t) : 0u;
        code_fact[g - n_ids] = id ? node_fact(tin, depth, iv, n_iv, id) : 0u;
    }
}

__device__ __forceinline__ u32 entry_fact(const DeviceTables& tb, const SliceArgs& f, const ListRef& r, u32 j) {
    if (!r.kind) return f.code_fact[r.raw[j]];
    const u32 id = find_id(tb.tid32, f.n_ids, (u32)r.raw[2 * j] | ((u32)r.raw[2 * j + 1] << 16));
    return id ? f.id_fact[id] : 0u;
}

// A lane per sorted record, as write_kernel: singletons and lists of up to kShortList entries are judged by their lane, the others by the
// whole wave in turn (entries in S summed, depths minimised across the lanes).  keep[i] = 1 iff every enabled test passes; a record that
// fails is charged to the first of taxon, depth, length.
__global__ __launch_bounds__(64 * kWavesPerBlock) void slice_kernel(DeviceTables tb, SliceArgs f, const u32* pays, u64 n, u32* keep, u64* fc) {
    const u32 lane = lane_id();
    const u64 i = ((u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * 64 + lane;
    const bool have = i < n;
    u32 pay = 0, len = 0, in = 0, mind = ~kInS;
    if (have) {
        pay = pays[i];
        if (pay < kListBase) {
            const u32 w = pay < f.n_ids ? f.id_fact[pay] : 0u;
            len = 1;
            in = w >> 31;
            mind = w & ~kInS;
        } else {
            len = list_len(tb, pay);
            if (len <= kShortList) {
                const ListRef r = list_ref(tb, pay);
                for (u32 j = 0; j < len; ++j) {
                    const u32 w = entry_fact(tb, f, r, j);
                    in += w >> 31;
                    mind = min(mind, w & ~kInS);
                }
            }
        }
    }
    u64 longs = __ballot(have && pay >= kListBase && len > kShortList);
    const u32 n_long = __popcll(longs);
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const u32 lp = __shfl(pay, src), ln = __shfl(len, src);
        const ListRef r = list_ref(tb, lp);
        u32 c = 0, d = ~kInS;
        for (u32 j = lane; j < ln; j += 64) {
            const u32 w = entry_fact(tb, f, r, j);
            c += w >> 31;
            d = min(d, w & ~kInS);
        }
        c = wave_sum(c);
        d = wave_reduce(d, [](u32 x, u32 y) { return x < y ? x : y; });
        if (lane == (u32)src) { in = c; mind = d; }
    }
    u32 v = 0;   // 0: kept, else the test that drops it
    if (have) {
        const bool taxon = f.mode == LMAT_SLICE_ANY ? in != 0 : f.mode == LMAT_SLICE_ALL ? in == len : f.mode == LMAT_SLICE_NONE ? in == 0 : true;
        if (!taxon) v = 1;
        else if (f.min_depth && mind < f.min_depth) v = 2;
        else if (f.max_entries && len > f.max_entries) v = 3;
        keep[i] = v == 0;
    }
    const u32 kept = __popcll(__ballot(have && v == 0)), t = __popcll(__ballot(v == 1)), d = __popcll(__ballot(v == 2)), l = __popcll(__ballot(v == 3));
    if (lane == 0) {
        if (kept) atomicAdd(&fc[F_KEPT], (u64)kept);
        if (t) atomicAdd(&fc[F_DROP_TAXON], (u64)t);
        if (d) atomicAdd(&fc[F_DROP_DEPTH], (u64)d);
        if (l) atomicAdd(&fc[F_DROP_LEN], (u64)l);
        if (n_long) atomicAdd(&fc[F_WAVE_LISTS], (u64)n_long);
    }
}

// the kept pairs to their place: pos is the exclusive scan of keep, so the order stays
__global__ __launch_bounds__(256) void scatter_kernel(const u64* keys, const u32* pays, const u32* keep, const u32* pos, u64 n, u64* keys_out, u32* pays_out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    keys_out[pos[i]] = keys[i];
    pays_out[pos[i]] = pays[i];
}

double host_ms(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct lmat_export {
    lmat_ctx* ctx = nullptr;
    std::string err;
    u64 budget = 0;
    int prefix_bits = -1;
    bool done = false, in_memory = false;
    std::vector<u64> kmers, list_off;
    std::vector<u32> tids;
    std::map<u32, u64> counts;     // lists that hold the taxid
    lmat_export_stats stats;
    // the filter (lmat_export_set_filter): `on` when a test is enabled; iv = the merged Euler intervals of S as (first, last) tick pairs
    struct Filter {
        bool on = false;
        int mode = 0;
        u32 min_depth = 0, max_entries = 0;
        std::vector<u32> iv;
    } filter;
    u64 fstats[6] = {0, 0, 0, 0, 0, 0};   // scanned, kept, dropped by taxon / depth / length, long lists judged by a wave
    double ms_select = 0;
    DevBuf f_tin, f_depth, f_iv, id_fact, code_fact;   // the filter's device arrays: the export's own, not the context's
};

namespace {

int xerr(lmat_export* e, int code, const std::string& msg) {
    e->err = msg;
    return code;
}

#define XHIP(e, call)                                                                            \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) return xerr(e, e__ == hipErrorOutOfMemory ? LMAT_E_NOMEM : LMAT_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

std::string kmer_text(u64 kmer, int k) {
    std::string s(k, 'A');
    for (int i = 0; i < k; ++i) s[k - 1 - i] = "ACGT"[(kmer >> (2 * i)) & 3];
    return s + " (" + std::to_string(kmer) + ")";
}

// the records of one pass on the host, and where they go
struct Sink {
    lmat_export* e = nullptr;
    FILE* f = nullptr;
    bool discard = false;            // counts only: the records go nowhere
    u64 written = 0;                 // records so far, across passes: the sanity word follows every 1500th
    std::vector<u64> h_kmers, h_off;
    std::vector<u32> h_tids;
    std::vector<uint8_t> bytes;

    bool header(int k, u64 count) {
        const uint32_t data_start = 29, version = 999, klen = (uint32_t)k;
        const uint64_t sanity = ~0ull;
        const char loc = 'N';
        return fwrite(&data_start, 4, 1, f) == 1 && fwrite(&count, 8, 1, f) == 1 && fwrite(&sanity, 8, 1, f) == 1 && fwrite(&version, 4, 1, f) == 1 &&
               fwrite(&loc, 1, 1, f) == 1 && fwrite(&klen, 4, 1, f) == 1;
    }
    // n records of the pass: h_kmers[n], h_off[n + 1], h_tids[h_off[n]]
    bool put(u64 n) {
        if (discard) { written += n; return true; }
        if (!f) {
            const u64 base = e->tids.size();
            e->kmers.insert(e->kmers.end(), h_kmers.begin(), h_kmers.begin() + n);
            for (u64 i = 1; i <= n; ++i) e->list_off.push_back(base + h_off[i]);
            e->tids.insert(e->tids.end(), h_tids.begin(), h_tids.begin() + h_off[n]);
            written += n;
            return true;
        }
        const uint64_t sanity = ~0ull;
        bytes.resize(n * 10 + h_off[n] * 4 + (n / 1500 + 1) * 8);
        size_t at = 0;
        for (u64 i = 0; i < n; ++i) {
            const u64 cnt = h_off[i + 1] - h_off[i];
            const uint16_t n16 = (uint16_t)cnt;
            memcpy(&bytes[at], &h_kmers[i], 8);
            memcpy(&bytes[at + 8], &n16, 2);
            memcpy(&bytes[at + 10], &h_tids[h_off[i]], cnt * 4);
            at += 10 + cnt * 4;
            if (++written % 1500 == 0) { memcpy(&bytes[at], &sanity, 8); at += 8; }
        }
        return fwrite(bytes.data(), 1, at, f) == at;
    }
};

struct ExportRun {
    lmat_export* e;
    lmat_ctx* c;
    hipStream_t st;
    int k, pb;
    u64 cap = 0, budget = 0;
    DevBuf counters, keysA, keysB, paysA, paysB, len, off, tids, tids_sorted, uniq, ucnt, n_runs, temp;
    DevBuf keep, pos, fcount;        // with a filter only
    u64 pair_bytes = kPairBytes;     // ... which adds kFilterPairBytes
    SliceArgs fa;
    LapTimer timer;
    u64 hc[X_N], fc[F_N];

    // the filter's per-entry facts, once per run
    int facts() {
        const lmat::HostTaxonomy& T = c->tax;
        const lmat_export::Filter& F = e->filter;
        const u32 n_ids = T.n + 1, n_iv = (u32)(F.iv.size() / 2);
        std::vector<u32> depth(T.path_len.begin(), T.path_len.end());
        XHIP(e, ensure_all({{&e->f_tin, (size_t)n_ids * 4}, {&e->f_depth, (size_t)n_ids * 4}, {&e->f_iv, F.iv.size() * 4}, {&e->id_fact, (size_t)n_ids * 4},
                            {&e->code_fact, 65536 * 4}, {&fcount, F_N * 8}}));
        XHIP(e, hipMemcpyAsync(e->f_tin.p, T.tin.data(), (size_t)n_ids * 4, hipMemcpyHostToDevice, st));
        XHIP(e, hipMemcpyAsync(e->f_depth.p, depth.data(), (size_t)n_ids * 4, hipMemcpyHostToDevice, st));
        if (n_iv) XHIP(e, hipMemcpyAsync(e->f_iv.p, F.iv.data(), F.iv.size() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(facts_kernel, dim3((n_ids + 65536 + 255) / 256), dim3(256), 0, st, c->dev.tid32, c->dev.conv, e->f_tin.as<u32>(), e->f_depth.as<u32>(),
                           e->f_iv.as<u32>(), n_iv, n_ids, e->id_fact.as<u32>(), e->code_fact.as<u32>());
        XHIP(e, hipGetLastError());
        XHIP(e, hipStreamSynchronize(st));   // depth goes out of scope
        fa = SliceArgs{e->id_fact.as<u32>(), e->code_fact.as<u32>(), n_ids, F.mode, F.min_depth, F.max_entries};
        return LMAT_OK;
    }

    // LMAT_OK; or `finer` set: the pass does not fit under this split
    int pass(u32 p, Sink& sink, bool& finer) {
        lmat_export_stats& S = e->stats;
        const DeviceTables& tb = c->dev;
        float ms = 0;
        XHIP(e, hipMemsetAsync(counters.p, 0, X_N * 8, st));
        XHIP(e, timer.start());
        ScanArgs a{reinterpret_cast<const uint4*>(tb.slots), tb.cpt.nb ? tb.cpt.nb : (u64)tb.nbuckets, tb.cpt, k, pb, p, keysA.as<u64>(), paysA.as<u32>(), cap,
                   counters.as<u64>()};
        if (tb.cpt.nb) {
            hipLaunchKernelGGL(scan_cpt_kernel, dim3(kScanBlocks), dim3(64 * kWavesPerBlock), 0, st, a);
            XHIP(e, hipGetLastError());
            a.table = reinterpret_cast<const uint4*>(tb.ovf_slots);
            a.n_buckets = tb.ovf_nbuckets;
        }
        if (a.n_buckets) {
            hipLaunchKernelGGL(scan_wide_kernel, dim3(kScanBlocks), dim3(64 * kWavesPerBlock), 0, st, a);
            XHIP(e, hipGetLastError());
        }
        XHIP(e, hipMemcpyAsync(hc, counters.p, X_N * 8, hipMemcpyDeviceToHost, st));
        XHIP(e, timer.lap(ms));
        S.ms_scan += ms;
        if (hc[X_OVERFLOW]) { finer = true; return LMAT_OK; }
        u64 n = hc[X_CURSOR];
        e->fstats[0] += n;
        S.from_buckets += hc[X_FROM_BUCKETS];
        S.from_overflow += hc[X_FROM_WIDE];
        if (!n) return LMAT_OK;
        ms = 0;
        XHIP(e, with_temp(temp, [&](void* t, size_t& tbytes) {
            return rocprim::radix_sort_pairs(t, tbytes, keysA.as<u64>(), keysB.as<u64>(), paysA.as<u32>(), paysB.as<u32>(), (size_t)n, 0, 2 * k, st);
        }));
        const u32 g256 = (u32)((n + 255) / 256);
        hipLaunchKernelGGL(dup_kernel, dim3(g256), dim3(256), 0, st, keysB.as<u64>(), n, counters.as<u64>());
        XHIP(e, hipGetLastError());
        XHIP(e, timer.lap(ms));
        S.ms_sort += ms;
        ms = 0;
        const u64 scanned = n;
        const u64* keys = keysB.as<u64>();
        const u32* pays = paysB.as<u32>();
        if (e->filter.on) {   // the kept pairs, still ascending, into the sort's free buffers; n is the number kept from here on
            XHIP(e, hipMemsetAsync(fcount.p, 0, F_N * 8, st));
            hipLaunchKernelGGL(slice_kernel, dim3((u32)((n + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock))), dim3(64 * kWavesPerBlock), 0, st, tb, fa, pays, n,
                               keep.as<u32>(), fcount.as<u64>());
            XHIP(e, hipGetLastError());
            XHIP(e, with_temp(temp, [&](void* t, size_t& tbytes) {
                return rocprim::exclusive_scan(t, tbytes, keep.as<u32>(), pos.as<u32>(), 0u, (size_t)n, rocprim::plus<u32>(), st);
            }));
            hipLaunchKernelGGL(scatter_kernel, dim3(g256), dim3(256), 0, st, keys, pays, keep.as<u32>(), pos.as<u32>(), n, keysA.as<u64>(), paysA.as<u32>());
            XHIP(e, hipGetLastError());
            XHIP(e, hipMemcpyAsync(hc, counters.p, X_N * 8, hipMemcpyDeviceToHost, st));
            XHIP(e, hipMemcpyAsync(fc, fcount.p, F_N * 8, hipMemcpyDeviceToHost, st));
            XHIP(e, timer.lap(ms));
            XHIP(e, hipStreamSynchronize(st));
            e->ms_select += ms;
            ms = 0;
            if (hc[X_DUP])
                return xerr(e, LMAT_E_INTERNAL, "the table holds k-mer " + kmer_text(hc[X_DUP_KMER], k) + " twice (" + std::to_string(hc[X_DUP]) + " repeated keys in pass " + std::to_string(p) + ")");
            e->fstats[2] += fc[F_DROP_TAXON];
            e->fstats[3] += fc[F_DROP_DEPTH];
            e->fstats[4] += fc[F_DROP_LEN];
            e->fstats[5] += fc[F_WAVE_LISTS];
            n = fc[F_KEPT];
            if (!n) return LMAT_OK;
            keys = keysA.as<u64>();
            pays = paysA.as<u32>();
        }
        hipLaunchKernelGGL(len_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, tb, pays, n, len.as<u64>(), counters.as<u64>());
        XHIP(e, hipGetLastError());
        XHIP(e, with_temp(temp, [&](void* t, size_t& tbytes) {
            return rocprim::exclusive_scan(t, tbytes, len.as<u64>(), off.as<u64>(), 0ull, (size_t)n, rocprim::plus<u64>(), st);
        }));
        XHIP(e, hipMemcpyAsync(hc, counters.p, X_N * 8, hipMemcpyDeviceToHost, st));
        XHIP(e, hipStreamSynchronize(st));
        if (hc[X_DUP])
            return xerr(e, LMAT_E_INTERNAL, "the table holds k-mer " + kmer_text(hc[X_DUP_KMER], k) + " twice (" + std::to_string(hc[X_DUP]) + " repeated keys in pass " + std::to_string(p) + ")");
        const u64 entries = hc[X_ENTRIES];
        if (entries > 0xFFFFFFF0ull || scanned * pair_bytes + entries * kEntryBytes > budget) { finer = true; return LMAT_OK; }
        XHIP(e, hipMemcpyAsync(off.as<u64>() + n, &hc[X_ENTRIES], 8, hipMemcpyHostToDevice, st));
        XHIP(e, ensure_all({{&tids, entries * 4}, {&tids_sorted, entries * 4}, {&uniq, entries * 4}, {&ucnt, entries * 4}}));
        hipLaunchKernelGGL(write_kernel, dim3((u32)((n + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock))), dim3(64 * kWavesPerBlock), 0, st, tb, pays, off.as<u64>(),
                           n, tids.as<u32>());
        XHIP(e, hipGetLastError());
        // per-taxid counts of the pass: its ids sorted, one run per id
        XHIP(e, with_temp(temp, [&](void* t, size_t& tbytes) { return rocprim::radix_sort_keys(t, tbytes, tids.as<u32>(), tids_sorted.as<u32>(), (size_t)entries, 0, 32, st); }));
        XHIP(e, with_temp(temp, [&](void* t, size_t& tbytes) {
            return rocprim::run_length_encode(t, tbytes, tids_sorted.as<u32>(), (unsigned)entries, uniq.as<u32>(), ucnt.as<u32>(), n_runs.as<u32>(), st);
        }));
        XHIP(e, timer.lap(ms));
        S.ms_lists += ms;
        // the pass to the host
        const auto t0 = std::chrono::steady_clock::now();
        u32 runs = 0;
        XHIP(e, hipMemcpy(&runs, n_runs.p, 4, hipMemcpyDeviceToHost));
        if (sink.h_kmers.size() < n) { sink.h_kmers.resize(n); sink.h_off.resize(n + 1); }
        if (sink.h_tids.size() < entries) sink.h_tids.resize(entries);
        std::vector<u32> hu(runs), hn(runs);
        XHIP(e, hipMemcpy(sink.h_kmers.data(), keys, n * 8, hipMemcpyDeviceToHost));
        XHIP(e, hipMemcpy(sink.h_off.data(), off.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        XHIP(e, hipMemcpy(sink.h_tids.data(), tids.p, entries * 4, hipMemcpyDeviceToHost));
        if (runs) {
            XHIP(e, hipMemcpy(hu.data(), uniq.p, (size_t)runs * 4, hipMemcpyDeviceToHost));
            XHIP(e, hipMemcpy(hn.data(), ucnt.p, (size_t)runs * 4, hipMemcpyDeviceToHost));
        }
        for (u32 i = 0; i < runs; ++i) e->counts[hu[i]] += hn[i];
        S.ms_fetch += host_ms(t0);
        const auto t1 = std::chrono::steady_clock::now();
        if (!sink.put(n)) return xerr(e, LMAT_E_IO, "write error on the tax_histo file");
        S.ms_write += host_ms(t1);
        S.records += n;
        S.entries += entries;
        S.singletons += hc[X_SINGLETONS];
        e->fstats[1] += n;
        return LMAT_OK;
    }
};

// one attempt under prefix_bits = pb; `finer`: a pass did not fit
int run_export(lmat_export* e, const char* fn, int pb, bool& finer) {
    lmat_ctx* c = e->ctx;
    ExportRun r;
    r.e = e; r.c = c; r.st = c->stream; r.k = c->dev.k; r.pb = pb;
    memset(&e->stats, 0, sizeof(e->stats));
    e->stats.prefix_bits = pb;
    e->kmers.clear(); e->tids.clear(); e->counts.clear();
    e->list_off.assign(1, 0);
    memset(e->fstats, 0, sizeof(e->fstats));
    e->ms_select = 0;
    if (e->filter.on) r.pair_bytes += kFilterPairBytes;
    u64 budget = e->budget;
    if (!budget) {
        size_t fr = 0, tot = 0;
        XHIP(e, hipMemGetInfo(&fr, &tot));
        budget = fr / 2;
    }
    r.budget = budget;
    // no pass holds more pairs than the table holds k-mers (a little slack, so that a key held twice is found and named, not refused)
    r.cap = std::min<u64>(std::min<u64>(budget / r.pair_bytes, c->n_kmers + c->n_kmers / 64 + 1024), 0x7FFFFF00ull);
    if (r.cap < 64) return xerr(e, LMAT_E_CAPACITY, "device budget of " + std::to_string(budget) + " bytes holds no pass");
    XHIP(e, ensure_all({{&r.counters, X_N * 8}, {&r.keysA, r.cap * 8}, {&r.keysB, r.cap * 8}, {&r.paysA, r.cap * 4}, {&r.paysB, r.cap * 4}, {&r.len, r.cap * 8},
                        {&r.off, (r.cap + 1) * 8}, {&r.n_runs, 8}}));
    if (e->filter.on) {
        XHIP(e, ensure_all({{&r.keep, r.cap * 4}, {&r.pos, r.cap * 4}}));
        if (const int rc = r.facts()) return rc;
    }
    XHIP(e, r.timer.init(r.st));
    Sink sink;
    sink.e = e;
    sink.discard = fn && !*fn;
    if (fn && *fn) {
        sink.f = fopen(fn, "wb");
        if (!sink.f) return xerr(e, LMAT_E_IO, std::string("cannot open ") + fn + " for writing");
        if (!sink.header(r.k, c->n_kmers)) { fclose(sink.f); return xerr(e, LMAT_E_IO, std::string("write error on ") + fn); }
    }
    int rc = LMAT_OK;
    const u32 n_pass = 1u << pb;
    for (u32 p = 0; p < n_pass && rc == LMAT_OK && !finer; ++p) rc = r.pass(p, sink, finer);
    e->stats.passes = n_pass;
    // with a filter the header count is known only now
    if (sink.f && e->filter.on && rc == LMAT_OK && !finer && (fseek(sink.f, 4, SEEK_SET) != 0 || fwrite(&sink.written, 8, 1, sink.f) != 1))
        rc = xerr(e, LMAT_E_IO, std::string("write error on ") + fn);
    if (sink.f && fclose(sink.f) != 0 && rc == LMAT_OK && !finer) rc = xerr(e, LMAT_E_IO, std::string("write error on ") + fn);
    if (rc == LMAT_OK && !finer && e->fstats[0] != c->n_kmers)
        rc = xerr(e, LMAT_E_INTERNAL, "the table gave " + std::to_string(e->fstats[0]) + " records, the database counts " + std::to_string(c->n_kmers) + " k-mers");
    return rc;
}

}  // namespace

extern "C" {

int lmat_export_create(lmat_ctx* ctx, lmat_export** out) {
    if (!out) return LMAT_E_ARG;
    *out = nullptr;
    if (!ctx) return LMAT_E_ARG;
    if (!ctx->db_ready || ctx->ingest) return lmat::set_err(ctx, LMAT_E_STATE, "the context holds no finalized database to export (lmat_db_finalize first)");
    if (ctx->synth_genome_len)
        return lmat::set_err(ctx, LMAT_E_STATE, "a synthetic database is not exported: its source is the generator's seed and its records are the generator's own");
    lmat_export* e = new lmat_export();
    e->ctx = ctx;
    memset(&e->stats, 0, sizeof(e->stats));
    *out = e;
    return LMAT_OK;
}

void lmat_export_destroy(lmat_export* e) { delete e; }
const char* lmat_export_error(const lmat_export* e) { return e ? e->err.c_str() : "null export"; }

int lmat_export_set_options(lmat_export* e, uint64_t device_budget_bytes, int prefix_bits) {
    if (!e) return LMAT_E_ARG;
    const int k = e->ctx->dev.k;
    if (prefix_bits < -1 || prefix_bits > 2 * k || prefix_bits > 24) return xerr(e, LMAT_E_ARG, "prefix_bits must be -1 (derive) or 0 .. min(2k, 24)");
    e->budget = device_budget_bytes;
    e->prefix_bits = prefix_bits;
    return LMAT_OK;
}

int lmat_export_set_filter(lmat_export* e, const lmat_export_filter* f) {
    if (!e) return LMAT_E_ARG;
    if (!f) { e->filter = lmat_export::Filter(); return LMAT_OK; }
    lmat_ctx* c = e->ctx;
    if (c->gene_mode) return xerr(e, LMAT_E_ARG, "a gene database holds gene ids, not taxids: its export takes no taxonomic filter");
    if (f->mode < 0 || f->mode > LMAT_SLICE_NONE) return xerr(e, LMAT_E_ARG, "filter mode must be 0 (no taxon test), LMAT_SLICE_ANY, LMAT_SLICE_ALL or LMAT_SLICE_NONE");
    if (f->mode && !f->n_taxa) return xerr(e, LMAT_E_ARG, "a taxon test needs at least one taxid");
    if (!f->mode && f->n_taxa) return xerr(e, LMAT_E_ARG, "taxa without a mode: say LMAT_SLICE_ANY, LMAT_SLICE_ALL or LMAT_SLICE_NONE");
    if (f->n_taxa && !f->taxa) return xerr(e, LMAT_E_ARG, "taxa is NULL");
    const lmat::HostTaxonomy& T = c->tax;
    std::vector<std::pair<u32, u32>> iv;
    for (u32 i = 0; i < f->n_taxa; ++i) {
        auto it = T.index_of.find(f->taxa[i]);
        if (it == T.index_of.end()) return xerr(e, LMAT_E_TAXONOMY, "taxid " + std::to_string(f->taxa[i]) + " of the filter is not in the taxonomy tree");
        iv.push_back(std::make_pair(T.tin[it->second], T.tout[it->second]));
    }
    std::sort(iv.begin(), iv.end());
    lmat_export::Filter F;
    for (const auto& v : iv) {   // subtrees nest or are disjoint: one that starts inside the last interval ends inside it too
        if (!F.iv.empty() && v.first <= F.iv.back()) F.iv.back() = std::max(F.iv.back(), v.second);
        else { F.iv.push_back(v.first); F.iv.push_back(v.second); }
    }
    F.mode = f->mode;
    F.min_depth = f->min_lca_depth;
    F.max_entries = f->max_entries;
    F.on = F.mode || F.min_depth || F.max_entries;
    e->filter = std::move(F);
    return LMAT_OK;
}

int lmat_export_filter_stats(const lmat_export* e, uint64_t out6[6], double* ms_select) {
    if (!e) return LMAT_E_ARG;
    if (!e->done) return xerr(const_cast<lmat_export*>(e), LMAT_E_STATE, "lmat_export_run first");
    if (out6) for (int i = 0; i < 6; ++i) out6[i] = e->fstats[i];
    if (ms_select) *ms_select = e->ms_select;
    return LMAT_OK;
}

// The slice goes through the ingest's own record parser as an in-memory stream of the file format, as lmat_db_build_from_genomes' result does.
int lmat_db_from_export(lmat_ctx* dst, lmat_export* e, uint64_t table_bytes) {
    if (!dst || !e) return LMAT_E_ARG;
    if (dst == e->ctx) return xerr(e, LMAT_E_ARG, "the slice of a context's database cannot replace that database: give another context");
    if (e->ctx->gene_mode) return xerr(e, LMAT_E_ARG, "a gene database is not sliced into a taxonomy context");
    if (!dst->tax.loaded) return xerr(e, LMAT_E_STATE, "the destination context has no taxonomy loaded");
    lmat_export_stats st;
    int rc = lmat_export_run(e, nullptr, &st);
    if (rc != LMAT_OK) return rc;
    if (!st.records) return xerr(e, LMAT_E_ARG, "the slice is empty: no k-mer of the database passes the filter");
    char* mem = nullptr;
    size_t mem_len = 0;
    FILE* w = open_memstream(&mem, &mem_len);
    if (!w) return xerr(e, LMAT_E_NOMEM, "open_memstream failed");
    Sink sink;
    sink.e = e;
    sink.f = w;
    sink.h_kmers.swap(e->kmers);   // lent to the writer, handed back below
    sink.h_tids.swap(e->tids);
    sink.h_off.swap(e->list_off);
    const bool ok = sink.header(e->ctx->dev.k, st.records) && sink.put(st.records);
    e->kmers.swap(sink.h_kmers);
    e->tids.swap(sink.h_tids);
    e->list_off.swap(sink.h_off);
    if (fclose(w) != 0 || !ok || !mem) { free(mem); return xerr(e, LMAT_E_NOMEM, "out of memory for the record stream"); }
    rc = lmat_db_begin(dst, e->ctx->dev.k, 0, table_bytes);
    if (rc == LMAT_OK) {
        FILE* r = fmemopen(mem, mem_len, "rb");
        if (!r) rc = lmat::set_err(dst, LMAT_E_NOMEM, "fmemopen failed");
        else if (!dst->ingest->add_taxhisto_stream(r, "<slice of a loaded database>")) {
            const bool tax = dst->ingest->err.compare(0, 3, "bad") == 0;   // an id the destination's taxonomy does not map
            rc = lmat::set_err(dst, tax ? LMAT_E_TAXONOMY : LMAT_E_IO, dst->ingest->err);
        }
    }
    free(mem);
    if (rc == LMAT_OK) rc = lmat_db_finalize(dst);
    if (rc != LMAT_OK) return xerr(e, rc, std::string("destination context: ") + lmat_last_error(dst));
    return LMAT_OK;
}

int lmat_export_run(lmat_export* e, const char* taxhisto_fn, lmat_export_stats* out) {
    if (!e) return LMAT_E_ARG;
    lmat_ctx* c = e->ctx;
    if (!c->db_ready || c->ingest) return xerr(e, LMAT_E_STATE, "the context holds no finalized database");
    if (hipSetDevice(c->device) != hipSuccess) return xerr(e, LMAT_E_DEVICE, "hipSetDevice failed");
    XHIP(e, hipStreamSynchronize(c->stream));
    e->done = false;
    const int pb_max = std::min(2 * c->dev.k, 24);
    int rc = LMAT_OK;
    for (int pb = e->prefix_bits < 0 ? 0 : e->prefix_bits;; ++pb) {
        bool finer = false;
        rc = run_export(e, taxhisto_fn, pb, finer);
        if (rc == LMAT_OK && finer) {
            if (e->prefix_bits >= 0)
                rc = xerr(e, LMAT_E_CAPACITY, "a pass of 2^" + std::to_string(pb) + " prefix passes does not fit the device budget: raise the budget or prefix_bits");
            else if (pb == pb_max) rc = xerr(e, LMAT_E_CAPACITY, "the device budget does not hold one pass of the finest prefix split");
            else continue;
        }
        break;
    }
    if (rc != LMAT_OK) {
        if (taxhisto_fn && *taxhisto_fn) remove(taxhisto_fn);
        e->kmers.clear(); e->tids.clear(); e->list_off.assign(1, 0); e->counts.clear();
        return rc;
    }
    e->done = true;
    e->in_memory = taxhisto_fn == nullptr;
    if (out) *out = e->stats;
    return LMAT_OK;
}

int lmat_export_fetch(lmat_export* e, uint64_t first, uint64_t count, uint64_t* kmers, uint64_t* list_off, uint32_t* tids, uint64_t tid_cap) {
    if (!e) return LMAT_E_ARG;
    if (!e->done || !e->in_memory) return xerr(e, LMAT_E_STATE, "lmat_export_run with taxhisto_fn = NULL first");
    if (first > e->kmers.size() || count > e->kmers.size() - first) return xerr(e, LMAT_E_ARG, "record range beyond the result");
    const u64 base = e->list_off[first], n = e->list_off[first + count] - base;
    if (kmers) memcpy(kmers, e->kmers.data() + first, count * 8);
    if (list_off) for (u64 i = 0; i <= count; ++i) list_off[i] = e->list_off[first + i] - base;
    if (tids) {
        if (n > tid_cap) return xerr(e, LMAT_E_CAPACITY, "tid_cap below the " + std::to_string(n) + " list entries of the range");
        memcpy(tids, e->tids.data() + base, n * 4);
    }
    return LMAT_OK;
}

int lmat_export_taxid_counts(lmat_export* e, uint32_t* tids, uint64_t* counts, uint64_t cap, uint64_t* n) {
    if (!e || !n) return LMAT_E_ARG;
    if (!e->done) return xerr(e, LMAT_E_STATE, "lmat_export_run first");
    *n = e->counts.size();
    if (*n > cap) return xerr(e, LMAT_E_CAPACITY, "cap below the " + std::to_string(*n) + " taxids with a count");
    if (*n && (!tids || !counts)) return LMAT_E_ARG;
    u64 j = 0;
    for (const auto& kv : e->counts) { tids[j] = kv.first; counts[j++] = kv.second; }
    return LMAT_OK;
}

}  // extern "C"
