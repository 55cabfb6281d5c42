// bins.hip -- reads pulled by called taxon on the GPU (the lmat_bins_* family of include/lmat_hip.h).
//
// Replaces the reference's bin/pull_reads.pl (run over the .out files by bin/pull_reads_mc.sh): per group of taxids one file with
// the reads called to them, plus the LowScore and NoDbHits groups.  The script takes the read from the .out record; here the
// selection runs on the result records a batch leaves on the device and the text comes from the packed reads, so a run that did not
// echo its reads, or whose reads have no host text, can be pulled from and only the pulled reads are copied back.  All on one stream:
//   bins_select_kernel   a lane per read: the record's printed fields (pullfmt.hpp: pull_fields), the script's branches in order, the
//                        listed ids by binary search in the sorted key table  ->  group (16 bits, 0xFFFF none)
//   rocPRIM radix sort   stable, pairs (group, read index): per group the indices ascending, the unselected reads last
//   bins_bounds_kernel   group_off[g] = first place of a key >= g (a lane per group)
//   bins_lens_kernel, rocPRIM exclusive scan, bins_gbase_kernel   the ASCII offset of every selected read, the bases per group
//   bins_unpack_kernel   (bases wanted) the selected records -> ACGT / N, one blob in group-major order
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <string>
#include <unordered_map>
#include <vector>
#include "bins.hpp"
#include "kmer_dev.hpp"
#include "pullfmt.hpp"

using lmat_dev::DevBuf;
using lmat_dev::u32;
using lmat_dev::u64;

struct lmat_bins {
    lmat_ctx* ctx = nullptr;
    std::string err;
    bool is_set = false, ran = false, have_bases = false;
    uint32_t n_groups = 0;
    uint32_t n_keys = 0;
    float thresh = 0, low_score = 0;
    int32_t min_kmer = 0;
    uint32_t low_grp = LMAT_BIN_NONE, nodb_grp = LMAT_BIN_NONE, rest_grp = LMAT_BIN_NONE;
    DevBuf keys, kgrp;                 // the listed ids ascending (u32) and the group of each (u16)
    lmat::BinsPart part;               // of the blocking path (lmat_bins_run, lmat_debug_bins_select)
    DevBuf lens, base, gbase, blob, dbg_results;
    std::vector<uint64_t> h_goff, h_gbase;   // [n_groups + 1] of the last run
};

namespace {

int bins_err(lmat_bins* b, int code, const std::string& msg) {
    b->err = msg;
    return code;
}
#define BHIP(b, call)                                                                                             \
    do {                                                                                                          \
        const hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) return bins_err(b, e_ == hipErrorOutOfMemory ? LMAT_E_NOMEM : LMAT_E_DEVICE,        \
                                              std::string(#call) + ": " + hipGetErrorString(e_));                 \
    } while (0)

struct SelectArgs {
    const lmat_read_result* res;
    u64 n;
    const u32* keys;
    const uint16_t* kgrp;
    u32 n_keys;
    float thresh, low_score;
    int min_kmer;
    u32 low_grp, nodb_grp, rest_grp;   // LMAT_BIN_NONE: there is no such group
    int k, prm_min_kmer;               // what the NoDbHits / ReadTooShort rows print as their score
    u32 n_groups, idx_base;
    uint16_t* grp;
    u32* key;                          // sort key: the group, n_groups for none (may be null with idx)
    u32* idx;
};

__global__ __launch_bounds__(256) void bins_select_kernel(SelectArgs a) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const lmat_read_result r = a.res[i];
    // the fields as printed: tid (-1 none), score, the third statistics field, and whether the type word is NoDbHits
    long long tid = -1;
    float score = -1.0f;
    int third = -1;
    bool nodb = false, printed = true;
    switch (r.status) {
        case LMAT_ST_SHORT_LEN: tid = r.read_len; score = (float)a.k; break;
        case LMAT_ST_SHORT_VALID: tid = r.valid_kmers; score = (float)a.prm_min_kmer; break;
        case LMAT_ST_NODBHITS: tid = r.read_len; score = (float)a.k; third = r.valid_kmers; nodb = true; break;
        case LMAT_ST_SILENT: printed = false; break;
        case LMAT_ST_PHIX: tid = r.call_tid; score = r.call_score; third = r.cand_kmer_cnt; break;
        default:
            third = r.cand_kmer_cnt;
            if (r.match_type == LMAT_MT_DIRECT || r.match_type == LMAT_MT_MULTI || r.match_type == LMAT_MT_PARTIAL) { tid = r.call_tid; score = r.call_score; }
            break;
    }
    u32 g = LMAT_BIN_NONE;
    if (printed) {
        const bool enough = third >= a.min_kmer;
        if (enough && tid >= 0 && score >= a.thresh) {   // branch 1
            const u32 t = (u32)tid;
            u32 lo = 0, hi = a.n_keys;
            while (lo < hi) { const u32 m = (lo + hi) >> 1; if (a.keys[m] < t) lo = m + 1; else hi = m; }
            if (lo < a.n_keys && a.keys[lo] == t) g = a.kgrp[lo];
        }
        if (g == LMAT_BIN_NONE && a.low_grp != LMAT_BIN_NONE && score < a.low_score && enough) g = a.low_grp;   // branch 2
        if (g == LMAT_BIN_NONE && nodb && enough) g = a.nodb_grp;                                               // branch 3
    }
    if (g == LMAT_BIN_NONE) g = a.rest_grp;
    a.grp[i] = (uint16_t)g;
    if (a.idx) {
        a.key[i] = g == LMAT_BIN_NONE ? a.n_groups : g;
        a.idx[i] = a.idx_base + (u32)i;
    }
}

// goff[g] = the first place of the sorted keys whose key is >= g, g = 0 .. n_groups (the last: the number of selected reads)
__global__ __launch_bounds__(256) void bins_bounds_kernel(const u32* __restrict__ key, u64 n, u32 n_groups, u64* __restrict__ goff) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g > n_groups) return;
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 m = (lo + hi) >> 1; if (key[m] < g) lo = m + 1; else hi = m; }
    goff[g] = lo;
}

// lens[j] = bases of the j-th read of the sorted order, 0 behind the selected ones and for the extra entry j == n
__global__ __launch_bounds__(256) void bins_lens_kernel(const u32* __restrict__ key, const u32* __restrict__ idx, u64 n, u32 n_groups,
                                                        const u32* __restrict__ words, const uint64_t* __restrict__ rec_off, u64* __restrict__ lens) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    lens[j] = j < n && key[j] < n_groups ? words[rec_off[idx[j]]] : 0;
}

__global__ __launch_bounds__(256) void bins_gbase_kernel(const u64* __restrict__ goff, const u64* __restrict__ base, u32 n_groups, u64* __restrict__ gbase) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    if (g <= n_groups) gbase[g] = base[goff[g]];
}

// The selected records as text.  Four reads per wave, 16 lanes a read; a lane makes one ALIGNED dword of the blob per step (the
// record's layout: len | ceil(len / 16) code words, 2 bits a base | ceil(len / 32) validity words).  A dword that lies inside the
// read is one store; the head and the tail of a read that share their dword with a neighbour are stored by bytes.
__global__ __launch_bounds__(256) void bins_unpack_kernel(const u32* __restrict__ words, const uint64_t* __restrict__ rec_off, const u32* __restrict__ idx,
                                                          const u64* __restrict__ base, const u64* __restrict__ goff, u32 n_groups,
                                                          uint8_t* __restrict__ out) {
    const u64 n_sel = goff[n_groups];
    const u32 lane = threadIdx.x & 63, sub = lane & 15u;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const u64 nw = (u64)gridDim.x * (blockDim.x >> 6);
    for (u64 j0 = wave * 4; j0 < n_sel; j0 += nw * 4) {
        const u64 j = j0 + (lane >> 4);
        const bool have = j < n_sel;
        const u32* rec = words + (have ? rec_off[idx[j]] : 0);
        const u32 len = have ? rec[0] : 0u;
        const u64 o = have ? base[j] : 0;
        const u32 nb = (len + 15) / 16, head = (u32)(o & 3);
        const u64 a0 = o - head;
        const u32 ndw = (head + len + 3) / 4;   // aligned dwords the read touches (0 for an empty read)
        for (u32 d0 = 0; __ballot(d0 < ndw) != 0; d0 += 16) {
            const u32 d = d0 + sub;
            if (d >= ndw) continue;
            u32 w = 0, inside = 0;
#pragma unroll
            for (u32 t = 0; t < 4; ++t) {
                const int p = (int)(4 * d + t) - (int)head;   // position in the read
                if (p < 0 || p >= (int)len) continue;
                const u32 code = (rec[1 + ((u32)p >> 4)] >> (2 * ((u32)p & 15))) & 3u;
                const u32 valid = (rec[1 + nb + ((u32)p >> 5)] >> ((u32)p & 31)) & 1u;
                const u32 ch = valid ? (0x54474341u >> (8 * code)) & 0xFFu : (u32)'N';
                w |= ch << (8 * t);
                inside |= 1u << t;
            }
            uint8_t* dst = out + a0 + 4ull * d;
            if (inside == 15u) *reinterpret_cast<u32*>(dst) = w;
            else
                for (u32 t = 0; t < 4; ++t)
                    if (inside >> t & 1u) dst[t] = (uint8_t)(w >> (8 * t));
        }
    }
}

int sort_bits(u32 n_groups) {   // keys are 0 .. n_groups
    int b = 1;
    while ((1u << b) <= n_groups) ++b;
    return b;
}

SelectArgs select_args(const lmat_bins* b, const lmat_read_result* d_results, u64 n) {
    SelectArgs a;
    memset(&a, 0, sizeof(a));
    a.res = d_results;
    a.n = n;
    a.keys = b->keys.as<u32>();
    a.kgrp = b->kgrp.as<uint16_t>();
    a.n_keys = b->n_keys;
    a.thresh = b->thresh;
    a.low_score = b->low_score;
    a.min_kmer = b->min_kmer;
    a.low_grp = b->low_grp;
    a.nodb_grp = b->nodb_grp;
    a.rest_grp = b->rest_grp;
    a.k = b->ctx->dev.k;
    a.prm_min_kmer = b->ctx->params.min_kmer;
    a.n_groups = b->n_groups;
    return a;
}

}  // namespace

namespace lmat {

lmat_ctx* bins_ctx(const lmat_bins* b) { return b->ctx; }
uint32_t bins_group_count(const lmat_bins* b) { return b->n_groups; }

int bins_part_alloc(lmat_bins* b, BinsPart& p, uint64_t max_reads, bool pinned) {
    if (max_reads > 0xFFFFFFFFull) return bins_err(b, LMAT_E_ARG, "batch above 2^32 reads");
    if (max_reads <= p.cap && p.goff.p && (!pinned || p.h_goff.p)) return LMAT_OK;
    const size_t n = (size_t)std::max<uint64_t>(max_reads, 1);
    size_t tb = 0;   // rocPRIM's storage for the largest sort the buffers can hold: 17 key bits cover every group count
    BHIP(b, rocprim::radix_sort_pairs(nullptr, tb, (u32*)nullptr, (u32*)nullptr, (u32*)nullptr, (u32*)nullptr, n, 0, 17, (hipStream_t)nullptr));
    tb = 2 * tb + (1u << 20);   // (a smaller batch may sort by another of rocPRIM's algorithms: bins_part_queue asks again for its own size)
    BHIP(b, lmat_dev::ensure_all({{&p.grp, n * 2}, {&p.keyA, n * 4}, {&p.keyB, n * 4}, {&p.idxA, n * 4}, {&p.idxB, n * 4}, {&p.temp, tb},
                                  {&p.goff, (size_t)kBinsOffWords * 8}}));
    if (pinned) {
        p.h_idx = PinnedBuf();
        if (!p.h_goff.p) BHIP(b, hipHostMalloc(&p.h_goff.p, (size_t)kBinsOffWords * 8, hipHostMallocDefault));
        BHIP(b, hipHostMalloc(&p.h_idx.p, n * 4, hipHostMallocDefault));
    }
    p.cap = max_reads;
    return LMAT_OK;
}

int bins_part_queue(lmat_bins* b, BinsPart& p, const lmat_read_result* d_results, uint64_t n, uint32_t idx_base, hipStream_t stream) {
    if (!b->is_set) return bins_err(b, LMAT_E_STATE, "lmat_bins_set first");
    if (n > p.cap) return bins_err(b, LMAT_E_ARG, "batch larger than the buffers of the partition");
    const u32 ng = b->n_groups;
    p.n_groups = ng;
    if (n == 0) {
        BHIP(b, hipMemsetAsync(p.goff.p, 0, ((size_t)ng + 1) * 8, stream));
    } else {
        SelectArgs a = select_args(b, d_results, n);
        a.idx_base = idx_base;
        a.grp = p.grp.as<uint16_t>();
        a.key = p.keyA.as<u32>();
        a.idx = p.idxA.as<u32>();
        hipLaunchKernelGGL(bins_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
        BHIP(b, hipGetLastError());
        size_t tb = 0;
        BHIP(b, rocprim::radix_sort_pairs(nullptr, tb, p.keyA.as<u32>(), p.keyB.as<u32>(), p.idxA.as<u32>(), p.idxB.as<u32>(), (size_t)n, 0, sort_bits(ng), stream));
        if (tb > p.temp.bytes) {
            if (p.h_goff.p) return bins_err(b, LMAT_E_INTERNAL, "the sort of " + std::to_string(n) + " reads asks for more storage than the slot was given");
            BHIP(b, p.temp.ensure(tb));
        }
        tb = p.temp.bytes;
        BHIP(b, rocprim::radix_sort_pairs(p.temp.p, tb, p.keyA.as<u32>(), p.keyB.as<u32>(), p.idxA.as<u32>(), p.idxB.as<u32>(), (size_t)n, 0, sort_bits(ng), stream));
        hipLaunchKernelGGL(bins_bounds_kernel, dim3((ng + 1 + 255) / 256), dim3(256), 0, stream, p.keyB.as<u32>(), (u64)n, ng, p.goff.as<u64>());
        BHIP(b, hipGetLastError());
    }
    if (p.h_goff.p) {
        BHIP(b, hipMemcpyAsync(p.h_goff.p, p.goff.p, ((size_t)ng + 1) * 8, hipMemcpyDeviceToHost, stream));
        if (n) BHIP(b, hipMemcpyAsync(p.h_idx.p, p.idxB.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    }
    p.valid = true;
    return LMAT_OK;
}

}  // namespace lmat

namespace {

// groups -> the sorted key table on the device
int set_groups(lmat_bins* b, const lmat_bin_group* groups, uint32_t n_groups, float thresh, int32_t min_kmer) {
    lmat_ctx* c = b->ctx;
    if (n_groups > 65534) return bins_err(b, LMAT_E_CAPACITY, std::to_string(n_groups) + " groups: group ids are 16 bits wide, at most 65534 groups");
    if (n_groups && !groups) return bins_err(b, LMAT_E_ARG, "groups is NULL");
    std::unordered_map<uint32_t, uint16_t> exact;
    uint32_t low = LMAT_BIN_NONE, nodb = LMAT_BIN_NONE, rest = LMAT_BIN_NONE;
    float low_score = 0;
    bool subtree = false;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const lmat_bin_group& G = groups[g];
        if (G.n_ids && !G.ids) return bins_err(b, LMAT_E_ARG, "group " + std::to_string(g) + ": ids is NULL");
        if (G.flags & ~(LMAT_BIN_SUBTREE | LMAT_BIN_REST | LMAT_BIN_LOWSCORE | LMAT_BIN_NODBHITS))
            return bins_err(b, LMAT_E_ARG, "group " + std::to_string(g) + ": unknown flag");
        for (uint32_t i = 0; i < G.n_ids; ++i) exact[G.ids[i]] = (uint16_t)g;   // the later group overwrites, as the script's hash does
        if (G.flags & LMAT_BIN_LOWSCORE) { low = g; low_score = G.low_score; }
        if (G.flags & LMAT_BIN_NODBHITS) nodb = g;
        if (G.flags & LMAT_BIN_REST) rest = g;
        subtree = subtree || (G.flags & LMAT_BIN_SUBTREE);
    }
    std::vector<std::pair<uint32_t, uint16_t>> table(exact.begin(), exact.end());
    if (subtree) {
        const lmat::HostTaxonomy& T = c->tax;
        if (!T.loaded) return bins_err(b, LMAT_E_STATE, "LMAT_BIN_SUBTREE needs a loaded taxonomy");
        // every node no group lists: the nearest ancestor that a SUBTREE group owns (paths: parent .. root)
        for (uint32_t t = 1; t <= T.n; ++t) {
            if (exact.count(T.tid32[t])) continue;
            const uint32_t* path = T.paths.data() + T.path_off[t];
            for (uint32_t d = 0; d < T.path_len[t]; ++d) {
                const auto it = exact.find(T.tid32[path[d]]);
                if (it != exact.end() && (groups[it->second].flags & LMAT_BIN_SUBTREE)) { table.emplace_back(T.tid32[t], it->second); break; }
            }
        }
    }
    std::sort(table.begin(), table.end());
    std::vector<uint32_t> keys(table.size());
    std::vector<uint16_t> kgrp(table.size());
    for (size_t i = 0; i < table.size(); ++i) { keys[i] = table[i].first; kgrp[i] = table[i].second; }
    hipSetDevice(c->device);
    BHIP(b, lmat_dev::ensure_all({{&b->keys, keys.size() * 4}, {&b->kgrp, kgrp.size() * 2}}));
    BHIP(b, hipDeviceSynchronize());   // a partition still queued (on the context's stream or a slot's joining stream) reads the old table
    if (!keys.empty()) {
        BHIP(b, hipMemcpy(b->keys.p, keys.data(), keys.size() * 4, hipMemcpyHostToDevice));
        BHIP(b, hipMemcpy(b->kgrp.p, kgrp.data(), kgrp.size() * 2, hipMemcpyHostToDevice));
    }
    b->n_keys = (uint32_t)keys.size();
    b->n_groups = n_groups;
    b->thresh = thresh;
    b->min_kmer = min_kmer;
    b->low_grp = low;
    b->low_score = low_score;
    b->nodb_grp = nodb;
    b->rest_grp = rest;
    b->is_set = true;
    b->ran = false;
    return LMAT_OK;
}

}  // namespace

extern "C" {

int lmat_bins_create(lmat_ctx* ctx, lmat_bins** out) {
    if (!out) return LMAT_E_ARG;
    *out = nullptr;
    if (!ctx) return LMAT_E_ARG;
    if (ctx->gene_mode) return lmat::set_err(ctx, LMAT_E_ARG, "a gene context has no taxids to pull reads by");
    lmat_bins* b = new lmat_bins();
    b->ctx = ctx;
    *out = b;
    return LMAT_OK;
}

void lmat_bins_destroy(lmat_bins* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    delete b;
}

const char* lmat_bins_error(const lmat_bins* b) { return b ? b->err.c_str() : "null bins object"; }

int lmat_bins_set(lmat_bins* b, const lmat_bin_group* groups, uint32_t n_groups, float thresh, int32_t min_kmer) {
    if (!b) return LMAT_E_ARG;
    return set_groups(b, groups, n_groups, thresh, min_kmer);
}

int lmat_bins_set_from_file(lmat_bins* b, const char* idfile, float thresh, int32_t min_kmer) {
    if (!b) return LMAT_E_ARG;
    if (!idfile) return bins_err(b, LMAT_E_ARG, "idfile is NULL");
    std::vector<lmat::PullGroup> pg;
    std::string msg;
    if (!lmat::parse_pull_idfile(idfile, pg, msg)) return bins_err(b, LMAT_E_IO, msg);
    if (pg.size() > 65534) return bins_err(b, LMAT_E_CAPACITY, std::to_string(pg.size()) + " groups in " + idfile + ": group ids are 16 bits wide, at most 65534 groups");
    std::vector<lmat_bin_group> g(pg.size());
    for (size_t i = 0; i < pg.size(); ++i) g[i] = {pg[i].ids.data(), (uint32_t)pg[i].ids.size(), pg[i].flags, pg[i].low_score};
    return set_groups(b, g.data(), (uint32_t)g.size(), thresh, min_kmer);
}

int lmat_bins_run(lmat_bins* b, const lmat_reads* reads, uint64_t first, uint64_t count, int want_bases) {
    if (!b) return LMAT_E_ARG;
    if (!reads) return bins_err(b, LMAT_E_ARG, "reads is NULL");
    if (!b->is_set) return bins_err(b, LMAT_E_STATE, "lmat_bins_set first");
    lmat_ctx* c = b->ctx;
    if (first + count > reads->n || first + count > 0xFFFFFFFFull) return bins_err(b, LMAT_E_ARG, "read range out of bounds");
    b->ran = false;
    lmat_ctx::BatchSet& s = c->set();
    if (count && (c->last_reads != reads || c->last_first != first || c->last_count != count || count * sizeof(lmat_read_result) > s.results.bytes))
        return bins_err(b, LMAT_E_STATE, "the most recent launch of the context was not for these reads, first and count: classify them first");
    hipSetDevice(c->device);
    hipStream_t st = c->stream;
    BHIP(b, hipStreamSynchronize(st));
    if (s.in_flight) BHIP(b, hipEventSynchronize(s.done));   // decision kernels on the side streams
    const u32 ng = b->n_groups;
    lmat::BinsPart& p = b->part;
    if (const int rc = lmat::bins_part_alloc(b, p, count, false)) return rc;
    if (const int rc = lmat::bins_part_queue(b, p, s.results.as<lmat_read_result>(), count, (u32)first, st)) return rc;
    BHIP(b, lmat_dev::ensure_all({{&b->lens, ((size_t)count + 1) * 8}, {&b->base, ((size_t)count + 1) * 8}, {&b->gbase, ((size_t)ng + 1) * 8}}));
    if (count) {
        hipLaunchKernelGGL(bins_lens_kernel, dim3((unsigned)((count + 1 + 255) / 256)), dim3(256), 0, st, p.keyB.as<u32>(), p.idxB.as<u32>(), (u64)count, ng,
                           reads->words, reads->rec_off, b->lens.as<u64>());
        BHIP(b, hipGetLastError());
        BHIP(b, lmat_dev::with_temp(p.temp, [&](void* t, size_t& tb) {
            return rocprim::exclusive_scan(t, tb, b->lens.as<u64>(), b->base.as<u64>(), 0ull, (size_t)count + 1, rocprim::plus<u64>(), st);
        }));
    } else BHIP(b, hipMemsetAsync(b->base.p, 0, 8, st));
    hipLaunchKernelGGL(bins_gbase_kernel, dim3((ng + 1 + 255) / 256), dim3(256), 0, st, p.goff.as<u64>(), b->base.as<u64>(), ng, b->gbase.as<u64>());
    BHIP(b, hipGetLastError());
    b->h_goff.assign((size_t)ng + 1, 0);
    b->h_gbase.assign((size_t)ng + 1, 0);
    BHIP(b, hipMemcpyAsync(b->h_goff.data(), p.goff.p, ((size_t)ng + 1) * 8, hipMemcpyDeviceToHost, st));
    BHIP(b, hipMemcpyAsync(b->h_gbase.data(), b->gbase.p, ((size_t)ng + 1) * 8, hipMemcpyDeviceToHost, st));
    BHIP(b, hipStreamSynchronize(st));
    b->have_bases = false;
    if (want_bases) {
        const u64 total = b->h_gbase[ng], n_sel = b->h_goff[ng];
        BHIP(b, b->blob.ensure((size_t)total + 8));   // (a dword store never passes the read's end: the pad is for an empty blob)
        if (n_sel && total) {
            const u64 blocks = std::min<u64>((n_sel + 15) / 16, 16384);
            hipLaunchKernelGGL(bins_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reads->words, reads->rec_off, p.idxB.as<u32>(), b->base.as<u64>(),
                               p.goff.as<u64>(), ng, b->blob.as<uint8_t>());
            BHIP(b, hipGetLastError());
            BHIP(b, hipStreamSynchronize(st));
        }
        b->have_bases = true;
    }
    b->ran = true;
    return LMAT_OK;
}

int lmat_bins_counts(lmat_bins* b, uint64_t* n_reads_per_group, uint64_t* n_bases_per_group) {
    if (!b) return LMAT_E_ARG;
    if (!b->ran) return bins_err(b, LMAT_E_STATE, "lmat_bins_run first");
    for (uint32_t g = 0; g < b->n_groups; ++g) {
        if (n_reads_per_group) n_reads_per_group[g] = b->h_goff[g + 1] - b->h_goff[g];
        if (n_bases_per_group) n_bases_per_group[g] = b->h_gbase[g + 1] - b->h_gbase[g];
    }
    return LMAT_OK;
}

int lmat_bins_fetch(lmat_bins* b, uint32_t group, uint32_t* read_idx, uint64_t* base_off, uint8_t* bases) {
    if (!b) return LMAT_E_ARG;
    if (!b->ran) return bins_err(b, LMAT_E_STATE, "lmat_bins_run first");
    if (group >= b->n_groups) return bins_err(b, LMAT_E_ARG, "no such group");
    if (bases && !b->have_bases) return bins_err(b, LMAT_E_STATE, "the run did not ask for bases");
    hipSetDevice(b->ctx->device);
    const u64 j0 = b->h_goff[group], n = b->h_goff[group + 1] - j0, o0 = b->h_gbase[group], nb = b->h_gbase[group + 1] - o0;
    if (read_idx && n) BHIP(b, hipMemcpy(read_idx, b->part.idxB.as<u32>() + j0, n * 4, hipMemcpyDeviceToHost));
    if (base_off) {
        BHIP(b, hipMemcpy(base_off, b->base.as<u64>() + j0, (n + 1) * 8, hipMemcpyDeviceToHost));
        for (u64 i = 0; i <= n; ++i) base_off[i] -= o0;
    }
    if (bases && nb) BHIP(b, hipMemcpy(bases, b->blob.as<uint8_t>() + o0, nb, hipMemcpyDeviceToHost));
    return LMAT_OK;
}

int lmat_debug_bins_select(lmat_bins* b, const lmat_read_result* host_results, uint64_t n, uint16_t* group_out) {
    if (!b) return LMAT_E_ARG;
    if (!b->is_set) return bins_err(b, LMAT_E_STATE, "lmat_bins_set first");
    if (!n) return LMAT_OK;
    if (!host_results || !group_out) return bins_err(b, LMAT_E_ARG, "host_results and group_out are required");
    lmat_ctx* c = b->ctx;
    hipSetDevice(c->device);
    DevBuf grp;
    BHIP(b, b->dbg_results.ensure((size_t)n * sizeof(lmat_read_result)));
    BHIP(b, grp.ensure((size_t)n * 2));
    BHIP(b, hipMemcpyAsync(b->dbg_results.p, host_results, (size_t)n * sizeof(lmat_read_result), hipMemcpyHostToDevice, c->stream));
    SelectArgs a = select_args(b, b->dbg_results.as<lmat_read_result>(), n);
    a.grp = grp.as<uint16_t>();
    hipLaunchKernelGGL(bins_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
    BHIP(b, hipGetLastError());
    BHIP(b, hipMemcpyAsync(group_out, grp.p, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    BHIP(b, hipStreamSynchronize(c->stream));
    return LMAT_OK;
}

}  // extern "C"
