// dbgen.hip -- the k-mer database built from genome FASTA on the GPU (the lmat_build_* family of include/lmat_hip.h).
//
// Replaces the reference's two offline CPU programs:
//   kmerPrefixCounter   genome FASTA -> canonical k-mers with the ids of the genomes that hold them
//                       (src/kmerPrefixCounter.cpp:114-147, include/Encoder.hpp:96-215)
//   tax_histo           -> per k-mer the owners plus every node up to their lowest common ancestor
//                       (src/tax_histo.cpp:210-284, TaxTree::getLcaMap src/kmerdb/TaxTree.hpp:160-260)
// and writes the file lmat_db_add_taxhisto (dbbuild.cpp) reads.  Pipeline per prefix pass, all on the context's stream:
//   extract_kernel  text chunk -> (canonical k-mer, owner index) pairs whose top prefix_bits equal the pass number
//   rocPRIM radix sort by (k-mer, owner)
//   seg_flag / seg_scatter   distinct (k-mer, owner) pairs and the heads of the runs of one k-mer
//   closure_kernel<count>, exclusive scan, closure_kernel<write>   CSR of ascending taxids per k-mer
// Owner indices are handed out in the order of an Euler tour of the taxonomy (owners the tree does not know behind all
// others), so the owners of one k-mer arrive in tour order and the closure needs no de-duplication: the first owner walks up
// to and including the LCA of the first and the last, every later owner walks up to -- not including -- its LCA with the owner
// before it; those pieces are disjoint and their union is the closure (the "virtual tree" of the owners).
//
// Existing tax_histo files as further inputs (lmat_build_add_taxhisto): inside the same prefix passes the slice
// of every input with the pass's prefix and the pass's own result from the genomes are merged per k-mer:
//   one key per input RECORD (k-mer << source bits | source), rocPRIM radix sort, mseg_flag / mseg_scatter (runs of one k-mer),
//   union_classify (one-source runs are sized, gathered sets beyond 64 entries get a side-buffer segment, sorted by segment),
//   union_kernel<count>, exclusive scan, union_kernel<write>: a one-source list is copied, the others are the closure of the union
//   of the stored entries taken as owners -- the same virtual-tree walk over the entries in Euler-tour order, equal neighbours dropped.
// A loaded database is one more such input (lmat_build_add_db): exported into host memory by dbexport.hip when it is added,
// its records then go through input_record like a parsed file's.
// hist_kernel counts, for either kind of run, the result records whose list holds each taxid (countTaxidFrequency's map).
//
// The id-set mode (lmat_genebuild_create, DESIGN section 13: gene databases) stops where kmerPrefixCounter does: no tree, no closure.  Owner
// indices are the ranks of the ids among all ids of the run, so idlist_kernel<count / write> (in closure_kernel's place) writes id_of[owner]
// in order; tax_histo inputs are not a second stage there -- their entries of a pass join the extracted pairs before the sort, marked by one
// flag bit below the owner (text_runs_kernel reads it back for the merge statistics).
//
// Written once for both: the walk (closure_walk, over a sequence accessor: OwnerSeq for the build, TourSeq for the merge) with claim_long,
// count_list and rank_store around it on the device; on the host the count -> CSR tail (write_lists) and write_records.  The text scan of the
// extraction, the wave helpers, DevBuf, with_temp and LapTimer are kmer_dev.hpp's, shared with kcov.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string.h>
#include <rocprim/rocprim.hpp>
#include <string>
#include <unordered_map>
#include <vector>
#include "lmat_internal.hpp"
#include "kmer_dev.hpp"

namespace {

using namespace lmat_dev;   // kmer_dev.hpp: the wave helpers, the two phases of the text scan, DevBuf, with_temp, LapTimer

constexpr u32 kNoNode = 0xFFFFFFFFu;
constexpr u32 kMaxList = 65535;   // the record's count field is 16 bits wide (tax_histo.cpp:258-259)

// counters of one pass (device, 64-bit words)
enum { C_CURSOR = 0, C_OVERFLOW, C_WINDOWS, C_DROPPED, C_SINGLETONS, C_ENTRIES, C_LONGEST, C_TOOLONG, C_LONG_RUNS, C_LONG_ENTRIES, C_N };

struct ExtractArgs {
    const uint8_t* buf;      // chunk bytes: buf[kLead + i] = text[chunk_lo + i]; every wave's 1024-byte window is allocated and filled
    u64 chunk_lo;            // text position of buf[kLead]
    u32 chunk_len;           // window ends of this chunk: text[chunk_lo .. chunk_lo + chunk_len)
    const u64* rec_start;    // [n_rec] text position of the first base of every record, ascending
    const u32* rec_owner;    // [n_rec]
    u32 n_rec;
    int k, prefix_bits, owner_bits;   // owner_bits >= 0: key = k-mer << owner_bits | owner; -1: separate arrays
    int flag_bits;           // 1: one more bit below the owner, 0 for a pair from text (id mode with tax_histo inputs, whose pairs carry 1)
    u32 pass;
    u64* keys;
    u32* vals;
    u64 cap;
    u64* counters;
};

// Every wave covers kSpan consecutive window ends.  Phase 1 (pack_span): the wave's 1024-byte window packed into LDS.  Phase 2: lane l
// of step s takes the window that ends at byte 32 + 64 s + l (window_kmer).  Both phases are kmer_dev.hpp's, shared with kcov.hip.
__global__ __launch_bounds__(64 * kWavesPerBlock) void extract_kernel(ExtractArgs a) {
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
    const u64 kmask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1);
    // the records this wave's span can touch
    u32 rlo, rhi;
    span_records(a.rec_start, a.n_rec, a.chunk_lo + wbase, a.chunk_lo + wbase + kSpan - 1, rlo, rhi);
    u64 n_windows = 0;
    for (int step = 0; step * 64 < kSpan; ++step) {
        const u32 q = step * 64 + lane;            // window end within the span
        const u32 t = q + kLead;                   // ... as a byte of the wave's window
        bool emit = false;
        u64 canon = 0;
        if (q < (u32)kSpan && wbase + q < a.chunk_len) {
            if (window_kmer(s_word[wv], s_inv[wv], s_last[wv], t, k, kmask, canon)) {
                emit = a.prefix_bits == 0 || (u32)(canon >> (2 * k - a.prefix_bits)) == a.pass;
                n_windows += 1;
            }
        }
        const u64 bal = __ballot(emit);
        if (bal) {
            const u32 cnt = __popcll(bal);
            u64 base = 0;
            if (lane == 0) base = atomicAdd(&a.counters[C_CURSOR], (u64)cnt);
            base = __shfl(base, 0);
            if (base + cnt > a.cap) {
                if (lane == 0) atomicMax(&a.counters[C_OVERFLOW], 1ull);   // the pass is repeated or refused by the host, never cut short
            } else if (emit) {
                const u64 pos = a.chunk_lo + wbase + q;
                const u32 owner = a.rec_owner[record_at(a.rec_start, rlo, rhi, pos)];
                const u64 dst = base + __popcll(bal & ((1ull << lane) - 1));
                if (a.owner_bits >= 0) a.keys[dst] = ((canon << a.owner_bits) | owner) << a.flag_bits;
                else { a.keys[dst] = canon; a.vals[dst] = owner << a.flag_bits; }
            }
        }
    }
    n_windows = wave_sum(n_windows);
    if (lane == 0 && n_windows) atomicAdd(&a.counters[C_WINDOWS], n_windows);
}

struct Sorted {   // the sorted pairs, either packing
    const u64* keys;
    const u32* vals;
    int owner_bits;
    int flag_bits;   // the source flag below the owner (ExtractArgs)
    __device__ __forceinline__ void get(u64 i, u64& km, u32& ow) const {
        if (owner_bits >= 0) { const u64 x = keys[i] >> flag_bits; km = x >> owner_bits; ow = (u32)(x & ((1ull << owner_bits) - 1)); }
        else { km = keys[i]; ow = vals[i] >> flag_bits; }
    }
    __device__ __forceinline__ bool from_text(u64 i) const { return !(((owner_bits >= 0) ? (u32)keys[i] : vals[i]) & (u32)flag_bits); }
};

// flag[i] = (head of a run of one k-mer) << 32 | (first of equal (k-mer, owner) pairs)
__global__ __launch_bounds__(256) void seg_flag_kernel(Sorted s, u64 n, u64* flag) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 km, pk = 0;
    u32 ow, po = 0;
    s.get(i, km, ow);
    if (i) s.get(i - 1, pk, po);
    const bool head = i == 0 || km != pk;
    const bool distinct = head || ow != po;
    flag[i] = ((u64)head << 32) | (u64)distinct;
}

// pos = exclusive scan of flag: the distinct pairs are compacted, run_start[r] = index of run r's first distinct pair
__global__ __launch_bounds__(256) void seg_scatter_kernel(Sorted s, u64 n, const u64* flag, const u64* pos, u64* d_kmer, u32* d_owner,
                                                            u32* run_start, u64* totals) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 f = flag[i], p = pos[i];
    const u32 j = (u32)p, r = (u32)(p >> 32);
    if (f & 1ull) {
        u64 km;
        u32 ow;
        s.get(i, km, ow);
        d_kmer[j] = km;
        d_owner[j] = ow;
    }
    if (f >> 32) run_start[r] = j;
    if (i == n - 1) {
        const u32 D = j + (u32)(f & 1ull), R = r + (u32)(f >> 32);
        run_start[R] = D;
        totals[0] = D;
        totals[1] = R;
    }
}

__global__ __launch_bounds__(256) void run_kmer_kernel(const u64* d_kmer, const u32* run_start, u32 R, u64* out) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) out[r] = d_kmer[run_start[r]];
}

// ------------------------------------------------------------------------- what the closure and the union kernel share
struct TreeArgs {
    const u32* parent;       // [n_nodes] dense; the root is its own parent
    const u32* depth;        // [n_nodes]
    const u32* node_tid;     // [n_nodes] ascending with the dense index
};

struct LongArgs {            // write pass: lists of more than 64 entries, unsorted, to be sorted by segment
    u32* tmp;
    u32* begin;              // [n_long] segment bounds in tmp
    u32* end;
    u32* run;                // [n_long] the run of the segment
};

// depth-levelled parent walk
__device__ __forceinline__ u32 lca2(const TreeArgs& t, u32 a, u32 b) {
    u32 da = t.depth[a], db = t.depth[b];
    while (da > db) { a = t.parent[a]; --da; }
    while (db > da) { b = t.parent[b]; --db; }
    while (a != b) { a = t.parent[a]; b = t.parent[b]; }
    return a;
}

// The closure of a sequence of n nodes in Euler-tour order, by the whole wave, 64 elements a step: the first element walks up to and including
// the LCA of the first and the last, every later one up to -- not including -- its LCA with the element before it; an element the sequence
// reports as a repeat of the one before it adds nothing.  Returns the length of the closure; the write pass stores its taxids, unordered,
// from dst on.  distinct = the elements that are no repeats.
template <bool WRITE, class Seq>
__device__ __forceinline__ u32 closure_walk(const TreeArgs& t, const Seq& seq, u32 n, u32 lane, u32* dst, u32& distinct) {
    const u32 top = lca2(t, seq.node(0), seq.node(n - 1));
    u32 total = 0;
    distinct = 0;
    for (u32 base = 0; base < n; base += 64) {
        const u32 j = base + lane;
        u32 node = 0, len = 0;
        bool fresh = false;
        if (j < n) {
            node = seq.node(j);
            fresh = j == 0 || !seq.repeat(j);
            if (j == 0) len = t.depth[node] - t.depth[top] + 1;
            else if (fresh) len = t.depth[node] - t.depth[lca2(t, seq.node(j - 1), node)];
        }
        u32 incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 o = __shfl_up(incl, d);
            if ((int)lane >= d) incl += o;
        }
        if (WRITE) {
            u32 at = total + incl - len;
            for (u32 x = node, i = 0; i < len; ++i, x = t.parent[x]) dst[at++] = t.node_tid[x];
        }
        total += __shfl(incl, 63);
        distinct += __popcll(__ballot(fresh));
    }
    return total;
}

// write pass: the segment of the side buffer for run rr's list of n > 64 entries, claimed by lane 0 with the two long-list counters
__device__ __forceinline__ u32* claim_long(const LongArgs& lg, u64* counters, u32 rr, u32 n, u32 lane) {
    u32 at = 0;
    if (lane == 0) {
        const u32 slot = (u32)atomicAdd(&counters[C_LONG_RUNS], 1ull);
        at = (u32)atomicAdd(&counters[C_LONG_ENTRIES], (u64)n);
        lg.begin[slot] = at;
        lg.end[slot] = at + n;
        lg.run[slot] = rr;
    }
    return lg.tmp + __shfl(at, 0);
}

// count pass, one lane: the length of a list the wave made, and what the pass's counters say about it
__device__ __forceinline__ void count_list(u64* cnt, u64* counters, u32 rr, u32 total) {
    cnt[rr] = total;
    atomicAdd(&counters[C_ENTRIES], (u64)total);
    atomicMax(&counters[C_LONGEST], (u64)total);
    if (total == 1) atomicAdd(&counters[C_SINGLETONS], 1ull);
    if (total > kMaxList) atomicMax(&counters[C_TOOLONG], (u64)total);
    if (total > 64) { atomicAdd(&counters[C_LONG_RUNS], 1ull); atomicAdd(&counters[C_LONG_ENTRIES], (u64)total); }
}

// write pass: the n <= 64 distinct entries of the wave's stage in ascending order to out; the rank of one is the number of smaller ones
__device__ __forceinline__ void rank_store(const u32* stage, u32 n, u32 lane, u32* out) {
    wave_sync();
    const u32 v = lane < n ? stage[lane] : 0xFFFFFFFFu;
    u32 rank = 0;
    for (u32 t = 0; t < n; ++t) rank += stage[t] < v ? 1u : 0u;
    if (lane < n) out[rank] = v;
    wave_sync();
}

// ------------------------------------------------------------------------------------------------------------- the build
struct ClosureArgs {
    u32 R;
    const u32* run_start;    // [R + 1]
    const u32* d_owner;      // distinct owners of every run, in Euler-tour order, unknown owners last
    u32 n_known;             // owner indices below this are tree nodes
    const u32* owner_node;   // [n_owner] dense node index
    TreeArgs tree;
    u64* cnt;                // count pass: [R] list length
    const u64* off;          // write pass: [R + 1]
    u32* tids;               // write pass: the CSR
    LongArgs lng;
    u64* counters;
};

struct OwnerSeq {            // the owners of one run the tree knows: distinct, in tour order
    const u32* owner_node;
    const u32* owner;
    __device__ __forceinline__ u32 node(u32 j) const { return owner_node[owner[j]]; }
    __device__ __forceinline__ bool repeat(u32) const { return false; }
};

// One run per lane.  Runs whose list is one taxid (a single owner, or a single owner the tree knows) and runs without a known
// owner are settled by their lane; the others are taken one after the other by the whole wave, owners on the lanes (several
// per lane beyond 64 owners).
template <bool WRITE>
__global__ __launch_bounds__(64 * kWavesPerBlock) void closure_kernel(ClosureArgs a) {
    __shared__ u32 s_stage[kWavesPerBlock][64];
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u64 r64 = ((u64)blockIdx.x * kWavesPerBlock + wv) * 64 + lane;
    const bool active = r64 < a.R;
    const u32 r = active ? (u32)r64 : 0;
    u32 s = 0, e = 0;
    int kind = -1;   // 0 dropped, 1 one taxid, 2 closure
    if (active) {
        s = a.run_start[r];
        e = a.run_start[r + 1];
        const u32 first = a.d_owner[s];
        if (first >= a.n_known) kind = 0;
        else if (e - s == 1 || a.d_owner[s + 1] >= a.n_known) kind = 1;
        else kind = 2;
        if (kind == 1 && WRITE) a.tids[a.off[r]] = a.tree.node_tid[a.owner_node[first]];
        if (kind < 2 && !WRITE) a.cnt[r] = (u64)kind;
    }
    if (!WRITE) {
        const u32 n0 = __popcll(__ballot(kind == 0)), n1 = __popcll(__ballot(kind == 1));
        if (lane == 0) {
            if (n0) atomicAdd(&a.counters[C_DROPPED], (u64)n0);
            if (n1) { atomicAdd(&a.counters[C_SINGLETONS], (u64)n1); atomicAdd(&a.counters[C_ENTRIES], (u64)n1); atomicMax(&a.counters[C_LONGEST], 1ull); }
        }
    }
    u64 multi = __ballot(kind == 2);
    while (multi) {
        const int b = __ffsll((long long)multi) - 1;
        multi &= multi - 1;
        const u32 rs = __shfl(s, b), re = __shfl(e, b), rr = __shfl(r, b);
        // the owners the tree knows are a prefix of the run
        u32 g = 0;
        for (u32 base = rs; base < re; base += 64) {
            const u32 i = base + lane;
            const u64 ok = __ballot(i < re && a.d_owner[i] < a.n_known);
            g += __popcll(ok);
            if (ok != ~0ull) break;
        }
        u32 n = 0;
        u32* dst = WRITE ? &s_stage[wv][0] : nullptr;
        if (WRITE) {
            n = (u32)(a.off[rr + 1] - a.off[rr]);
            if (n > 64) dst = claim_long(a.lng, a.counters, rr, n, lane);
        }
        u32 distinct;
        const u32 total = closure_walk<WRITE>(a.tree, OwnerSeq{a.owner_node, a.d_owner + rs}, g, lane, dst, distinct);
        if (!WRITE) {
            if (lane == 0) count_list(a.cnt, a.counters, rr, total);
        } else if (n <= 64) rank_store(&s_stage[wv][0], n, lane, a.tids + a.off[rr]);
    }
}

// the sorted long lists back into their places in the CSR
__global__ __launch_bounds__(256) void long_copy_kernel(const u32* sorted, const u32* long_begin, const u32* long_end, const u32* long_run,
                                                         const u64* off, u32* tids) {
    const u32 q = blockIdx.x;
    const u32 b = long_begin[q], n = long_end[q] - b;
    u32* dst = tids + off[long_run[q]];
    for (u32 i = threadIdx.x; i < n; i += blockDim.x) dst[i] = sorted[b + i];
}

// ------------------------------------------------------------------------------------------------------------ id-set mode
// No tree and no closure (lmat_genebuild_create): the list of a run is the ids of its distinct owners.  Owner indices are the ranks of the
// ids among all ids of the run's inputs, so the owners of a run arrive in ascending id order and the list is id_of[owner] in order.
struct IdListArgs {
    u32 R;
    const u32* run_start;    // [R + 1]
    const u32* d_owner;      // distinct owners of every run, ascending
    const u32* id_of;        // [n_owner] ascending
    u64* cnt;                // count pass: [R]
    const u64* off;          // write pass: [R + 1]
    u32* tids;               // write pass: the CSR
    u64* counters;
};

// One run per lane.  Count: the number of distinct pairs of the run.  Write: runs of up to 64 entries are written by their lanes, the longer
// ones one after the other by the whole wave.  Nothing here feeds the side buffers of the long lists: the order is there already.
template <bool WRITE>
__global__ __launch_bounds__(64 * kWavesPerBlock) void idlist_kernel(IdListArgs a) {
    const u32 lane = lane_id();
    const u64 r64 = ((u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * 64 + lane;
    const bool active = r64 < a.R;
    const u32 r = active ? (u32)r64 : 0;
    u32 s = 0, n = 0;
    if (active) { s = a.run_start[r]; n = a.run_start[r + 1] - s; }
    if (!WRITE) {
        if (active) a.cnt[r] = n;
        const u64 entries = wave_sum<u64>(n);
        const u32 longest = wave_max<u32>(n);
        const u32 singles = __popcll(__ballot(n == 1));
        if (lane == 0 && entries) {
            atomicAdd(&a.counters[C_ENTRIES], entries);
            atomicMax(&a.counters[C_LONGEST], (u64)longest);
            if (singles) atomicAdd(&a.counters[C_SINGLETONS], (u64)singles);
            if (longest > kMaxList) atomicMax(&a.counters[C_TOOLONG], (u64)longest);
        }
        return;
    }
    u64 o = 0;
    if (active) {
        o = a.off[r];
        if (n <= 64) for (u32 i = 0; i < n; ++i) a.tids[o + i] = a.id_of[a.d_owner[s + i]];
    }
    u64 wide = __ballot(n > 64);
    while (wide) {
        const int b = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const u32 rs = __shfl(s, b), rn = __shfl(n, b);
        const u64 ro = ((u64)__shfl((u32)(o >> 32), b) << 32) | __shfl((u32)o, b);
        for (u32 i = lane; i < rn; i += 64) a.tids[ro + i] = a.id_of[a.d_owner[rs + i]];
    }
}

// has_text[r] = 1 when a pair of run r came from text (its flag bit is 0); flag / pos are those of seg_flag_kernel and its scan
__global__ __launch_bounds__(256) void text_runs_kernel(Sorted s, u64 n, const u64* flag, const u64* pos, u32* has_text) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && s.from_text(i)) has_text[(u32)(pos[i] >> 32) + (u32)(flag[i] >> 32) - 1] = 1u;
}

// ---------------------------------------------------------------------------------------------- merge of tax_histo inputs
// counters of the union, behind the C_* words of the same array
enum { M_EMPTY = C_N, M_ONE, M_MERGED, M_GROWN, M_BIG_RUNS, M_BIG_ENTRIES, M_TOTAL };
constexpr u32 kSmall = 0xFFFFFFFFu;   // aux of a run with several sources whose gathered entries fit the wave

__global__ __launch_bounds__(256) void iota_kernel(u32* v, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

// index of taxid t in the ascending node_tid (every taxid that gets here is a node of the tree)
__device__ __forceinline__ u32 node_of_tid(const u32* node_tid, u32 n_nodes, u32 t) {
    u32 lo = 0, hi = n_nodes;
    while (hi - lo > 1) { const u32 m = (lo + hi) >> 1; if (node_tid[m] <= t) lo = m; else hi = m; }
    return lo;
}

__global__ __launch_bounds__(256) void tid_to_node_kernel(const u32* tids, u64 n, const u32* node_tid, u32 n_nodes, u32* out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = node_of_tid(node_tid, n_nodes, tids[i]);
}

// The pass's result from the genomes as one more source: record rec_base + r, entries from ent_base on.  A run without a known owner has
// no list: its key gets the bit above the k-mer, the sort puts it behind all others and the host cuts them off.
__global__ __launch_bounds__(256) void genome_source_kernel(u32 R, const u64* g_kmer, const u64* g_off, u32 rec_base, u32 ent_base, u32 src, int src_bits,
                                                             int key_bits, u64* keys, u32* rec_off, u64* counters) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    bool empty = false;
    if (r < R) {
        const u64 e = g_off[r + 1];
        empty = e == g_off[r];
        keys[rec_base + r] = (g_kmer[r] << src_bits) | src | (empty ? 1ull << key_bits : 0ull);
        rec_off[rec_base + r + 1] = ent_base + (u32)e;
    }
    const u32 n = __popcll(__ballot(empty));
    if (n && lane_id() == 0) atomicAdd(&counters[M_EMPTY], (u64)n);
}

__global__ __launch_bounds__(256) void mseg_flag_kernel(const u64* keys, u32 n, int src_bits, u32* flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || (keys[i] >> src_bits) != (keys[i - 1] >> src_bits)) ? 1u : 0u;
}

// pos = exclusive scan of flag; run_start[r] = first sorted record of run r, run_start[R] = n
__global__ __launch_bounds__(256) void mseg_scatter_kernel(const u32* flag, const u32* pos, u32 n, u32* run_start, u64* totals) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) run_start[pos[i]] = i;
    if (i == n - 1) {
        const u32 R = pos[i] + flag[i];
        run_start[R] = n;
        totals[0] = R;
    }
}

__global__ __launch_bounds__(256) void mrun_kmer_kernel(const u64* keys, const u32* run_start, u32 R, int src_bits, u64 kmask, u64* out) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) out[r] = (keys[run_start[r]] >> src_bits) & kmask;
}

struct UnionArgs {
    u32 R;
    const u32* run_start;    // [R + 1] into rec
    const u32* rec;          // sorted: index of the record in rec_off
    const u32* rec_off;      // [records + 1] into ent
    const u32* ent;          // dense node index of every stored entry
    const u32* tin;          // [n_nodes] Euler-tour entry time of the node
    const u32* node_at;      // [n_nodes] its inverse
    TreeArgs tree;
    u32* aux;               // [R] runs with several sources: kSmall, or the slot of the side-buffer segment
    u32* big_run;            // [slots]
    u32* big_begin;          // [slots] segment of the gathered tour indices
    u32* big_end;
    const u32* big_sorted;
    u64* cnt;                // [R]
    const u64* off;          // write pass: [R + 1]
    u32* tids;
    LongArgs lng;
    u64* counters;
};

struct TourSeq {             // tour indices in order; equal neighbours are one entry
    const u32* node_at;
    const u32* tour;
    __device__ __forceinline__ u32 node(u32 j) const { return node_at[tour[j]]; }
    __device__ __forceinline__ bool repeat(u32 j) const { return tour[j] == tour[j - 1]; }
};

// One run per lane.  A run with one source has its list's length (a copy follows); a run with several gets kSmall when the entries of all its
// lists together fit the 64 lanes, else a segment of the side buffer, filled by big_gather_kernel and ordered by rocPRIM's segmented sort.
__global__ __launch_bounds__(256) void union_classify_kernel(UnionArgs a) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = r < a.R;
    u32 ns = 0, G = 0;
    if (active) {
        const u32 s = a.run_start[r], e = a.run_start[r + 1];
        ns = e - s;
        for (u32 i = s; i < e; ++i) { const u32 q = a.rec[i]; G += a.rec_off[q + 1] - a.rec_off[q]; }
    }
    const bool one = active && ns == 1;
    if (one) a.cnt[r] = G;
    if (active && ns > 1) {
        u32 slot = kSmall;
        if (G > 64) {
            slot = (u32)atomicAdd(&a.counters[M_BIG_RUNS], 1ull);
            const u32 at = (u32)atomicAdd(&a.counters[M_BIG_ENTRIES], (u64)G);
            a.big_run[slot] = r;
            a.big_begin[slot] = at;
            a.big_end[slot] = at + G;
        }
        a.aux[r] = slot;
    }
    const u32 n_one = __popcll(__ballot(one)), n_multi = __popcll(__ballot(active && ns > 1)), n_single = __popcll(__ballot(one && G == 1));
    const u32 n_long = __popcll(__ballot(one && G > 64));
    const u64 entries = wave_sum<u64>(one ? G : 0), long_entries = wave_sum<u64>(one && G > 64 ? G : 0);
    const u32 longest = wave_max<u32>(one ? G : 0);
    if (lane_id() == 0) {
        if (n_one) { atomicAdd(&a.counters[M_ONE], (u64)n_one); atomicAdd(&a.counters[C_ENTRIES], entries); atomicMax(&a.counters[C_LONGEST], (u64)longest); }
        if (n_multi) atomicAdd(&a.counters[M_MERGED], (u64)n_multi);
        if (n_single) atomicAdd(&a.counters[C_SINGLETONS], (u64)n_single);
        if (n_long) { atomicAdd(&a.counters[C_LONG_RUNS], (u64)n_long); atomicAdd(&a.counters[C_LONG_ENTRIES], long_entries); }
    }
}

// one block per side-buffer segment: the tour index of every entry of every list of the run
__global__ __launch_bounds__(256) void big_gather_kernel(UnionArgs a, u32* big_tmp) {
    const u32 q = blockIdx.x, r = a.big_run[q];
    u32 at = a.big_begin[q];
    for (u32 i = a.run_start[r]; i < a.run_start[r + 1]; ++i) {
        const u32 rc = a.rec[i], b0 = a.rec_off[rc], n = a.rec_off[rc + 1] - b0;
        for (u32 t = threadIdx.x; t < n; t += blockDim.x) big_tmp[at + t] = a.tin[a.ent[b0 + t]];
        at += n;
    }
}

// One run per lane.  One source: the list is copied -- by the lane while it ascends (a list this builder wrote), else by the wave, ranked; beyond
// 64 entries through the side buffer of the long lists.  Several sources: the wave orders the entries of all lists by tour index (in LDS, or
// the segment sorted beforehand), equal neighbours are one entry, and closure_walk gives the closure in disjoint pieces.
template <bool WRITE>
__global__ __launch_bounds__(64 * kWavesPerBlock) void union_kernel(UnionArgs a) {
    __shared__ u32 s_stage[kWavesPerBlock][64];   // gathered tour indices, later the list to be ranked
    __shared__ u32 s_seq[kWavesPerBlock][64];     // tour indices in order
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u64 r64 = ((u64)blockIdx.x * kWavesPerBlock + wv) * 64 + lane;
    const bool active = r64 < a.R;
    const u32 r = active ? (u32)r64 : 0;
    u32 s = 0, e = 0;
    bool wave_job = false;
    if (active) {
        s = a.run_start[r];
        e = a.run_start[r + 1];
        if (e - s > 1) wave_job = true;
        else if (WRITE) {
            const u32 q = a.rec[s], b0 = a.rec_off[q], n = a.rec_off[q + 1] - b0;
            if (n > 64) wave_job = true;
            else {
                u32* dst = a.tids + a.off[r];
                u32 prev = 0;
                for (u32 i = 0; i < n; ++i) {
                    const u32 x = a.ent[b0 + i];
                    if (i && x <= prev) { wave_job = true; break; }
                    dst[i] = a.tree.node_tid[x];
                    prev = x;
                }
            }
        }
    }
    u64 jobs = __ballot(wave_job);
    while (jobs) {
        const int b = __ffsll((long long)jobs) - 1;
        jobs &= jobs - 1;
        const u32 rs = __shfl(s, b), re = __shfl(e, b), rr = __shfl(r, b);
        u32 n = 0;
        u32* dst = &s_stage[wv][0];
        if (WRITE) {
            n = (u32)(a.off[rr + 1] - a.off[rr]);
            if (n > 64) dst = claim_long(a.lng, a.counters, rr, n, lane);
        }
        if (re - rs == 1) {   // write pass only: the copy of a list that does not ascend or is long
            const u32 q = a.rec[rs], b0 = a.rec_off[q];
            for (u32 i = lane; i < n; i += 64) dst[i] = a.tree.node_tid[a.ent[b0 + i]];
        } else {
            const u32 slot = a.aux[rr];
            const u32* seq;
            u32 G;
            if (slot == kSmall) {
                G = 0;
                for (u32 i = rs; i < re; ++i) {
                    const u32 q = a.rec[i], b0 = a.rec_off[q], m = a.rec_off[q + 1] - b0;
                    if (lane < m) s_stage[wv][G + lane] = a.tin[a.ent[b0 + lane]];   // G + m <= 64: union_classify summed the same lengths
                    G += m;
                }
                wave_sync();
                const u32 v = lane < G ? s_stage[wv][lane] : 0xFFFFFFFFu;
                u32 rank = 0;
                for (u32 t = 0; t < G; ++t) { const u32 o = s_stage[wv][t]; rank += (o < v || (o == v && t < lane)) ? 1u : 0u; }
                wave_sync();   // the stage is free for the list from here on
                if (lane < G) s_seq[wv][rank] = v;
                wave_sync();
                seq = &s_seq[wv][0];
            } else {
                seq = a.big_sorted + a.big_begin[slot];
                G = a.big_end[slot] - a.big_begin[slot];
            }
            u32 distinct;
            const u32 total = closure_walk<WRITE>(a.tree, TourSeq{a.node_at, seq}, G, lane, dst, distinct);
            if (!WRITE && lane == 0) {
                count_list(a.cnt, a.counters, rr, total);
                if (total > distinct) atomicAdd(&a.counters[M_GROWN], 1ull);
            }
        }
        if (WRITE && n <= 64) rank_store(&s_stage[wv][0], n, lane, a.tids + a.off[rr]);
    }
}

// hist[node] += 1 for every entry of the final lists: the number of records whose list holds the taxid
__global__ __launch_bounds__(256) void hist_kernel(const u32* tids, u64 n, const u32* node_tid, u32 n_nodes, u64* hist) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&hist[node_of_tid(node_tid, n_nodes, tids[i])], 1ull);
}

// ------------------------------------------------------------------------------------------------------------------ host
struct LongBufs {   // the side buffers of the lists beyond 64 entries
    DevBuf tmp, sorted, begin, end, run;
    LongArgs args() const { return LongArgs{tmp.as<u32>(), begin.as<u32>(), end.as<u32>(), run.as<u32>()}; }
};

}  // namespace

struct lmat_build {
    lmat_ctx* ctx = nullptr;
    int k = 0;
    bool id_mode = false;                // lmat_genebuild_create: no tree; node_tid is the ascending ids of all inputs, set by every run
    std::string err;
    // taxonomy, dense: index = rank of the taxid among the tree's node ids
    std::vector<u32> node_tid, parent, depth, tin;
    std::unordered_map<u32, u32> node_of;
    // input
    std::vector<uint8_t> text;          // sequences, one '\n' behind each record
    std::vector<u64> rec_start;
    std::vector<u32> rec_taxid;
    u64 bases = 0;
    // options
    u64 budget = 0;
    int prefix_bits = -1;
    u32 chunk_bases = 0;
    // result
    bool done = false;
    std::vector<u64> kmers;
    std::vector<u64> list_off;           // [records + 1]
    std::vector<u32> tids;
    lmat_build_stats stats;
    // tax_histo files to be merged in (lmat_build_add_taxhisto): parsed when added, lists as dense node indices in file order
    struct Input {
        std::string fn;
        std::vector<u64> kmers;          // strictly ascending
        std::vector<u64> off;            // [records + 1]
        std::vector<u32> nodes;          // id mode: the ids as stored
    };
    std::vector<Input> inputs;
    lmat_merge_stats mstats;
    std::vector<u64> node_counts;        // [n_nodes] result records whose list holds the node
};

namespace {

int berr(lmat_build* b, int code, const std::string& msg) {
    b->err = msg;
    return code;
}

#define BHIP(b, call)                                                                            \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) return berr(b, e__ == hipErrorOutOfMemory ? LMAT_E_NOMEM : LMAT_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// "id nchild child.. parent" / name line pairs behind three header lines (TaxTree.hpp:24-57), as taxonomy.cpp reads them
int load_tree(lmat_build* b, const char* fn) {
    FILE* f = fopen(fn, "r");
    if (!f) return berr(b, LMAT_E_IO, std::string("failed to open ") + fn + " for reading");
    char* line = nullptr;
    size_t cap = 0;
    for (int i = 0; i < 3; ++i) if (getline(&line, &cap, f) < 0) break;
    std::vector<std::pair<u32, u32>> edges;
    while (getline(&line, &cap, f) >= 0) {
        u32 first = 0, last = 0;
        int n = 0;
        for (char* p = line;;) {
            char* e = nullptr;
            const unsigned long long v = strtoull(p, &e, 10);
            if (e == p) break;
            if (!n++) first = (u32)v;
            last = (u32)v;
            p = e;
        }
        if (n >= 3) edges.push_back(std::make_pair(first, last));
        else if (n != 0) { free(line); fclose(f); return berr(b, LMAT_E_IO, "malformed taxonomy node line"); }
        if (getline(&line, &cap, f) < 0) break;  // name
    }
    free(line);
    fclose(f);
    if (edges.empty()) return berr(b, LMAT_E_IO, std::string("no taxonomy nodes in ") + fn);
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end(), [](const std::pair<u32, u32>& x, const std::pair<u32, u32>& y) { return x.first == y.first; }), edges.end());
    const u32 n = (u32)edges.size();
    b->node_tid.resize(n);
    for (u32 i = 0; i < n; ++i) { b->node_tid[i] = edges[i].first; b->node_of[edges[i].first] = i; }
    b->parent.resize(n);
    u32 roots = 0;
    for (u32 i = 0; i < n; ++i) {
        auto it = b->node_of.find(edges[i].second);
        if (it == b->node_of.end()) return berr(b, LMAT_E_TAXONOMY, "failed to find parent TaxNode " + std::to_string(edges[i].second) + " of taxid " + std::to_string(edges[i].first));
        b->parent[i] = it->second;
        if (it->second == i) ++roots;
    }
    if (roots != 1) return berr(b, LMAT_E_TAXONOMY, "the taxonomy has " + std::to_string(roots) + " roots; the LCA closure needs exactly one");
    // depth, children, Euler-tour entry times
    std::vector<std::vector<u32>> children(n);
    u32 root = 0;
    for (u32 i = 0; i < n; ++i) {
        if (b->parent[i] == i) root = i;
        else children[b->parent[i]].push_back(i);
    }
    b->depth.assign(n, 0);
    b->tin.assign(n, 0xFFFFFFFFu);
    std::vector<std::pair<u32, size_t>> st;
    u32 clock = 0;
    st.push_back(std::make_pair(root, (size_t)0));
    b->tin[root] = clock++;
    while (!st.empty()) {
        auto& top = st.back();
        if (top.second < children[top.first].size()) {
            const u32 ch = children[top.first][top.second++];
            b->tin[ch] = clock++;
            b->depth[ch] = b->depth[top.first] + 1;
            st.push_back(std::make_pair(ch, (size_t)0));
        } else st.pop_back();
    }
    if (clock != n) return berr(b, LMAT_E_TAXONOMY, "cycle in taxonomy: " + std::to_string(n - clock) + " nodes do not hang off the root");
    return LMAT_OK;
}

void add_record(lmat_build* b, u32 taxid) {
    b->rec_start.push_back(b->text.size());
    b->rec_taxid.push_back(taxid);
}

int run_build(lmat_build* b, int pb_forced, int pb_start, bool& retry);

// Record i of an input -- of a parsed file, or of a loaded database (lmat_build_add_db) -- into `in`: its n taxids (4 bytes each, unaligned)
// as dense node indices in stored order; every one must be in the tree and none may repeat.  A record without a list carries nothing.
int input_record(lmat_build* b, lmat_build::Input& in, const std::string& name, u64 i, u64 km, const uint8_t* tid_bytes, u32 n, std::vector<u32>& chk) {
    if (!n) return LMAT_OK;
    const size_t at = in.nodes.size();
    in.nodes.resize(at + n);
    for (u32 j = 0; j < n; ++j) {
        u32 t;
        memcpy(&t, tid_bytes + 4 * (size_t)j, 4);
        auto it = b->node_of.find(t);
        if (it == b->node_of.end()) {
            in.nodes.resize(at);
            return berr(b, LMAT_E_TAXONOMY, name + ": taxid " + std::to_string(t) + " of record " + std::to_string(i) + " is not in the taxonomy tree");
        }
        in.nodes[at + j] = it->second;
    }
    if (n > 1) {
        chk.assign(in.nodes.begin() + at, in.nodes.end());
        std::sort(chk.begin(), chk.end());
        auto dup = std::adjacent_find(chk.begin(), chk.end());
        if (dup != chk.end()) return berr(b, LMAT_E_IO, name + ": taxid " + std::to_string(b->node_tid[*dup]) + " repeated in the list of record " + std::to_string(i));
    }
    in.kmers.push_back(km);
    in.off.push_back(in.nodes.size());
    return LMAT_OK;
}

// id mode: the n ids as stored; none is looked up, none may be 0 or repeat
int input_record_ids(lmat_build* b, lmat_build::Input& in, const std::string& name, u64 i, u64 km, const uint8_t* tid_bytes, u32 n, std::vector<u32>& chk) {
    if (!n) return LMAT_OK;
    chk.resize(n);
    memcpy(chk.data(), tid_bytes, 4 * (size_t)n);
    in.nodes.insert(in.nodes.end(), chk.begin(), chk.end());
    std::sort(chk.begin(), chk.end());
    if (chk[0] == 0) return berr(b, LMAT_E_IO, name + ": id 0 in the list of record " + std::to_string(i));
    auto dup = std::adjacent_find(chk.begin(), chk.end());
    if (dup != chk.end()) return berr(b, LMAT_E_IO, name + ": id " + std::to_string(*dup) + " repeated in the list of record " + std::to_string(i));
    in.kmers.push_back(km);
    in.off.push_back(in.nodes.size());
    return LMAT_OK;
}

int any_record(lmat_build* b, lmat_build::Input& in, const std::string& name, u64 i, u64 km, const uint8_t* tid_bytes, u32 n, std::vector<u32>& chk) {
    return b->id_mode ? input_record_ids(b, in, name, i, km, tid_bytes, n, chk) : input_record(b, in, name, i, km, tid_bytes, n, chk);
}

// KmerFileMetaData.cpp:16-31 + tax_histo.cpp:250-266, as dbbuild.cpp reads it -- but strict: the header's count of records must be there
int parse_taxhisto(lmat_build* b, const char* fn, lmat_build::Input& in) {
    const std::string name(fn);
    FILE* f = fopen(fn, "rb");
    if (!f) return berr(b, LMAT_E_IO, "failed to open " + name + " for reading");
    std::vector<uint8_t> buf;
    fseek(f, 0, SEEK_END);
    const long fsz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (fsz > 0) buf.resize((size_t)fsz);
    const bool rd = fsz >= 0 && (buf.empty() || fread(buf.data(), 1, buf.size(), f) == buf.size());
    fclose(f);
    if (!rd) return berr(b, LMAT_E_IO, "read error on " + name);
    if (buf.size() < 29) return berr(b, LMAT_E_IO, name + ": truncated tax_histo header");
    uint32_t version, klen;
    uint64_t count, test;
    memcpy(&count, &buf[4], 8);
    memcpy(&test, &buf[12], 8);
    memcpy(&version, &buf[20], 4);
    memcpy(&klen, &buf[25], 4);
    if (test != ~0ull) return berr(b, LMAT_E_IO, name + ": kmer data file is invalid; should have read 64 1s, but didn't");
    if (version != 999 || buf[24] != 'N') return berr(b, LMAT_E_IO, name + ": not a tax_histo file (version/location flag)");
    if ((int)klen != b->k) return berr(b, LMAT_E_ARG, name + ": k-mer length " + std::to_string(klen) + " of the file differs from the builder's " + std::to_string(b->k));
    in.fn = name;
    in.off.assign(1, 0);
    size_t pos = 29;
    const size_t end = buf.size();
    std::vector<u32> chk;
    u64 prev = 0;
    for (u64 i = 0; i < count; ++i) {
        if (end - pos < 10) return berr(b, LMAT_E_IO, name + ": truncated tax_histo record " + std::to_string(i) + " of " + std::to_string(count));
        u64 km;
        uint16_t n;
        memcpy(&km, &buf[pos], 8);
        memcpy(&n, &buf[pos + 8], 2);
        pos += 10;
        if (km >> (2 * b->k)) return berr(b, LMAT_E_IO, name + ": k-mer wider than 2k bits in record " + std::to_string(i));
        if (i && km <= prev) return berr(b, LMAT_E_IO, name + ": k-mers not strictly ascending at record " + std::to_string(i));
        prev = km;
        if (end - pos < (size_t)n * 4) return berr(b, LMAT_E_IO, name + ": truncated taxid list in record " + std::to_string(i));
        if (const int rc = any_record(b, in, name, i, km, &buf[pos], n, chk)) return rc;
        pos += (size_t)n * 4;
        if ((i + 1) % 1500 == 0) {
            if (end - pos < 8 || memcmp(&buf[pos], &test, 8) != 0) return berr(b, LMAT_E_IO, name + ": tax_histo sanity word missing after record " + std::to_string(i));
            pos += 8;
        }
    }
    if (pos != end) return berr(b, LMAT_E_IO, name + ": " + std::to_string(end - pos) + " bytes behind the last record");
    return LMAT_OK;
}

// The result in the file format: KmerFileMetaData.cpp:16-31 with tax_histo's version; lists are written in ascending taxid order (the
// reference writes them in unordered_map iteration order; readers do not rely on either).  False when a write failed.
bool write_records(FILE* f, const lmat_build* b) {
    const uint32_t data_start = 29, version = 999, klen = (uint32_t)b->k;
    const uint64_t count = b->kmers.size(), sanity = ~0ull;
    const char loc = 'N';
    bool ok = fwrite(&data_start, 4, 1, f) == 1 && fwrite(&count, 8, 1, f) == 1 && fwrite(&sanity, 8, 1, f) == 1 &&
              fwrite(&version, 4, 1, f) == 1 && fwrite(&loc, 1, 1, f) == 1 && fwrite(&klen, 4, 1, f) == 1;
    for (u64 i = 0; i < count && ok; ++i) {
        const u64 n = b->list_off[i + 1] - b->list_off[i];
        const uint16_t n16 = (uint16_t)n;
        ok = fwrite(&b->kmers[i], 8, 1, f) == 1 && fwrite(&n16, 2, 1, f) == 1 && fwrite(&b->tids[b->list_off[i]], 4, n, f) == n;
        if (ok && (i + 1) % 1500 == 0) ok = fwrite(&sanity, 8, 1, f) == 1;
    }
    return ok;
}

}  // namespace

extern "C" {

int lmat_build_create(lmat_ctx* ctx, int k, const char* tree_fn, lmat_build** out) {
    if (!out) return LMAT_E_ARG;
    *out = nullptr;
    if (!ctx) return LMAT_E_ARG;
    if (k < 1 || k > 20) return lmat::set_err(ctx, LMAT_E_ARG, "k must be in 1..20 (40-bit keys)");
    if (!tree_fn) return lmat::set_err(ctx, LMAT_E_ARG, "a taxonomy tree file is required");
    lmat_build* b = new lmat_build();
    b->ctx = ctx;
    b->k = k;
    memset(&b->stats, 0, sizeof(b->stats));
    memset(&b->mstats, 0, sizeof(b->mstats));
    const int rc = load_tree(b, tree_fn);
    if (rc) { lmat::set_err(ctx, rc, b->err); delete b; return rc; }
    *out = b;
    return LMAT_OK;
}

int lmat_genebuild_create(lmat_ctx* ctx, int k, lmat_build** out) {
    if (!out) return LMAT_E_ARG;
    *out = nullptr;
    if (!ctx) return LMAT_E_ARG;
    if (k < 1 || k > 20) return lmat::set_err(ctx, LMAT_E_ARG, "k must be in 1..20 (40-bit keys)");
    lmat_build* b = new lmat_build();
    b->ctx = ctx;
    b->k = k;
    b->id_mode = true;
    memset(&b->stats, 0, sizeof(b->stats));
    memset(&b->mstats, 0, sizeof(b->mstats));
    *out = b;
    return LMAT_OK;
}

void lmat_build_destroy(lmat_build* b) { delete b; }
const char* lmat_build_error(const lmat_build* b) { return b ? b->err.c_str() : "null build"; }

int lmat_build_set_options(lmat_build* b, uint64_t device_budget_bytes, int prefix_bits, uint32_t chunk_bases) {
    if (!b) return LMAT_E_ARG;
    if (prefix_bits < -1 || prefix_bits > 2 * b->k || prefix_bits > 24) return berr(b, LMAT_E_ARG, "prefix_bits must be -1 (derive) or 0 .. min(2k, 24)");
    b->budget = device_budget_bytes;
    b->prefix_bits = prefix_bits;
    b->chunk_bases = chunk_bases;
    return LMAT_OK;
}

int lmat_build_add_sequence(lmat_build* b, uint32_t taxid, const uint8_t* ascii, uint64_t n) {
    if (!b || (!ascii && n)) return LMAT_E_ARG;
    if (b->id_mode && taxid == 0) return berr(b, LMAT_E_ARG, "id 0 stands for no gene: ids are 1 .. 2^32-1");
    add_record(b, taxid);
    for (u64 i = 0; i < n; ++i)
        if (ascii[i] != '\n' && ascii[i] != '\r') { b->text.push_back(ascii[i]); ++b->bases; }
    b->text.push_back('\n');
    b->done = false;
    return LMAT_OK;
}

// ">" + decimal taxid headers (kmerPrefixCounter.cpp:121-128); the sequence of a record may span lines
int lmat_build_add_fasta(lmat_build* b, const char* fn) {
    if (!b || !fn) return LMAT_E_ARG;
    FILE* f = fopen(fn, "r");
    if (!f) return berr(b, LMAT_E_IO, std::string("failed to open ") + fn + " for reading");
    char* line = nullptr;
    size_t cap = 0;
    ssize_t len;
    bool open = false;
    u64 lineno = 0;
    int rc = LMAT_OK;
    const size_t text0 = b->text.size(), rec0 = b->rec_start.size();   // id mode: a file that fails adds nothing
    const u64 bases0 = b->bases;
    while ((len = getline(&line, &cap, f)) >= 0) {
        ++lineno;
        while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) --len;
        if (len == 0) continue;
        if (line[0] == '>') {
            if (len < 2 || line[1] < '0' || line[1] > '9') {
                rc = berr(b, LMAT_E_IO, std::string("bad FASTA header (want '>' + decimal taxid) at line ") + std::to_string(lineno) + " of " + fn);
                break;
            }
            if (b->id_mode) {   // 1 .. 2^32-1: 0 is "no gene" in the result records, a wider value would wrap
                const unsigned long long v = strtoull(line + 1, nullptr, 10);
                if (v == 0 || v > 0xFFFFFFFFull) {
                    rc = berr(b, LMAT_E_IO, std::string("gene id out of 1 .. 4294967295 in the FASTA header at line ") + std::to_string(lineno) + " of " + fn);
                    break;
                }
            }
            if (open) b->text.push_back('\n');
            add_record(b, (u32)strtoul(line + 1, nullptr, 10));
            open = true;
        } else {
            if (!open) { rc = berr(b, LMAT_E_IO, std::string("header[0] != '>' for line number ") + std::to_string(lineno) + " of " + fn); break; }
            b->text.insert(b->text.end(), (const uint8_t*)line, (const uint8_t*)line + len);
            b->bases += (u64)len;
        }
    }
    if (open) b->text.push_back('\n');
    free(line);
    fclose(f);
    if (rc && b->id_mode) {
        b->text.resize(text0);
        b->rec_start.resize(rec0);
        b->rec_taxid.resize(rec0);
        b->bases = bases0;
    }
    b->done = false;
    return rc;
}

int lmat_build_add_taxhisto(lmat_build* b, const char* fn) {
    if (!b || !fn) return LMAT_E_ARG;
    if (b->inputs.size() >= 0xFFFFu) return berr(b, LMAT_E_CAPACITY, "at most 65535 tax_histo inputs");
    lmat_build::Input in;
    const int rc = parse_taxhisto(b, fn, in);
    if (rc) return rc;
    b->inputs.push_back(std::move(in));
    b->done = false;
    return LMAT_OK;
}

// A loaded database as an input: exported into host memory now (dbexport.hip), its records then take input_record's path like a file's
int lmat_build_add_db(lmat_build* b, lmat_ctx* src) {
    if (!b || !src) return LMAT_E_ARG;
    if (b->inputs.size() >= 0xFFFFu) return berr(b, LMAT_E_CAPACITY, "at most 65535 tax_histo inputs");
    if (src->gene_mode && !b->id_mode) return berr(b, LMAT_E_ARG, "a gene database holds gene ids, not taxids: it is no input of a merge");
    if (!src->gene_mode && b->id_mode) return berr(b, LMAT_E_ARG, "a taxonomy database holds taxids, not gene ids: it is no input of an id-set build");
    if (src->db_ready && src->dev.k != b->k)
        return berr(b, LMAT_E_ARG, "k-mer length " + std::to_string(src->dev.k) + " of the loaded database differs from the builder's " + std::to_string(b->k));
    lmat_export* x = nullptr;
    int rc = lmat_export_create(src, &x);
    if (rc) return berr(b, rc, lmat_last_error(src));
    lmat_export_stats xs;
    rc = lmat_export_set_options(x, b->budget, -1);
    if (!rc) rc = lmat_export_run(x, nullptr, &xs);
    std::vector<uint64_t> km, off;
    std::vector<uint32_t> td;
    if (!rc) {
        km.resize(xs.records);
        off.resize(xs.records + 1);
        td.resize(std::max<u64>(xs.entries, 1));
        rc = lmat_export_fetch(x, 0, xs.records, km.data(), off.data(), td.data(), td.size());
    }
    if (rc) berr(b, rc, std::string("loaded database: ") + lmat_export_error(x));
    lmat_export_destroy(x);
    if (rc) return rc;
    lmat_build::Input in;
    in.fn = "loaded database";
    in.off.assign(1, 0);
    std::vector<u32> chk;
    for (u64 i = 0; i < km.size(); ++i)
        if ((rc = any_record(b, in, in.fn, i, km[i], reinterpret_cast<const uint8_t*>(td.data() + off[i]), (u32)(off[i + 1] - off[i]), chk))) return rc;
    b->inputs.push_back(std::move(in));
    b->done = false;
    return LMAT_OK;
}

int lmat_build_merge_stats(const lmat_build* b, lmat_merge_stats* out) {
    if (!b || !out) return LMAT_E_ARG;
    if (!b->done) return LMAT_E_ARG;
    *out = b->mstats;
    return LMAT_OK;
}

int lmat_build_taxid_counts(lmat_build* b, uint32_t* tids, uint64_t* counts, uint64_t cap, uint64_t* n) {
    if (!b || !n) return LMAT_E_ARG;
    if (!b->done) return berr(b, LMAT_E_ARG, "lmat_build_run first");
    u64 m = 0;
    for (u64 c : b->node_counts) m += c ? 1 : 0;
    *n = m;
    if (m > cap) return berr(b, LMAT_E_CAPACITY, "cap below the " + std::to_string(m) + " taxids with a count");
    if (m && (!tids || !counts)) return LMAT_E_ARG;
    u64 j = 0;
    for (size_t i = 0; i < b->node_counts.size(); ++i)
        if (b->node_counts[i]) { tids[j] = b->node_tid[i]; counts[j++] = b->node_counts[i]; }
    return LMAT_OK;
}

int lmat_build_run(lmat_build* b, lmat_build_stats* out) {
    if (!b) return LMAT_E_ARG;
    if (hipSetDevice(b->ctx->device) != hipSuccess) return berr(b, LMAT_E_DEVICE, "hipSetDevice failed");
    int pb = b->prefix_bits;   // -1: derived
    int start = 0;
    for (;;) {
        bool retry = false;
        const int rc = run_build(b, pb, start, retry);
        if (rc == LMAT_OK) break;
        if (!retry) return rc;
        start = (int)b->stats.prefix_bits + 1;   // a derived pass count proved too small for the skew of this input
        if (start > std::min(2 * b->k, 24)) return berr(b, LMAT_E_CAPACITY, "the device budget does not hold one pass of the finest prefix split");
    }
    b->done = true;
    if (out) *out = b->stats;
    return LMAT_OK;
}

int lmat_build_write_taxhisto(lmat_build* b, const char* fn) {
    if (!b || !fn) return LMAT_E_ARG;
    if (!b->done) return berr(b, LMAT_E_ARG, "lmat_build_run first");
    FILE* f = fopen(fn, "wb");
    if (!f) return berr(b, LMAT_E_IO, std::string("cannot open ") + fn + " for writing");
    bool ok = write_records(f, b);
    if (fclose(f) != 0) ok = false;
    return ok ? LMAT_OK : berr(b, LMAT_E_IO, std::string("write error on ") + fn);
}

int lmat_build_fetch(lmat_build* b, uint64_t first, uint64_t count, uint64_t* kmers, uint64_t* list_off, uint32_t* tids, uint64_t tid_cap) {
    if (!b) return LMAT_E_ARG;
    if (!b->done) return berr(b, LMAT_E_ARG, "lmat_build_run first");
    if (first > b->kmers.size() || count > b->kmers.size() - first) return berr(b, LMAT_E_ARG, "record range beyond the result");
    const u64 base = b->list_off[first], n = b->list_off[first + count] - base;
    if (kmers) memcpy(kmers, b->kmers.data() + first, count * 8);
    if (list_off) for (u64 i = 0; i <= count; ++i) list_off[i] = b->list_off[first + i] - base;
    if (tids) {
        if (n > tid_cap) return berr(b, LMAT_E_CAPACITY, "tid_cap below the " + std::to_string(n) + " list entries of the range");
        memcpy(tids, b->tids.data() + base, n * 4);
    }
    return LMAT_OK;
}

}  // extern "C"

namespace {

// bytes of device memory the merge holds per input record and per stored entry of one pass (keys and record numbers twice for the sort, list bounds,
// flag, position, run start, count, offset, slot, the run's k-mer; the entry as a node and its place in the result)
constexpr u64 kMergeRecBytes = 72, kMergeEntBytes = 12;

// the most one prefix pass takes of the tax_histo inputs, in bytes of the model above; also checks the 32-bit indices of one pass
u64 merge_need(const lmat_build* b, int pb, bool& too_many) {
    too_many = false;
    if (b->inputs.empty()) return 0;
    std::vector<u64> rec((size_t)1 << pb, 0), ent((size_t)1 << pb, 0);
    const int shift = 2 * b->k - pb;
    for (const auto& in : b->inputs)
        for (size_t i = 0; i < in.kmers.size(); ++i) {
            const size_t p = pb ? (size_t)(in.kmers[i] >> shift) : 0;
            rec[p] += 1;
            ent[p] += in.off[i + 1] - in.off[i];
        }
    u64 need = 0;
    for (size_t p = 0; p < rec.size(); ++p) {
        need = std::max(need, rec[p] * kMergeRecBytes + ent[p] * kMergeEntBytes);
        if (rec[p] > 0x3FFFFFFFull || ent[p] > 0x7FFFFFFFull) too_many = true;
    }
    return need;
}

// The tail the build and the merge share, count -> CSR: the counts scanned to offsets, the pass's counters read (n_counters words into hc), the
// list buffer and the side buffers of the lists beyond 64 entries sized exactly, the write pass launched (launch_write(off, tids, long buffers)
// enqueues it), the long lists ordered by segment and copied into place.  Leaves R + 1 offsets in off and hc[C_ENTRIES] taxids in out.
template <class Launch>
int write_lists(lmat_build* b, hipStream_t st, const char* what, u32 R, u64* cnt, u64* off, u64* counters, u64* hc, size_t n_counters, DevBuf& out,
                LongBufs& lg, DevBuf& temp, Launch launch_write) {
    BHIP(b, with_temp(temp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, cnt, off, 0ull, (size_t)R, rocprim::plus<u64>(), st); }));
    BHIP(b, hipMemcpyAsync(hc, counters, n_counters * 8, hipMemcpyDeviceToHost, st));
    BHIP(b, hipStreamSynchronize(st));
    if (hc[C_TOOLONG])
        return berr(b, LMAT_E_CAPACITY, std::string("a ") + what + " of " + std::to_string(hc[C_TOOLONG]) + " entries: the tax_histo record holds at most 65535");
    const u64 entries = hc[C_ENTRIES], n_long = hc[C_LONG_RUNS], long_entries = hc[C_LONG_ENTRIES];
    if (long_entries > 0xFFFFFFF0ull) return berr(b, LMAT_E_CAPACITY, "more than 2^32 entries in lists beyond 64 taxids in one pass: raise prefix_bits");
    BHIP(b, hipMemcpyAsync(off + R, &hc[C_ENTRIES], 8, hipMemcpyHostToDevice, st));
    BHIP(b, out.ensure(entries * 4));
    if (n_long) BHIP(b, ensure_all({{&lg.tmp, long_entries * 4}, {&lg.sorted, long_entries * 4}, {&lg.begin, n_long * 4}, {&lg.end, n_long * 4}, {&lg.run, n_long * 4}}));
    // the write pass hands out the long lists' places with the two counters the count pass filled
    BHIP(b, hipMemsetAsync(counters + C_LONG_RUNS, 0, 16, st));
    BHIP(b, launch_write(off, out.as<u32>(), lg.args()));
    if (n_long) {
        BHIP(b, with_temp(temp, [&](void* t, size_t& tb) {
            return rocprim::segmented_radix_sort_keys(t, tb, lg.tmp.as<u32>(), lg.sorted.as<u32>(), (unsigned)long_entries, (unsigned)n_long, lg.begin.as<u32>(),
                                                      lg.end.as<u32>(), 0, 32, st);
        }));
        hipLaunchKernelGGL(long_copy_kernel, dim3((u32)n_long), dim3(256), 0, st, lg.sorted.as<u32>(), lg.begin.as<u32>(), lg.end.as<u32>(), lg.run.as<u32>(), off,
                           out.as<u32>());
        BHIP(b, hipGetLastError());
    }
    return LMAT_OK;
}

// The tail of every pass: the merge with the tax_histo inputs (when there are any) and the per-taxid histogram of the final lists.
struct MergeState {
    lmat_build* b = nullptr;
    hipStream_t st = nullptr;
    LapTimer* timer = nullptr;            // the build's: a pass of the merge runs between two of its marks
    bool merging = false;
    int pb = 0, sb = 1;
    std::vector<size_t> cursor;           // next record of every input: the passes ascend, an input's slices follow each other
    std::vector<u32> node_at;
    DevBuf tin, d_node_at, hist, counters, totals, keysA, keysB, valsA, valsB, rec_off, ent, flag, pos, run, cnt, off, aux, big_run, big_begin, big_end,
        big_tmp, big_sorted, out, out_km, temp;
    LongBufs lng;
    TreeArgs tree = {nullptr, nullptr, nullptr};
    u32 n_nodes = 0;
    u64 hc[M_TOTAL];
    u64 singletons = 0, entries = 0, longest = 0;

    int key_bits() const { return 2 * b->k + sb; }

    int begin(lmat_build* b_, int pb_, const TreeArgs& tree_, LapTimer* timer_) {
        b = b_;
        st = b->ctx->stream;
        pb = pb_;
        tree = tree_;
        timer = timer_;
        n_nodes = (u32)b->node_tid.size();
        merging = !b->inputs.empty() && !b->id_mode;   // id mode unites its inputs inside the build's own sort (BuildRun::slice_inputs)
        memset(&b->mstats, 0, sizeof(b->mstats));
        b->node_counts.assign(n_nodes, 0);
        BHIP(b, hist.ensure((size_t)n_nodes * 8));
        BHIP(b, hipMemsetAsync(hist.p, 0, (size_t)n_nodes * 8, st));
        if (!merging) return LMAT_OK;
        sb = 1;
        while ((1ull << sb) < b->inputs.size() + 1) ++sb;   // the genomes' own result is the source behind the inputs
        cursor.assign(b->inputs.size(), 0);
        node_at.assign(n_nodes, 0);
        for (u32 i = 0; i < n_nodes; ++i) node_at[b->tin[i]] = i;
        BHIP(b, ensure_all({{&tin, (size_t)n_nodes * 4}, {&d_node_at, (size_t)n_nodes * 4}, {&counters, M_TOTAL * 8}, {&totals, 16}}));
        BHIP(b, hipMemcpyAsync(tin.p, b->tin.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, st));
        BHIP(b, hipMemcpyAsync(d_node_at.p, node_at.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, st));
        BHIP(b, hipStreamSynchronize(st));
        b->mstats.inputs = (uint32_t)b->inputs.size();
        b->mstats.passes = 1u << pb;
        for (const auto& in : b->inputs) { b->mstats.records_in += in.kmers.size(); b->mstats.entries_in += in.nodes.size(); }
        return LMAT_OK;
    }

    // the histogram of a finished CSR on the device
    int count_lists(const u32* d_tids, u64 n) {
        if (!n) return LMAT_OK;
        hipLaunchKernelGGL(hist_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_tids, n, tree.node_tid, n_nodes, hist.as<u64>());
        BHIP(b, hipGetLastError());
        return LMAT_OK;
    }

    // Stage 1: the inputs' slices with the pass's prefix and the genomes' result of the pass as the last source -> one key per record in keysA,
    // record numbers in valsA, list bounds in rec_off, entries as node indices in ent.  Nr = 0: the pass holds nothing.
    int upload(u32 pass_no, u32 gR, const u64* g_kmer, const u64* g_off, const u32* g_tids, u64 g_entries, u32& Nr) {
        const int k = b->k;
        const size_t n_in = b->inputs.size();
        std::vector<u64> h_keys;
        std::vector<u32> h_off(1, 0), h_ent;
        for (size_t s = 0; s < n_in; ++s) {
            const auto& in = b->inputs[s];
            const size_t lo = cursor[s];
            size_t hi = in.kmers.size();
            if (pb) {
                const u64 lim = ((u64)pass_no + 1) << (2 * k - pb);   // first k-mer of the next prefix
                hi = (size_t)(std::lower_bound(in.kmers.begin() + lo, in.kmers.end(), lim) - in.kmers.begin());
            }
            cursor[s] = hi;
            if (hi == lo) continue;
            const u64 e0 = in.off[lo], e1 = in.off[hi];
            if (h_ent.size() + (e1 - e0) > 0x7FFFFFFFull || h_keys.size() + (hi - lo) > 0x3FFFFFFFull)
                return berr(b, LMAT_E_CAPACITY, "more than 2^31 list entries or 2^30 records of the tax_histo inputs in one prefix pass: raise prefix_bits");
            for (size_t i = lo; i < hi; ++i) {
                h_keys.push_back((in.kmers[i] << sb) | (u64)s);
                h_off.push_back((u32)(h_ent.size() + (in.off[i + 1] - e0)));
            }
            h_ent.insert(h_ent.end(), in.nodes.begin() + e0, in.nodes.begin() + e1);
        }
        const u64 Nin = h_keys.size(), Ein = h_ent.size();
        const u64 Nr64 = Nin + gR, Ne64 = Ein + g_entries;
        Nr = 0;
        if (Nr64 == 0) return LMAT_OK;
        if (Nr64 > 0x7FFFFFFFull || Ne64 > 0xFFFFFF00ull) return berr(b, LMAT_E_CAPACITY, "more than 2^31 records or 2^32 list entries to merge in one prefix pass: raise prefix_bits");
        Nr = (u32)Nr64;
        const u32 slots = (u32)(Ne64 / 65 + 1);   // a side-buffer segment holds more than 64 entries
        const size_t n = Nr;
        BHIP(b, ensure_all({{&keysA, n * 8}, {&keysB, n * 8}, {&valsA, n * 4}, {&valsB, n * 4}, {&rec_off, (n + 1) * 4}, {&ent, (size_t)Ne64 * 4}, {&flag, n * 4},
                            {&pos, n * 4}, {&run, (n + 1) * 4}, {&cnt, n * 8}, {&off, (n + 1) * 8}, {&aux, n * 4}, {&out_km, n * 8}, {&big_run, (size_t)slots * 4},
                            {&big_begin, (size_t)slots * 4}, {&big_end, (size_t)slots * 4}}));
        BHIP(b, hipMemsetAsync(counters.p, 0, M_TOTAL * 8, st));
        BHIP(b, timer->start());
        if (Nin) BHIP(b, hipMemcpyAsync(keysA.p, h_keys.data(), (size_t)Nin * 8, hipMemcpyHostToDevice, st));
        BHIP(b, hipMemcpyAsync(rec_off.p, h_off.data(), ((size_t)Nin + 1) * 4, hipMemcpyHostToDevice, st));
        if (Ein) BHIP(b, hipMemcpyAsync(ent.p, h_ent.data(), (size_t)Ein * 4, hipMemcpyHostToDevice, st));
        if (gR) {
            hipLaunchKernelGGL(genome_source_kernel, dim3((gR + 255) / 256), dim3(256), 0, st, gR, g_kmer, g_off, (u32)Nin, (u32)Ein, (u32)n_in, sb, key_bits(),
                               keysA.as<u64>(), rec_off.as<u32>(), counters.as<u64>());
            BHIP(b, hipGetLastError());
            if (g_entries) {
                hipLaunchKernelGGL(tid_to_node_kernel, dim3((u32)((g_entries + 255) / 256)), dim3(256), 0, st, g_tids, g_entries, tree.node_tid, n_nodes,
                                   ent.as<u32>() + Ein);
                BHIP(b, hipGetLastError());
            }
        }
        hipLaunchKernelGGL(iota_kernel, dim3((Nr + 255) / 256), dim3(256), 0, st, valsA.as<u32>(), Nr);
        BHIP(b, hipGetLastError());
        BHIP(b, hipStreamSynchronize(st));   // the host vectors go out of use here
        BHIP(b, timer->lap(b->mstats.upload_ms));
        return LMAT_OK;
    }

    // Stage 2: one key per record, sorted by (k-mer, source) into keysB / valsB, records without a list behind all others and cut off; then the
    // runs of one k-mer.  R = 0: no record of the pass has a list.
    int sort_runs(u32 Nr, u32& R) {
        lmat_merge_stats& M = b->mstats;
        R = 0;
        BHIP(b, with_temp(temp, [&](void* t, size_t& tb) {
            return rocprim::radix_sort_pairs(t, tb, keysA.as<u64>(), keysB.as<u64>(), valsA.as<u32>(), valsB.as<u32>(), Nr, 0, key_bits() + 1, st);
        }));
        BHIP(b, hipMemcpyAsync(hc, counters.p, M_TOTAL * 8, hipMemcpyDeviceToHost, st));
        BHIP(b, timer->lap(M.sort_ms));
        const u32 Nv = Nr - (u32)hc[M_EMPTY];
        if (Nv == 0) return LMAT_OK;
        const u32 gridN = (Nv + 255) / 256;
        hipLaunchKernelGGL(mseg_flag_kernel, dim3(gridN), dim3(256), 0, st, keysB.as<u64>(), Nv, sb, flag.as<u32>());
        BHIP(b, hipGetLastError());
        BHIP(b, with_temp(temp, [&](void* t, size_t& tb) {
            return rocprim::exclusive_scan(t, tb, flag.as<u32>(), pos.as<u32>(), 0u, (size_t)Nv, rocprim::plus<u32>(), st);
        }));
        hipLaunchKernelGGL(mseg_scatter_kernel, dim3(gridN), dim3(256), 0, st, flag.as<u32>(), pos.as<u32>(), Nv, run.as<u32>(), totals.as<u64>());
        BHIP(b, hipGetLastError());
        u64 tot[2];
        BHIP(b, hipMemcpyAsync(tot, totals.p, 16, hipMemcpyDeviceToHost, st));
        BHIP(b, timer->lap(M.segment_ms));
        R = (u32)tot[0];
        return LMAT_OK;
    }

    // Stage 3, the union: classify, side-buffer segments in tour order, count, and the shared tail -> the CSR in off / out, the k-mers in out_km
    int unite(u32 R) {
        UnionArgs ua;
        memset(&ua, 0, sizeof(ua));
        ua.R = R;
        ua.run_start = run.as<u32>();
        ua.rec = valsB.as<u32>();
        ua.rec_off = rec_off.as<u32>();
        ua.ent = ent.as<u32>();
        ua.tin = tin.as<u32>();
        ua.node_at = d_node_at.as<u32>();
        ua.tree = tree;
        ua.aux = aux.as<u32>();
        ua.big_run = big_run.as<u32>();
        ua.big_begin = big_begin.as<u32>();
        ua.big_end = big_end.as<u32>();
        ua.cnt = cnt.as<u64>();
        ua.counters = counters.as<u64>();
        hipLaunchKernelGGL(union_classify_kernel, dim3((R + 255) / 256), dim3(256), 0, st, ua);
        BHIP(b, hipGetLastError());
        BHIP(b, hipMemcpyAsync(hc, counters.p, M_TOTAL * 8, hipMemcpyDeviceToHost, st));
        BHIP(b, hipStreamSynchronize(st));
        const u64 n_big = hc[M_BIG_RUNS], big_entries = hc[M_BIG_ENTRIES];
        if (n_big) {
            BHIP(b, ensure_all({{&big_tmp, big_entries * 4}, {&big_sorted, big_entries * 4}}));
            hipLaunchKernelGGL(big_gather_kernel, dim3((u32)n_big), dim3(256), 0, st, ua, big_tmp.as<u32>());
            BHIP(b, hipGetLastError());
            BHIP(b, with_temp(temp, [&](void* t, size_t& tb) {
                return rocprim::segmented_radix_sort_keys(t, tb, big_tmp.as<u32>(), big_sorted.as<u32>(), (unsigned)big_entries, (unsigned)n_big, big_begin.as<u32>(),
                                                          big_end.as<u32>(), 0, 32, st);
            }));
            ua.big_sorted = big_sorted.as<u32>();
        }
        const u32 gridR = (u32)(((u64)R + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock));
        hipLaunchKernelGGL(union_kernel<false>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ua);
        BHIP(b, hipGetLastError());
        const int rc = write_lists(b, st, "merged taxid list", R, cnt.as<u64>(), off.as<u64>(), counters.as<u64>(), hc, M_TOTAL, out, lng, temp,
                                   [&](const u64* d_off, u32* d_tids, const LongArgs& lg) {
                                       ua.off = d_off;
                                       ua.tids = d_tids;
                                       ua.lng = lg;
                                       hipLaunchKernelGGL(union_kernel<true>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ua);
                                       return hipGetLastError();
                                   });
        if (rc) return rc;
        const u64 kmask = (1ull << (2 * b->k)) - 1;
        hipLaunchKernelGGL(mrun_kmer_kernel, dim3((R + 255) / 256), dim3(256), 0, st, keysB.as<u64>(), run.as<u32>(), R, sb, kmask, out_km.as<u64>());
        BHIP(b, hipGetLastError());
        BHIP(b, timer->lap(b->mstats.union_ms));
        return LMAT_OK;
    }

    // One prefix pass: the inputs' slices and the genomes' result of the pass (gR runs: k-mer, CSR of ascending taxids, runs without a list
    // included) -> records appended to the builder's result.
    int pass(u32 pass_no, u32 gR, const u64* g_kmer, const u64* g_off, const u32* g_tids, u64 g_entries) {
        u32 Nr = 0, R = 0;
        if (const int rc = upload(pass_no, gR, g_kmer, g_off, g_tids, g_entries, Nr)) return rc;
        if (Nr == 0) return LMAT_OK;
        if (const int rc = sort_runs(Nr, R)) return rc;
        if (R == 0) return LMAT_OK;
        if (const int rc = unite(R)) return rc;
        lmat_merge_stats& M = b->mstats;
        const u64 n_entries = hc[C_ENTRIES];
        if (const int rc = count_lists(out.as<u32>(), n_entries)) return rc;
        BHIP(b, timer->lap(M.histogram_ms));

        // ---- to the host: every run has a list
        std::vector<u64> h_o((size_t)R + 1);
        const size_t k0 = b->kmers.size(), t0 = b->tids.size();
        b->kmers.resize(k0 + R);
        b->tids.resize(t0 + n_entries);
        BHIP(b, hipMemcpy(b->kmers.data() + k0, out_km.p, (size_t)R * 8, hipMemcpyDeviceToHost));
        BHIP(b, hipMemcpy(h_o.data(), off.p, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost));
        if (n_entries) BHIP(b, hipMemcpy(b->tids.data() + t0, out.p, n_entries * 4, hipMemcpyDeviceToHost));
        for (u32 r = 0; r < R; ++r) b->list_off.push_back(t0 + h_o[r + 1]);
        M.records_one_source += hc[M_ONE];
        M.records_merged += hc[M_MERGED];
        M.records_grown += hc[M_GROWN];
        singletons += hc[C_SINGLETONS];
        entries += n_entries;
        longest = std::max<u64>(longest, hc[C_LONGEST]);
        return LMAT_OK;
    }

    int finish() {
        if (n_nodes) BHIP(b, hipMemcpy(b->node_counts.data(), hist.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost));
        return LMAT_OK;
    }
};

// One run of the build: what the owner numbering and the memory model decide, and the device buffers of its passes.
struct BuildRun {
    lmat_build* b = nullptr;
    hipStream_t st = nullptr;
    u64 T = 0;                            // bytes of genome text
    // owners
    u32 n_rec = 0, n_owner = 0, n_known = 0;
    int ob = 1;                           // bits of an owner index
    int fb = 0;                           // id mode with tax_histo inputs: the source flag below the owner (ExtractArgs::flag_bits)
    bool packed = true;                   // one 64-bit key per pair
    std::vector<u32> rec_owner, owner_node;
    // id mode, tax_histo inputs: every entry's owner index; per pass the next record of every input, the slices taken and their pairs
    std::vector<std::vector<u32>> in_owner;
    std::vector<size_t> cursor;
    struct Slice { size_t input, lo, hi; };
    std::vector<Slice> slices;
    std::vector<u64> in_keys;
    std::vector<u32> in_vals;
    u64 in_pairs = 0;
    DevBuf has_text;
    // memory model
    u32 chunk = 0;
    u64 chunk_alloc = 0, cap = 0;
    int pb = 0;
    // device
    DevBuf text, rec_start, d_rec_owner, d_owner_node, parent, depth, node_tid, counters, totals, keysA, keysB, valsA, valsB, flag, pos, dk, downer, run, temp,
        tids;
    LongBufs lng;
    uint8_t* stage = nullptr;             // pinned: one chunk of text on its way up
    LapTimer timer;
    u64 hc[C_N];
    ~BuildRun() { if (stage) hipHostFree(stage); }

    TreeArgs tree() const { return TreeArgs{parent.as<u32>(), depth.as<u32>(), node_tid.as<u32>()}; }

    // owners: distinct taxids; the tree's own in Euler-tour order, the others behind them
    void number_owners() {
        if (b->id_mode) {   // the owner of an id is its rank among the ids of all inputs (b->node_tid): sorting by (k-mer, owner) gives ascending ids
            const std::vector<u32>& ids = b->node_tid;
            auto rank = [&](u32 id) { return (u32)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
            n_owner = n_known = (u32)ids.size();
            rec_owner.resize(n_rec);
            for (u32 r = 0; r < n_rec; ++r) rec_owner[r] = rank(b->rec_taxid[r]);
            in_owner.resize(b->inputs.size());
            for (size_t s = 0; s < b->inputs.size(); ++s) {
                in_owner[s].resize(b->inputs[s].nodes.size());
                for (size_t i = 0; i < in_owner[s].size(); ++i) in_owner[s][i] = rank(b->inputs[s].nodes[i]);
            }
            cursor.assign(b->inputs.size(), 0);
            fb = b->inputs.empty() ? 0 : 1;
            while ((1ull << ob) < n_owner) ++ob;
            packed = 2 * b->k + ob + fb <= 64;
            if (const char* e = getenv("LMAT_DBGEN_SORT")) if (!strcmp(e, "pairs")) packed = false;
            return;
        }
        std::vector<u32> owners(b->rec_taxid);
        std::sort(owners.begin(), owners.end());
        owners.erase(std::unique(owners.begin(), owners.end()), owners.end());
        std::vector<std::pair<u64, u32>> order;   // (sort key, taxid)
        for (u32 t : owners) {
            auto it = b->node_of.find(t);
            if (it != b->node_of.end()) { order.push_back(std::make_pair((u64)b->tin[it->second], t)); ++n_known; }
            else order.push_back(std::make_pair((1ull << 32) | t, t));
        }
        std::sort(order.begin(), order.end());
        n_owner = (u32)order.size();
        std::unordered_map<u32, u32> owner_of;
        owner_node.assign(n_owner, kNoNode);
        for (u32 i = 0; i < n_owner; ++i) {
            owner_of[order[i].second] = i;
            if (i < n_known) owner_node[i] = b->node_of[order[i].second];
        }
        rec_owner.resize(n_rec);
        for (u32 r = 0; r < n_rec; ++r) rec_owner[r] = owner_of[b->rec_taxid[r]];
        while ((1ull << ob) < n_owner) ++ob;
        // one 64-bit key when the owner fits behind the k-mer, else (owner, k-mer) pairs sorted twice; LMAT_DBGEN_SORT=pairs forces the latter
        packed = 2 * b->k + ob <= 64;
        if (const char* e = getenv("LMAT_DBGEN_SORT")) if (!strcmp(e, "pairs")) packed = false;
    }

    // memory model: everything on the device is sized by cap, the pairs one pass may emit; prefix_bits is forced or the smallest split that fits
    int plan(int pb_forced, int pb_start) {
        const int k = b->k;
        u64 budget = b->budget;
        if (!budget) {
            size_t fr = 0, tot = 0;
            BHIP(b, hipMemGetInfo(&fr, &tot));
            budget = fr / 2;
        }
        chunk = T == 0 ? 1024u : b->chunk_bases ? std::max<u32>(b->chunk_bases, 1024) : (1u << 24);   // T == 0: a merge of tax_histo inputs alone
        const u64 chunk_waves = ((u64)chunk + kSpan - 1) / kSpan;
        chunk_alloc = chunk_waves * kSpan + kLead + 64;
        const u64 fixed = chunk_alloc + (u64)n_rec * 12 + (u64)b->node_tid.size() * 12 + (u64)n_owner * 4 + (64u << 20);   // + sort scratch and slack
        const u64 per_pair = 8 + 8 + 8 + 8 + 8 + 4 + 4 + (packed ? 0 : 8) + 16 + (fb ? 4 : 0);   // keys x2, flag, pos, distinct pair, run start, (vals x2), list entries (estimate), (text flag of a run)
        if (budget <= fixed || (budget <= fixed + per_pair * 1024 && T != 0)) return berr(b, LMAT_E_NOMEM, "device budget of " + std::to_string(budget) + " bytes is below the fixed buffers");
        cap = std::min<u64>((budget - fixed) / per_pair, 0x7FFFFF00ull);
        pb = pb_forced;
        if (pb < 0) {
            // canonical k-mers crowd the low prefixes (min of a k-mer and its reverse complement): up to twice the even share
            pb = pb_start;
            while (pb < std::min(2 * k, 24) && (double)T * 2.0 / (double)(1ull << pb) > (double)cap && T > cap) ++pb;
            if (pb == 0 && T > cap) pb = 1;
        }
        if (fb) {
            // id mode: the inputs' entries of a pass are pairs beside the extracted ones, known exactly; the text shares what they leave of cap
            const u64 cap_budget = cap;
            const int pb_max = std::min(2 * k, 24);
            for (pb = pb_forced < 0 ? pb_start : pb_forced;; ++pb) {
                std::vector<u64> ent((size_t)1 << pb, 0);
                for (const auto& in : b->inputs)
                    for (size_t i = 0; i < in.kmers.size(); ++i) ent[pb ? (size_t)(in.kmers[i] >> (2 * k - pb)) : 0] += in.off[i + 1] - in.off[i];
                const u64 in_max = *std::max_element(ent.begin(), ent.end());
                const bool in_fit = in_max <= cap_budget;
                const u64 room = in_fit ? cap_budget - in_max : 0;
                const bool seq_fit = in_fit && (T <= room || (double)T * 2.0 / (double)(1ull << pb) <= (double)room);
                cap = std::min<u64>(cap_budget, T + in_max);
                if (in_fit && (seq_fit || pb_forced >= 0)) return LMAT_OK;   // a forced split that the text overflows is found by the extraction
                if (pb_forced >= 0 || pb >= pb_max)
                    return berr(b, LMAT_E_CAPACITY, "the tax_histo inputs hold " + std::to_string(in_max) + " entries in one of the " + std::to_string(1ull << pb) +
                                                       " prefix passes, the device budget holds " + std::to_string(cap_budget) + " pairs: raise the budget or prefix_bits");
            }
        }
        if (!b->inputs.empty()) {
            // The slices of the inputs are known exactly; what they take of a pass comes off the budget first, the pairs of the genomes share the rest
            // with the records and entries their own result adds to the merge (at most one record per pair, lists as the estimate above has them).
            const u64 avail = budget - fixed;
            const u64 per_pair_m = per_pair + kMergeRecBytes + 2 * kMergeEntBytes;
            const int pb_max = std::min(2 * k, 24);
            for (pb = pb_forced < 0 ? pb_start : pb_forced;; ++pb) {
                bool too_many = false;
                const u64 need = merge_need(b, pb, too_many);
                const bool in_fit = !too_many && need + (T ? per_pair_m * 1024 : 0) < avail;
                if (in_fit) cap = std::min<u64>((avail - need) / per_pair_m, 0x7FFFFF00ull);
                const bool seq_fit = in_fit && (T <= cap || (double)T * 2.0 / (double)(1ull << pb) <= (double)cap);
                if (in_fit && (seq_fit || pb_forced >= 0)) break;   // a forced split that the genomes overflow is found by the extraction, as without inputs
                if (pb_forced >= 0 || pb >= pb_max)
                    return berr(b, LMAT_E_CAPACITY, "the tax_histo inputs take " + std::to_string(need) + " bytes in one of the " + std::to_string(1ull << pb) +
                                                       " prefix passes, the device budget leaves " + std::to_string(avail) + ": raise the budget or prefix_bits");
            }
        }
        cap = std::min<u64>(cap, T);   // no pass emits more pairs than there are bases
        return LMAT_OK;
    }

    // the buffers of a pass, the records, the owners and the tree on the device
    int alloc() {
        BHIP(b, ensure_all({{&text, chunk_alloc}, {&rec_start, (size_t)n_rec * 8}, {&d_rec_owner, (size_t)n_rec * 4}, {&d_owner_node, (size_t)n_owner * 4},
                            {&parent, b->parent.size() * 4}, {&depth, b->depth.size() * 4}, {&node_tid, b->node_tid.size() * 4}, {&counters, C_N * 8}, {&totals, 16},
                            {&keysA, cap * 8}, {&keysB, cap * 8}, {&flag, cap * 8}, {&pos, cap * 8}, {&dk, cap * 8}, {&downer, cap * 4}, {&run, (cap + 1) * 4}}));
        if (!packed) BHIP(b, ensure_all({{&valsA, cap * 4}, {&valsB, cap * 4}}));
        if (n_rec) {
            BHIP(b, hipMemcpyAsync(rec_start.p, b->rec_start.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
            BHIP(b, hipMemcpyAsync(d_rec_owner.p, rec_owner.data(), (size_t)n_rec * 4, hipMemcpyHostToDevice, st));
            if (!owner_node.empty()) BHIP(b, hipMemcpyAsync(d_owner_node.p, owner_node.data(), (size_t)n_owner * 4, hipMemcpyHostToDevice, st));
        }
        if (!b->parent.empty()) {   // (id mode has no tree)
            BHIP(b, hipMemcpyAsync(parent.p, b->parent.data(), b->parent.size() * 4, hipMemcpyHostToDevice, st));
            BHIP(b, hipMemcpyAsync(depth.p, b->depth.data(), b->depth.size() * 4, hipMemcpyHostToDevice, st));
        }
        if (!b->node_tid.empty()) BHIP(b, hipMemcpyAsync(node_tid.p, b->node_tid.data(), b->node_tid.size() * 4, hipMemcpyHostToDevice, st));
        BHIP(b, hipStreamSynchronize(st));
        BHIP(b, hipHostMalloc((void**)&stage, chunk_alloc));
        BHIP(b, timer.init(st));
        return LMAT_OK;
    }

    // id mode: the slice of every input with the pass's prefix as (k-mer, owner) pairs with the source flag set, on the host; cap minus their
    // number is what the extraction of the pass may emit
    void slice_inputs(u32 pass) {
        slices.clear();
        in_keys.clear();
        in_vals.clear();
        const int k = b->k;
        for (size_t s = 0; s < b->inputs.size(); ++s) {
            const auto& in = b->inputs[s];
            const size_t lo = cursor[s];
            size_t hi = in.kmers.size();
            if (pb) hi = (size_t)(std::lower_bound(in.kmers.begin() + lo, in.kmers.end(), ((u64)pass + 1) << (2 * k - pb)) - in.kmers.begin());
            cursor[s] = hi;
            if (hi == lo) continue;
            slices.push_back(Slice{s, lo, hi});
            for (size_t i = lo; i < hi; ++i)
                for (u64 e = in.off[i]; e < in.off[i + 1]; ++e) {
                    const u32 ow = in_owner[s][e];
                    if (packed) in_keys.push_back((((in.kmers[i] << ob) | ow) << 1) | 1ull);
                    else { in_keys.push_back(in.kmers[i]); in_vals.push_back((ow << 1) | 1u); }
                }
        }
        in_pairs = in_keys.size();   // <= cap: plan() sized cap by the largest slice
    }

    // ... behind the N extracted pairs
    int append_inputs(u64 N) {
        if (!in_pairs) return LMAT_OK;
        BHIP(b, hipMemcpyAsync(keysA.as<u64>() + N, in_keys.data(), in_pairs * 8, hipMemcpyHostToDevice, st));
        if (!packed) BHIP(b, hipMemcpyAsync(valsA.as<u32>() + N, in_vals.data(), in_pairs * 4, hipMemcpyHostToDevice, st));
        BHIP(b, hipStreamSynchronize(st));
        BHIP(b, timer.lap(b->mstats.upload_ms));
        return LMAT_OK;
    }

    // the pairs of one prefix pass into keysA (valsA); the pass's counters into hc
    int extract(u32 pass) {
        BHIP(b, hipMemsetAsync(counters.p, 0, C_N * 8, st));
        BHIP(b, timer.start());
        for (u64 lo = 0; lo < T; lo += chunk) {
            const u32 len = (u32)std::min<u64>(chunk, T - lo);
            const u64 waves = ((u64)len + kSpan - 1) / kSpan;
            const u64 bytes = waves * kSpan + kLead;
            const u64 lead = std::min<u64>(lo, kLead);
            memset(stage, 'N', kLead - lead);
            memcpy(stage + kLead - lead, b->text.data() + lo - lead, lead);
            const u64 avail = std::min<u64>(T - lo, bytes - kLead);   // bases behind the chunk's end are read but never end a window of it
            memcpy(stage + kLead, b->text.data() + lo, avail);
            memset(stage + kLead + avail, 'N', bytes - kLead - avail);
            BHIP(b, hipMemcpyAsync(text.p, stage, bytes, hipMemcpyHostToDevice, st));
            ExtractArgs a;
            a.buf = text.as<uint8_t>();
            a.chunk_lo = lo;
            a.chunk_len = len;
            a.rec_start = rec_start.as<u64>();
            a.rec_owner = d_rec_owner.as<u32>();
            a.n_rec = n_rec;
            a.k = b->k;
            a.prefix_bits = pb;
            a.owner_bits = packed ? ob : -1;
            a.flag_bits = fb;
            a.pass = pass;
            a.keys = keysA.as<u64>();
            a.vals = valsA.as<u32>();
            a.cap = cap - in_pairs;
            a.counters = counters.as<u64>();
            const u32 grid = (u32)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
            hipLaunchKernelGGL(extract_kernel, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, a);
            BHIP(b, hipGetLastError());
            BHIP(b, hipStreamSynchronize(st));   // the staging buffer is refilled next
        }
        BHIP(b, timer.lap(b->stats.extract_ms));
        BHIP(b, hipMemcpy(hc, counters.p, C_N * 8, hipMemcpyDeviceToHost));
        return LMAT_OK;
    }

    // The N pairs of a pass -> its R runs: the k-mers in pos, the CSR of ascending taxids in *off_buf (R + 1 offsets) and tids (hc[C_ENTRIES]).
    int lists(u64 N, u32& R, DevBuf*& off_buf) {
        const int k = b->k;
        lmat_build_stats& S = b->stats;
        // ---- sort by (k-mer, owner)
        Sorted sorted;
        sorted.owner_bits = packed ? ob : -1;
        sorted.flag_bits = fb;
        if (packed) {
            BHIP(b, with_temp(temp, [&](void* t, size_t& tb) { return rocprim::radix_sort_keys(t, tb, keysA.as<u64>(), keysB.as<u64>(), N, 0, 2 * k + ob + fb, st); }));
            sorted.keys = keysB.as<u64>();
            sorted.vals = nullptr;
        } else {
            BHIP(b, with_temp(temp, [&](void* t, size_t& tb) {   // by owner, then -- stable -- by k-mer: one storage for both
                size_t tb1 = tb, tb2 = tb;
                hipError_t e = rocprim::radix_sort_pairs(t, tb1, valsA.as<u32>(), valsB.as<u32>(), keysA.as<u64>(), keysB.as<u64>(), N, 0, ob + fb, st);
                if (e == hipSuccess) e = rocprim::radix_sort_pairs(t, tb2, keysB.as<u64>(), keysA.as<u64>(), valsB.as<u32>(), valsA.as<u32>(), N, 0, 2 * k, st);
                tb = std::max(tb1, tb2);
                return e;
            }));
            sorted.keys = keysA.as<u64>();
            sorted.vals = valsA.as<u32>();
        }
        BHIP(b, timer.lap(S.sort_ms));

        // ---- distinct pairs and run heads
        const u32 gridN = (u32)((N + 255) / 256);
        hipLaunchKernelGGL(seg_flag_kernel, dim3(gridN), dim3(256), 0, st, sorted, N, flag.as<u64>());
        BHIP(b, hipGetLastError());
        BHIP(b, with_temp(temp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, flag.as<u64>(), pos.as<u64>(), 0ull, N, rocprim::plus<u64>(), st); }));
        hipLaunchKernelGGL(seg_scatter_kernel, dim3(gridN), dim3(256), 0, st, sorted, N, flag.as<u64>(), pos.as<u64>(), dk.as<u64>(), downer.as<u32>(), run.as<u32>(),
                           totals.as<u64>());
        BHIP(b, hipGetLastError());
        u64 tot[2];
        BHIP(b, hipMemcpyAsync(tot, totals.p, 16, hipMemcpyDeviceToHost, st));
        BHIP(b, timer.lap(S.segment_ms));
        R = (u32)tot[1];
        S.distinct_kmers += R;
        if (b->id_mode) return id_lists(sorted, N, R, off_buf);

        // ---- closure: count, then the shared tail.  cnt reuses the flag array, off a key buffer (both are R + 1 <= N + 1 long at most)
        ClosureArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.R = R;
        ca.run_start = run.as<u32>();
        ca.d_owner = downer.as<u32>();
        ca.n_known = n_known;
        ca.owner_node = d_owner_node.as<u32>();
        ca.tree = tree();
        ca.cnt = flag.as<u64>();
        ca.counters = counters.as<u64>();
        const u32 gridR = (u32)(((u64)R + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock));
        hipLaunchKernelGGL(closure_kernel<false>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ca);
        BHIP(b, hipGetLastError());
        // offsets: R + 1 entries in a buffer of their own size class (keysA is free once the pairs are sorted and scattered ... unless it holds them)
        off_buf = packed ? &keysA : &keysB;
        if ((u64)R + 1 > cap) BHIP(b, off_buf->ensure(((u64)R + 1) * 8));
        const int rc = write_lists(b, st, "taxid list", R, flag.as<u64>(), off_buf->as<u64>(), counters.as<u64>(), hc, C_N, tids, lng, temp,
                                   [&](const u64* d_off, u32* d_tids, const LongArgs& lg) {
                                       ca.off = d_off;
                                       ca.tids = d_tids;
                                       ca.lng = lg;
                                       hipLaunchKernelGGL(closure_kernel<true>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ca);
                                       return hipGetLastError();
                                   });
        if (rc) return rc;
        // the k-mer of every run, into the scan's old output
        hipLaunchKernelGGL(run_kmer_kernel, dim3((R + 255) / 256), dim3(256), 0, st, dk.as<u64>(), run.as<u32>(), R, pos.as<u64>());
        BHIP(b, hipGetLastError());
        BHIP(b, timer.lap(S.closure_ms));
        return LMAT_OK;
    }

    // id mode, behind the segmentation: which runs hold a pair from text (while flag and pos still are the segmentation's), then the list stage
    int id_lists(const Sorted& sorted, u64 N, u32 R, DevBuf*& off_buf) {
        if (fb) {
            BHIP(b, has_text.ensure((size_t)R * 4));
            BHIP(b, hipMemsetAsync(has_text.p, 0, (size_t)R * 4, st));
            hipLaunchKernelGGL(text_runs_kernel, dim3((u32)((N + 255) / 256)), dim3(256), 0, st, sorted, N, flag.as<u64>(), pos.as<u64>(), has_text.as<u32>());
            BHIP(b, hipGetLastError());
        }
        IdListArgs ia;
        memset(&ia, 0, sizeof(ia));
        ia.R = R;
        ia.run_start = run.as<u32>();
        ia.d_owner = downer.as<u32>();
        ia.id_of = node_tid.as<u32>();
        ia.cnt = flag.as<u64>();
        ia.counters = counters.as<u64>();
        const u32 gridR = (u32)(((u64)R + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock));
        hipLaunchKernelGGL(idlist_kernel<false>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ia);
        BHIP(b, hipGetLastError());
        off_buf = packed ? &keysA : &keysB;
        if ((u64)R + 1 > cap) BHIP(b, off_buf->ensure(((u64)R + 1) * 8));
        const int rc = write_lists(b, st, "gene id list", R, flag.as<u64>(), off_buf->as<u64>(), counters.as<u64>(), hc, C_N, tids, lng, temp,
                                   [&](const u64* d_off, u32* d_tids, const LongArgs&) {
                                       ia.off = d_off;
                                       ia.tids = d_tids;
                                       hipLaunchKernelGGL(idlist_kernel<true>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ia);
                                       return hipGetLastError();
                                   });
        if (rc) return rc;
        hipLaunchKernelGGL(run_kmer_kernel, dim3((R + 255) / 256), dim3(256), 0, st, dk.as<u64>(), run.as<u32>(), R, pos.as<u64>());
        BHIP(b, hipGetLastError());
        BHIP(b, timer.lap(b->stats.closure_ms));
        return LMAT_OK;
    }

    // id mode with inputs: the sources of every record of the pass -- the text (has_text) and every input whose slice holds the k-mer
    int source_stats(u32 R, const std::vector<u64>& h_km) {
        std::vector<u32> n_src(R);
        BHIP(b, hipMemcpy(n_src.data(), has_text.p, (size_t)R * 4, hipMemcpyDeviceToHost));
        for (const Slice& sl : slices) {
            const auto& in = b->inputs[sl.input];
            size_t j = 0;
            for (size_t i = sl.lo; i < sl.hi; ++i) {   // both ascend, and every k-mer of an input is a record of the result
                while (j < R && h_km[j] < in.kmers[i]) ++j;
                if (j < R) n_src[j] += 1;
            }
        }
        for (u32 r = 0; r < R; ++r) (n_src[r] > 1 ? b->mstats.records_merged : b->mstats.records_one_source) += 1;
        return LMAT_OK;
    }

    // the pass's records to the host: those without a known owner are left out (tax_histo.cpp:239-248)
    int fetch(u32 R, const DevBuf& off_buf) {
        const u64 entries = hc[C_ENTRIES];
        std::vector<u64> h_km(R), h_off((size_t)R + 1);
        const size_t t0 = b->tids.size();
        b->tids.resize(t0 + entries);
        BHIP(b, hipMemcpy(h_km.data(), pos.p, (size_t)R * 8, hipMemcpyDeviceToHost));
        BHIP(b, hipMemcpy(h_off.data(), off_buf.p, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost));
        if (entries) BHIP(b, hipMemcpy(b->tids.data() + t0, tids.p, entries * 4, hipMemcpyDeviceToHost));
        if (fb) if (const int rc = source_stats(R, h_km)) return rc;
        for (u32 r = 0; r < R; ++r) {
            if (h_off[r + 1] == h_off[r]) continue;
            b->kmers.push_back(h_km[r]);
            b->list_off.push_back(t0 + h_off[r + 1]);
        }
        return LMAT_OK;
    }
};

int run_build(lmat_build* b, int pb_forced, int pb_start, bool& retry) {
    lmat_build_stats& S = b->stats;
    memset(&S, 0, sizeof(S));
    b->kmers.clear();
    b->tids.clear();
    b->list_off.assign(1, 0);
    S.bases = b->bases;
    if (b->rec_start.size() > 0x7FFFFFFFull) return berr(b, LMAT_E_CAPACITY, "more than 2^31 FASTA records");
    const bool merging = !b->inputs.empty() && !b->id_mode, any_input = !b->inputs.empty();
    if (b->id_mode) {   // the ids of this run's inputs, ascending: what the tree's node ids are to a tree-mode build
        std::vector<u32>& ids = b->node_tid;
        ids = b->rec_taxid;
        for (const auto& in : b->inputs) ids.insert(ids.end(), in.nodes.begin(), in.nodes.end());
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        if (ids.size() > 0x7FFFFFFFull) return berr(b, LMAT_E_CAPACITY, "more than 2^31 distinct ids");
    }
    b->node_counts.assign(b->node_tid.size(), 0);
    memset(&b->mstats, 0, sizeof(b->mstats));
    BuildRun r;
    r.b = b;
    r.st = b->ctx->stream;
    r.T = b->text.size();
    r.n_rec = (u32)b->rec_start.size();
    if ((r.T == 0 || r.n_rec == 0) && !any_input) return LMAT_OK;
    r.number_owners();
    if (const int rc = r.plan(pb_forced, pb_start)) return rc;
    const int pb = r.pb;
    S.prefix_bits = (uint32_t)pb;
    S.passes = 1u << pb;
    if (const int rc = r.alloc()) return rc;

    // the per-taxid histogram of the final lists, and the merge with the tax_histo inputs when there are any
    MergeState tail;
    if (const int rc = tail.begin(b, pb, r.tree(), &r.timer)) return rc;
    if (r.fb) {
        b->mstats.inputs = (uint32_t)b->inputs.size();
        b->mstats.passes = 1u << pb;
        for (const auto& in : b->inputs) { b->mstats.records_in += in.kmers.size(); b->mstats.entries_in += in.nodes.size(); }
    }

    for (u32 pass = 0; pass < (1u << pb); ++pass) {
        if (r.fb) r.slice_inputs(pass);
        if (const int rc = r.extract(pass)) return rc;
        if (r.hc[C_OVERFLOW]) {
            if (pb_forced < 0) { retry = true; return berr(b, LMAT_E_CAPACITY, "pass buffer too small"); }
            return berr(b, LMAT_E_CAPACITY, "prefix pass " + std::to_string(pass) + " of " + std::to_string(1u << pb) + " emits " + std::to_string(r.hc[C_CURSOR]) +
                                               " pairs, the device budget holds " + std::to_string(r.cap) + ": raise the budget or prefix_bits");
        }
        u64 N = r.hc[C_CURSOR];
        if (pass == 0) S.windows = r.hc[C_WINDOWS];   // every pass sees every window; only the emitted pairs differ
        S.emitted_pairs += N;
        if (r.fb) {
            if (const int rc = r.append_inputs(N)) return rc;
            N += r.in_pairs;
        }
        if (N == 0) {
            if (merging) if (const int rc = tail.pass(pass, 0, nullptr, nullptr, nullptr, 0)) return rc;
            continue;
        }
        u32 R = 0;
        DevBuf* off = nullptr;
        if (const int rc = r.lists(N, R, off)) return rc;
        const u64 entries = r.hc[C_ENTRIES];
        S.dropped_unknown += r.hc[C_DROPPED];
        if (merging) {   // the pass's result stays on the device and is one more source of the merge
            if (const int rc = tail.pass(pass, R, r.pos.as<u64>(), off->as<u64>(), r.tids.as<u32>(), entries)) return rc;
            continue;
        }
        if (const int rc = tail.count_lists(r.tids.as<u32>(), entries)) return rc;
        if (const int rc = r.fetch(R, *off)) return rc;
        S.singletons += r.hc[C_SINGLETONS];
        S.total_list_entries += entries;
        S.longest_list = std::max<u64>(S.longest_list, r.hc[C_LONGEST]);
    }
    S.records_written = b->kmers.size();
    if (merging) {   // these four describe the merged result
        S.singletons = tail.singletons;
        S.total_list_entries = tail.entries;
        S.longest_list = tail.longest;
    }
    return tail.finish();
}

}  // namespace

extern "C" {

int lmat_db_begin(lmat_ctx* ctx, int k, uint64_t n_kmers_hint, uint64_t table_bytes);
int lmat_genedb_begin(lmat_ctx* ctx, int k, uint64_t n_kmers_hint, uint64_t table_bytes);
int lmat_db_finalize(lmat_ctx* ctx);

// The result goes through the ingest's own record parser as an in-memory stream of the file format, so the table is the one
// lmat_db_begin / lmat_db_add_taxhisto / lmat_db_finalize build from the written file.
int lmat_db_build_from_genomes(lmat_ctx* ctx, lmat_build* b, uint64_t table_bytes) {
    if (!ctx || !b) return LMAT_E_ARG;
    if (b->id_mode) return lmat::set_err(ctx, LMAT_E_ARG, "an id-set builder holds gene ids: lmat_genedb_build_from_genes makes its table");
    if (!b->done) return lmat::set_err(ctx, LMAT_E_ARG, "lmat_build_run first");
    if (!ctx->tax.loaded) return lmat::set_err(ctx, LMAT_E_ARG, "load the taxonomy before the k-mer database");
    char* mem = nullptr;
    size_t mem_len = 0;
    FILE* w = open_memstream(&mem, &mem_len);
    if (!w) return lmat::set_err(ctx, LMAT_E_NOMEM, "open_memstream failed");
    const bool ok = write_records(w, b);
    if (fclose(w) != 0 || !ok || !mem) { free(mem); return lmat::set_err(ctx, LMAT_E_NOMEM, "out of memory for the record stream"); }
    int rc = lmat_db_begin(ctx, b->k, 0, table_bytes);
    if (rc == LMAT_OK) {
        FILE* r = fmemopen(mem, mem_len, "rb");
        if (!r) rc = lmat::set_err(ctx, LMAT_E_NOMEM, "fmemopen failed");
        else if (!ctx->ingest->add_taxhisto_stream(r, "<built from genomes>")) {
            const bool tax = ctx->ingest->err.compare(0, 3, "bad") == 0;
            rc = lmat::set_err(ctx, tax ? LMAT_E_TAXONOMY : LMAT_E_IO, ctx->ingest->err);
        }
    }
    free(mem);
    if (rc == LMAT_OK) rc = lmat_db_finalize(ctx);
    return rc;
}

// The same for an id-set builder and a gene context (lmat_genedb_begin): no taxonomy anywhere.
int lmat_genedb_build_from_genes(lmat_ctx* ctx, lmat_build* b, uint64_t table_bytes) {
    if (!ctx || !b) return LMAT_E_ARG;
    if (!b->id_mode) return lmat::set_err(ctx, LMAT_E_ARG, "a tree-mode builder holds taxids: lmat_db_build_from_genomes makes its table");
    if (!b->done) return lmat::set_err(ctx, LMAT_E_ARG, "lmat_build_run first");
    char* mem = nullptr;
    size_t mem_len = 0;
    FILE* w = open_memstream(&mem, &mem_len);
    if (!w) return lmat::set_err(ctx, LMAT_E_NOMEM, "open_memstream failed");
    const bool ok = write_records(w, b);
    if (fclose(w) != 0 || !ok || !mem) { free(mem); return lmat::set_err(ctx, LMAT_E_NOMEM, "out of memory for the record stream"); }
    int rc = lmat_genedb_begin(ctx, b->k, 0, table_bytes);
    if (rc == LMAT_OK) {
        FILE* r = fmemopen(mem, mem_len, "rb");
        if (!r) rc = lmat::set_err(ctx, LMAT_E_NOMEM, "fmemopen failed");
        else if (!ctx->ingest->add_taxhisto_stream(r, "<built from genes>")) rc = lmat::set_err(ctx, LMAT_E_IO, ctx->ingest->err);
    }
    free(mem);
    if (rc == LMAT_OK) rc = lmat_db_finalize(ctx);
    return rc;
}

}  // extern "C"
