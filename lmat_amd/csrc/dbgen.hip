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
// hist_kernel counts, for either kind of run, the result records whose list holds each taxid (countTaxidFrequency's map).
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

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;

constexpr int kSpan = 992;        // window ends one wave covers: 62 blocks of 16 bases, behind 2 blocks (32 bases >= k - 1) of lead-in
constexpr int kLead = 32;         // bytes of text in front of a chunk (the k - 1 overlap, rounded up to the 16-byte loads)
constexpr int kWavesPerBlock = 4;
constexpr u32 kNoNode = 0xFFFFFFFFu;
constexpr u32 kMaxList = 65535;   // the record's count field is 16 bits wide (tax_histo.cpp:258-259)

// counters of one pass (device, 64-bit words)
enum { C_CURSOR = 0, C_OVERFLOW, C_WINDOWS, C_DROPPED, C_SINGLETONS, C_ENTRIES, C_LONGEST, C_TOOLONG, C_LONG_RUNS, C_LONG_ENTRIES, C_N };

__device__ __forceinline__ u32 lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// the memory of the wave's own LDS / global writes made visible to its other lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// reverse complement of a k-mer held in the low 2k bits (Encoder::rc): 2-bit groups reversed, complemented
__device__ __forceinline__ u64 revcomp(u64 x, int k) {
    u64 r = __brevll(x);
    r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
    return (~r) >> (64 - 2 * k);
}

struct ExtractArgs {
    const uint8_t* buf;      // chunk bytes: buf[kLead + i] = text[chunk_lo + i]; every wave's 1024-byte window is allocated and filled
    u64 chunk_lo;            // text position of buf[kLead]
    u32 chunk_len;           // window ends of this chunk: text[chunk_lo .. chunk_lo + chunk_len)
    const u64* rec_start;    // [n_rec] text position of the first base of every record, ascending
    const u32* rec_owner;    // [n_rec]
    u32 n_rec;
    int k, prefix_bits, owner_bits;   // owner_bits >= 0: key = k-mer << owner_bits | owner; -1: separate arrays
    u32 pass;
    u64* keys;
    u32* vals;
    u64 cap;
    u64* counters;
};

// Every wave covers kSpan consecutive window ends.  Phase 1: lane l packs the 16 bases at byte 16 l of the wave's 1024-byte
// window into one 32-bit word (first base in the high bits) and a mask of its invalid bytes; an inclusive max-scan over the
// lanes gives, per block, the last invalid byte at or before its end.  Phase 2: lane l of step s takes the window that ends at
// byte 32 + 64 s + l: the run of valid bases that ends there is the distance to the last invalid byte (the scan's value of the
// block before + the own block's mask), the k-mer is 2k bits cut from three packed words.
__global__ __launch_bounds__(64 * kWavesPerBlock) void extract_kernel(ExtractArgs a) {
    __shared__ u32 s_word[kWavesPerBlock][64];
    __shared__ int s_last[kWavesPerBlock][64];
    __shared__ u32 s_inv[kWavesPerBlock][64];
    const u32 lane = lane_id();
    const u32 wv = threadIdx.x >> 6;
    const u64 wave = (u64)blockIdx.x * kWavesPerBlock + wv;
    const u64 wbase = wave * kSpan;               // first window end of the wave, relative to the chunk
    if (wbase >= a.chunk_len) return;             // whole waves only: no block-wide barrier below
    {
        const uint4 q = *reinterpret_cast<const uint4*>(a.buf + wbase + 16 * lane);
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
        s_word[wv][lane] = word;
        s_inv[wv][lane] = inv;
        s_last[wv][lane] = last;
    }
    wave_sync();
    const int k = a.k;
    const u64 kmask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1);
    // the records this wave's span can touch
    u32 rlo, rhi;
    {
        const u64 p0 = a.chunk_lo + wbase, p1 = p0 + kSpan - 1;
        u32 lo = 0, hi = a.n_rec;
        while (lo < hi) { const u32 m = (lo + hi) >> 1; if (a.rec_start[m] <= p0) lo = m + 1; else hi = m; }
        rlo = lo ? lo - 1 : 0;
        hi = a.n_rec;
        while (lo < hi) { const u32 m = (lo + hi) >> 1; if (a.rec_start[m] <= p1) lo = m + 1; else hi = m; }
        rhi = lo;   // records [rlo, rhi)
    }
    u64 n_windows = 0;
    for (int step = 0; step * 64 < kSpan; ++step) {
        const u32 q = step * 64 + lane;            // window end within the span
        const u32 t = q + kLead;                   // ... as a byte of the wave's window
        bool emit = false;
        u64 canon = 0;
        if (q < (u32)kSpan && wbase + q < a.chunk_len) {
            const u32 bt = t >> 4, in = t & 15u;
            const u32 m = s_inv[wv][bt] & ((2u << in) - 1u);
            const int last = m ? (int)(16 * bt) + 31 - __clz((int)m) : s_last[wv][bt - 1];
            if ((int)t - last >= k) {
                const u64 lo = ((u64)s_word[wv][bt - 1] << 32) | s_word[wv][bt];
                const unsigned __int128 x = ((unsigned __int128)s_word[wv][bt - 2] << 64) | lo;
                const u64 fwd = (u64)(x >> (2 * (15 - in))) & kmask;
                const u64 rc = revcomp(fwd, k);
                canon = fwd < rc ? fwd : rc;
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
                u32 lo = rlo, hi = rhi;              // last record that starts at or before pos
                while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (a.rec_start[mid] <= pos) lo = mid; else hi = mid; }
                const u32 owner = a.rec_owner[lo];
                const u64 dst = base + __popcll(bal & ((1ull << lane) - 1));
                if (a.owner_bits >= 0) a.keys[dst] = (canon << a.owner_bits) | owner;
                else { a.keys[dst] = canon; a.vals[dst] = owner; }
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n_windows += __shfl_xor(n_windows, d);
    if (lane == 0 && n_windows) atomicAdd(&a.counters[C_WINDOWS], n_windows);
}

struct Sorted {   // the sorted pairs, either packing
    const u64* keys;
    const u32* vals;
    int owner_bits;
    __device__ __forceinline__ void get(u64 i, u64& km, u32& ow) const {
        if (owner_bits >= 0) { const u64 x = keys[i]; km = x >> owner_bits; ow = (u32)(x & ((1ull << owner_bits) - 1)); }
        else { km = keys[i]; ow = vals[i]; }
    }
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

struct ClosureArgs {
    u32 R;
    const u32* run_start;    // [R + 1]
    const u32* d_owner;      // distinct owners of every run, in Euler-tour order, unknown owners last
    u32 n_known;             // owner indices below this are tree nodes
    const u32* owner_node;   // [n_owner] dense node index
    const u32* parent;       // [n_nodes] dense; the root is its own parent
    const u32* depth;        // [n_nodes]
    const u32* node_tid;     // [n_nodes] ascending with the dense index
    u64* cnt;                // count pass: [R] list length
    const u64* off;          // write pass: [R + 1]
    u32* tids;               // write pass: the CSR
    u32* long_tmp;           // write pass: lists of more than 64 entries, unsorted, to be sorted by segment
    u32* long_begin;         // [n_long] segment bounds in long_tmp
    u32* long_end;
    u32* long_run;           // [n_long] the run of the segment
    u64* counters;
};

// depth-levelled parent walk
__device__ __forceinline__ u32 lca2(const u32* parent, const u32* depth, u32 a, u32 b) {
    u32 da = depth[a], db = depth[b];
    while (da > db) { a = parent[a]; --da; }
    while (db > da) { b = parent[b]; --db; }
    while (a != b) { a = parent[a]; b = parent[b]; }
    return a;
}

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
        if (kind == 1 && WRITE) a.tids[a.off[r]] = a.node_tid[a.owner_node[first]];
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
        const u32 top = lca2(a.parent, a.depth, a.owner_node[a.d_owner[rs]], a.owner_node[a.d_owner[rs + g - 1]]);
        u32 n = 0;
        bool is_long = false;
        u32 long_at = 0, long_slot = 0;
        u32* dst = nullptr;
        if (WRITE) {
            n = (u32)(a.off[rr + 1] - a.off[rr]);
            is_long = n > 64;
            if (is_long) {
                if (lane == 0) {
                    long_slot = (u32)atomicAdd(&a.counters[C_LONG_RUNS], 1ull);
                    long_at = (u32)atomicAdd(&a.counters[C_LONG_ENTRIES], (u64)n);
                    a.long_begin[long_slot] = long_at;
                    a.long_end[long_slot] = long_at + n;
                    a.long_run[long_slot] = rr;
                }
                long_at = __shfl(long_at, 0);
                dst = a.long_tmp + long_at;
            } else dst = &s_stage[wv][0];
        }
        u32 total = 0;
        for (u32 base = 0; base < g; base += 64) {
            const u32 j = base + lane;
            u32 node = 0, len = 0;
            if (j < g) {
                node = a.owner_node[a.d_owner[rs + j]];
                if (j == 0) len = a.depth[node] - a.depth[top] + 1;
                else len = a.depth[node] - a.depth[lca2(a.parent, a.depth, a.owner_node[a.d_owner[rs + j - 1]], node)];
            }
            u32 incl = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u32 o = __shfl_up(incl, d);
                if ((int)lane >= d) incl += o;
            }
            if (WRITE) {
                u32 at = total + incl - len;
                for (u32 x = node, i = 0; i < len; ++i, x = a.parent[x]) dst[at++] = a.node_tid[x];
            }
            total += __shfl(incl, 63);
        }
        if (!WRITE) {
            if (lane == 0) {
                a.cnt[rr] = total;
                atomicAdd(&a.counters[C_ENTRIES], (u64)total);
                atomicMax(&a.counters[C_LONGEST], (u64)total);
                if (total == 1) atomicAdd(&a.counters[C_SINGLETONS], 1ull);
                if (total > kMaxList) atomicMax(&a.counters[C_TOOLONG], (u64)total);
                if (total > 64) { atomicAdd(&a.counters[C_LONG_RUNS], 1ull); atomicAdd(&a.counters[C_LONG_ENTRIES], (u64)total); }
            }
        } else if (!is_long) {
            // ascending order within the wave: the entries are distinct, the rank of one is the number of smaller ones
            wave_sync();
            const u32 v = lane < n ? s_stage[wv][lane] : 0xFFFFFFFFu;
            u32 rank = 0;
            for (u32 t = 0; t < n; ++t) rank += s_stage[wv][t] < v ? 1u : 0u;
            if (lane < n) a.tids[a.off[rr] + rank] = v;
            wave_sync();
        }
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
    const u32* parent;
    const u32* depth;
    const u32* node_tid;
    u32* aux;                // [R] runs with several sources: kSmall, or the slot of the side-buffer segment
    u32* big_run;            // [slots]
    u32* big_begin;          // [slots] segment of the gathered tour indices
    u32* big_end;
    const u32* big_sorted;
    u64* cnt;                // [R]
    const u64* off;          // write pass: [R + 1]
    u32* tids;
    u32* long_tmp;
    u32* long_begin;
    u32* long_end;
    u32* long_run;
    u64* counters;
};

template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

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
    u32 longest = one ? G : 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) longest = max(longest, (u32)__shfl_xor(longest, d));
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
// the segment sorted beforehand), equal neighbours are one entry, and the walk of closure_kernel gives the closure in disjoint pieces.
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
                    dst[i] = a.node_tid[x];
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
        bool is_long = false;
        u32 long_at = 0;
        u32* dst = &s_stage[wv][0];
        if (WRITE) {
            n = (u32)(a.off[rr + 1] - a.off[rr]);
            is_long = n > 64;
            if (is_long) {
                if (lane == 0) {
                    const u32 slot = (u32)atomicAdd(&a.counters[C_LONG_RUNS], 1ull);
                    long_at = (u32)atomicAdd(&a.counters[C_LONG_ENTRIES], (u64)n);
                    a.long_begin[slot] = long_at;
                    a.long_end[slot] = long_at + n;
                    a.long_run[slot] = rr;
                }
                long_at = __shfl(long_at, 0);
                dst = a.long_tmp + long_at;
            }
        }
        if (re - rs == 1) {   // write pass only: the copy of a list that does not ascend or is long
            const u32 q = a.rec[rs], b0 = a.rec_off[q];
            for (u32 i = lane; i < n; i += 64) dst[i] = a.node_tid[a.ent[b0 + i]];
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
            const u32 top = lca2(a.parent, a.depth, a.node_at[seq[0]], a.node_at[seq[G - 1]]);
            u32 total = 0, distinct = 0;
            for (u32 base = 0; base < G; base += 64) {
                const u32 j = base + lane;
                u32 node = 0, len = 0;
                bool fresh = false;
                if (j < G) {
                    const u32 t = seq[j];
                    node = a.node_at[t];
                    if (j == 0) { len = a.depth[node] - a.depth[top] + 1; fresh = true; }
                    else {
                        const u32 tp = seq[j - 1];
                        fresh = tp != t;
                        if (fresh) len = a.depth[node] - a.depth[lca2(a.parent, a.depth, a.node_at[tp], node)];
                    }
                }
                u32 incl = len;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const u32 o = __shfl_up(incl, d);
                    if ((int)lane >= d) incl += o;
                }
                if (WRITE) {
                    u32 at = total + incl - len;
                    for (u32 x = node, i = 0; i < len; ++i, x = a.parent[x]) dst[at++] = a.node_tid[x];
                }
                total += __shfl(incl, 63);
                distinct += __popcll(__ballot(fresh));
            }
            if (!WRITE && lane == 0) {
                a.cnt[rr] = total;
                atomicAdd(&a.counters[C_ENTRIES], (u64)total);
                atomicMax(&a.counters[C_LONGEST], (u64)total);
                if (total == 1) atomicAdd(&a.counters[C_SINGLETONS], 1ull);
                if (total > distinct) atomicAdd(&a.counters[M_GROWN], 1ull);
                if (total > kMaxList) atomicMax(&a.counters[C_TOOLONG], (u64)total);
                if (total > 64) { atomicAdd(&a.counters[C_LONG_RUNS], 1ull); atomicAdd(&a.counters[C_LONG_ENTRIES], (u64)total); }
            }
        }
        if (WRITE && !is_long) {
            // ascending order within the wave: the entries are distinct, the rank of one is the number of smaller ones
            wave_sync();
            const u32 v = lane < n ? s_stage[wv][lane] : 0xFFFFFFFFu;
            u32 rank = 0;
            for (u32 t = 0; t < n; ++t) rank += s_stage[wv][t] < v ? 1u : 0u;
            if (lane < n) a.tids[a.off[rr] + rank] = v;
            wave_sync();
        }
    }
}

// hist[node] += 1 for every entry of the final lists: the number of records whose list holds the taxid
__global__ __launch_bounds__(256) void hist_kernel(const u32* tids, u64 n, const u32* node_tid, u32 n_nodes, u64* hist) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&hist[node_of_tid(node_tid, n_nodes, tids[i])], 1ull);
}

// ------------------------------------------------------------------------------------------------------------------ host
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        if (p) { hipFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, std::max<size_t>(n, 256));
        if (e == hipSuccess) bytes = std::max<size_t>(n, 256);
        return e;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace

struct lmat_build {
    lmat_ctx* ctx = nullptr;
    int k = 0;
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
        std::vector<u32> nodes;
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
        if (n) {
            const size_t at = in.nodes.size();
            in.nodes.resize(at + n);
            for (u32 j = 0; j < n; ++j) {
                u32 t;
                memcpy(&t, &buf[pos + 4 * (size_t)j], 4);
                auto it = b->node_of.find(t);
                if (it == b->node_of.end()) return berr(b, LMAT_E_TAXONOMY, name + ": taxid " + std::to_string(t) + " of record " + std::to_string(i) + " is not in the taxonomy tree");
                in.nodes[at + j] = it->second;
            }
            if (n > 1) {
                chk.assign(in.nodes.begin() + at, in.nodes.end());
                std::sort(chk.begin(), chk.end());
                auto dup = std::adjacent_find(chk.begin(), chk.end());
                if (dup != chk.end()) return berr(b, LMAT_E_IO, name + ": taxid " + std::to_string(b->node_tid[*dup]) + " repeated in the list of record " + std::to_string(i));
            }
            in.kmers.push_back(km);      // a record without a list carries nothing
            in.off.push_back(in.nodes.size());
        }
        pos += (size_t)n * 4;
        if ((i + 1) % 1500 == 0) {
            if (end - pos < 8 || memcmp(&buf[pos], &test, 8) != 0) return berr(b, LMAT_E_IO, name + ": tax_histo sanity word missing after record " + std::to_string(i));
            pos += 8;
        }
    }
    if (pos != end) return berr(b, LMAT_E_IO, name + ": " + std::to_string(end - pos) + " bytes behind the last record");
    return LMAT_OK;
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
    while ((len = getline(&line, &cap, f)) >= 0) {
        ++lineno;
        while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) --len;
        if (len == 0) continue;
        if (line[0] == '>') {
            if (len < 2 || line[1] < '0' || line[1] > '9') {
                rc = berr(b, LMAT_E_IO, std::string("bad FASTA header (want '>' + decimal taxid) at line ") + std::to_string(lineno) + " of " + fn);
                break;
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
    // KmerFileMetaData.cpp:16-31 with tax_histo's version; lists are written in ascending taxid order (the reference writes
    // them in unordered_map iteration order; readers do not rely on either)
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

// The tail of every pass: the merge with the tax_histo inputs (when there are any) and the per-taxid histogram of the final lists.
struct MergeState {
    lmat_build* b = nullptr;
    hipStream_t st = nullptr;
    bool merging = false;
    int pb = 0, sb = 1;
    std::vector<size_t> cursor;           // next record of every input: the passes ascend, an input's slices follow each other
    std::vector<u32> node_at;
    DevBuf tin, d_node_at, hist, counters, totals, keysA, keysB, valsA, valsB, rec_off, ent, flag, pos, run, cnt, off, aux, big_run, big_begin, big_end,
        big_tmp, big_sorted, out, out_km, long_tmp, long_sorted, long_begin, long_end, long_run, temp;
    const u32 *parent = nullptr, *depth = nullptr, *node_tid = nullptr;
    u32 n_nodes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    u64 singletons = 0, entries = 0, longest = 0;
    ~MergeState() { if (ev[0]) hipEventDestroy(ev[0]); if (ev[1]) hipEventDestroy(ev[1]); }

    hipError_t lap(float& acc) {
        hipError_t e = hipEventRecord(ev[1], st);
        if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
        acc += ms;
        if (e == hipSuccess) e = hipEventRecord(ev[0], st);
        return e;
    }

    int begin(lmat_build* b_, int pb_, const u32* d_parent, const u32* d_depth, const u32* d_node_tid) {
        b = b_;
        st = b->ctx->stream;
        pb = pb_;
        parent = d_parent;
        depth = d_depth;
        node_tid = d_node_tid;
        n_nodes = (u32)b->node_tid.size();
        merging = !b->inputs.empty();
        memset(&b->mstats, 0, sizeof(b->mstats));
        b->node_counts.assign(n_nodes, 0);
        BHIP(b, hist.ensure((size_t)n_nodes * 8));
        BHIP(b, hipMemsetAsync(hist.p, 0, (size_t)n_nodes * 8, st));
        if (!merging) return LMAT_OK;
        BHIP(b, hipEventCreate(&ev[0]));
        BHIP(b, hipEventCreate(&ev[1]));
        sb = 1;
        while ((1ull << sb) < b->inputs.size() + 1) ++sb;   // the genomes' own result is the source behind the inputs
        cursor.assign(b->inputs.size(), 0);
        node_at.assign(n_nodes, 0);
        for (u32 i = 0; i < n_nodes; ++i) node_at[b->tin[i]] = i;
        BHIP(b, tin.ensure((size_t)n_nodes * 4));
        BHIP(b, d_node_at.ensure((size_t)n_nodes * 4));
        BHIP(b, counters.ensure(M_TOTAL * 8));
        BHIP(b, totals.ensure(16));
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
        hipLaunchKernelGGL(hist_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, d_tids, n, node_tid, n_nodes, hist.as<u64>());
        BHIP(b, hipGetLastError());
        return LMAT_OK;
    }

    // One prefix pass: the inputs' slices and the genomes' result of the pass (gR runs: k-mer, CSR of ascending taxids, runs without a list
    // included) -> records appended to the builder's result.
    int pass(u32 pass_no, u32 gR, const u64* g_kmer, const u64* g_off, const u32* g_tids, u64 g_entries) {
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
        if (Nr64 == 0) return LMAT_OK;
        if (Nr64 > 0x7FFFFFFFull || Ne64 > 0xFFFFFF00ull) return berr(b, LMAT_E_CAPACITY, "more than 2^31 records or 2^32 list entries to merge in one prefix pass: raise prefix_bits");
        const u32 Nr = (u32)Nr64;
        lmat_merge_stats& M = b->mstats;
        const u32 slots = (u32)(Ne64 / 65 + 1);   // a side-buffer segment holds more than 64 entries
        BHIP(b, keysA.ensure((size_t)Nr * 8));
        BHIP(b, keysB.ensure((size_t)Nr * 8));
        BHIP(b, valsA.ensure((size_t)Nr * 4));
        BHIP(b, valsB.ensure((size_t)Nr * 4));
        BHIP(b, rec_off.ensure(((size_t)Nr + 1) * 4));
        BHIP(b, ent.ensure((size_t)Ne64 * 4));
        BHIP(b, flag.ensure((size_t)Nr * 4));
        BHIP(b, pos.ensure((size_t)Nr * 4));
        BHIP(b, run.ensure(((size_t)Nr + 1) * 4));
        BHIP(b, cnt.ensure((size_t)Nr * 8));
        BHIP(b, off.ensure(((size_t)Nr + 1) * 8));
        BHIP(b, aux.ensure((size_t)Nr * 4));
        BHIP(b, out_km.ensure((size_t)Nr * 8));
        BHIP(b, big_run.ensure((size_t)slots * 4));
        BHIP(b, big_begin.ensure((size_t)slots * 4));
        BHIP(b, big_end.ensure((size_t)slots * 4));
        BHIP(b, hipMemsetAsync(counters.p, 0, M_TOTAL * 8, st));
        BHIP(b, hipEventRecord(ev[0], st));
        if (Nin) BHIP(b, hipMemcpyAsync(keysA.p, h_keys.data(), (size_t)Nin * 8, hipMemcpyHostToDevice, st));
        BHIP(b, hipMemcpyAsync(rec_off.p, h_off.data(), ((size_t)Nin + 1) * 4, hipMemcpyHostToDevice, st));
        if (Ein) BHIP(b, hipMemcpyAsync(ent.p, h_ent.data(), (size_t)Ein * 4, hipMemcpyHostToDevice, st));
        const int key_bits = 2 * k + sb;
        if (gR) {
            hipLaunchKernelGGL(genome_source_kernel, dim3((gR + 255) / 256), dim3(256), 0, st, gR, g_kmer, g_off, (u32)Nin, (u32)Ein, (u32)n_in, sb, key_bits,
                               keysA.as<u64>(), rec_off.as<u32>(), counters.as<u64>());
            BHIP(b, hipGetLastError());
            if (g_entries) {
                hipLaunchKernelGGL(tid_to_node_kernel, dim3((u32)((g_entries + 255) / 256)), dim3(256), 0, st, g_tids, g_entries, node_tid, n_nodes, ent.as<u32>() + Ein);
                BHIP(b, hipGetLastError());
            }
        }
        hipLaunchKernelGGL(iota_kernel, dim3((Nr + 255) / 256), dim3(256), 0, st, valsA.as<u32>(), Nr);
        BHIP(b, hipGetLastError());
        BHIP(b, hipStreamSynchronize(st));   // the host vectors go out of use here
        BHIP(b, lap(M.upload_ms));

        // ---- one key per record, sorted by (k-mer, source); records without a list behind all others
        {
            size_t tb = 0;
            BHIP(b, rocprim::radix_sort_pairs(nullptr, tb, keysA.as<u64>(), keysB.as<u64>(), valsA.as<u32>(), valsB.as<u32>(), Nr, 0, key_bits + 1, st));
            BHIP(b, temp.ensure(tb));
            BHIP(b, rocprim::radix_sort_pairs(temp.p, tb, keysA.as<u64>(), keysB.as<u64>(), valsA.as<u32>(), valsB.as<u32>(), Nr, 0, key_bits + 1, st));
        }
        u64 hc[M_TOTAL];
        BHIP(b, hipMemcpyAsync(hc, counters.p, M_TOTAL * 8, hipMemcpyDeviceToHost, st));
        BHIP(b, lap(M.sort_ms));
        const u32 Nv = Nr - (u32)hc[M_EMPTY];
        if (Nv == 0) return LMAT_OK;

        // ---- runs of one k-mer
        const u32 gridN = (Nv + 255) / 256;
        hipLaunchKernelGGL(mseg_flag_kernel, dim3(gridN), dim3(256), 0, st, keysB.as<u64>(), Nv, sb, flag.as<u32>());
        BHIP(b, hipGetLastError());
        {
            size_t tb = 0;
            BHIP(b, rocprim::exclusive_scan(nullptr, tb, flag.as<u32>(), pos.as<u32>(), 0u, (size_t)Nv, rocprim::plus<u32>(), st));
            BHIP(b, temp.ensure(tb));
            BHIP(b, rocprim::exclusive_scan(temp.p, tb, flag.as<u32>(), pos.as<u32>(), 0u, (size_t)Nv, rocprim::plus<u32>(), st));
        }
        hipLaunchKernelGGL(mseg_scatter_kernel, dim3(gridN), dim3(256), 0, st, flag.as<u32>(), pos.as<u32>(), Nv, run.as<u32>(), totals.as<u64>());
        BHIP(b, hipGetLastError());
        u64 tot[2];
        BHIP(b, hipMemcpyAsync(tot, totals.p, 16, hipMemcpyDeviceToHost, st));
        BHIP(b, lap(M.segment_ms));
        const u32 R = (u32)tot[0];

        // ---- union: classify, side-buffer segments in tour order, count, scan, write
        UnionArgs ua;
        memset(&ua, 0, sizeof(ua));
        ua.R = R;
        ua.run_start = run.as<u32>();
        ua.rec = valsB.as<u32>();
        ua.rec_off = rec_off.as<u32>();
        ua.ent = ent.as<u32>();
        ua.tin = tin.as<u32>();
        ua.node_at = d_node_at.as<u32>();
        ua.parent = parent;
        ua.depth = depth;
        ua.node_tid = node_tid;
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
            BHIP(b, big_tmp.ensure(big_entries * 4));
            BHIP(b, big_sorted.ensure(big_entries * 4));
            hipLaunchKernelGGL(big_gather_kernel, dim3((u32)n_big), dim3(256), 0, st, ua, big_tmp.as<u32>());
            BHIP(b, hipGetLastError());
            size_t tb = 0;
            BHIP(b, rocprim::segmented_radix_sort_keys(nullptr, tb, big_tmp.as<u32>(), big_sorted.as<u32>(), (unsigned)big_entries, (unsigned)n_big,
                                                       big_begin.as<u32>(), big_end.as<u32>(), 0, 32, st));
            BHIP(b, temp.ensure(tb));
            BHIP(b, rocprim::segmented_radix_sort_keys(temp.p, tb, big_tmp.as<u32>(), big_sorted.as<u32>(), (unsigned)big_entries, (unsigned)n_big,
                                                       big_begin.as<u32>(), big_end.as<u32>(), 0, 32, st));
            ua.big_sorted = big_sorted.as<u32>();
        }
        const u32 gridR = (u32)(((u64)R + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock));
        hipLaunchKernelGGL(union_kernel<false>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ua);
        BHIP(b, hipGetLastError());
        {
            size_t tb = 0;
            BHIP(b, rocprim::exclusive_scan(nullptr, tb, cnt.as<u64>(), off.as<u64>(), 0ull, (size_t)R, rocprim::plus<u64>(), st));
            BHIP(b, temp.ensure(tb));
            BHIP(b, rocprim::exclusive_scan(temp.p, tb, cnt.as<u64>(), off.as<u64>(), 0ull, (size_t)R, rocprim::plus<u64>(), st));
        }
        BHIP(b, hipMemcpyAsync(hc, counters.p, M_TOTAL * 8, hipMemcpyDeviceToHost, st));
        BHIP(b, hipStreamSynchronize(st));
        if (hc[C_TOOLONG])
            return berr(b, LMAT_E_CAPACITY, "a merged taxid list of " + std::to_string(hc[C_TOOLONG]) + " entries: the tax_histo record holds at most 65535");
        const u64 n_entries = hc[C_ENTRIES], n_long = hc[C_LONG_RUNS], long_entries = hc[C_LONG_ENTRIES];
        if (long_entries > 0xFFFFFFF0ull) return berr(b, LMAT_E_CAPACITY, "more than 2^32 entries in lists beyond 64 taxids in one pass: raise prefix_bits");
        BHIP(b, hipMemcpyAsync(off.as<u64>() + R, &n_entries, 8, hipMemcpyHostToDevice, st));
        BHIP(b, out.ensure(n_entries * 4));
        if (n_long) {
            BHIP(b, long_tmp.ensure(long_entries * 4));
            BHIP(b, long_sorted.ensure(long_entries * 4));
            BHIP(b, long_begin.ensure(n_long * 4));
            BHIP(b, long_end.ensure(n_long * 4));
            BHIP(b, long_run.ensure(n_long * 4));
        }
        BHIP(b, hipMemsetAsync(counters.as<u64>() + C_LONG_RUNS, 0, 16, st));   // the write pass hands out the long lists' places with them
        ua.off = off.as<u64>();
        ua.tids = out.as<u32>();
        ua.long_tmp = long_tmp.as<u32>();
        ua.long_begin = long_begin.as<u32>();
        ua.long_end = long_end.as<u32>();
        ua.long_run = long_run.as<u32>();
        hipLaunchKernelGGL(union_kernel<true>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ua);
        BHIP(b, hipGetLastError());
        if (n_long) {
            size_t tb = 0;
            BHIP(b, rocprim::segmented_radix_sort_keys(nullptr, tb, long_tmp.as<u32>(), long_sorted.as<u32>(), (unsigned)long_entries, (unsigned)n_long,
                                                       long_begin.as<u32>(), long_end.as<u32>(), 0, 32, st));
            BHIP(b, temp.ensure(tb));
            BHIP(b, rocprim::segmented_radix_sort_keys(temp.p, tb, long_tmp.as<u32>(), long_sorted.as<u32>(), (unsigned)long_entries, (unsigned)n_long,
                                                       long_begin.as<u32>(), long_end.as<u32>(), 0, 32, st));
            hipLaunchKernelGGL(long_copy_kernel, dim3((u32)n_long), dim3(256), 0, st, long_sorted.as<u32>(), long_begin.as<u32>(), long_end.as<u32>(),
                               long_run.as<u32>(), off.as<u64>(), out.as<u32>());
            BHIP(b, hipGetLastError());
        }
        const u64 kmask = (1ull << (2 * k)) - 1;
        hipLaunchKernelGGL(mrun_kmer_kernel, dim3((R + 255) / 256), dim3(256), 0, st, keysB.as<u64>(), run.as<u32>(), R, sb, kmask, out_km.as<u64>());
        BHIP(b, hipGetLastError());
        BHIP(b, lap(M.union_ms));
        const int rc = count_lists(out.as<u32>(), n_entries);
        if (rc) return rc;
        BHIP(b, lap(M.histogram_ms));

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

int run_build(lmat_build* b, int pb_forced, int pb_start, bool& retry) {
    lmat_ctx* c = b->ctx;
    hipStream_t st = c->stream;
    const int k = b->k;
    lmat_build_stats& S = b->stats;
    memset(&S, 0, sizeof(S));
    b->kmers.clear();
    b->tids.clear();
    b->list_off.assign(1, 0);
    S.bases = b->bases;
    const u64 T = b->text.size();
    const u32 n_rec = (u32)b->rec_start.size();
    if (b->rec_start.size() > 0x7FFFFFFFull) return berr(b, LMAT_E_CAPACITY, "more than 2^31 FASTA records");
    const bool merging = !b->inputs.empty();
    b->node_counts.assign(b->node_tid.size(), 0);
    memset(&b->mstats, 0, sizeof(b->mstats));
    if ((T == 0 || n_rec == 0) && !merging) return LMAT_OK;

    // owners: distinct taxids; the tree's own in Euler-tour order, the others behind them
    std::vector<u32> owners(b->rec_taxid);
    std::sort(owners.begin(), owners.end());
    owners.erase(std::unique(owners.begin(), owners.end()), owners.end());
    std::vector<std::pair<u64, u32>> order;   // (sort key, taxid)
    u32 n_known = 0;
    for (u32 t : owners) {
        auto it = b->node_of.find(t);
        if (it != b->node_of.end()) { order.push_back(std::make_pair((u64)b->tin[it->second], t)); ++n_known; }
        else order.push_back(std::make_pair((1ull << 32) | t, t));
    }
    std::sort(order.begin(), order.end());
    const u32 n_owner = (u32)order.size();
    std::unordered_map<u32, u32> owner_of;
    std::vector<u32> owner_node(n_owner, kNoNode);
    for (u32 i = 0; i < n_owner; ++i) {
        owner_of[order[i].second] = i;
        if (i < n_known) owner_node[i] = b->node_of[order[i].second];
    }
    std::vector<u32> rec_owner(n_rec);
    for (u32 r = 0; r < n_rec; ++r) rec_owner[r] = owner_of[b->rec_taxid[r]];
    int ob = 1;
    while ((1ull << ob) < n_owner) ++ob;
    // one 64-bit key when the owner fits behind the k-mer, else (owner, k-mer) pairs sorted twice; LMAT_DBGEN_SORT=pairs forces the latter
    bool packed = 2 * k + ob <= 64;
    if (const char* e = getenv("LMAT_DBGEN_SORT")) if (!strcmp(e, "pairs")) packed = false;

    // memory model: everything below is sized by cap, the pairs one pass may emit
    u64 budget = b->budget;
    if (!budget) {
        size_t fr = 0, tot = 0;
        BHIP(b, hipMemGetInfo(&fr, &tot));
        budget = fr / 2;
    }
    const u32 chunk = T == 0 ? 1024u : b->chunk_bases ? std::max<u32>(b->chunk_bases, 1024) : (1u << 24);   // T == 0: a merge of tax_histo inputs alone
    const u64 chunk_waves = ((u64)chunk + kSpan - 1) / kSpan;
    const u64 chunk_alloc = chunk_waves * kSpan + kLead + 64;
    const u64 fixed = chunk_alloc + (u64)n_rec * 12 + (u64)b->node_tid.size() * 12 + (u64)n_owner * 4 + (64u << 20);   // + sort scratch and slack
    const u64 per_pair = 8 + 8 + 8 + 8 + 8 + 4 + 4 + (packed ? 0 : 8) + 16;   // keys x2, flag, pos, distinct pair, run start, (vals x2), list entries (estimate)
    if (budget <= fixed || (budget <= fixed + per_pair * 1024 && T != 0)) return berr(b, LMAT_E_NOMEM, "device budget of " + std::to_string(budget) + " bytes is below the fixed buffers");
    u64 cap = std::min<u64>((budget - fixed) / per_pair, 0x7FFFFF00ull);
    int pb = pb_forced;
    if (pb < 0) {
        // canonical k-mers crowd the low prefixes (min of a k-mer and its reverse complement): up to twice the even share
        pb = pb_start;
        while (pb < std::min(2 * k, 24) && (double)T * 2.0 / (double)(1ull << pb) > (double)cap && T > cap) ++pb;
        if (pb == 0 && T > cap) pb = 1;
    }
    if (merging) {
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
    S.prefix_bits = (uint32_t)pb;
    S.passes = 1u << pb;

    DevBuf d_text, d_rec_start, d_rec_owner, d_owner_node, d_parent, d_depth, d_node_tid, d_counters, d_keysA, d_keysB, d_valsA, d_valsB,
        d_flag, d_pos, d_dk, d_do, d_run, d_temp, d_tids, d_long_tmp, d_long_sorted, d_long_begin, d_long_end, d_long_run, d_totals;
    BHIP(b, d_text.ensure(chunk_alloc));
    BHIP(b, d_rec_start.ensure((size_t)n_rec * 8));
    BHIP(b, d_rec_owner.ensure((size_t)n_rec * 4));
    BHIP(b, d_owner_node.ensure((size_t)n_owner * 4));
    BHIP(b, d_parent.ensure(b->parent.size() * 4));
    BHIP(b, d_depth.ensure(b->depth.size() * 4));
    BHIP(b, d_node_tid.ensure(b->node_tid.size() * 4));
    BHIP(b, d_counters.ensure(C_N * 8));
    BHIP(b, d_totals.ensure(16));
    BHIP(b, d_keysA.ensure(cap * 8));
    BHIP(b, d_keysB.ensure(cap * 8));
    if (!packed) { BHIP(b, d_valsA.ensure(cap * 4)); BHIP(b, d_valsB.ensure(cap * 4)); }
    BHIP(b, d_flag.ensure(cap * 8));
    BHIP(b, d_pos.ensure(cap * 8));
    BHIP(b, d_dk.ensure(cap * 8));
    BHIP(b, d_do.ensure(cap * 4));
    BHIP(b, d_run.ensure((cap + 1) * 4));
    if (n_rec) {
        BHIP(b, hipMemcpyAsync(d_rec_start.p, b->rec_start.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
        BHIP(b, hipMemcpyAsync(d_rec_owner.p, rec_owner.data(), (size_t)n_rec * 4, hipMemcpyHostToDevice, st));
        BHIP(b, hipMemcpyAsync(d_owner_node.p, owner_node.data(), (size_t)n_owner * 4, hipMemcpyHostToDevice, st));
    }
    BHIP(b, hipMemcpyAsync(d_parent.p, b->parent.data(), b->parent.size() * 4, hipMemcpyHostToDevice, st));
    BHIP(b, hipMemcpyAsync(d_depth.p, b->depth.data(), b->depth.size() * 4, hipMemcpyHostToDevice, st));
    BHIP(b, hipMemcpyAsync(d_node_tid.p, b->node_tid.data(), b->node_tid.size() * 4, hipMemcpyHostToDevice, st));
    BHIP(b, hipStreamSynchronize(st));
    uint8_t* stage = nullptr;
    BHIP(b, hipHostMalloc((void**)&stage, chunk_alloc));
    struct StageFree { uint8_t* p; ~StageFree() { hipHostFree(p); } } stage_free{stage};
    hipEvent_t ev[2];
    BHIP(b, hipEventCreate(&ev[0]));
    BHIP(b, hipEventCreate(&ev[1]));
    struct EvFree { hipEvent_t* e; ~EvFree() { hipEventDestroy(e[0]); hipEventDestroy(e[1]); } } ev_free{ev};
    auto lap = [&](float& acc) -> hipError_t {   // time on the stream since the last mark
        hipError_t e = hipEventRecord(ev[1], st);
        if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
        acc += ms;
        if (e == hipSuccess) e = hipEventRecord(ev[0], st);
        return e;
    };

    // the per-taxid histogram of the final lists, and the merge with the tax_histo inputs when there are any
    MergeState tail;
    if (const int rc = tail.begin(b, pb, d_parent.as<u32>(), d_depth.as<u32>(), d_node_tid.as<u32>())) return rc;

    u64 host_c[C_N];
    for (u32 pass = 0; pass < (1u << pb); ++pass) {
        BHIP(b, hipMemsetAsync(d_counters.p, 0, C_N * 8, st));
        BHIP(b, hipEventRecord(ev[0], st));
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
            BHIP(b, hipMemcpyAsync(d_text.p, stage, bytes, hipMemcpyHostToDevice, st));
            ExtractArgs a;
            a.buf = d_text.as<uint8_t>();
            a.chunk_lo = lo;
            a.chunk_len = len;
            a.rec_start = d_rec_start.as<u64>();
            a.rec_owner = d_rec_owner.as<u32>();
            a.n_rec = n_rec;
            a.k = k;
            a.prefix_bits = pb;
            a.owner_bits = packed ? ob : -1;
            a.pass = pass;
            a.keys = d_keysA.as<u64>();
            a.vals = d_valsA.as<u32>();
            a.cap = cap;
            a.counters = d_counters.as<u64>();
            const u32 grid = (u32)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
            hipLaunchKernelGGL(extract_kernel, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, a);
            BHIP(b, hipGetLastError());
            BHIP(b, hipStreamSynchronize(st));   // the staging buffer is refilled next
        }
        BHIP(b, lap(S.extract_ms));
        BHIP(b, hipMemcpy(host_c, d_counters.p, C_N * 8, hipMemcpyDeviceToHost));
        if (host_c[C_OVERFLOW]) {
            if (pb_forced < 0) { retry = true; return berr(b, LMAT_E_CAPACITY, "pass buffer too small"); }
            return berr(b, LMAT_E_CAPACITY, "prefix pass " + std::to_string(pass) + " of " + std::to_string(1u << pb) + " emits " + std::to_string(host_c[C_CURSOR]) +
                                               " pairs, the device budget holds " + std::to_string(cap) + ": raise the budget or prefix_bits");
        }
        const u64 N = host_c[C_CURSOR];
        if (pass == 0) S.windows = host_c[C_WINDOWS];   // every pass sees every window; only the emitted pairs differ
        S.emitted_pairs += N;
        if (N == 0) {
            if (merging) if (const int rc = tail.pass(pass, 0, nullptr, nullptr, nullptr, 0)) return rc;
            continue;
        }

        // ---- sort by (k-mer, owner)
        Sorted sorted;
        sorted.owner_bits = packed ? ob : -1;
        if (packed) {
            size_t tb = 0;
            BHIP(b, rocprim::radix_sort_keys(nullptr, tb, d_keysA.as<u64>(), d_keysB.as<u64>(), N, 0, 2 * k + ob, st));
            BHIP(b, d_temp.ensure(tb));
            BHIP(b, rocprim::radix_sort_keys(d_temp.p, tb, d_keysA.as<u64>(), d_keysB.as<u64>(), N, 0, 2 * k + ob, st));
            sorted.keys = d_keysB.as<u64>();
            sorted.vals = nullptr;
        } else {
            size_t tb1 = 0, tb2 = 0;
            BHIP(b, rocprim::radix_sort_pairs(nullptr, tb1, d_valsA.as<u32>(), d_valsB.as<u32>(), d_keysA.as<u64>(), d_keysB.as<u64>(), N, 0, ob, st));
            BHIP(b, rocprim::radix_sort_pairs(nullptr, tb2, d_keysB.as<u64>(), d_keysA.as<u64>(), d_valsB.as<u32>(), d_valsA.as<u32>(), N, 0, 2 * k, st));
            BHIP(b, d_temp.ensure(std::max(tb1, tb2)));
            BHIP(b, rocprim::radix_sort_pairs(d_temp.p, tb1, d_valsA.as<u32>(), d_valsB.as<u32>(), d_keysA.as<u64>(), d_keysB.as<u64>(), N, 0, ob, st));
            BHIP(b, rocprim::radix_sort_pairs(d_temp.p, tb2, d_keysB.as<u64>(), d_keysA.as<u64>(), d_valsB.as<u32>(), d_valsA.as<u32>(), N, 0, 2 * k, st));
            sorted.keys = d_keysA.as<u64>();
            sorted.vals = d_valsA.as<u32>();
        }
        BHIP(b, lap(S.sort_ms));

        // ---- distinct pairs and run heads
        const u32 gridN = (u32)((N + 255) / 256);
        hipLaunchKernelGGL(seg_flag_kernel, dim3(gridN), dim3(256), 0, st, sorted, N, d_flag.as<u64>());
        BHIP(b, hipGetLastError());
        {
            size_t tb = 0;
            BHIP(b, rocprim::exclusive_scan(nullptr, tb, d_flag.as<u64>(), d_pos.as<u64>(), 0ull, N, rocprim::plus<u64>(), st));
            BHIP(b, d_temp.ensure(tb));
            BHIP(b, rocprim::exclusive_scan(d_temp.p, tb, d_flag.as<u64>(), d_pos.as<u64>(), 0ull, N, rocprim::plus<u64>(), st));
        }
        hipLaunchKernelGGL(seg_scatter_kernel, dim3(gridN), dim3(256), 0, st, sorted, N, d_flag.as<u64>(), d_pos.as<u64>(), d_dk.as<u64>(), d_do.as<u32>(),
                           d_run.as<u32>(), d_totals.as<u64>());
        BHIP(b, hipGetLastError());
        u64 totals[2];
        BHIP(b, hipMemcpyAsync(totals, d_totals.p, 16, hipMemcpyDeviceToHost, st));
        BHIP(b, lap(S.segment_ms));
        const u32 R = (u32)totals[1];
        S.distinct_kmers += R;

        // ---- closure: count, scan, write.  cnt reuses the flag array, off the scan's output (both are R + 1 <= N + 1 long at most: cap + 1 was not
        // allocated for them, so the last offset is kept on the host)
        ClosureArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.R = R;
        ca.run_start = d_run.as<u32>();
        ca.d_owner = d_do.as<u32>();
        ca.n_known = n_known;
        ca.owner_node = d_owner_node.as<u32>();
        ca.parent = d_parent.as<u32>();
        ca.depth = d_depth.as<u32>();
        ca.node_tid = d_node_tid.as<u32>();
        ca.cnt = d_flag.as<u64>();
        ca.counters = d_counters.as<u64>();
        const u32 gridR = (u32)(((u64)R + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock));
        hipLaunchKernelGGL(closure_kernel<false>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ca);
        BHIP(b, hipGetLastError());
        // offsets: R + 1 entries in a buffer of their own size class (keysA is free once the pairs are sorted and scattered ... unless it holds them)
        DevBuf& d_off = packed ? d_keysA : d_keysB;
        if ((u64)R + 1 > cap) BHIP(b, d_off.ensure(((u64)R + 1) * 8));
        {
            size_t tb = 0;
            BHIP(b, rocprim::exclusive_scan(nullptr, tb, d_flag.as<u64>(), d_off.as<u64>(), 0ull, (size_t)R, rocprim::plus<u64>(), st));
            BHIP(b, d_temp.ensure(tb));
            BHIP(b, rocprim::exclusive_scan(d_temp.p, tb, d_flag.as<u64>(), d_off.as<u64>(), 0ull, (size_t)R, rocprim::plus<u64>(), st));
        }
        BHIP(b, hipMemcpyAsync(host_c, d_counters.p, C_N * 8, hipMemcpyDeviceToHost, st));
        BHIP(b, hipStreamSynchronize(st));
        if (host_c[C_TOOLONG])
            return berr(b, LMAT_E_CAPACITY, "a taxid list of " + std::to_string(host_c[C_TOOLONG]) + " entries: the tax_histo record holds at most 65535");
        const u64 entries = host_c[C_ENTRIES];
        const u64 n_long = host_c[C_LONG_RUNS], long_entries = host_c[C_LONG_ENTRIES];
        if (long_entries > 0xFFFFFFF0ull) return berr(b, LMAT_E_CAPACITY, "more than 2^32 entries in lists beyond 64 taxids in one pass: raise prefix_bits");
        BHIP(b, hipMemcpyAsync(d_off.as<u64>() + R, &entries, 8, hipMemcpyHostToDevice, st));
        BHIP(b, d_tids.ensure(entries * 4));
        if (n_long) {
            BHIP(b, d_long_tmp.ensure(long_entries * 4));
            BHIP(b, d_long_sorted.ensure(long_entries * 4));
            BHIP(b, d_long_begin.ensure(n_long * 4));
            BHIP(b, d_long_end.ensure(n_long * 4));
            BHIP(b, d_long_run.ensure(n_long * 4));
        }
        // the write pass hands out the long lists' places with the two counters the count pass filled
        BHIP(b, hipMemsetAsync(d_counters.as<u64>() + C_LONG_RUNS, 0, 16, st));
        ca.off = d_off.as<u64>();
        ca.tids = d_tids.as<u32>();
        ca.long_tmp = d_long_tmp.as<u32>();
        ca.long_begin = d_long_begin.as<u32>();
        ca.long_end = d_long_end.as<u32>();
        ca.long_run = d_long_run.as<u32>();
        hipLaunchKernelGGL(closure_kernel<true>, dim3(gridR), dim3(64 * kWavesPerBlock), 0, st, ca);
        BHIP(b, hipGetLastError());
        if (n_long) {
            size_t tb = 0;
            BHIP(b, rocprim::segmented_radix_sort_keys(nullptr, tb, d_long_tmp.as<u32>(), d_long_sorted.as<u32>(), (unsigned)long_entries, (unsigned)n_long,
                                                       d_long_begin.as<u32>(), d_long_end.as<u32>(), 0, 32, st));
            BHIP(b, d_temp.ensure(tb));
            BHIP(b, rocprim::segmented_radix_sort_keys(d_temp.p, tb, d_long_tmp.as<u32>(), d_long_sorted.as<u32>(), (unsigned)long_entries, (unsigned)n_long,
                                                       d_long_begin.as<u32>(), d_long_end.as<u32>(), 0, 32, st));
            hipLaunchKernelGGL(long_copy_kernel, dim3((u32)n_long), dim3(256), 0, st, d_long_sorted.as<u32>(), d_long_begin.as<u32>(), d_long_end.as<u32>(),
                               d_long_run.as<u32>(), d_off.as<u64>(), d_tids.as<u32>());
            BHIP(b, hipGetLastError());
        }
        // the k-mer of every run, into the scan's old output
        hipLaunchKernelGGL(run_kmer_kernel, dim3((R + 255) / 256), dim3(256), 0, st, d_dk.as<u64>(), d_run.as<u32>(), R, d_pos.as<u64>());
        BHIP(b, hipGetLastError());
        BHIP(b, lap(S.closure_ms));
        if (merging) {   // the pass's result stays on the device and is one more source of the merge
            if (const int rc = tail.pass(pass, R, d_pos.as<u64>(), d_off.as<u64>(), d_tids.as<u32>(), entries)) return rc;
            S.dropped_unknown += host_c[C_DROPPED];
            continue;
        }
        if (const int rc = tail.count_lists(d_tids.as<u32>(), entries)) return rc;

        // ---- to the host: records without a known owner are left out (tax_histo.cpp:239-248)
        std::vector<u64> h_km(R), h_off((size_t)R + 1);
        const size_t t0 = b->tids.size();
        b->tids.resize(t0 + entries);
        BHIP(b, hipMemcpy(h_km.data(), d_pos.p, (size_t)R * 8, hipMemcpyDeviceToHost));
        BHIP(b, hipMemcpy(h_off.data(), d_off.p, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost));
        if (entries) BHIP(b, hipMemcpy(b->tids.data() + t0, d_tids.p, entries * 4, hipMemcpyDeviceToHost));
        for (u32 r = 0; r < R; ++r) {
            if (h_off[r + 1] == h_off[r]) continue;
            b->kmers.push_back(h_km[r]);
            b->list_off.push_back(t0 + h_off[r + 1]);
        }
        S.dropped_unknown += host_c[C_DROPPED];
        S.singletons += host_c[C_SINGLETONS];
        S.total_list_entries += entries;
        S.longest_list = std::max<u64>(S.longest_list, host_c[C_LONGEST]);
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
int lmat_db_finalize(lmat_ctx* ctx);

// The result goes through the ingest's own record parser as an in-memory stream of the file format, so the table is the one
// lmat_db_begin / lmat_db_add_taxhisto / lmat_db_finalize build from the written file.
int lmat_db_build_from_genomes(lmat_ctx* ctx, lmat_build* b, uint64_t table_bytes) {
    if (!ctx || !b) return LMAT_E_ARG;
    if (!b->done) return lmat::set_err(ctx, LMAT_E_ARG, "lmat_build_run first");
    if (!ctx->tax.loaded) return lmat::set_err(ctx, LMAT_E_ARG, "load the taxonomy before the k-mer database");
    char* mem = nullptr;
    size_t mem_len = 0;
    FILE* w = open_memstream(&mem, &mem_len);
    if (!w) return lmat::set_err(ctx, LMAT_E_NOMEM, "open_memstream failed");
    const uint32_t data_start = 29, version = 999, klen = (uint32_t)b->k;
    const uint64_t count = b->kmers.size(), sanity = ~0ull;
    const char loc = 'N';
    fwrite(&data_start, 4, 1, w); fwrite(&count, 8, 1, w); fwrite(&sanity, 8, 1, w); fwrite(&version, 4, 1, w); fwrite(&loc, 1, 1, w); fwrite(&klen, 4, 1, w);
    for (u64 i = 0; i < count; ++i) {
        const u64 n = b->list_off[i + 1] - b->list_off[i];
        const uint16_t n16 = (uint16_t)n;
        fwrite(&b->kmers[i], 8, 1, w); fwrite(&n16, 2, 1, w); fwrite(&b->tids[b->list_off[i]], 4, n, w);
        if ((i + 1) % 1500 == 0) fwrite(&sanity, 8, 1, w);
    }
    if (fclose(w) != 0 || !mem) { free(mem); return lmat::set_err(ctx, LMAT_E_NOMEM, "out of memory for the record stream"); }
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

}  // extern "C"
