// bins.hpp -- what the streamed boundary (lmat_api.cpp) needs of bins.hip: the buffers one batch slot owns for its index lists
// and the call that queues select + partition behind the slot's classify launches.
#pragma once
#include "lmat_internal.hpp"

namespace lmat {

// page-locked host memory that frees itself (inline: the slots of a stream own some, whether or not bins.hip is linked in)
struct PinnedBuf {
    void* p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p, o.p); return *this; }
    ~PinnedBuf() { if (p) hipHostFree(p); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The partition of one batch: device buffers sized once for max_reads, and (pinned == true) the host twins the lists are copied to.
struct BinsPart {
    lmat_dev::DevBuf grp, keyA, keyB, idxA, idxB, temp, goff;   // u16[n] | u32[n] x 4 | rocPRIM's storage | u64[kBinsOffWords]
    uint64_t cap = 0;             // reads the buffers hold
    PinnedBuf h_goff;             // u64[kBinsOffWords]
    PinnedBuf h_idx;              // u32[cap]
    uint32_t n_groups = 0;        // of the bins the last bins_part_queue ran under
    bool valid = false;           // the slot's current batch was partitioned
};
static const uint32_t kBinsOffWords = 65536;   // group_off[n_groups + 1], n_groups <= 65534

int bins_part_alloc(lmat_bins* b, BinsPart& p, uint64_t max_reads, bool pinned);
// Queues on `stream`: select on d_results[0 .. n), the stable sort by group of the indices idx_base + i, the group offsets; with
// pinned buffers also the copies of group_off[n_groups + 1] and of the n sorted indices (the first group_off[n_groups] count).
int bins_part_queue(lmat_bins* b, BinsPart& p, const lmat_read_result* d_results, uint64_t n, uint32_t idx_base, hipStream_t stream);
lmat_ctx* bins_ctx(const lmat_bins* b);
uint32_t bins_group_count(const lmat_bins* b);

}  // namespace lmat
