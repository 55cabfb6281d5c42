// the launchers of kernels.hpp on the host: classify launches do nothing (their buffers stay zero: no errors, no candidates); the pack
// and offset launchers make the reads and writes of their kernels, index for index, so that ASan sees them against the buffers' sizes
#include <cstring>
#include "kernels.hpp"
namespace lmat {
static void touch16(const uint8_t* bases, uint64_t b0, uint32_t mlen, uint32_t q, volatile uint32_t& sink) {
    const uint64_t addr = b0 + q, a4 = addr & ~3ull, end = b0 + mlen;
    for (int j = 0; j < 5; ++j) if (a4 + 4u * j < end) { uint32_t w; memcpy(&w, bases + a4 + 4 * j, 4); sink ^= w; }
}
void launch_fill_offsets(uint64_t* off, uint64_t* rec_off, uint64_t n, uint32_t len, hipStream_t) {
    for (uint64_t i = 0; i <= n; ++i) { off[i] = i * len; rec_off[i] = i * rec_words(len); }
}
void launch_pack_reads(const uint8_t* bases, const uint64_t* off, const uint64_t* rec_off, uint32_t* words, uint64_t n, hipStream_t) {
    volatile uint32_t sink = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t b0 = off[r]; const uint32_t len = (uint32_t)(off[r + 1] - b0), nb = (len + 15) / 16;
        uint32_t* rec = words + rec_off[r];
        rec[0] = len;
        for (uint32_t p = 0; p < len; p += 16) { touch16(bases, b0, len, p, sink); rec[1 + (p >> 4)] = 0; if (!(p & 16)) rec[1 + nb + (p >> 5)] = 0; }
    }
}
void launch_fill_pair_offsets(uint64_t* off, uint64_t* rec_off, uint64_t n, uint32_t l1, uint32_t l2, bool two_block, hipStream_t) {
    const uint32_t w = rec_words(l1 + 1 + l2);
    for (uint64_t i = 0; i <= n; ++i) {
        rec_off[i] = i * w;
        if (two_block) { off[i] = i * l1; off[n + i] = n * l1 + i * l2; }
        else { off[2 * i] = i * ((uint64_t)l1 + l2); if (i < n) off[2 * i + 1] = i * ((uint64_t)l1 + l2) + l1; }
    }
}
void launch_pack_pairs(const uint8_t* bases, const uint64_t* off1, const uint64_t* off2, uint32_t s, const uint64_t* rec_off, uint32_t* words,
                       uint64_t n, hipStream_t) {
    volatile uint32_t sink = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t b1 = off1[r * s], b2 = off2[r * s];
        const uint32_t l1 = (uint32_t)(off1[r * s + 1] - b1), l2 = (uint32_t)(off2[r * s + 1] - b2), len = l1 + 1 + l2, nb = (len + 15) / 16;
        uint32_t* rec = words + rec_off[r];
        rec[0] = len;
        for (uint32_t p = 0; p < len; p += 16) {
            if (p < l1) touch16(bases, b1, l1, p, sink);
            if (p + 15u > l1 && l2) { const uint32_t t = p > l1 ? 0u : l1 + 1u - p; touch16(bases, b2, l2, t ? 0u : p - l1 - 1u, sink); }
            rec[1 + (p >> 4)] = 0;
            if (!(p & 16)) rec[1 + nb + (p >> 5)] = 0;
        }
    }
}
void launch_insert_pairs(const DeviceTables&, const uint64_t*, const uint32_t*, uint64_t, uint32_t*, hipStream_t) {}
void launch_synth_db(const DeviceTables&, const SynthGeo&, int, const uint16_t*, const uint32_t*, uint64_t, uint32_t, uint32_t, uint32_t*, unsigned long long*, hipStream_t) {}
void launch_table_count(const DeviceTables&, unsigned long long*, hipStream_t) {}
void launch_synth_reads(uint32_t*, const uint64_t*, const uint32_t*, uint32_t, uint64_t, uint64_t, const SynthGeo&, hipStream_t) {}
void launch_lookup(const DeviceTables&, const uint64_t*, uint64_t, uint32_t*, uint32_t*, uint32_t, hipStream_t) {}
void launch_div_check(unsigned long long*, hipStream_t) {}
void launch_probe_stats(const DeviceTables&, const uint64_t*, uint64_t, unsigned long long*, hipStream_t) {}
void launch_tail(const ClassifyArgs&, hipStream_t) {}
bool launch_classify(const ClassifyArgs&, uint32_t max_read_len, int, hipStream_t) { return max_read_len <= 32787; }
void launch_k4_begin(const ClassifyArgs&, hipStream_t, hipStream_t, hipStream_t, hipStream_t, hipEvent_t) {}
void launch_k4_end(const ClassifyArgs&, hipStream_t, hipStream_t, hipStream_t, hipStream_t, hipEvent_t, hipEvent_t, hipEvent_t, hipEvent_t) {}
void launch_k4_debug(const ClassifyArgs&, const uint32_t*, const float*, const uint64_t*, const float*, uint64_t, hipStream_t) {}
void launch_k4_debug_counts(const ClassifyArgs&, const uint32_t*, const uint32_t*, const uint64_t*, const uint32_t*, uint64_t, bool, hipStream_t, const uint32_t*, uint8_t*) {}
void classify_variant_launches(int, uint64_t out[2]) { out[0] = out[1] = 0; }
uint64_t classify_uniform_launches(int) { return 0; }
uint32_t classify_last_grid(int) { return 0; }
int classify_max_read_len(int k) { return 32768 + (k >= 1 && k <= 20 ? k : 20) - 1; }
size_t classify_gmem_scratch_bytes() { return 1 << 20; }
void launch_gather_bench(const uint64_t*, uint32_t, uint64_t, uint64_t, unsigned long long*, hipStream_t, int) {}
}
