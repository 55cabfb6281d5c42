// pairs.hip -- paired-end reads joined while they are packed (K0 for pairs).  The record of pair r is word for
// word the record pack_reads_kernel (kernels.hip) writes for the bytes  mate1 . 'N' . mate2  -- what upstream's
// merge_fastq_reads_with_N_separator.pl writes to disk before read_label sees it -- so every kernel behind K0 runs unchanged.
//
// Shape of pack_reads_kernel: four pairs per wave, a lane per code word of the joined record, 256 joined positions a step.  A
// word that lies inside one mate is that kernel's translation from the mate's own address (five guarded dword loads, a funnel
// shift by addr & 3, the letter tests as zero-byte tests).  The word that holds the end of mate 1, the joint or the start of
// mate 2 is the OR of two such translations: mate 1's bases from p on, cut to l1 - p by the translation's own end mask, and
// mate 2's first bases moved up by t = l1 + 1 - p positions (codes by 2t bits, validity by t).  The joint itself is nobody's
// base: code 0, invalid.  Loads are guarded per mate -- only dwords that hold a base of that mate -- and every byte behind a
// mate's end is masked before it is looked at: the next mate's letters and a slot's stale bytes lie there.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels.hpp"

namespace {

__device__ __forceinline__ uint32_t zero_bytes(uint32_t z) {  // 0x80 in every byte of z that is zero, 0 elsewhere (exact)
    const uint32_t t = (z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | z | 0x7F7F7F7Fu);
}

// 16 bases of the mate at bases[b0 .. b0 + mlen) from its position q on (q < mlen): 2-bit codes and validity bits, zero from the
// mate's end on.  pack_reads_kernel's inner step.
__device__ __forceinline__ void translate16(const uint8_t* __restrict__ bases, uint64_t b0, uint32_t mlen, uint32_t q, uint32_t& code,
                                            uint32_t& valid16) {
    const uint64_t addr = b0 + q, a4 = addr & ~3ull, end = b0 + mlen;
    const uint32_t sh = (uint32_t)(addr & 3) * 8u;
    const uint32_t* src = (const uint32_t*)(bases + a4);
    uint32_t d[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) d[j] = a4 + 4u * j < end ? src[j] : 0u;  // only dwords that hold a base of this mate
    const uint32_t left = mlen - q;  // bases from q on (16 or more: the whole word)
    code = 0;
    valid16 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t w = __builtin_amdgcn_alignbit(d[j + 1], d[j], sh);
        if (left < 4u * j + 4u) w &= left > 4u * j ? (1u << (8u * (left - 4u * j))) - 1u : 0u;  // bytes past the mate's end
        const uint32_t x = w & 0xDFDFDFDFu;  // case-insensitive, as ENCODE is
        const uint32_t vm = zero_bytes(x ^ 0x41414141u) | zero_bytes(x ^ 0x43434343u) | zero_bytes(x ^ 0x47474747u) | zero_bytes(x ^ 0x54545454u);
        const uint32_t v1 = vm >> 7;  // 1 per valid byte
        const uint32_t c2 = (((x >> 1) & 0x03030303u) ^ ((x >> 2) & 0x01010101u)) & (v1 * 3u);
        code |= ((c2 | (c2 >> 6) | (c2 >> 12) | (c2 >> 18)) & 0xFFu) << (8 * j);
        valid16 |= ((v1 | (v1 >> 7) | (v1 >> 14) | (v1 >> 21)) & 0xFu) << (4 * j);
    }
}

// mates of pair r: bases[off1[r * s] .. off1[r * s + 1]) and bases[off2[r * s] .. off2[r * s + 1])
__global__ __launch_bounds__(256) void pack_pairs_kernel(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off1,
                                                         const uint64_t* __restrict__ off2, uint32_t s,
                                                         const uint64_t* __restrict__ rec_off, uint32_t* __restrict__ words, uint64_t n) {
    const int lane = threadIdx.x & 63;
    const uint32_t sub = (uint32_t)lane & 15u;   // this lane's code word within a stretch of 256 joined positions
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r0 = wave * 4; r0 < n; r0 += nw * 4) {
        const uint64_t r = r0 + ((uint32_t)lane >> 4);
        const bool have = r < n;
        const uint64_t b1 = have ? off1[r * s] : 0, b2 = have ? off2[r * s] : 0;
        const uint32_t l1 = have ? (uint32_t)(off1[r * s + 1] - b1) : 0u, l2 = have ? (uint32_t)(off2[r * s + 1] - b2) : 0u;
        const uint32_t len = have ? l1 + 1u + l2 : 0u;
        uint32_t* rec = words + (have ? rec_off[r] : 0);
        if (have && sub == 0) rec[0] = len;
        const uint32_t nb = (len + 15) / 16;
        for (uint32_t p0 = 0; __ballot(p0 < len) != 0; p0 += 256) {
            const uint32_t p = p0 + 16u * sub;
            uint32_t code = 0, valid16 = 0;
            if (p < len) {
                if (p < l1) translate16(bases, b1, l1, p, code, valid16);  // (cut to l1 - p where mate 1 ends inside this word)
                if (p + 15u > l1 && l2) {   // positions l1 + 1 .. of the joined text in this word: mate 2 from its position max(0, p - l1 - 1) on
                    const uint32_t t = p > l1 ? 0u : l1 + 1u - p;  // how far up mate 2's first base sits in this word (1..15), 0: the word starts inside mate 2
                    uint32_t c2, v2;
                    translate16(bases, b2, l2, t ? 0u : p - l1 - 1u, c2, v2);
                    code |= c2 << (2u * t);
                    valid16 |= (v2 << t) & 0xFFFFu;
                }
                rec[1 + (p >> 4)] = code;
            }
            // a validity word covers 32 joined positions: this lane's 16 bits and its odd neighbour's
            const uint32_t other = (uint32_t)__shfl_xor((int)valid16, 1);
            if (p < len && (sub & 1u) == 0) rec[1 + nb + (p >> 5)] = valid16 | (other << 16);
        }
    }
}

// pairs of one geometry (every mate 1 of l1 bases, every mate 2 of l2) whose offsets start at 0: the offsets the kernel above reads
// and the record offsets, made here instead of on the host.  two_block: off[0..n] mates 1, off[n..2n] mates 2 behind them; else
// off[0..2n] interleaved.
__global__ __launch_bounds__(256) void fill_pair_offsets_kernel(uint64_t* __restrict__ off, uint64_t* __restrict__ rec_off, uint64_t n, uint32_t l1,
                                                                uint32_t l2, uint32_t words_per_rec, bool two_block) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    rec_off[i] = i * words_per_rec;
    if (two_block) {
        off[i] = i * l1;
        off[n + i] = n * l1 + i * l2;   // (i = 0 writes off[n] a second time, with the same value)
    } else {
        off[2 * i] = i * ((uint64_t)l1 + l2);
        if (i < n) off[2 * i + 1] = i * ((uint64_t)l1 + l2) + l1;
    }
}

}  // namespace

namespace lmat {

void launch_fill_pair_offsets(uint64_t* off, uint64_t* rec_off, uint64_t n, uint32_t l1, uint32_t l2, bool two_block, hipStream_t stream) {
    fill_pair_offsets_kernel<<<dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream>>>(off, rec_off, n, l1, l2, rec_words(l1 + 1 + l2), two_block);
}
void launch_pack_pairs(const uint8_t* bases, const uint64_t* off1, const uint64_t* off2, uint32_t stride, const uint64_t* rec_off, uint32_t* words,
                       uint64_t n, hipStream_t stream) {
    uint64_t blocks = (n + 15) / 16;   // 4 waves x 4 pairs per block and pass
    if (blocks < 1) blocks = 1;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(pack_pairs_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, bases, off1, off2, stride, rec_off, words, n);
}

}  // namespace lmat
