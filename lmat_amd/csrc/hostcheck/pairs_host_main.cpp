// drives lmat_reads_upload_pairs and the three forms of stream submit through the library's own host code, built with ASan + UBSan
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <random>
#include <vector>
#include "lmat_internal.hpp"
#include "lmat_hip.h"
static std::mt19937_64 rng(7);
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "line %d: rc %d (%s)\n", __LINE__, rc_, lmat_last_error(c)); exit(1); } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { fprintf(stderr, "line %d: accepted\n", __LINE__); exit(1); } } while (0)
struct Blocks { std::vector<uint8_t> b1, b2, il; std::vector<uint64_t> o1, o2, oi; };
static Blocks make(uint64_t n, int l1max, int l2max, bool fixed, uint64_t lead1 = 0, uint64_t lead2 = 0) {
    Blocks B;
    B.b1.assign(lead1, 'A'); B.b2.assign(lead2, 'C');
    B.o1.push_back(lead1); B.o2.push_back(lead2); B.oi.push_back(0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t l1 = fixed ? l1max : rng() % (l1max + 1), l2 = fixed ? l2max : rng() % (l2max + 1);
        for (uint64_t j = 0; j < l1; ++j) { B.b1.push_back("ACGTN"[rng() % 5]); B.il.push_back(B.b1.back()); }
        B.oi.push_back(B.il.size());
        for (uint64_t j = 0; j < l2; ++j) { B.b2.push_back("ACGTN"[rng() % 5]); B.il.push_back(B.b2.back()); }
        B.oi.push_back(B.il.size());
        B.o1.push_back(B.b1.size()); B.o2.push_back(B.b2.size());
    }
    B.b1.shrink_to_fit(); B.b2.shrink_to_fit(); B.il.shrink_to_fit();   // (the last base ends the allocation)
    return B;
}
static void take(lmat_ctx* c, lmat_stream* st, uint64_t want_n) {
    const lmat_read_result* r; const lmat_cand* cd; uint64_t n, nc, tag;
    OK(lmat_stream_next(st, &r, &cd, &n, &nc, &tag));
    if (n != want_n) { fprintf(stderr, "batch of %llu came back as %llu\n", (unsigned long long)want_n, (unsigned long long)n); exit(1); }
    OK(lmat_stream_release(st));
}
int main() {
    lmat_ctx* c = nullptr;
    lmat_params prm = {1.0f, 3.0f, 0.0f, 35, 1, 1, 1};
    if (lmat_ctx_create(0, &prm, &c)) return 1;
    c->db_ready = true; c->dev.k = 20; c->dev.n_ids = 8; c->counts_bytes = 8 * 16 + 24;
    hipMalloc(&c->d_counts, c->counts_bytes);
    // uploads
    for (uint64_t n : {0ull, 1ull, 2ull, 5ull, 17ull, 300ull}) {
        for (int fixed = 0; fixed < 2; ++fixed) {
            Blocks B = make(n, 70, 90, fixed, n % 3, n % 5);
            lmat_reads* r = nullptr;
            OK(lmat_reads_upload_pairs(c, B.b1.data(), B.o1.data(), B.b2.data(), B.o2.data(), n, &r));
            if (n) {
                std::vector<lmat_read_result> res(n);
                std::vector<lmat_cand> cd(64 * n);
                uint64_t nc = 0;
                OK(lmat_classify(c, r, 0, n, res.data(), cd.data(), cd.size(), &nc));
                std::vector<uint64_t> off(n + 1);
                OK(lmat_reads_download_ascii(c, r, 0, n, nullptr, off.data()));
                std::vector<uint8_t> bases(off[n] + 1);
                OK(lmat_reads_download_ascii(c, r, 0, n, bases.data(), off.data()));
            }
            lmat_reads_free(c, r);
        }
    }
    { Blocks B = make(1, 20000, 12787, true); lmat_reads* r = nullptr;
      OK(lmat_reads_upload_pairs(c, B.b1.data(), B.o1.data(), B.b2.data(), B.o2.data(), 1, &r));
      lmat_read_result res; REFUSED(lmat_classify(c, r, 0, 1, &res, nullptr, 0, nullptr)); lmat_reads_free(c, r); }
    // streams: sizes around the limits, every form, calls only and with candidates, one and three slots
    for (uint64_t n : {0ull, 1ull, 4ull, 33ull, 1000ull, (1ull << 18) + 5}) {
        for (int fixed = 0; fixed < 2; ++fixed) {
            const int l1 = n > 100000 ? 9 : 74, l2 = n > 100000 ? 7 : 75;
            Blocks B = make(n, l1, l2, fixed, 5, 7);
            const uint64_t total = B.il.size();
            for (int slots : {1, 3}) {
                lmat_stream* st = nullptr;
                OK(lmat_stream_create(c, std::max<uint64_t>(2 * n, 2), std::max<uint64_t>(total + n, 1), slots == 1 ? 8 : 0, slots, &st));   // exactly at both limits
                uint8_t* hb; uint64_t* ho;
                for (int round = 0; round < 2; ++round) {
                    OK(lmat_stream_acquire(st, &hb, &ho));
                    if (total) memcpy(hb, B.il.data(), total);
                    memcpy(ho, B.oi.data(), (2 * n + 1) * 8);
                    OK(lmat_stream_submit_pairs(st, n, 1));
                    if (slots == 1) take(c, st, n);
                    OK(lmat_stream_acquire(st, &hb, &ho));
                    OK(lmat_stream_submit_pairs_from(st, B.b1.data(), B.o1.data(), B.b2.data(), B.o2.data(), n, 2));
                    if (slots == 1) take(c, st, n);
                    // a pair too many, a base too many: refused, the slot stays usable
                    Blocks M = make(n + 1, l1, l2, true);
                    OK(lmat_stream_acquire(st, &hb, &ho));
                    REFUSED(lmat_stream_submit_pairs_from(st, M.b1.data(), M.o1.data(), M.b2.data(), M.o2.data(), n + 1, 3));
                    if (n) {
                        std::vector<uint64_t> o2 = B.o2; std::vector<uint8_t> b2 = B.b2; o2[n] += 1; b2.push_back('A');
                        OK(lmat_stream_acquire(st, &hb, &ho));
                        REFUSED(lmat_stream_submit_pairs_from(st, B.b1.data(), B.o1.data(), b2.data(), o2.data(), n, 4));
                        OK(lmat_stream_acquire(st, &hb, &ho));
                        memcpy(ho, B.oi.data(), (2 * n + 1) * 8); ho[2 * n] += 1;
                        REFUSED(lmat_stream_submit_pairs(st, n, 5));
                    }
                    // the single-read forms on the interleaved text as 2n reads
                    OK(lmat_stream_acquire(st, &hb, &ho));
                    OK(lmat_stream_submit_from(st, B.il.data(), B.oi.data(), 2 * n, 6));
                    if (slots == 3) { take(c, st, n); take(c, st, n); }
                    take(c, st, 2 * n);
                }
                uint64_t s6[6]; OK(lmat_debug_stream_stats(st, s6));
                lmat_stream_destroy(st);
            }
        }
    }
    {   // no pairs, no pointers
        lmat_stream* st = nullptr; uint8_t* hb; uint64_t* ho;
        OK(lmat_stream_create(c, 4, 64, 0, 1, &st));
        OK(lmat_stream_acquire(st, &hb, &ho));
        OK(lmat_stream_submit_pairs_from(st, nullptr, nullptr, nullptr, nullptr, 0, 1));
        take(c, st, 0);
        OK(lmat_stream_acquire(st, &hb, &ho));
        OK(lmat_stream_submit_from(st, nullptr, nullptr, 0, 1));
        take(c, st, 0);
        lmat_stream_destroy(st);
        lmat_reads* r = nullptr;
        OK(lmat_reads_upload_pairs(c, nullptr, nullptr, nullptr, nullptr, 0, &r));
        lmat_reads_free(c, r);
    }
    lmat_ctx_destroy(c);
    puts("pairs host paths: clean");
    return 0;
}
