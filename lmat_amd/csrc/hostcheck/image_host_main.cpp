// drives lmat_db_save_image / lmat_db_load_image of a device image (LMATIMG2) through the library's own host code, built with
// ASan + UBSan: one good round trip, byte-compared; every damaged header the loader must refuse; files cut at every section
// boundary -1 / +0 / +1.  The "device" tables of the contexts are heap blocks (hip_stub.cpp), fabricated here as
// pairs_host_main.cpp fabricates db_ready: what the sections hold is never interpreted by either call.
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include <unistd.h>
#include "lmat_internal.hpp"
#include "lmat_hip.h"
static std::mt19937_64 rng(11);
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "line %d: rc %d (%s)\n", __LINE__, rc_, lmat_last_error(c)); exit(1); } } while (0)
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); exit(1); } } while (0)
// ImgHdr2 of lmat_api.cpp, restated: the layout of the header page is part of the format
struct Hdr {
    char magic[8];
    uint32_t version, k;
    uint64_t nb;
    uint32_t W, lowbits, m; int32_t wshift;
    uint32_t nbuckets, ovf_nbuckets, list_shift, n_ids;
    uint64_t n_kmers, arena_words, n_lists, tax_fingerprint, mode_fingerprint;
    uint64_t off_slots, bytes_slots, off_ovf, bytes_ovf, off_arena, bytes_arena;
};
static_assert(sizeof(Hdr) == 144, "header layout");
static std::vector<char> slurp(const std::string& fn) {
    std::vector<char> v;
    FILE* f = fopen(fn.c_str(), "rb");
    if (!f) return v;
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
static void spit(const std::string& fn, const std::vector<char>& v, size_t n) {
    FILE* f = fopen(fn.c_str(), "wb");
    CHECK(f && fwrite(v.data(), 1, n, f) == n);
    fclose(f);
}
static void fill(void* p, size_t n) { for (size_t i = 0; i < n; ++i) ((unsigned char*)p)[i] = (unsigned char)(rng() | 1); }
// a context that "holds" a finalized compact table of k = 12 at the minimum size (or, wide: a wide-layout table of k = 9)
static lmat_ctx* make_ctx(bool wide, uint64_t arena_words) {
    lmat_ctx* c = nullptr;
    lmat_params prm = {1.0f, 3.0f, 0.0f, 35, 1, 1, 1};
    if (lmat_ctx_create(0, &prm, &c)) exit(1);
    c->tax.loaded = true;
    c->dev.n_ids = 77;
    if (wide) {
        c->dev.k = 9; c->dev.nbuckets = 300;
        hipMalloc((void**)&c->dev.slots, 300 * 64); fill(c->dev.slots, 300 * 64);
    } else {
        c->dev.cpt = lmat::cpt_geometry(12, 1);
        CHECK(c->dev.cpt.nb == 2065 && c->dev.cpt.W == 127 && c->dev.cpt.wshift == -1);
        c->dev.k = 12; c->dev.nbuckets = 2065; c->dev.ovf_nbuckets = 1030;
        hipMalloc((void**)&c->dev.slots, 2065 * 64); fill(c->dev.slots, 2065 * 64);
        hipMalloc((void**)&c->dev.ovf_slots, 1030 * 64); fill(c->dev.ovf_slots, 1030 * 64);
    }
    c->arena_words = arena_words; c->n_kmers = 12345; c->n_lists = 7;
    hipMalloc((void**)&c->dev.arena, arena_words * 2 + 64); fill(c->dev.arena, arena_words * 2);
    c->db_ready = true;
    return c;
}
struct Snapshot {
    void *slots, *ovf, *arena; uint64_t nb, n_kmers, arena_words; uint32_t W, nbuckets, onb, shift; int k; bool ready;
    std::vector<char> bytes;
    explicit Snapshot(const lmat_ctx* c) : slots(c->dev.slots), ovf(c->dev.ovf_slots), arena(c->dev.arena), nb(c->dev.cpt.nb), n_kmers(c->n_kmers),
        arena_words(c->arena_words), W(c->dev.cpt.W), nbuckets(c->dev.nbuckets), onb(c->dev.ovf_nbuckets), shift(c->dev.list_shift), k(c->dev.k), ready(c->db_ready) {
        const size_t ns = (size_t)(nb ? nb : nbuckets) * 64, no = (size_t)onb * 64, na = (size_t)arena_words * 2;
        bytes.insert(bytes.end(), (char*)slots, (char*)slots + ns);
        if (no) bytes.insert(bytes.end(), (char*)ovf, (char*)ovf + no);
        bytes.insert(bytes.end(), (char*)arena, (char*)arena + na);
    }
    bool operator==(const Snapshot& o) const {
        return slots == o.slots && ovf == o.ovf && arena == o.arena && nb == o.nb && n_kmers == o.n_kmers && arena_words == o.arena_words && W == o.W &&
               nbuckets == o.nbuckets && onb == o.onb && shift == o.shift && k == o.k && ready == o.ready && bytes == o.bytes;
    }
};
static int n_refused = 0;
// the file must be refused with LMAT_E_IO by lmat_image_check and by a load into `holder`, which keeps what it held
static void refused(lmat_ctx* holder, const std::string& fn, const char* what) {
    const Snapshot before(holder);
    char msg[512];
    const int rc0 = lmat_image_check(fn.c_str(), msg, sizeof msg);
    const int rc = lmat_db_load_image(holder, fn.c_str(), 0);
    if (rc0 != LMAT_E_IO || rc != LMAT_E_IO) { fprintf(stderr, "%s: lmat_image_check %d, lmat_db_load_image %d, both should be LMAT_E_IO\n", what, rc0, rc); exit(1); }
    if (!(Snapshot(holder) == before)) { fprintf(stderr, "%s: the refused load changed the context\n", what); exit(1); }
    ++n_refused;
}
int main() {
    char tmpl[] = "/tmp/lmat_image_host_XXXXXX";
    CHECK(mkdtemp(tmpl));
    const std::string dir = tmpl, good = dir + "/good.img", again = dir + "/again.img", bad = dir + "/bad.img";
    for (int wide = 0; wide < 2; ++wide) {
        for (uint64_t arena_words : {8ull, 2048ull, 4099ull}) {   // 4099: an arena that ends off every boundary
            lmat_ctx* c = make_ctx(wide, arena_words);
            OK(lmat_db_save_image(c, good.c_str()));
            char msg[256];
            CHECK(lmat_image_check(good.c_str(), msg, sizeof msg) == LMAT_OK && !msg[0]);
            lmat_ctx* d = make_ctx(!wide, 16);   // holds another database: the load replaces it
            { lmat_ctx* c = d; OK(lmat_db_load_image(c, good.c_str(), 0)); OK(lmat_db_save_image(c, again.c_str())); }
            const std::vector<char> a = slurp(good), b = slurp(again);
            CHECK(a.size() > 4096 && a == b);
            CHECK(d->dev.k == c->dev.k && d->n_kmers == c->n_kmers && d->arena_words == c->arena_words && d->dev.cpt.nb == c->dev.cpt.nb && d->dev.cpt.W == c->dev.cpt.W &&
                  d->dev.cpt.wshift == c->dev.cpt.wshift && d->dev.nbuckets == c->dev.nbuckets && d->dev.ovf_nbuckets == c->dev.ovf_nbuckets && d->db_ready);
            const Snapshot sc(c), sd(d);
            CHECK(sc.bytes == sd.bytes);
            Hdr h;
            memcpy(&h, a.data(), sizeof h);
            CHECK(a.size() == h.off_arena + h.bytes_arena);
            // files cut at every section boundary -1, +0, +1; one byte MORE than the whole file stays accepted (trailing bytes)
            for (uint64_t edge : {(uint64_t)8, (uint64_t)sizeof(Hdr), (uint64_t)4096, h.off_slots + h.bytes_slots, h.off_ovf, h.off_ovf + h.bytes_ovf, h.off_arena, h.off_arena + h.bytes_arena})
                for (int delta = -1; delta <= 1; ++delta) {
                    const uint64_t n = edge + delta;
                    if (n >= a.size()) continue;
                    spit(bad, a, n);
                    refused(d, bad, "cut file");
                }
            { std::vector<char> more = a; more.push_back(7); spit(bad, more, more.size()); lmat_ctx* c = d; OK(lmat_db_load_image(c, bad.c_str(), 0)); CHECK(Snapshot(d).bytes == sc.bytes); }
            spit(bad, a, 0);
            { lmat_ctx* c = d; CHECK(lmat_db_load_image(c, bad.c_str(), 0) == LMAT_E_IO && Snapshot(d).bytes == sc.bytes); }
            // every damaged header
            auto damage = [&](const char* what, auto&& edit) {
                Hdr x = h;
                edit(x);
                std::vector<char> v = a;
                memcpy(v.data(), &x, sizeof x);
                spit(bad, v, v.size());
                refused(d, bad, what);
            };
            const uint64_t beyond = (a.size() + 4095) / 4096 * 4096 + 4096;
            damage("version 1", [](Hdr& x) { x.version = 1; });
            damage("version 3", [](Hdr& x) { x.version = 3; });
            damage("version 0", [](Hdr& x) { x.version = 0; });
            damage("k 0", [](Hdr& x) { x.k = 0; });
            damage("k 21", [](Hdr& x) { x.k = 21; });
            damage("list_shift 5", [](Hdr& x) { x.list_shift = 5; });
            damage("list_shift huge", [](Hdr& x) { x.list_shift = 0xFFFFFFFFu; });
            damage("nbuckets + 1", [](Hdr& x) { x.nbuckets += 1; });
            damage("nbuckets - 1", [](Hdr& x) { x.nbuckets -= 1; });
            damage("off_slots unaligned", [](Hdr& x) { x.off_slots += 512; });
            damage("off_slots 0", [](Hdr& x) { x.off_slots = 0; });
            damage("off_slots beyond", [&](Hdr& x) { x.off_slots = beyond; });
            damage("off_slots huge", [](Hdr& x) { x.off_slots = ~0ull << 12; });
            damage("off_ovf unaligned", [](Hdr& x) { x.off_ovf += 512; });
            damage("off_ovf into the buckets", [](Hdr& x) { x.off_ovf = x.off_slots; });
            damage("off_ovf beyond", [&](Hdr& x) { x.off_ovf = beyond; });
            damage("off_arena unaligned", [](Hdr& x) { x.off_arena += 512; });
            damage("off_arena into the buckets", [](Hdr& x) { x.off_arena = x.off_slots; });
            damage("off_arena beyond", [&](Hdr& x) { x.off_arena = beyond; });
            damage("off_arena huge", [](Hdr& x) { x.off_arena = ~0ull << 12; });
            damage("bytes_slots + 64", [](Hdr& x) { x.bytes_slots += 64; });
            damage("bytes_slots - 64", [](Hdr& x) { x.bytes_slots -= 64; });
            damage("bytes_slots + 1", [](Hdr& x) { x.bytes_slots += 1; });
            damage("bytes_ovf + 64", [](Hdr& x) { x.bytes_ovf += 64; });
            damage("bytes_arena + 2", [](Hdr& x) { x.bytes_arena += 2; });
            damage("bytes_arena huge", [](Hdr& x) { x.bytes_arena = 1ull << 63; });
            damage("arena_words odd", [](Hdr& x) { x.arena_words += 1; });
            damage("arena_words huge", [](Hdr& x) { x.arena_words = 1ull << 63; x.bytes_arena = 0; });   // (2 * arena_words wraps to 0)
            if (!wide) {
                damage("W + 1", [](Hdr& x) { x.W += 1; });
                damage("W - 1", [](Hdr& x) { x.W -= 1; });
                damage("W 0", [](Hdr& x) { x.W = 0; });
                damage("W huge", [](Hdr& x) { x.W = 0x80000000u; });
                damage("wshift 0", [](Hdr& x) { x.wshift = 0; });
                damage("wshift 6", [](Hdr& x) { x.wshift = 6; });
                damage("wshift -2", [](Hdr& x) { x.wshift = -2; });
                damage("lowbits 2", [](Hdr& x) { x.lowbits = 2; });
                damage("lowbits huge", [](Hdr& x) { x.lowbits = 64; });
                damage("m - 1", [](Hdr& x) { x.m -= 1; });
                damage("m + 1", [](Hdr& x) { x.m += 1; });
                damage("m huge", [](Hdr& x) { x.m = 40; });
                damage("nb + 1", [](Hdr& x) { x.nb += 1; });
                damage("nb - 1", [](Hdr& x) { x.nb -= 1; });
                damage("nb 2^40", [](Hdr& x) { x.nb = 1ull << 40; });
                damage("k 13", [](Hdr& x) { x.k = 13; });
                damage("k 11", [](Hdr& x) { x.k = 11; });
                damage("k 9", [](Hdr& x) { x.k = 9; });
                damage("bytes_ovf 0", [](Hdr& x) { x.bytes_ovf = 0; });
            } else {
                damage("W in a wide image", [](Hdr& x) { x.W = 1; });
                damage("m in a wide image", [](Hdr& x) { x.m = 6; });
                damage("lowbits in a wide image", [](Hdr& x) { x.lowbits = 1; });
                damage("wshift -2 in a wide image", [](Hdr& x) { x.wshift = -2; });
                damage("nbuckets 15", [](Hdr& x) { x.nbuckets = 15; x.bytes_slots = 15 * 64; });
                damage("nb in a wide image", [](Hdr& x) { x.nb = 300; });
            }
            // other fingerprints: refused with their own codes, and before anything is freed as well
            for (int which = 0; which < 2; ++which) {
                Hdr x = h;
                (which ? x.mode_fingerprint : x.tax_fingerprint) ^= 1;
                std::vector<char> v = a;
                memcpy(v.data(), &x, sizeof x);
                spit(bad, v, v.size());
                const Snapshot before(d);
                CHECK(lmat_db_load_image(d, bad.c_str(), 0) == (which ? LMAT_E_ARG : LMAT_E_TAXONOMY));
                CHECK(Snapshot(d) == before);
            }
            {   // a missing file, a directory that does not exist
                const Snapshot before(d);
                CHECK(lmat_db_load_image(d, (dir + "/none.img").c_str(), 0) == LMAT_E_IO && Snapshot(d) == before);
                CHECK(lmat_db_save_image(d, (dir + "/none/x.img").c_str()) == LMAT_E_IO && Snapshot(d) == before);
            }
            lmat_ctx_destroy(c);
            lmat_ctx_destroy(d);
        }
    }
    {   // nothing to save
        lmat_ctx* c = nullptr;
        lmat_params prm = {1.0f, 3.0f, 0.0f, 35, 1, 1, 1};
        if (lmat_ctx_create(0, &prm, &c)) return 1;
        CHECK(lmat_db_save_image(c, good.c_str()) == LMAT_E_ARG);
        lmat_ctx_destroy(c);
    }
    unlink(good.c_str()); unlink(again.c_str()); unlink(bad.c_str());
    rmdir(dir.c_str());
    CHECK(n_refused > 300);
    puts("image host paths: clean");
    return 0;
}
