// dump_tax_histo -- a database image (device or ingest format) back out as the tax_histo binary it was made from, exported on the GPU
// (lmat_export_*).  The option letters of the files a context needs are read_label's.  With -C the per-taxid k-mer
// counts of the database are written as the reference's frequency_counter writes them (src/frequency_counter.cpp:132-143).
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/lmat_hip.h"

static void usage() {
    fprintf(stderr,
            "Usage:\n"
            " -d <string>  - database image (lmat_db_save_image / make_db_image)\n"
            " -c <string>  - tax tree data file\n"
            " -e <string>  - taxid depth file\n"
            " -w <string>  - taxid rank file\n"
            " -f <string>  - 32->16 id map of the database; optional (a database of 32-bit taxids has none)\n"
            " -o <string>  - output tax_histo filename\n"
            " -C <string>  - counts prefix: writes <prefix>.par.kcnt ('<taxid> <count>' lines, ascending); optional\n"
            " -b <float>   - device memory budget in GiB; optional; default: half of the free memory\n"
            " -p <int>     - prefix bits: the k-mer space is exported in 2^p passes; optional; default: derived from the budget\n"
            " -h           - print help and exit\n\n");
}

int main(int argc, char* argv[]) {
    std::string image_fn, tree_fn, depth_fn, rank_fn, map_fn, out_fn, counts_prefix;
    int prefix_bits = -1;
    double budget_gib = 0;
    int c;
    while ((c = getopt(argc, argv, "d:c:e:w:f:o:C:b:p:h")) != -1) {
        switch (c) {
            case 'd': image_fn = optarg; break;
            case 'c': tree_fn = optarg; break;
            case 'e': depth_fn = optarg; break;
            case 'w': rank_fn = optarg; break;
            case 'f': map_fn = optarg; break;
            case 'o': out_fn = optarg; break;
            case 'C': counts_prefix = optarg; break;
            case 'b': budget_gib = atof(optarg); break;
            case 'p': prefix_bits = atoi(optarg); break;
            default: usage(); return c == 'h' ? 0 : 255;
        }
    }
    if (image_fn.empty() || tree_fn.empty() || depth_fn.empty() || out_fn.empty()) { usage(); return 255; }
    lmat_ctx* ctx = nullptr;
    if (lmat_ctx_create(0, nullptr, &ctx) != LMAT_OK) { fprintf(stderr, "ERROR! no usable HIP device (the engine has no CPU path)\n"); return 1; }
    int rc = lmat_taxonomy_load_files(ctx, tree_fn.c_str(), depth_fn.c_str(), rank_fn.empty() ? nullptr : rank_fn.c_str(),
                                      map_fn.empty() ? nullptr : map_fn.c_str(), nullptr);
    if (rc == LMAT_OK) rc = lmat_db_load_image(ctx, image_fn.c_str(), 0);
    if (rc == LMAT_OK) rc = lmat_db_finalize(ctx);
    if (rc != LMAT_OK) { fprintf(stderr, "ERROR! %s\n", lmat_last_error(ctx)); lmat_ctx_destroy(ctx); return 1; }
    lmat_export* x = nullptr;
    if (lmat_export_create(ctx, &x) != LMAT_OK) { fprintf(stderr, "ERROR! %s\n", lmat_last_error(ctx)); lmat_ctx_destroy(ctx); return 1; }
    auto fail = [&](const char* what) {
        fprintf(stderr, "ERROR! %s: %s\n", what, lmat_export_error(x));
        lmat_export_destroy(x);
        lmat_ctx_destroy(ctx);
        return 1;
    };
    if (lmat_export_set_options(x, (uint64_t)(budget_gib * 1073741824.0), prefix_bits) != LMAT_OK) return fail("options");
    const auto t0 = std::chrono::steady_clock::now();
    lmat_export_stats s;
    if (lmat_export_run(x, out_fn.c_str(), &s) != LMAT_OK) return fail("export");
    const double tm = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("kmer count: %llu\n", (unsigned long long)s.records);
    printf("from buckets: %llu from overflow: %llu passes: %llu\n", (unsigned long long)s.from_buckets, (unsigned long long)s.from_overflow, (unsigned long long)s.passes);
    printf("ms: scan %.3f sort %.3f lists %.3f fetch %.3f write %.3f\n", s.ms_scan, s.ms_sort, s.ms_lists, s.ms_fetch, s.ms_write);
    printf("kmers per second: %g\n", tm > 0 ? (double)s.records / tm : 0.0);
    if (!counts_prefix.empty()) {
        uint64_t n = 0;
        lmat_export_taxid_counts(x, nullptr, nullptr, 0, &n);
        std::vector<uint32_t> tids(n ? n : 1);
        std::vector<uint64_t> counts(n ? n : 1);
        if (lmat_export_taxid_counts(x, tids.data(), counts.data(), n, &n) != LMAT_OK) return fail("counts");
        const std::string fn = counts_prefix + ".par.kcnt";
        printf("\nwriting output to: %s\n", fn.c_str());
        FILE* cf = fopen(fn.c_str(), "w");
        if (!cf) { fprintf(stderr, "ERROR! cannot open %s for writing\n", fn.c_str()); lmat_export_destroy(x); lmat_ctx_destroy(ctx); return 1; }
        for (uint64_t i = 0; i < n; ++i) fprintf(cf, "%u %llu\n", tids[i], (unsigned long long)counts[i]);
        if (fclose(cf) != 0) { fprintf(stderr, "ERROR! write error on %s\n", fn.c_str()); lmat_export_destroy(x); lmat_ctx_destroy(ctx); return 1; }
        printf("Total-tid: %llu\n", (unsigned long long)s.entries);
        printf("Singletons: %llu\n", (unsigned long long)s.singletons);
    }
    lmat_export_destroy(x);
    lmat_ctx_destroy(ctx);
    return 0;
}
