// dump_tax_histo -- a database image (device or ingest format) back out as the tax_histo binary it was made from, exported on the GPU
// (lmat_export_*).  The option letters of the files a context needs are read_label's.  With -C the per-taxid k-mer
// counts of the database are written as the reference's frequency_counter writes them (src/frequency_counter.cpp:132-143).
// -T / -M / -L / -N export a taxonomic slice instead (lmat_export_set_filter): file and counts then describe the slice.
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
            " -T <taxid[,taxid...]> - slice: the taxa whose subtrees form the set S; repeatable; optional\n"
            " -M <string>  - slice: any | all | none -- keep a k-mer iff any / every / no list entry lies in S; default with -T: any\n"
            " -L <int>     - slice: keep a k-mer iff every list entry has tree depth >= this (for closed lists: the depth of the LCA); optional\n"
            " -N <int>     - slice: keep a k-mer iff its list has at most this many entries; optional\n"
            " -h           - print help and exit\n\n");
}

int main(int argc, char* argv[]) {
    std::string image_fn, tree_fn, depth_fn, rank_fn, map_fn, out_fn, counts_prefix;
    int prefix_bits = -1;
    double budget_gib = 0;
    std::vector<uint32_t> taxa;
    std::string mode_name;
    uint32_t min_depth = 0, max_entries = 0;
    int c;
    while ((c = getopt(argc, argv, "d:c:e:w:f:o:C:b:p:T:M:L:N:h")) != -1) {
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
            case 'T':
                for (const char* s = optarg; *s;) {
                    char* end = nullptr;
                    const unsigned long t = strtoul(s, &end, 10);
                    if (end == s || (*end && *end != ',')) { fprintf(stderr, "ERROR! -T takes taxids separated by commas, got '%s'\n", optarg); return 255; }
                    taxa.push_back((uint32_t)t);
                    s = *end ? end + 1 : end;
                }
                break;
            case 'M': mode_name = optarg; break;
            case 'L': min_depth = (uint32_t)strtoul(optarg, nullptr, 10); break;
            case 'N': max_entries = (uint32_t)strtoul(optarg, nullptr, 10); break;
            default: usage(); return c == 'h' ? 0 : 255;
        }
    }
    if (image_fn.empty() || tree_fn.empty() || depth_fn.empty() || out_fn.empty()) { usage(); return 255; }
    int mode = 0;
    if (mode_name.empty()) mode = taxa.empty() ? 0 : LMAT_SLICE_ANY;
    else if (mode_name == "any") mode = LMAT_SLICE_ANY;
    else if (mode_name == "all") mode = LMAT_SLICE_ALL;
    else if (mode_name == "none") mode = LMAT_SLICE_NONE;
    else { fprintf(stderr, "ERROR! -M takes any, all or none\n"); return 255; }
    const bool slicing = mode || !taxa.empty() || min_depth || max_entries;
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
    if (slicing) {
        const lmat_export_filter flt = {taxa.empty() ? nullptr : taxa.data(), (uint32_t)taxa.size(), mode, min_depth, max_entries};
        if (lmat_export_set_filter(x, &flt) != LMAT_OK) return fail("filter");
    }
    const auto t0 = std::chrono::steady_clock::now();
    lmat_export_stats s;
    if (lmat_export_run(x, out_fn.c_str(), &s) != LMAT_OK) return fail("export");
    const double tm = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("kmer count: %llu\n", (unsigned long long)s.records);
    printf("from buckets: %llu from overflow: %llu passes: %llu\n", (unsigned long long)s.from_buckets, (unsigned long long)s.from_overflow, (unsigned long long)s.passes);
    printf("ms: scan %.3f sort %.3f lists %.3f fetch %.3f write %.3f\n", s.ms_scan, s.ms_sort, s.ms_lists, s.ms_fetch, s.ms_write);
    printf("kmers per second: %g\n", tm > 0 ? (double)s.records / tm : 0.0);
    if (slicing) {
        uint64_t f6[6];
        double ms_select = 0;
        if (lmat_export_filter_stats(x, f6, &ms_select) != LMAT_OK) return fail("filter statistics");
        printf("slice: scanned %llu kept %llu dropped: taxon %llu depth %llu length %llu; long lists %llu; select ms %.3f\n", (unsigned long long)f6[0],
               (unsigned long long)f6[1], (unsigned long long)f6[2], (unsigned long long)f6[3], (unsigned long long)f6[4], (unsigned long long)f6[5], ms_select);
    }
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
