// build_tax_histo -- genome FASTA + taxonomy tree -> the tax_histo binary read_label -d / make_db_image ingest, on the GPU.
// One tool for the reference's kmerPrefixCounter (src/kmerPrefixCounter.cpp) + tax_histo (src/tax_histo.cpp) pair; the
// closing stdout lines keep tax_histo's wording (tax_histo.cpp:297-313).  With -m existing tax_histo files are merged in (adding genomes to
// a database), with -G a gene database is built (gene FASTA -> per k-mer the ids of the records that hold it; no tree), with -D a loaded database image is (needs -e / -w and, for a 16-bit database, -f: the files a context loads); -c writes the per-taxid k-mer counts of the result as countTaxidFrequency does (src/countTaxidFrequency.cpp:133-139).
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "../../include/lmat_hip.h"

static void usage() {
    fprintf(stderr,
            "Usage:\n"
            " -i <string>  - input fasta_fn (headers: '>' + decimal taxid), or with -l a file that lists fasta files; optional with -m\n"
            " -l           - -i names a list of fasta files, one per line\n"
            " -k <int>     - kmer length (1..20)\n"
            " -t <string>  - tax tree data file\n"
            " -G           - gene database: headers are '>' + gene id (1..4294967295), lists are the ids that hold the k-mer; takes no -t, no -D\n"
            " -o <string>  - output filename\n"
            " -b <float>   - device memory budget in GiB; optional; default: half of the free memory\n"
            " -m <string>  - existing tax_histo file to merge in (same -k); repeatable; optional\n"
            " -D <string>  - device or ingest image of a database to merge in, exported on the GPU; repeatable; needs -e -w [-f]\n"
            " -e <string>  - taxid depth file, -w <string> - rank file, -f <string> - 32->16 id map: the taxonomy files of the -D images\n"
            " -c <string>  - write '<taxid> <count>' lines, ascending: the result's k-mers per taxid; optional\n"
            " -p <int>     - prefix bits: the k-mer space is built in 2^p passes; optional; default: derived from the budget\n"
            " -V           - print version and exit\n"
            " -h           - print help and exit\n\n");
}

int main(int argc, char* argv[]) {
    printf("invocation: ");
    for (int j = 0; j < argc; j++) printf("%s ", argv[j]);
    printf("\n");
    std::string input_fn, tree_fn, out_fn, counts_fn;
    std::vector<std::string> merge_fns, image_fns;
    std::string depth_fn, rank_fn, map_fn;
    int k = 0, prefix_bits = -1;
    bool is_list = false, genes = false;
    double budget_gib = 0;
    int c;
    while ((c = getopt(argc, argv, "i:lk:t:o:b:p:m:c:D:e:w:f:GVh")) != -1) {
        switch (c) {
            case 'i': input_fn = optarg; break;
            case 'l': is_list = true; break;
            case 'k': k = atoi(optarg); break;
            case 't': tree_fn = optarg; break;
            case 'o': out_fn = optarg; break;
            case 'b': budget_gib = atof(optarg); break;
            case 'p': prefix_bits = atoi(optarg); break;
            case 'm': merge_fns.push_back(optarg); break;
            case 'c': counts_fn = optarg; break;
            case 'D': image_fns.push_back(optarg); break;
            case 'e': depth_fn = optarg; break;
            case 'w': rank_fn = optarg; break;
            case 'f': map_fn = optarg; break;
            case 'G': genes = true; break;
            case 'V': printf("build_tax_histo (lmat_hip) 1\n"); return 0;
            default: usage(); return c == 'h' ? 0 : 255;
        }
    }
    if (genes && !image_fns.empty()) { fprintf(stderr, "-D is not available with -G: device images hold taxonomy databases; merge gene databases as files (-m)\n"); return 255; }
    if (genes && !tree_fn.empty()) { fprintf(stderr, "-G takes no taxonomy tree (-t)\n"); usage(); return 255; }
    if (!image_fns.empty() && depth_fn.empty()) { fprintf(stderr, "-D needs the taxonomy files of the image: -e <depth> -w <rank> [-f <map>]\n"); usage(); return 255; }
    if ((input_fn.empty() && merge_fns.empty() && image_fns.empty()) || (tree_fn.empty() && !genes) || out_fn.empty() || k == 0) { usage(); return 255; }
    std::vector<std::string> fastas;
    if (input_fn.empty()) {
    } else if (is_list) {
        std::ifstream in(input_fn);
        if (!in) { fprintf(stderr, "failed to open %s for reading\n", input_fn.c_str()); return 1; }
        std::string line;
        while (std::getline(in, line)) if (!line.empty()) fastas.push_back(line);
    } else fastas.push_back(input_fn);

    lmat_ctx* ctx = nullptr;
    if (lmat_ctx_create(0, nullptr, &ctx) != LMAT_OK) { fprintf(stderr, "ERROR! no usable HIP device (the engine has no CPU path)\n"); return 1; }
    if (!genes) printf("info: starting tax tree load from filename: %s\n", tree_fn.c_str());
    lmat_build* b = nullptr;
    int rc = genes ? lmat_genebuild_create(ctx, k, &b) : lmat_build_create(ctx, k, tree_fn.c_str(), &b);
    if (rc != LMAT_OK) { fprintf(stderr, "ERROR! %s\n", lmat_last_error(ctx)); lmat_ctx_destroy(ctx); return 1; }
    auto fail = [&](const char* what) {
        fprintf(stderr, "ERROR! %s: %s\n", what, lmat_build_error(b));
        lmat_build_destroy(b);
        lmat_ctx_destroy(ctx);
        return 1;
    };
    if (lmat_build_set_options(b, (uint64_t)(budget_gib * 1073741824.0), prefix_bits, 0) != LMAT_OK) return fail("options");
    for (auto& fn : fastas) {
        printf("opening: %s\n", fn.c_str());
        if (lmat_build_add_fasta(b, fn.c_str()) != LMAT_OK) return fail("input");
    }
    for (auto& fn : merge_fns) {
        printf("merging: %s\n", fn.c_str());
        if (lmat_build_add_taxhisto(b, fn.c_str()) != LMAT_OK) return fail("input");
    }
    for (auto& fn : image_fns) {   // a context of its own holds the image while it is exported into the builder
        printf("merging database image: %s\n", fn.c_str());
        lmat_ctx* src = nullptr;
        if (lmat_ctx_create(0, nullptr, &src) != LMAT_OK) { fprintf(stderr, "ERROR! no usable HIP device\n"); lmat_build_destroy(b); lmat_ctx_destroy(ctx); return 1; }
        int r2 = lmat_taxonomy_load_files(src, tree_fn.c_str(), depth_fn.c_str(), rank_fn.empty() ? nullptr : rank_fn.c_str(), map_fn.empty() ? nullptr : map_fn.c_str(), nullptr);
        if (r2 == LMAT_OK) r2 = lmat_db_load_image(src, fn.c_str(), 0);
        if (r2 == LMAT_OK) r2 = lmat_db_finalize(src);
        if (r2 != LMAT_OK) { fprintf(stderr, "ERROR! %s: %s\n", fn.c_str(), lmat_last_error(src)); lmat_ctx_destroy(src); lmat_build_destroy(b); lmat_ctx_destroy(ctx); return 1; }
        r2 = lmat_build_add_db(b, src);
        lmat_ctx_destroy(src);
        if (r2 != LMAT_OK) return fail("input");
    }
    const auto t0 = std::chrono::steady_clock::now();
    lmat_build_stats s;
    if (lmat_build_run(b, &s) != LMAT_OK) return fail("build");
    const double tm = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "opening for writing: %s\n", out_fn.c_str());
    if (lmat_build_write_taxhisto(b, out_fn.c_str()) != LMAT_OK) return fail("output");
    if (!counts_fn.empty()) {
        uint64_t n = 0;
        lmat_build_taxid_counts(b, nullptr, nullptr, 0, &n);
        std::vector<uint32_t> tids(n ? n : 1);
        std::vector<uint64_t> counts(n ? n : 1);
        if (lmat_build_taxid_counts(b, tids.data(), counts.data(), n, &n) != LMAT_OK) return fail("counts");
        FILE* cf = fopen(counts_fn.c_str(), "w");
        if (!cf) { fprintf(stderr, "ERROR! cannot open %s for writing\n", counts_fn.c_str()); lmat_build_destroy(b); lmat_ctx_destroy(ctx); return 1; }
        for (uint64_t i = 0; i < n; ++i) fprintf(cf, "%u %llu\n", tids[i], (unsigned long long)counts[i]);
        if (fclose(cf) != 0) { fprintf(stderr, "ERROR! write error on %s\n", counts_fn.c_str()); lmat_build_destroy(b); lmat_ctx_destroy(ctx); return 1; }
    }
    printf("bases: %llu windows: %llu distinct kmers: %llu passes: %u\n", (unsigned long long)s.bases, (unsigned long long)s.windows,
           (unsigned long long)s.distinct_kmers, s.passes);
    printf("kernel ms: extract %.3f sort %.3f segment %.3f closure %.3f\n", s.extract_ms, s.sort_ms, s.segment_ms, s.closure_ms);
    if (!merge_fns.empty() || !image_fns.empty()) {
        lmat_merge_stats m;
        if (lmat_build_merge_stats(b, &m) != LMAT_OK) return fail("merge statistics");
        printf("merge: inputs %u records in %llu one source %llu merged %llu grown %llu\n", m.inputs, (unsigned long long)m.records_in,
               (unsigned long long)m.records_one_source, (unsigned long long)m.records_merged, (unsigned long long)m.records_grown);
        printf("merge ms: upload %.3f sort %.3f segment %.3f union %.3f histogram %.3f\n", m.upload_ms, m.sort_ms, m.segment_ms, m.union_ms, m.histogram_ms);
    }
    printf("longest list: %llu\n", (unsigned long long)s.longest_list);
    printf("total taxids: %llu\nrem kmer cnt: %llu\n", (unsigned long long)s.total_list_entries, (unsigned long long)s.dropped_unknown);
    printf("singletons: %llu\n", (unsigned long long)s.singletons);
    printf("\ntotal annotate time: %g\n", tm);
    printf("num mapping kmers processed: %llu\n", (unsigned long long)s.records_written);
    printf("kmers per second (not counting startup time): %g\n", tm > 0 ? (double)(merge_fns.empty() && image_fns.empty() ? s.distinct_kmers : s.records_written) / tm : 0.0);
    lmat_build_destroy(b);
    lmat_ctx_destroy(ctx);
    return 0;
}
