// content_summ -- the consumer of read_label's .out files that bin/run_cs.sh runs (src/content_summ.cpp, argv at
// bin/run_cs.sh:148): the taxonomy tree of everything a run called, with read counts, and per rank the k-mer coverage
// of the reads called to a node -- how many distinct canonical k-mers (k = 8,10,12,14,17 by default of the script) those
// reads hold and how often each occurs.  No database lookups: a re-scan of the text records.  Same getopt letters, same
// report files (<o>, <o>.<rank>_kmer_cov) and stdout lines as upstream, byte for byte on the reference's example run
// (tests/test_content_summ.py).  Host code only; one worker per input file like upstream's OpenMP region (:361-413).
//
// Restated quirks that shape the files:
//   * the FIRST node of every rank the tree walk meets gets its <rank>_kmer_cov file created but no rows: upstream's new
//     stream lands in a shadowed variable (:522-531), so `kos` is still NULL for that node;
//   * rows are written only for nodes with more than one read (:534);
//   * a called taxid without a rank-table entry reads as rank "" (operator[] inserts): a file "<o>._kmer_cov" appears;
//   * strain -> species folding uses the FIRST species on the path (map::insert keeps the first, :342-351);
//   * a read's k-mers are counted once per read (set no_dups, :131-150).
//
// -G (a letter upstream's getopt string leaves free) or LMAT_CS_GPU=1 moves the k-mer counting to the GPU: the engine is loaded at
// run time (LMAT_LIB, else ../liblmat_hip.so beside the executable), the workers keep the text and the taxid of every selected read
// instead of counting, one lmat_cov_run (include/lmat_hip.h) serves all k sizes, and the rows are printed from its
// reports by the same statements.  Without the switch nothing of this is touched and no library is loaded.  There is no fallback:
// a library that cannot be loaded, no usable HIP device or a failing lmat_cov_* call ends the run with a message and a non-zero exit.
#include <dlfcn.h>
#include <getopt.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iostream>
#include <list>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "outfmt.hpp"
#include "../../include/lmat_hip.h"   // types and prototypes only: the functions are looked up with dlsym

#define LMAT_VERSION "1.2.4_2018a"

typedef uint32_t tid_t;
typedef std::map<uint64_t, uint64_t> kmer_cnt_t;

static std::unordered_set<int> gLowNumPlasmid;
static bool is_plasmid(tid_t t) { return (t >= 10000000 && t < 11000000) || gLowNumPlasmid.count((int)t); }  // :58
static bool is_human(tid_t t) { return t == 9606 || t == 63221 || t == 741158; }                              // tid_checks.hpp:15-28

// TaxTree<TID_T>(file) + getPathToRoot + getName (src/kmerdb/TaxTree.hpp:24-95, TaxNode.hpp:131-147)
struct Tree {
    std::unordered_map<tid_t, tid_t> parent;
    std::unordered_map<tid_t, std::string> name;
    bool load(const char* fn) {
        std::ifstream in(fn);
        if (!in.is_open()) { std::cerr << "failed to open " << fn << " for reading\n"; return false; }
        std::string line;
        std::getline(in, line);
        std::getline(in, line);
        int count;
        in >> count;
        std::getline(in, line);
        while (true) {
            std::streampos p = in.tellg();
            if (in.eof() || !in.good() || (int)p == -1) break;
            tid_t id = 0, ct = 0, c = 0, par = 0;
            in >> id >> ct;
            for (tid_t j = 0; j < ct; ++j) in >> c;
            in >> par;
            std::string nm;
            std::getline(in, nm);
            std::getline(in, nm);
            if (!in && nm.empty() && id == 0) break;
            parent[id] = par;
            name[id] = nm;
        }
        return true;
    }
    void path_to_root(tid_t t, std::vector<tid_t>& out) const {  // parent .. root
        out.clear();
        auto it = parent.find(t);
        size_t guard = 0;
        while (it != parent.end() && it->second != t && guard++ < 100000) {
            t = it->second;
            out.push_back(t);
            it = parent.find(t);
        }
    }
    std::string get_name(tid_t t) const { auto it = name.find(t); return it == name.end() ? "" : it->second; }
};

// the distinct canonical k-mers of one read, for every tracked k, counted once per read (:113-152)
static void store_kmers(const std::string& s, const std::vector<int>& klen, tid_t taxid, std::vector<std::map<tid_t, kmer_cnt_t>>& track) {
    const unsigned kls = (unsigned)klen.size();
    std::vector<int> k(kls, 0), high(kls, 0);
    std::vector<uint64_t> mask(kls, 0), fwd(kls, 0), rev(kls, 0);
    std::vector<std::set<uint64_t>> no_dups(kls);
    for (unsigned i = 0; i < kls; ++i) { high[i] = (klen[i] - 1) * 2; mask[i] = ((uint64_t)1 << klen[i] * 2) - 1; }
    for (size_t j = 0; j < s.size(); ++j) {
        int t;
        switch (s[j]) {
            case 'a': case 'A': t = 0; break;
            case 'c': case 'C': t = 1; break;
            case 'g': case 'G': t = 2; break;
            case 't': case 'T': t = 3; break;
            default: t = -1;
        }
        for (unsigned i = 0; i < kls; ++i) {
            if (t < 0) { k[i] = 0; continue; }
            fwd[i] = ((fwd[i] << 2) | (uint64_t)t) & mask[i];
            rev[i] = ((uint64_t)(t ^ 3) << high[i]) | (rev[i] >> 2);
            if (++k[i] >= klen[i]) {
                const uint64_t id = fwd[i] < rev[i] ? fwd[i] : rev[i];
                if (!no_dups[i].insert(id).second) continue;
                track[i][taxid][id] += 1;
            }
        }
    }
}

static void comp_kmer_cov(const std::vector<std::vector<std::map<tid_t, kmer_cnt_t>>>& track, tid_t tid, std::ofstream& ofs,
                          const std::vector<int>& kv) {  // :538-571
    for (unsigned ksi = 0; ksi < kv.size(); ++ksi) {
        kmer_cnt_t merge;
        uint64_t kmer_cnt = 0;
        int kcnt_sum = 0;
        for (auto& th : track) {
            auto it = th[ksi].find(tid);
            if (it == th[ksi].end()) continue;
            for (auto& kc : it->second) {
                kcnt_sum += (int)kc.second;
                auto m = merge.find(kc.first);
                if (m == merge.end()) { merge[kc.first] = kc.second; ++kmer_cnt; }
                else m->second += kc.second;
            }
        }
        std::vector<unsigned> ids;
        std::map<unsigned, unsigned> hist;
        for (auto& kc : merge) {
            const int cnt = (int)kc.second;
            if (!hist.count(cnt)) { hist[cnt] = 1; ids.push_back(cnt); }
            else hist[cnt] += 1;
        }
        std::sort(ids.begin(), ids.end());
        ofs << "taxid=" << tid << " distinct_kmer_cnt=" << kmer_cnt << " k_size=" << kv[ksi] << " tot_kmer_cnt=" << kcnt_sum << std::endl;
        for (unsigned id : ids) ofs << tid << " " << kv[ksi] << " " << id << " " << hist[id] << std::endl;
    }
}

// The engine, loaded at run time, and the coverage object of the run (-G / LMAT_CS_GPU=1).
struct GpuCov {
    void* so = nullptr;
    decltype(&lmat_ctx_create) ctx_create = nullptr;
    decltype(&lmat_ctx_destroy) ctx_destroy = nullptr;
    decltype(&lmat_cov_create) create = nullptr;
    decltype(&lmat_cov_destroy) destroy = nullptr;
    decltype(&lmat_cov_error) error = nullptr;
    decltype(&lmat_cov_add_reads) add_reads = nullptr;
    decltype(&lmat_cov_run) run = nullptr;
    decltype(&lmat_cov_summary) summary = nullptr;
    decltype(&lmat_cov_histogram) histogram = nullptr;
    lmat_ctx* ctx = nullptr;
    lmat_cov* cov = nullptr;
    lmat_cov_stats stats;
    std::vector<std::map<tid_t, std::pair<uint64_t, uint64_t>>> summ;   // [k index][taxid] -> (distinct, total)

    [[noreturn]] void fail(const std::string& what, int rc) {
        std::cerr << "content_summ -G: " << what << " failed (" << rc << "): " << (cov ? error(cov) : "") << std::endl;
        exit(1);
    }
    template <class F> void sym(F& f, const char* name, const std::string& lib) {
        f = reinterpret_cast<F>(dlsym(so, name));
        if (!f) { std::cerr << "content_summ -G: " << lib << " has no " << name << ": " << dlerror() << std::endl; exit(1); }
    }
    void open(const std::vector<int>& k_size) {
        std::string lib;
        if (const char* e = getenv("LMAT_LIB")) lib = e;
        if (lib.empty()) {
            char self[4096];
            const ssize_t n = readlink("/proc/self/exe", self, sizeof(self) - 1);
            std::string dir = n > 0 ? std::string(self, (size_t)n) : std::string(".");
            const size_t sl = dir.rfind('/');
            dir = sl == std::string::npos ? "." : dir.substr(0, sl);
            lib = dir + "/../liblmat_hip.so";
        }
        so = dlopen(lib.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!so) { std::cerr << "content_summ -G: cannot load " << lib << ": " << dlerror() << std::endl; exit(1); }
        sym(ctx_create, "lmat_ctx_create", lib);
        sym(ctx_destroy, "lmat_ctx_destroy", lib);
        sym(create, "lmat_cov_create", lib);
        sym(destroy, "lmat_cov_destroy", lib);
        sym(error, "lmat_cov_error", lib);
        sym(add_reads, "lmat_cov_add_reads", lib);
        sym(run, "lmat_cov_run", lib);
        sym(summary, "lmat_cov_summary", lib);
        sym(histogram, "lmat_cov_histogram", lib);
        int rc = ctx_create(0, nullptr, &ctx);
        if (rc != LMAT_OK) {   // no context, so no message of the library's: LMAT_E_DEVICE is what it returns without a device it can set up
            if (rc == LMAT_E_DEVICE) std::cerr << "content_summ -G: no usable HIP device (lmat_ctx_create: LMAT_E_DEVICE)";
            else std::cerr << "content_summ -G: lmat_ctx_create failed with code " << rc << (rc == LMAT_E_NOMEM ? " (out of memory)" : "");
            std::cerr << "; there is no host fallback with -G" << std::endl;
            exit(1);
        }
        rc = create(ctx, k_size.data(), (int)k_size.size(), &cov);
        if (rc != LMAT_OK) { std::cerr << "content_summ -G: lmat_cov_create failed (" << rc << ")" << std::endl; exit(1); }
    }
    // the selected reads of one file, in file order
    void add(const std::vector<std::string>& reads, const std::vector<tid_t>& tids) {
        std::string blob;
        std::vector<uint64_t> off(1, 0);
        for (const std::string& r : reads) { blob += r; off.push_back(blob.size()); }
        blob.push_back('\0');
        const int rc = add_reads(cov, (const uint8_t*)blob.data(), off.data(), reads.size(), tids.data());
        if (rc != LMAT_OK) fail("lmat_cov_add_reads", rc);
    }
    void count(size_t n_k) {
        int rc = run(cov, &stats);
        if (rc != LMAT_OK) fail("lmat_cov_run", rc);
        summ.resize(n_k);
        for (size_t ksi = 0; ksi < n_k; ++ksi) {
            uint64_t n = 0;
            rc = summary(cov, (int)ksi, nullptr, nullptr, nullptr, 0, &n);
            if (rc != LMAT_OK && rc != LMAT_E_CAPACITY) fail("lmat_cov_summary", rc);
            std::vector<uint32_t> g(n + 1);
            std::vector<uint64_t> d(n + 1), t(n + 1);
            rc = summary(cov, (int)ksi, g.data(), d.data(), t.data(), n, &n);
            if (rc != LMAT_OK) fail("lmat_cov_summary", rc);
            for (uint64_t i = 0; i < n; ++i) summ[ksi][g[i]] = std::make_pair(d[i], t[i]);
        }
    }
    void close() {
        if (cov) destroy(cov);
        if (ctx) ctx_destroy(ctx);
        cov = nullptr;
        ctx = nullptr;
    }
};

// comp_kmer_cov from the device's reports: the same lines through the same types
static void comp_kmer_cov_gpu(GpuCov& G, tid_t tid, std::ofstream& ofs, const std::vector<int>& kv) {
    for (unsigned ksi = 0; ksi < kv.size(); ++ksi) {
        uint64_t kmer_cnt = 0;
        int kcnt_sum = 0;
        auto it = G.summ[ksi].find(tid);
        if (it != G.summ[ksi].end()) { kmer_cnt = it->second.first; kcnt_sum = (int)(uint32_t)it->second.second; }
        uint64_t n = 0;
        int rc = G.histogram(G.cov, (int)ksi, tid, nullptr, nullptr, 0, &n);
        if (rc != LMAT_OK && rc != LMAT_E_CAPACITY) G.fail("lmat_cov_histogram", rc);
        std::vector<uint64_t> mult(n + 1), cnt(n + 1);
        if (n) {
            rc = G.histogram(G.cov, (int)ksi, tid, mult.data(), cnt.data(), n, &n);
            if (rc != LMAT_OK) G.fail("lmat_cov_histogram", rc);
        }
        ofs << "taxid=" << tid << " distinct_kmer_cnt=" << kmer_cnt << " k_size=" << kv[ksi] << " tot_kmer_cnt=" << kcnt_sum << std::endl;
        for (uint64_t i = 0; i < n; ++i) ofs << tid << " " << kv[ksi] << " " << (unsigned)(int)mult[i] << " " << (unsigned)cnt[i] << std::endl;
    }
}

int main(int argc, char* argv[]) {
    float threshold = 0.0f;
    std::string query_fn_lst, lmat_sum, ofbase, tax_tree_fn, rank_table_file, low_num_plasmid_file, k_size_str, rank_check_str;
    bool skip_human = false, do_human_reg = false;
    bool gpu = false;
    if (const char* e = getenv("LMAT_CS_GPU")) gpu = !strcmp(e, "1");
    int c;
    while ((c = getopt(argc, argv, "m:f:a:h:njb:ye:wp:k:c:v:k:i:d:l:t:sr:o:x:f:q:VG")) != -1) {
        switch (c) {
            case 'G': gpu = true; break;
            case 'n': do_human_reg = true; break;
            case 'a': rank_check_str = optarg; break;
            case 'p': low_num_plasmid_file = optarg; break;
            case 's': skip_human = true; break;
            case 'r': rank_table_file = optarg; break;
            case 'y': break;  // verbose dumps are not produced
            case 'l': lmat_sum = optarg; break;
            case 'v': threshold = (float)atof(optarg); break;
            case 'c': tax_tree_fn = optarg; break;
            case 'k': k_size_str = optarg; break;
            case 'f': query_fn_lst = optarg; break;
            case 'i': break;
            case 'o': ofbase = optarg; break;
            case 'V': std::cout << "LMAT version " << LMAT_VERSION << "\n"; return 0;
            default: std::cout << "Unrecognized option: " << (char)c << ", ignore." << std::endl;
        }
    }
    std::vector<int> k_size;
    if (k_size_str.empty()) k_size = {8, 10, 14, 20};
    else {
        std::stringstream ss(k_size_str);
        std::string tok;
        while (std::getline(ss, tok, ',')) if (!tok.empty()) k_size.push_back(atoi(tok.c_str()));
    }
    for (int k : k_size) if (k < 1 || k > 31) { std::cerr << "k sizes must lie in 1..31" << std::endl; return -1; }
    std::set<std::string> rank_check;
    {
        std::stringstream ss(rank_check_str);
        std::string tok;
        while (std::getline(ss, tok, ',')) if (!tok.empty()) { std::cout << "rank store: [" << tok << "]" << std::endl; rank_check.insert(tok); }
    }
    for (int k : k_size) std::cout << "track k size=" << k << std::endl;
    GpuCov G;
    if (gpu) G.open(k_size);   // before any work: without the engine or a device the run ends here
    if (!low_num_plasmid_file.empty()) {
        std::ifstream ifs(low_num_plasmid_file.c_str());
        if (!ifs) std::cerr << "Unexpected reading error: " << low_num_plasmid_file << std::endl;
        tid_t pid;
        while (ifs >> pid) gLowNumPlasmid.insert((int)pid);
    }
    std::unordered_map<tid_t, std::string> rank_table;
    if (!rank_table_file.empty()) {
        std::ifstream ifs(rank_table_file.c_str());
        tid_t t;
        std::string rank;
        while (ifs >> t >> rank) rank_table.insert(std::make_pair(t, rank));
    }
    std::vector<std::string> files;
    {
        std::ifstream ifs(query_fn_lst.c_str());
        std::string fn;
        while (ifs >> fn) files.push_back(fn);
    }
    const int n_threads = (int)files.size();
    std::cout << "set threads=" << n_threads << std::endl;
    if (n_threads < 1) { std::cerr << "no input files in [" << query_fn_lst << "]" << std::endl; return -1; }
    std::cout << "Read taxonomy tree: " << tax_tree_fn << std::endl;
    Tree tree;
    if (!tree.load(tax_tree_fn.c_str())) return -1;
    std::cout << "Done Read taxonomy tree: " << tax_tree_fn << std::endl;
    std::map<tid_t, float> weighted_readcnt;
    std::map<tid_t, int> read_cnts;
    std::ifstream call_ifs(lmat_sum.c_str());
    if (!call_ifs) { std::cerr << "Failed to open " << lmat_sum << " must exit now" << std::endl; return -1; }
    std::list<tid_t> clst;
    std::unordered_map<tid_t, tid_t> strain2spec;
    auto is_fold_rank = [&](tid_t t) {
        const std::string& r = rank_table[t];
        return (r == "species" && !do_human_reg) || (r == "region" && do_human_reg);
    };
    {
        std::string buff;
        while (std::getline(call_ifs, buff)) {
            if (buff.find("\tNULL\t") != std::string::npos) continue;
            std::istringstream istrm(buff);
            tid_t tid = 0;
            unsigned read_cnt = 0;
            std::string descrip;
            float wght_rc = 0;
            istrm >> wght_rc >> read_cnt >> tid >> descrip;
            weighted_readcnt.insert(std::make_pair(tid, wght_rc));
            read_cnts.insert(std::make_pair(tid, (int)read_cnt));
            if (is_fold_rank(tid)) strain2spec.insert(std::make_pair(tid, tid));
            if (!is_plasmid(tid)) {
                std::vector<tid_t> ptor;
                tree.path_to_root(tid, ptor);
                for (tid_t a : ptor) if (is_fold_rank(a)) strain2spec.insert(std::make_pair(tid, a));
            }
            clst.push_back(tid);
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::vector<std::map<tid_t, kmer_cnt_t>>> kmer_track(n_threads, std::vector<std::map<tid_t, kmer_cnt_t>>(k_size.size()));
    std::vector<std::vector<std::string>> sel_read(n_threads);   // -G: the selected reads of every file and the taxid each counts under
    std::vector<std::vector<tid_t>> sel_tid(n_threads);
    {
        std::vector<std::thread> th;
        std::vector<int> bad(n_threads, 0);
        for (int t = 0; t < n_threads; ++t)
            th.emplace_back([&, t]() {
                std::ifstream ifs(files[t].c_str());
                if (!ifs) { bad[t] = 1; return; }
                std::string line;
                while (std::getline(ifs, line)) {
                    const size_t p1 = line.find('\t'), p2 = line.find('\t', p1 + 1), p3 = line.find('\t', p2 + 1), p4 = line.find('\t', p3 + 1),
                                 p5 = line.find('\t', p4 + 1);
                    if (p1 == std::string::npos || p2 == std::string::npos) continue;
                    const std::string read_buff = line.substr(p1 + 1, p2 - p1 - 1);
                    const std::string call = line.substr(p4 + 1, p5 - p4 - 1);  // (npos + 1 == 0: a record without the candidate column reads from its start, as upstream)
                    if (call.empty() || call[0] == 'N' || call[0] == 'R') continue;
                    std::istringstream istrm(call);
                    float score = 0;
                    tid_t taxid = 0;
                    std::string match_type;
                    istrm >> taxid >> score >> match_type;
                    if (is_human(taxid) && skip_human) continue;
                    if (score < threshold) continue;
                    tid_t use_tid = taxid;
                    auto s2 = strain2spec.find(taxid);
                    if (s2 != strain2spec.end() && !is_plasmid(taxid)) use_tid = s2->second;
                    auto rk = rank_table.find(use_tid);
                    const std::string rnk = rk != rank_table.end() ? rk->second : "undef";
                    if (rank_check.count(rnk) || is_plasmid(taxid)) {
                        if (gpu) { sel_read[t].push_back(read_buff); sel_tid[t].push_back(use_tid); }
                        else store_kmers(read_buff, k_size, use_tid, kmer_track[t]);
                    }
                }
            });
        for (auto& x : th) x.join();
        for (int t = 0; t < n_threads; ++t)
            if (bad[t]) { std::cerr << "did not open for reading: [" << files[t] << "] tid: [" << t << "]" << std::endl; return -1; }
    }
    if (gpu) {
        for (int t = 0; t < n_threads; ++t) {
            G.add(sel_read[t], sel_tid[t]);
            std::vector<std::string>().swap(sel_read[t]);
        }
        G.count(k_size.size());
    }
    // the tree of the called taxids (:415-440) and its walk, children in reverse order of arrival (:447-536)
    std::set<tid_t> seen;
    std::ofstream ofs(ofbase.c_str());
    std::map<tid_t, std::list<tid_t>> child;
    for (tid_t tid : clst) {
        std::vector<tid_t> ptor;
        tree.path_to_root(tid, ptor);
        tid_t child_node = tid;
        for (tid_t ptid : ptor) {
            if (!seen.count(child_node)) {
                seen.insert(child_node);
                child[ptid].push_back(child_node);
            }
            child_node = ptid;
        }
    }
    ofs << "Name\tTaxID\tReads\tWReads" << std::endl;
    std::map<tid_t, std::string> tab_lst;
    std::list<tid_t> open;
    open.push_back(1);  // "should always be root"
    std::map<std::string, std::ofstream*> rank_ofs;
    while (!open.empty()) {
        const tid_t tid = open.front();
        open.pop_front();
        const std::list<tid_t>& lst = child[tid];
        const std::string chk = tab_lst[tid] + "\t";
        for (tid_t ch : lst) { tab_lst[ch] = chk; open.push_front(ch); }
        const unsigned tot_read_cnt = (unsigned)read_cnts[tid];
        float wrdc = 0;
        if (tot_read_cnt > 0) {
            wrdc = weighted_readcnt[tid];
            std::string rank = rank_table[tid];
            if (rank != "no_rank") {
                if (is_plasmid(tid)) rank = "plasmid";
                std::ofstream* kos = nullptr;
                auto it = rank_ofs.find(rank);
                if (it != rank_ofs.end()) kos = it->second;
                else {
                    const std::string fn = ofbase + "." + rank + "_kmer_cov";
                    std::ofstream* made = new std::ofstream(fn.c_str());
                    if (!(*made)) std::cout << "Unable to write to " << fn << " will try to continue" << std::endl;
                    rank_ofs.insert(std::make_pair(rank, made));  // upstream's `kos` stays NULL here: the first node of a rank writes no rows
                }
                if (kos && tot_read_cnt > 1) {
                    if (gpu) comp_kmer_cov_gpu(G, tid, *kos, k_size);
                    else comp_kmer_cov(kmer_track, tid, *kos, k_size);
                }
            }
        }
        std::string s = tab_lst[tid];
        s += tree.get_name(tid);
        s += '\t'; lmat::put_int(s, (long long)tid);
        s += '\t'; lmat::put_int(s, (long long)tot_read_cnt);
        s += '\t'; lmat::put_float(s, wrdc);
        ofs << s << std::endl;
    }
    for (auto& p : rank_ofs) { p.second->close(); delete p.second; }
    if (gpu) {
        std::cout << "kmer coverage on device: reads=" << G.stats.reads << " windows=" << G.stats.windows << " passes=" << G.stats.passes << std::endl;
        G.close();
    }
    std::cout << "query time: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << std::endl;
    return 0;
}
