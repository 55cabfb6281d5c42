// pullfmt.hpp -- the id file and the output of upstream's read puller (bin/pull_reads.pl, run by bin/pull_reads_mc.sh), host only:
//   parse_pull_idfile   the script's id-file grammar (:36-67), line by line, into the groups lmat_bins_set takes
//   pull_fields         the four fields the script cuts out of a .out record (:77-78), taken from a result record exactly as
//                       outfmt.hpp prints them
//   PullWriter          the files the script writes for one .out file: names (:18), header line (:80), 80-column lines (:21-28)
// Shared by bins.hip (lmat_bins_set_from_file) and read_label -B; needs no device.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "outfmt.hpp"

namespace lmat {

struct PullGroup {
    std::string name;            // first token of the line: the suffix of the group's file
    std::vector<uint32_t> ids;   // every token of the line that is a printed taxid
    uint32_t flags = 0;          // LMAT_BIN_*
    float low_score = 0;
};

// A token can equal a printed taxid only if it is that number's canonical decimal text (the script's hash is keyed by strings).
inline bool pull_token_id(const std::string& t, uint32_t& id) {
    if (t.empty() || t.size() > 10 || (t.size() > 1 && t[0] == '0')) return false;
    uint64_t v = 0;
    for (char ch : t) {
        if (ch < '0' || ch > '9') return false;
        v = v * 10 + (uint64_t)(ch - '0');
    }
    if (v > 0xFFFFFFFFull) return false;
    id = (uint32_t)v;
    return true;
}

// One group per line, in file order (lines of one first token share a file; their ids still overwrite in line order).
//   ^LowScore\s+   the LowScore group; the second token is its score (missing: 0)
//   ^ReadTooShort  a file that stays empty (the script's branch looks up a handle it never opens)
//   else           first token = name; every token, the first included, is an id of the group; the name NoDbHits makes it the
//                  group of the NoDbHits reads
// Blank lines are skipped and leading blanks ignored (the script would make a group with an empty name of them).
inline bool parse_pull_idfile(const char* fn, std::vector<PullGroup>& out, std::string& err) {
    std::ifstream f(fn);
    if (!f) { err = std::string("cannot open id file ") + fn; return false; }
    std::string line;
    while (std::getline(f, line)) {
        std::vector<std::string> tok;
        size_t i = 0;
        while (i < line.size()) {
            while (i < line.size() && isspace((unsigned char)line[i])) ++i;
            size_t j = i;
            while (j < line.size() && !isspace((unsigned char)line[j])) ++j;
            if (j > i) tok.push_back(line.substr(i, j - i));
            i = j;
        }
        if (tok.empty()) continue;
        PullGroup g;
        g.name = tok[0];
        const size_t at = line.find(tok[0]);
        const bool blank_behind = at + tok[0].size() < line.size();   // (the token ended at a blank)
        if (tok[0] == "LowScore" && blank_behind) {
            g.flags = LMAT_BIN_LOWSCORE;
            g.low_score = tok.size() > 1 ? strtof(tok[1].c_str(), nullptr) : 0.0f;
        } else if (tok[0].compare(0, 12, "ReadTooShort") == 0) {
            g.name = "ReadTooShort";
        } else {
            if (tok[0] == "NoDbHits") g.flags = LMAT_BIN_NODBHITS;
            for (const std::string& t : tok) {
                uint32_t id;
                if (pull_token_id(t, id)) g.ids.push_back(id);
            }
        }
        out.push_back(std::move(g));
    }
    return true;
}

struct PullFields {
    long long tid;       // -1: none
    float score;
    long long third;     // third field of the statistics column (`valid_kmers` in the script)
    const char* type;
    bool printed;        // false: the record has no text (LMAT_ST_SILENT)
};
inline PullFields pull_fields(const lmat_params& p, int k, const lmat_read_result& r) {
    switch (r.status) {
        case LMAT_ST_SHORT_LEN: return {r.read_len, (float)k, -1, "ReadTooShort", true};
        case LMAT_ST_SHORT_VALID: return {r.valid_kmers, (float)p.min_kmer, -1, "ReadTooShort", true};
        case LMAT_ST_NODBHITS: return {r.read_len, (float)k, r.valid_kmers, "NoDbHits", true};
        case LMAT_ST_SILENT: return {-1, -1.0f, -1, "", false};
        case LMAT_ST_PHIX: return {r.call_tid, r.call_score, r.cand_kmer_cnt, "DirectMatch", true};
        default: break;
    }
    if (r.match_type == LMAT_MT_DIRECT || r.match_type == LMAT_MT_MULTI || r.match_type == LMAT_MT_PARTIAL)
        return {r.call_tid, r.call_score, r.cand_kmer_cnt, match_name(r.match_type), true};
    return {-1, -1.0f, r.cand_kmer_cnt, r.match_type == LMAT_MT_NOMATCH ? "NoMatch" : "Unmatched", true};
}

inline std::string pull_basename(const std::string& s) {
    const size_t p = s.find_last_of('/');
    return p == std::string::npos ? s : s.substr(p + 1);
}

// The pulled files of ONE .out file: <odir>/<out basename>.<idfile basename>.pulled.<group name>, all created at open.
struct PullWriter {
    std::vector<std::unique_ptr<std::ofstream>> files;
    std::vector<int> file_of;    // group -> file (groups of one name share one)
    std::string src;
    uint64_t uid = 0;            // counts the reads written, across all groups
    bool open(const std::string& odir, const std::string& out_fn, const std::string& idfile, const std::vector<PullGroup>& groups, std::string& err) {
        src = pull_basename(out_fn);
        const std::string base = odir + "/" + src + "." + pull_basename(idfile) + ".pulled.";
        std::map<std::string, int> by_name;
        for (const PullGroup& g : groups) {
            auto it = by_name.find(g.name);
            if (it == by_name.end()) {
                it = by_name.emplace(g.name, (int)files.size()).first;
                files.emplace_back(new std::ofstream(base + g.name, std::ios::binary | std::ios::trunc));
                if (!*files.back()) { err = "cannot create " + base + g.name; return false; }
            }
            file_of.push_back(it->second);
        }
        return true;
    }
    // hdr: the first column of the .out record; read: the text the record echoes (or would echo without -a)
    void put(int group, const char* hdr, size_t hdr_len, const char* read, size_t read_len, const PullFields& f) {
        std::string s;
        s.reserve(hdr_len + read_len + read_len / 80 + 160);
        s.push_back('>');
        s.append(hdr, hdr_len);
        s += ";tid=";
        put_int(s, f.tid);
        s += ";score=";
        put_float(s, f.score);
        s += ";mtype=";
        s += f.type;
        s += ";valid_kmers=";
        put_int(s, f.third);
        s += ";uid=";
        put_int(s, (long long)uid++);
        s += ";src=";
        s += src;
        s.push_back('\n');
        for (size_t i = 0; i < read_len; i += 80) {
            s.append(read + i, std::min<size_t>(80, read_len - i));
            s.push_back('\n');
        }
        files[(size_t)file_of[(size_t)group]]->write(s.data(), (std::streamsize)s.size());
    }
    bool close() {
        bool ok = true;
        for (auto& f : files) { f->close(); ok = ok && !f->fail(); }
        return ok;
    }
};

}  // namespace lmat
