/* lmat_hip.h -- C ABI of the MI355X-native read-labeling engine (liblmat_hip.so).
 *
 * The reference (LivGen/LMAT) has no plugin/FFI interface for this path; the
 * engine is a drop-in at the three seams SURVEY.md 8(b) names.  Each entry
 * point below cites the reference interface it replaces (paths relative to the
 * LMAT source tree).  Plain pointers and sizes only; every function returns 0
 * on success or a negative LMAT_E_* code and never throws; lmat_last_error()
 * gives the message.  One context per GPU; distinct contexts are independent.
 *
 * The engine has NO CPU fallback: if no HIP device is usable, lmat_ctx_create
 * fails with LMAT_E_DEVICE.
 */
#ifndef LMAT_HIP_H
#define LMAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMAT_OK 0
#define LMAT_E_ARG (-1)       /* bad argument / call order */
#define LMAT_E_IO (-2)        /* file missing or malformed */
#define LMAT_E_DEVICE (-3)    /* HIP error / no device */
#define LMAT_E_CAPACITY (-4)  /* a fixed on-device capacity was exceeded (message says which) */
#define LMAT_E_TAXONOMY (-5)  /* inconsistent taxonomy inputs */
#define LMAT_E_NOMEM (-6)
#define LMAT_E_STATE (-7)     /* the object is not in the state the call needs (lmat_export_*) */
#define LMAT_E_INTERNAL (-8)  /* the engine found its own data inconsistent (message says what) */

typedef struct lmat_ctx lmat_ctx;
typedef struct lmat_reads lmat_reads;
typedef struct lmat_ingest lmat_ingest;
typedef struct lmat_stream lmat_stream;

/* ScoreOptions + the scalar thresholds proc_line takes
 * (src/read_label.cpp:487-497, :1211-1212, getopt cases :1353-1441). */
typedef struct {
    float sdiff;        /* -b  ScoreOptions::_diff_thresh   (default 1.0) */
    float hbias;        /* -l  ScoreOptions::_diff_thresh2  (default 3.0) */
    float min_score;    /* -x  min_label_score              (default 0)   */
    int32_t min_kmer;   /* -j  min valid k-mers             (default 35)  */
    int32_t min_fnd_kmer; /* -z                             (default 1)   */
    int32_t prn_all;    /* -p  ScoreOptions::_prn_all                      */
    int32_t screen_phix; /* 1 unless -h (screenPhiXGlobal)                 */
} lmat_params;

/* What one .out record needs (src/read_label.cpp:844-848,894-937,1218,1233,1271). */
enum {
    LMAT_ST_CALL = 0,           /* stats + candidates + call line              */
    LMAT_ST_PHIX = 1,           /* PhiX short-circuit record (:841-848)        */
    LMAT_ST_SHORT_LEN = 2,      /* ri_len < k      ReadTooShort (:1217-1218)   */
    LMAT_ST_SHORT_VALID = 3,    /* valid < min     ReadTooShort (:1232-1233)   */
    LMAT_ST_NODBHITS = 4,       /* no taxid registered (:1271)                 */
    LMAT_ST_SILENT = 5          /* construct_labels returned before writing (:727-733): no record text, tallied NoDbHits */
};
enum { LMAT_MT_DIRECT = 0, LMAT_MT_MULTI = 1, LMAT_MT_PARTIAL = 2, LMAT_MT_NOMATCH = 3, LMAT_MT_LCA_ERROR = 4 };

typedef struct {
    uint8_t status;        /* LMAT_ST_*                                         */
    uint8_t match_type;    /* LMAT_MT_* (status CALL only)                      */
    uint16_t cand_kmer_cnt; /* distinct valid k-mers with first>=0              */
    int32_t valid_kmers;   /* valid k-mer positions (dups included)             */
    int32_t read_len;
    float log_avg;         /* exact float bits; host formats with %g            */
    float stdev;
    uint32_t call_tid;     /* 32-bit NCBI id (0 => printed as -1 -1)            */
    float call_score;
    uint32_t cand_off;     /* first candidate of this read in the cands array   */
    uint32_t n_cand;       /* candidates to print, best first                   */
    int32_t bin_sel;       /* GC decile (read_label.cpp:1205-1206), the null-model input: 0 unless null models are loaded */
} lmat_read_result;

typedef struct {
    uint32_t tid;
    float score;
} lmat_cand;

/* ---- context ------------------------------------------------------------ */
int lmat_device_count(void);   /* usable HIP devices (0 when there is none) */
int lmat_ctx_create(int device, const lmat_params* params, lmat_ctx** out);
void lmat_ctx_destroy(lmat_ctx* ctx);
const char* lmat_last_error(const lmat_ctx* ctx);
int lmat_set_params(lmat_ctx* ctx, const lmat_params* params);

/* ---- taxonomy + id maps ---------------------------------------------------
 * Replaces TaxTree<uint32_t>(file) + getPathToRoot (src/kmerdb/TaxTree.hpp:24-91),
 * the depth map (read_label.cpp:1574-1582), gRank_table (:1560-1567), conv_map
 * (:1585-1602) and gLowNumPlasmid (:499-510).  rank_fn / plasmid_fn may be NULL.
 * idmap_fn NULL = a database of 32-bit taxids (TID_SIZE=32 build): see lmat_ingest_idmap_from_tree. */
int lmat_taxonomy_load_files(lmat_ctx* ctx, const char* tree_fn, const char* depth_fn, const char* rank_fn,
                             const char* idmap_fn, const char* plasmid_fn);

/* ---- k-mer database --------------------------------------------------------
 * Replaces the PERM-mapped SortedDb (read_label.cpp:1477-1491; lookup contract
 * SortedDb::begin_/next, src/kmerdb/SortedDb.hpp:188,366, wrapped by
 * TaxNodeStat::begin/next/taxid/taxidCount, src/kmerdb/TaxNodeStat.hpp:60,208,258,262)
 * by an open-addressed hash in HBM.  Ingest format = make_db_table's input
 * (tax_histo binary, SortedDb::add_data src/kmerdb/SortedDb.cpp:84-751, un-pruned path).
 * table_bytes == 0 sizes the table for a 0.8 load factor.
 * n_kmers_hint or table_bytes non-zero: the table is allocated at once and the files stream through the insert
 * kernel in chunks (only the distinct lists stay on the host); then n_kmers_hint must not be below the real
 * count, the label / rand modes must be set before lmat_db_begin, and lmat_db_save_image is unavailable.
 * Both zero: the k-mers are buffered on the host until lmat_db_finalize. */
int lmat_db_begin(lmat_ctx* ctx, int k, uint64_t n_kmers_hint, uint64_t table_bytes);
int lmat_db_add_taxhisto(lmat_ctx* ctx, const char* fn);
int lmat_db_finalize(lmat_ctx* ctx);
/* make_db_table's content-changing options (src/make_db_table.cpp:150-213,303-313): build-time pruning of
 * lists longer than tid_cutoff by the rank map (-g N -m file; SortedDb.cpp:296-409), human k-mer feed (-j;
 * SortedDb.cpp:170-233,475-530,664-715), adaptor k-mer feed (-u; SortedDb.cpp:190-204,275-292).  Call between
 * lmat_db_begin and the first lmat_db_add_taxhisto; NULL / 0 disables an option. */
int lmat_db_set_build_options(lmat_ctx* ctx, int tid_cutoff, const char* rank_map_fn, const char* human_kmers_fn,
                              const char* adaptor_kmers_fn, uint32_t adaptor_tid);
/* Engine-native image of the ingested database (replaces the PERM heap image make_db_table leaves on disk,
 * src/make_db_table.cpp:330-343,429): save between begin and finalize; load + finalize to use it. */
int lmat_db_save_image(lmat_ctx* ctx, const char* fn);
int lmat_db_load_image(lmat_ctx* ctx, const char* fn, uint64_t table_bytes);
/* Two image formats, told apart by their first 8 bytes:
 *   LMATIMG1  the ingest's view (sorted k-mers + canonical 16-bit lists; what make_db_image writes without a GPU): saved between
 *             lmat_db_begin and lmat_db_finalize; loading it sizes a table and inserts every k-mer on the GPU.
 *   LMATIMG2  the DEVICE layout itself (bucket array, overflow table, list arena, geometry): lmat_db_save_image on a FINALIZED
 *             database streams it out of HBM, lmat_db_load_image streams it back in through pinned buffers -- the counterpart of
 *             the reference mapping its database file (src/read_label.cpp:1477-1491); lmat_db_finalize is then a no-op.  Its list
 *             records hold internal taxid indices built under the context's label modes: loading checks fingerprints of both
 *             (LMAT_E_TAXONOMY / LMAT_E_ARG on a mismatch).  table_bytes is ignored for it.
 *             Layout (little-endian; DESIGN.md, "The device image format"; tests/img2_model.py states it in numpy): a 4 KiB header
 *             page -- magic, version, k, the geometry of the compact table (nb, W, lowbits, m, wshift), nbuckets, ovf_nbuckets,
 *             list_shift, n_ids, n_kmers, arena_words, n_lists, the two fingerprints, offset and size of the three sections --
 *             then the bucket array, the overflow table and the list arena, each on a 4 KiB boundary, in that order.
 *             VERIFIED on load, before the context gives up anything it holds (a refused image leaves its database in place):
 *             magic and version; k; that the geometry is self-consistent (m = k - 3, lowbits, 1 <= W <= 127 >> lowbits, nb the
 *             count W implies or the fractional form, wshift the one W implies, nbuckets = min(nb, 2^32 - 1), list_shift <= 4); that
 *             the section sizes are what the counts imply and the sections are aligned, ordered and inside the file (bytes behind
 *             the arena are ignored) -- LMAT_E_IO, the message names the field; then the taxonomy fingerprint (ids, depths, flags,
 *             lineages AND the 16 -> 32 id map, through which lookups and exports translate the stored codes) with n_ids, and the
 *             fingerprint of the label modes (-s, -g / -m, rand mode, gene mode, wide taxonomy).
 *             NOT VERIFIED: the body.  Slot contents and arena records are trusted as written: a checksum would cost a pass over a
 *             file whose point is to start at link rate.
 *             A change of the layout, or of what a fingerprint covers, bumps `version`; images of another version are refused
 *             (version 1 did not cover the id map: build such a database again from its files).  LMATIMG1 is checked against its
 *             file by the ingest (dbbuild.cpp). */
/* The header checks of an LMATIMG2 file alone, without a context or a device: LMAT_OK, or LMAT_E_IO with the reason in msg (up to
 * cap bytes, NUL-terminated).  What a context adds on load are the two fingerprints and n_ids. */
int lmat_image_check(const char* fn, char* msg, uint64_t cap);
/* A replica of src's finalized database in dst (another GPU of the node, or the same one): the k-mer table, its
 * overflow table and the list arena are copied device to device (hipMemcpyPeer: over xGMI between GPUs), instead of
 * every GPU parsing the files again.  dst must hold the same taxonomy and label modes as src and no database yet. */
int lmat_db_clone(lmat_ctx* dst, lmat_ctx* src);
int lmat_db_kmer_length(const lmat_ctx* ctx);   /* SortedDb::get_kmer_length (SortedDb.hpp:433) */
uint64_t lmat_db_size(const lmat_ctx* ctx);      /* SortedDb::size (SortedDb.hpp:438)            */
uint64_t lmat_db_list_count(const lmat_ctx* ctx); /* distinct taxid-list records of a synthetic database (0: not counted) */
uint64_t lmat_db_arena_bytes(const lmat_ctx* ctx); /* size of the taxid-list arena on the device */
uint64_t lmat_db_table_bytes(const lmat_ctx* ctx);

/* TaxNodeStat-style lookup of n k-mers on the GPU: counts[i] = taxidCount (0 = miss),
 * tids[i*stride .. ] = taxid() sequence (32-bit, stored order), up to stride each. */
int lmat_db_lookup(lmat_ctx* ctx, const uint64_t* kmers, uint64_t n, uint32_t* counts, uint32_t* tids, uint32_t stride);

/* Synthetic DB generated on the device straight into the hash (bench configs;
 * SURVEY.md 8d).  Requires lmat_synth_taxonomy() first.  genome_len = bases per
 * strain genome. */
int lmat_synth_taxonomy(lmat_ctx* ctx, const uint32_t* branching6);
int lmat_synth_db_build(lmat_ctx* ctx, int k, uint64_t genome_len, uint64_t seed, uint64_t table_bytes);
/* ... with the share (in 1/1000) of every genome that is a block shared by the species of its genus (SURVEY 8d asks
 * for 10 %: lmat_synth_db_build passes 100) and the number of copies of the taxid-list records the payloads are spread
 * over (1 = every list once; more make the arena as large as a real database's, beyond the caches). */
int lmat_synth_db_build2(lmat_ctx* ctx, int k, uint64_t genome_len, uint64_t seed, uint64_t table_bytes,
                         uint32_t genus_block_permille, uint32_t list_replicas);
/* ... and with a HEAVY TAIL of taxid lists (real LMAT lists run to thousands of ids, doc/lmat-doc.txt:914-931): behind the genus
 * block three conserved blocks of conserved_permille3[0..2] thousandths of every genome, shared -- without strain substitutions --
 * by all species of a family, of a phylum, of a superkingdom: k-mers whose lists hold every strain, species and inner node of the
 * group (69 / 277 / 1109 taxids in the bench taxonomy).  {0, 0, 0} is lmat_synth_db_build2. */
int lmat_synth_db_build3(lmat_ctx* ctx, int k, uint64_t genome_len, uint64_t seed, uint64_t table_bytes,
                         uint32_t genus_block_permille, uint32_t list_replicas, const uint32_t* conserved_permille3);

/* Measurement hook: the 16 per-launch counters of the most recent launch, read after lmat_sync: [0] candidate cursor, [2] reads the
 * fast classes passed on to the E = 512 class, [3] reads that class passed on to the middle tier (T = 256), [10] reads the middle
 * tier passed on to the large LDS class (T = 1024), [7] reads that class passed on to the global-memory class. */
int lmat_debug_last_counters(lmat_ctx* ctx, uint32_t* out16);

/* Measurement hook: where the lookups of these (forward-encoded) k-mers end in the compact table -- out5[0] found in the home
 * bucket, [1] absent and the bucket never spilled (one 64-byte request in all), [2] found in the overflow table, [3] absent after
 * the overflow table was asked too, [4] overflow buckets read.  bench.py reports the share of a read sample's lookups that need
 * the second request (`overflow_probe_share`). */
int lmat_debug_probe_stats(lmat_ctx* ctx, const uint64_t* kmers, uint64_t n, uint64_t* out5);
/* Debug: the 4-instruction division the decision step on the wave uses for count / candidate-k-mers (integers below 1024,
 * read_label.cpp:821) against the IEEE division on every pair of its domain, and -- the two averages of the statistics, :806-880 --
 * on 2^26 drawn pairs (float >= 0, integer 1..64): out4 = {pairs that differ, pairs tried, drawn pairs that differ, drawn pairs tried}. */
int lmat_debug_div_check(lmat_ctx* ctx, uint64_t* out4);
/* Debug: which kernel the 160-k-mer fast class ran as -- its launches on a compact table with a 16-bit taxonomy and without -s (the
 * instantiation the plain-run variant belongs to) on the context's device since the library was loaded, out2[0] by the generic
 * kernel, out2[1] by the variant (LMAT_PLAIN=0 turns the variant off). */
int lmat_debug_variant_launches(lmat_ctx* ctx, uint64_t* out2);
/* of the launches counted in out2[1]: those that ran as the fixed-geometry variant (every read of 148 .. 151 bases at k = 20) */
int lmat_debug_uniform_launches(lmat_ctx* ctx, uint64_t* out);
/* the grid of the last launch counted in out2 (0: none yet): its wave b classified reads b, b + grid, b + 2 grid, ... of the launch */
int lmat_debug_classify_grid(lmat_ctx* ctx, uint32_t* out);

/* Test hook for the synthetic database: what it must hold for the window of `species` (0-based) that starts at base `pos` of the
 * species ancestor -- the canonical k-mer and its taxid list (the strains that carry the window unmutated; with two or more
 * owners also their species, and the genus when they span species) -- computed on the HOST from the generator's functions, never
 * read from the device table.  *n = 0: no strain kept the window.  (The table itself may hold a different list for that k-mer
 * when another window yields the same 20-mer: about 1 % of them at 6.4 G k-mers; the smaller payload wins.) */
int lmat_synth_window(lmat_ctx* ctx, uint32_t species, uint64_t pos, uint64_t* kmer, uint32_t* tids, uint32_t cap, uint32_t* n);
/* ... and for a synthetic READ: the k-mers read r of lmat_reads_synth(lengths, n_lengths, seed) must find, with their lists, derived
 * on the host from the read generator and the genome generator alone -- every window that lies in the read's strain genome
 * without a substituted base: the ancestor window's list where the strain carries it unmutated, else the strain alone.  Windows
 * with an error, random and low-complexity reads yield nothing (what the table returns for those is a chance hit).
 * kmers[cap], tids[cap][stride], counts[cap]; *n = windows written. */
int lmat_synth_read_windows(lmat_ctx* ctx, const uint32_t* lengths, uint32_t n_lengths, uint64_t seed, uint64_t r, uint64_t* kmers,
                            uint32_t* tids, uint32_t* counts, uint32_t cap, uint32_t stride, uint32_t* n, uint32_t* read_len);

/* ---- gene databases (src/gene_label.cpp) ---------------------------------------------------
 * gene_label runs the same lookup against a database whose lists are 32-bit GENE ids (INDEXDB<uint32_t>, TaxNodeStat
 * <uint32_t>, gene_label.cpp:15-22,218-267) and has no taxonomy step.  A context opened with lmat_genedb_begin (instead of a
 * taxonomy + lmat_db_begin) ingests such a database -- same tax_histo record format, ids stored as read --; then
 * lmat_db_add_taxhisto / lmat_db_finalize / lmat_db_lookup work as usual, and every classification entry point (lmat_classify,
 * lmat_stream_*) returns gene_label's vote instead of the taxonomic call (proc_line, gene_label.cpp:269-313):
 *   status LMAT_ST_CALL: call_tid = the gene std::sort(Cmp) puts first, n_cand = its vote count, cand_kmer_cnt = distinct
 *   valid k-mers of the read, call_score = n_cand / cand_kmer_cnt;  LMAT_ST_NODBHITS / LMAT_ST_SHORT_LEN: no gene (upstream
 *   prints nothing for such a read). */
int lmat_genedb_begin(lmat_ctx* ctx, int k, uint64_t n_kmers_hint, uint64_t table_bytes);

/* ---- label modes -------------------------------------------------------------------
 * -s permissive match (gPERMISSIVE_MATCH, read_label.cpp:1050-1058,1075-1102,1143) and run-time pruning of
 * lists longer than tid_cutoff (-g N [-m numeric ranks]; TaxNodeStat::begin, TaxNodeStat.hpp:76-203).  Both are
 * functions of a k-mer's taxid list alone, so they are applied when the list records are built: call before
 * lmat_db_finalize.  rank_map_fn may be NULL (then only the first stored taxid survives, as upstream). */
int lmat_set_label_modes(lmat_ctx* ctx, int permissive, int tid_cutoff, const char* rank_map_fn);

/* ---- null models (-n) -----------------------------------------------------------
 * Replaces loadRandHits (read_label.cpp:512-678) and switches scoring to log(label_prob / null_prob)
 * (construct_labels :735-819, log_odds_score :680-690).  list_fn holds `<kmer_count> <gz file relative to
 * $LMAT_DIR>` lines.  A taxid met during classification without a null-model entry is an error
 * (LMAT_E_TAXONOMY), as upstream's assert is. */
int lmat_nullmodel_load(lmat_ctx* ctx, const char* list_fn);
int lmat_nullmodel_clear(lmat_ctx* ctx);

/* ---- reads ----------------------------------------------------------------
 * A batch of reads packed on the device (2-bit bases + validity bits).
 * Replaces the (read,hdr) queue hand-off of main() (read_label.cpp:1716-1746):
 * bases = concatenated ASCII, off[n+1] byte offsets. */
int lmat_reads_upload(lmat_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint64_t n, lmat_reads** out);
/* Paired-end reads: read i of the result is mate i of bases1/off1, an 'N', mate i of bases2/off2 -- the record upstream's
 * bin/merge_fastq_reads_with_N_separator.pl makes on disk -- joined on the device while the reads are packed.  An ordinary
 * lmat_reads of n_pairs reads in every respect (classify, download: the image of a pair is mate1 N mate2).  Either mate
 * may be empty; offsets need not start at 0. */
int lmat_reads_upload_pairs(lmat_ctx* ctx, const uint8_t* bases1, const uint64_t* off1, const uint8_t* bases2,
                            const uint64_t* off2, uint64_t n_pairs, lmat_reads** out);
int lmat_reads_synth(lmat_ctx* ctx, uint64_t n, const uint32_t* lengths, uint32_t n_lengths, uint64_t seed,
                     lmat_reads** out);
int lmat_reads_download_ascii(lmat_ctx* ctx, const lmat_reads* r, uint64_t first, uint64_t count, uint8_t* bases,
                              uint64_t* off);
/* Test hook: the packed records of reads first .. first + count as they lie on the device -- rec_off[count + 1] word
 * offsets counted from the first of them, and (words != NULL) those rec_off[count] words.  A plain device-to-host copy. */
int lmat_debug_reads_words(lmat_ctx* ctx, const lmat_reads* reads, uint64_t first, uint64_t count, uint32_t* words,
                           uint64_t* rec_off);
uint64_t lmat_reads_count(const lmat_reads* r);
uint64_t lmat_reads_device_bytes(const lmat_reads* r);
void lmat_reads_free(lmat_ctx* ctx, lmat_reads* r);

/* ---- classification --------------------------------------------------------
 * Replaces proc_line (read_label.cpp:1211-1279) for reads [first, first+count).
 * results[count]; cands/cand_cap may be NULL/0 for calls-only output; *n_cands
 * receives the number of candidate pairs written.  Per-taxid tallies
 * (read_label.cpp:1241-1276) accumulate in the context until lmat_counts_reset; a call that fails (e.g.
 * LMAT_E_CAPACITY because cand_cap was too small) leaves them as they were, so it can simply be retried. */
int lmat_classify(lmat_ctx* ctx, const lmat_reads* reads, uint64_t first, uint64_t count, lmat_read_result* results,
                  lmat_cand* cands, uint64_t cand_cap, uint64_t* n_cands);

/* Same kernels, results left in device memory (throughput runs).  Asynchronous on
 * the context's stream; lmat_sync waits and reports an error raised by ANY launch since the last report
 * (device-side error flags are sticky until reported).  kernel_ms_total (may be NULL) = HIP-event time of
 * all kernels of those launches; lmat_last_timing splits it per kernel.  The device-side result
 * buffer holds the records of the most recent launch only (lmat_results_fetch reads those); the
 * tallies accumulate over all launches. */
int lmat_classify_async(lmat_ctx* ctx, const lmat_reads* reads, uint64_t first, uint64_t count);
/* The same with the candidate pairs of `-p` (read_label.cpp:898-910; bin/run_rl.sh:243 always passes -p) written to a
 * device-side buffer of cand_cap pairs (grown on demand, one per set of in-flight buffers); lmat_read_result.cand_off /
 * n_cand index it.  cand_cap = 0: calls only, as lmat_classify_async.  A buffer that proves too small raises
 * LMAT_E_CAPACITY at the next lmat_sync. */
int lmat_classify_async_cands(lmat_ctx* ctx, const lmat_reads* reads, uint64_t first, uint64_t count, uint64_t cand_cap);
int lmat_sync(lmat_ctx* ctx, float* kernel_ms_total, uint64_t* kernel_launches);
/* HIP-event times accumulated by the launches the last lmat_sync waited for, split per kernel:
 * classify_ms = classify_kernel (extract + probe + registration/closure, the HBM-bound kernel),
 * decide_ms = the K4 kernels (score + LCA decision) + the larger-class re-runs. */
int lmat_last_timing(const lmat_ctx* ctx, float* classify_ms, float* decide_ms, uint64_t* launches);
int lmat_results_fetch(lmat_ctx* ctx, uint64_t first, uint64_t count, lmat_read_result* results);

/* ---- streamed boundary -------------------------------------------------------
 * Replaces the reader thread + (read, hdr) queue of main() (src/read_label.cpp:1651-1746): a ring of n_slots batch slots
 * whose pinned host buffers and device buffers are allocated once.  Host-to-device copy, packing + classification and
 * the copy of the results back overlap across consecutive batches; nothing is allocated per batch.
 *   acquire  -> pointers to the next slot's pinned input buffers: bases (concatenated ASCII, up to max_bases) and
 *               off[n + 1] byte offsets; the caller fills them (LMAT_E_ARG when every slot is in use)
 *   submit   -> queues the slot: n reads, an opaque tag that comes back with the results; asynchronous
 *   next     -> waits for the OLDEST submitted batch; pointers into its pinned result buffers (cands in the order of
 *               lmat_read_result.cand_off), valid until lmat_stream_release; returns 1 when nothing is in flight
 *   release  -> the batch handed out by lmat_stream_next is consumed, its slot is free again
 * cands_per_read = 0: calls only; otherwise the slot holds cands_per_read x max_reads + 1024 x 2048 candidate pairs and
 * grows itself when a batch needs more: fourfold, running the batch again inside lmat_stream_next without tallying it
 * again.  Tallies accumulate in the context as with lmat_classify.  One thread drives a stream. */
int lmat_stream_create(lmat_ctx* ctx, uint64_t max_reads, uint64_t max_bases, uint32_t cands_per_read, int n_slots,
                       lmat_stream** out);
int lmat_stream_acquire(lmat_stream* st, uint8_t** bases, uint64_t** off);
int lmat_stream_submit(lmat_stream* st, uint64_t n_reads, uint64_t tag);
/* As lmat_stream_submit, but the reads are off[0..n_reads] inside the caller's OWN pinned buffer `bases` (from
 * lmat_host_alloc; off need not start at 0), which the device reads directly: no copy into the slot.  The buffer must
 * stay untouched until lmat_stream_next has returned this batch. */
int lmat_stream_submit_from(lmat_stream* st, const uint8_t* bases, const uint64_t* off, uint64_t n_reads, uint64_t tag);
/* Paired-end batches (joined on the device as by lmat_reads_upload_pairs).  A batch of n_pairs gives n_pairs results whose
 * read_len is l1 + 1 + l2.  It counts 2 x n_pairs reads against max_reads and sum(l1 + l2) + n_pairs bases against
 * max_bases (LMAT_E_ARG above either, the slot goes back untouched); a joined length above what one read may have is
 * refused like a read of that length.
 *   submit_pairs       the acquired slot holds 2 x n_pairs reads, mates 1 and 2 in turn, under off[2 x n_pairs + 1]
 *   submit_pairs_from  mates 1 are off1[0..n_pairs] inside the caller's own pinned buffer bases1, mates 2 off2[0..n_pairs]
 *                      inside bases2 (one buffer or two), with the rules of lmat_stream_submit_from */
int lmat_stream_submit_pairs(lmat_stream* st, uint64_t n_pairs, uint64_t tag);
int lmat_stream_submit_pairs_from(lmat_stream* st, const uint8_t* bases1, const uint64_t* off1, const uint8_t* bases2,
                                  const uint64_t* off2, uint64_t n_pairs, uint64_t tag);
/* Page-locked host memory for buffers handed to lmat_stream_submit_from / lmat_stream_submit_pairs_from. */
int lmat_host_alloc(uint64_t bytes, void** out);
void lmat_host_free(void* p);
int lmat_stream_next(lmat_stream* st, const lmat_read_result** results, const lmat_cand** cands, uint64_t* n_reads,
                     uint64_t* n_cands, uint64_t* tag);
/* Also drops a batch whose error lmat_stream_next has just reported (the error comes back for as long as the batch is
 * asked for; the batches queued behind it are untouched and come next). */
int lmat_stream_release(lmat_stream* st);
void lmat_stream_destroy(lmat_stream* st);
/* Test hook, host bookkeeping only (no kernel, no copy): out6[0] queued submits whose offsets were made on the device
 * (reads of one length, off[0] == 0), [1] queued submits whose offsets were copied in, [2] submits partitioned on more
 * than one host thread, [3] submits whose length-class lists were sent (more than one class in use), [4] grow re-runs
 * so far (a slot whose batch printed more pairs than it holds grows fourfold and runs the batch again), [5] the largest
 * candidate capacity among the slots, in pairs (at creation cands_per_read x max_reads + 1024 x 2048 each: the second
 * term is what the sub-cursors may leave unused). */
int lmat_debug_stream_stats(const lmat_stream* st, uint64_t* out6);

/* ---- tallies (merge step read_label.cpp:1760-1800) --------------------------
 * Dense arrays indexed by the engine's internal taxid index; n_ids = number of
 * internal ids + 1.  counts_device_ptr exposes the device buffer
 * [u64 count[n_ids] | f64 score[n_ids] | u64 nomatch[3]] for an RCCL all-reduce
 * done by the caller (one process per GPU). */
int lmat_counts_reset(lmat_ctx* ctx);
int lmat_counts_layout(const lmat_ctx* ctx, uint32_t* n_ids, uint64_t* bytes);
void* lmat_counts_device_ptr(lmat_ctx* ctx);
int lmat_counts_get(lmat_ctx* ctx, uint32_t* tid32, uint64_t* count, double* score, uint32_t cap, uint32_t* n_nonzero,
                    uint64_t nomatch3[3]);
/* The same merge across the contexts of ONE process (one per GPU, read_label -t N on an N-GPU node): afterwards every
 * context holds the sum of all.  Contexts on distinct devices: RCCL over xGMI (ncclCommInitAll over their devices, kept
 * for the next call, + one grouped ncclAllReduce per array on each context's stream).  Contexts that share a device
 * cannot be ranks of one communicator: those are summed through the host. */
int lmat_counts_allreduce(lmat_ctx** ctxs, int n_ctx);

/* ... and across PROCESSES, one context (= one GPU) per rank, whatever launched them: rank 0 makes an id
 * (ncclGetUniqueId), the launcher's own channel hands its LMAT_COMM_ID_BYTES bytes to the other ranks, every rank calls
 * lmat_comm_init (ncclCommInitRank; collective), then lmat_comm_allreduce_counts sums the tallies in place on all ranks
 * (ncclAllReduce on the context's stream, u64 counts / f64 score sums / u64 nomatch; returns when it is complete).
 * librccl is opened on first use of these entry points, never by a one-GPU run. */
#define LMAT_COMM_ID_BYTES 128
/* 1 when librccl and every entry point the engine uses could be loaded in this process (a pre-flight every rank runs BEFORE
 * any rank enters lmat_comm_init, so that a rank without the library cannot leave the others waiting inside it), else 0. */
int lmat_comm_available(void);
int lmat_comm_unique_id(uint8_t* id /* [LMAT_COMM_ID_BYTES] */);
int lmat_comm_init(lmat_ctx* ctx, const uint8_t* id, int n_ranks, int rank);
int lmat_comm_allreduce_counts(lmat_ctx* ctx);
int lmat_comm_size(const lmat_ctx* ctx);   /* ranks of the communicator, 0 = none */
void lmat_comm_destroy(lmat_ctx* ctx);

/* ---- rand_read_label: the null-model generator (src/rand_read_label.cpp) on the same kernels -----------
 * Replaces its proc_line/construct_labels (:185-213, :372-398) over src/rkmer.hpp's retrieve_kmer_labels, which is
 * read_label's without the human folding.  Per (taxid, GC bucket): the largest fraction label_prob =
 * count / valid_kmers over the reads given, and the number of reads that hit the taxid -- the two columns of
 * the .rand_lst file (:741-754).  lmat_rand_mode(ctx, 1) before lmat_db_finalize; lmat_rand_reset sizes and
 * clears the tables; lmat_rand_label adds a range of reads, gc_bucket[i] (host) being the bucket of read
 * first + i; lmat_rand_get returns the rows with any hit, ascending taxid, row-major [n_rows][n_buckets]
 * (call with cap 0 for the row count). */
int lmat_rand_mode(lmat_ctx* ctx, int on);
int lmat_rand_reset(lmat_ctx* ctx, uint32_t n_buckets);
int lmat_rand_label(lmat_ctx* ctx, const lmat_reads* reads, uint64_t first, uint64_t count, const uint8_t* gc_bucket);
int lmat_rand_get(lmat_ctx* ctx, uint32_t* tid32, float* max_prob, uint32_t* count, uint32_t cap, uint32_t* n_rows);

/* ---- GPU-free ingest (the make_db_image tool; also usable without any device) ----------------------
 * Same parsing and options as above, producing the canonical (k-mer, 16-bit taxid list) form;
 * lmat_ingest_lookup returns the stored list of one k-mer (16-bit DB ids, stored order; 0 = absent). */
int lmat_ingest_create(int k, const char* idmap_fn, lmat_ingest** out);   /* idmap_fn NULL: call lmat_ingest_idmap_from_tree */
/* A database of 32-bit taxids (the reference's TID_SIZE=32 build, CMakeLists.txt:92-105; make_db_table without -f):
 * the storage code of a taxid is its rank among the taxonomy tree's node ids (at most 65534 nodes).
 * lmat_taxonomy_load_files with idmap_fn NULL derives the same codes. */
int lmat_ingest_idmap_from_tree(lmat_ingest* ing, const char* tree_fn);
void lmat_ingest_destroy(lmat_ingest* ing);
const char* lmat_ingest_error(const lmat_ingest* ing);
int lmat_ingest_set_options(lmat_ingest* ing, int tid_cutoff, const char* rank_map_fn, const char* human_kmers_fn,
                            const char* adaptor_kmers_fn, uint32_t adaptor_tid);
int lmat_ingest_add_taxhisto(lmat_ingest* ing, const char* fn);
int lmat_ingest_save_image(const lmat_ingest* ing, const char* fn);
int lmat_ingest_load_image(const char* fn, lmat_ingest** out);
uint64_t lmat_ingest_size(const lmat_ingest* ing);
int lmat_ingest_kmer_length(const lmat_ingest* ing);
int lmat_ingest_lookup(const lmat_ingest* ing, uint64_t kmer, uint16_t* tids16, int cap);
int lmat_db_from_ingest(lmat_ctx* ctx, lmat_ingest* ing, uint64_t table_bytes);

/* ---- the database from genome FASTA (lmat_amd/csrc/dbgen.hip) ------------------------------------
 * Replaces the reference's two offline CPU programs: kmerPrefixCounter (src/kmerPrefixCounter.cpp:114-147: genome FASTA ->
 * canonical k-mers with the ids of the genomes that hold them) and tax_histo (src/tax_histo.cpp:210-284, TaxTree::getLcaMap
 * src/kmerdb/TaxTree.hpp:160-260: per k-mer the owners the tree knows plus every node on their paths up to and including
 * their lowest common ancestor).  The result is the tax_histo binary lmat_db_add_taxhisto reads, records in ascending k-mer
 * order, every list in ASCENDING TAXID order (the reference writes unordered_map iteration order).
 *   input    FASTA records headed ">" + decimal taxid; a sequence may span lines; records of one taxid are one owner.  Every
 *            window of k consecutive ACGTacgt gives min(forward, reverse complement); any other byte breaks the run.
 *   memory   everything on the device is sized by device_budget_bytes (0: half of the free memory); the k-mer space is cut into
 *            2^prefix_bits passes by the top bits of the canonical k-mer (the reference's -l / -f), derived from the budget and
 *            the base count unless given; the genome text is uploaded in chunks of chunk_bases (0: 16 Mi) with an overlap.
 *   errors   a list of more than 65535 taxids is LMAT_E_CAPACITY (the reference truncates the 16-bit count silently); a pass
 *            that does not fit a forced prefix_bits is LMAT_E_CAPACITY; nothing is ever cut short.
 *   deviation: owners that are the root or a child of the root are treated like any other (the reference, built without
 *            NDEBUG, asserts on them, TaxTree.hpp:204). */
typedef struct lmat_build lmat_build;
typedef struct {
    uint64_t bases;               /* sequence bytes given                                                   */
    uint64_t windows;             /* windows of k valid bases                                               */
    uint64_t emitted_pairs;       /* (k-mer, owner) pairs the extraction emitted over all passes            */
    uint64_t distinct_kmers;
    uint64_t records_written;     /* distinct k-mers with at least one owner in the tree                    */
    uint64_t dropped_unknown;     /* distinct k-mers none of whose owners is in the tree: no record         */
    uint64_t singletons;          /* records whose list is one taxid                                        */
    uint64_t total_list_entries;
    uint64_t longest_list;
    uint32_t passes;
    uint32_t prefix_bits;
    float extract_ms, sort_ms, segment_ms, closure_ms;   /* HIP-event time per stage, summed over the passes */
} lmat_build_stats;
int lmat_build_create(lmat_ctx* ctx, int k, const char* tree_fn, lmat_build** out);
void lmat_build_destroy(lmat_build* b);
const char* lmat_build_error(const lmat_build* b);
int lmat_build_set_options(lmat_build* b, uint64_t device_budget_bytes, int prefix_bits /* -1: derive */, uint32_t chunk_bases /* 0: default */);
int lmat_build_add_fasta(lmat_build* b, const char* fn);
int lmat_build_add_sequence(lmat_build* b, uint32_t taxid, const uint8_t* ascii, uint64_t n);
int lmat_build_run(lmat_build* b, lmat_build_stats* out);
int lmat_build_write_taxhisto(lmat_build* b, const char* fn);
/* Records [first, first + count) of the result: kmers[count], list_off[count + 1] (relative to the first record's list),
 * tids[up to tid_cap] (LMAT_E_CAPACITY when the range holds more).  Any of the three may be NULL. */
int lmat_build_fetch(lmat_build* b, uint64_t first, uint64_t count, uint64_t* kmers, uint64_t* list_off, uint32_t* tids, uint64_t tid_cap);
/* The classify table straight from the result, without a file: needs a context with a taxonomy loaded; ends in the table
 * lmat_db_begin / lmat_db_add_taxhisto / lmat_db_finalize build from the written file (the records go through the same parser). */
int lmat_db_build_from_genomes(lmat_ctx* ctx, lmat_build* b, uint64_t table_bytes);

/* ---- adding genomes to an existing database: tax_histo files as further inputs of a build ----
 * lmat_build_add_taxhisto (any number, before lmat_build_run) makes an existing tax_histo file an input beside, or instead of,
 * sequence.  lmat_build_run then produces the merge of the files and -- if any sequence was added -- of what the genomes alone
 * would give; records in ascending k-mer order, lists in ascending taxid order, through lmat_build_write_taxhisto,
 * lmat_build_fetch and lmat_db_build_from_genomes as before.  Per k-mer, with X the union of the entries of every source
 * that holds it:
 *   one source                  its list, ascending.  The list is COPIED, NOT RE-CLOSED: inputs are taken to be closed lists, as
 *                               tax_histo and this builder write them
 *   several sources, |X| = 1    that taxid
 *   otherwise                   X plus every node on the path from each source's shallowest entry up to and including the LCA
 *                               of those shallowest entries, every taxid once (for closed lists this is the closure of the
 *                               union of the original owners; the engine computes it as the closure of X taken as owners)
 * Lists of an input may be in any order and of any length the format holds; the output bytes do not depend on prefix_bits, the
 * budget or the order in which inputs were added.  The merge runs inside the prefix passes: a pass takes the contiguous slice
 * of every input with its prefix; device_budget_bytes bounds it and the derived prefix_bits accounts for the inputs' record and
 * entry counts (72 bytes per record, 12 per entry of the largest slice); a forced prefix_bits that does not fit is
 * LMAT_E_CAPACITY.  The files themselves are parsed when they are added and held on the host until the builder is destroyed.
 *   errors   (the message names the file)  header k differs from the builder's: LMAT_E_ARG.  Malformed or truncated file, bad
 *            sanity word, k-mer wider than 2k bits, k-mers not strictly ascending, bytes behind the last record, A TAXID
 *            REPEATED INSIDE ONE LIST: LMAT_E_IO.  A taxid the builder's tree does not know: LMAT_E_TAXONOMY, naming it.  A
 *            merged list of more than 65535 entries: LMAT_E_CAPACITY (from lmat_build_run).  A record with an empty list
 *            carries nothing and is skipped.  A file that fails is not added; the builder stays usable.
 *   stats    lmat_build_stats keeps its layout: with tax_histo inputs records_written, singletons, total_list_entries and
 *            longest_list describe the final result, bases / windows / emitted_pairs / distinct_kmers / dropped_unknown the
 *            genome part only; without inputs every field is what it was. */
typedef struct {
    uint32_t inputs;               /* tax_histo files added                                                     */
    uint32_t passes;
    uint64_t records_in;           /* records with a list, over all files                                       */
    uint64_t entries_in;           /* their list entries                                                        */
    uint64_t records_one_source;   /* result records whose k-mer one source held (a file, or the genomes)       */
    uint64_t records_merged;       /* ... two or more sources held                                              */
    uint64_t records_grown;        /* merged records whose list holds a node that no source list held           */
    float upload_ms, sort_ms, segment_ms, union_ms, histogram_ms;   /* HIP-event time per merge stage, summed over the passes */
} lmat_merge_stats;
int lmat_build_add_taxhisto(lmat_build* b, const char* fn);
int lmat_build_merge_stats(const lmat_build* b, lmat_merge_stats* out);   /* after lmat_build_run; all zero without tax_histo inputs */
/* After lmat_build_run, with or without tax_histo inputs: for every taxid that occurs, the number of result records whose list
 * holds it, ascending by taxid (the map of the reference's countTaxidFrequency, src/countTaxidFrequency.cpp:105-139), counted
 * on the device.  *n is the number of such taxids, set even when cap is too small (LMAT_E_CAPACITY): a cap of 0 asks for it. */
int lmat_build_taxid_counts(lmat_build* b, uint32_t* tids, uint64_t* counts, uint64_t cap, uint64_t* n);

/* ---- a loaded database back out as tax_histo records ----
 * The way out of the k-mer table: every k-mer the finalized database of ctx holds, ascending, each with its taxid list AS STORED
 * (the order and the 32-bit ids of the tax_histo record it came from, whatever label modes shaped the list records) -- from a table
 * built from files, from either image format, from genomes or from a merge.  What make_db_table's options did to the content
 * (pruned lists, human / adaptor k-mers) is part of the database and therefore of the export.
 *   lmat_export_set_options  device_budget_bytes 0: half of the free device memory; prefix_bits -1: the smallest split of the k-mer
 *                            space (by the top bits of the k-mer) whose pass fits the budget, else 0 .. min(2k, 24)
 *   lmat_export_run          taxhisto_fn: the file lmat_db_add_taxhisto reads (header count = lmat_db_size), streamed pass by pass;
 *                            NULL: the records stay in host memory for lmat_export_fetch; "": they are dropped (counts only).  Always the per-taxid counts
 *                            (frequency_counter, src/frequency_counter.cpp:86-144) are kept for lmat_export_taxid_counts.
 *   lmat_export_fetch        as lmat_build_fetch;  lmat_export_taxid_counts  as lmat_build_taxid_counts (lists that hold the taxid)
 *   errors   no finalized database, a fetch before a run or after a run to a file: LMAT_E_STATE.  A synthetic database
 *            (lmat_synth_db_build*): LMAT_E_STATE.  A pass that does not fit the budget under a forced prefix_bits, or under the
 *            finest split: LMAT_E_CAPACITY.  The table holds a k-mer twice, or the records written differ from lmat_db_size:
 *            LMAT_E_INTERNAL.  A failed run leaves no file behind. */
typedef struct lmat_export lmat_export;
typedef struct {
    uint64_t records, entries, singletons;   /* records written, their list entries (Total-tid), lists of one entry */
    uint64_t from_buckets, from_overflow;    /* records read from the compact buckets | from 8 x u64 slot buckets (overflow table, wide layout) */
    uint64_t passes;
    int prefix_bits;
    double ms_scan, ms_sort, ms_lists, ms_fetch, ms_write;   /* HIP-event time of the device stages; host time of the fetch and the file */
} lmat_export_stats;
int lmat_export_create(lmat_ctx* ctx, lmat_export** out);          /* ctx holds a finalized database */
void lmat_export_destroy(lmat_export* e);
const char* lmat_export_error(const lmat_export* e);
int lmat_export_set_options(lmat_export* e, uint64_t device_budget_bytes, int prefix_bits /* -1: derive */);
int lmat_export_run(lmat_export* e, const char* taxhisto_fn /* NULL: keep the result in host memory */, lmat_export_stats* out);
int lmat_export_fetch(lmat_export* e, uint64_t first, uint64_t count, uint64_t* kmers, uint64_t* list_off, uint32_t* tids, uint64_t tid_cap);
int lmat_export_taxid_counts(lmat_export* e, uint32_t* tids, uint64_t* counts, uint64_t cap, uint64_t* n);

/* ---- a taxonomic slice of the export: a filter on the device, ahead of the fetch ----
 * A filter is a property of an lmat_export, set before lmat_export_run; a k-mer is kept iff ALL enabled tests pass.
 *   where it looks   the list AS STORED: the ids, in the order, that the unfiltered export writes.  Label modes do not change it.
 *   S                the nodes `taxa` of ctx's tree and all their descendants.  Taxa may repeat or nest (the intervals are merged).
 *   depth            the number of proper ancestors in ctx's tree (root = 0), not the -e file's value; for a closed list
 *                    min_lca_depth therefore tests the depth of the list's LCA.
 *   unknown ids      an entry the context's taxonomy does not hold (conv[code] == 0 included) is OUTSIDE S and has DEPTH 0.
 *   what is kept     ascending by k-mer and otherwise unchanged; the sanity word follows every 1500th KEPT record, counted across
 *                    passes; the header count is the number kept (written first, patched after the last pass: 8 bytes at offset 4).
 *                    lmat_export_stats keeps its layout: records / entries / singletons, lmat_export_fetch and
 *                    lmat_export_taxid_counts describe the kept records.  The "records differ from lmat_db_size" check
 *                    (LMAT_E_INTERNAL) applies to the records SCANNED.
 *   stats            out6 = scanned, kept, dropped by the taxon test, dropped by depth, dropped by length, long lists (more than 8
 *                    entries) judged by a whole wave; a record failing several tests is charged to the first in that order.
 *                    ms_select: HIP-event time of the filter stage (0 without a filter).  Before a run: LMAT_E_STATE.
 *   no filter        (never set, NULL, or one that enables no test) the run is the unfiltered run: launches, budget model, bytes.
 *   memory           with a filter a pass takes 48 device bytes per scanned pair instead of 40 (keep flag and position), and the
 *                    run 4 bytes per taxonomy node times three plus 256 KiB for the per-entry facts.
 *   errors           a taxid the tree does not hold: LMAT_E_TAXONOMY.  mode != 0 with n_taxa == 0, mode == 0 with n_taxa != 0, a
 *                    mode outside 0..3, taxa == NULL with n_taxa != 0: LMAT_E_ARG.  Any filter on a gene database: LMAT_E_ARG.
 * lmat_db_from_export runs e (with its filter, into host memory) and hands the records to dst's ingest through the in-memory
 * stream lmat_db_build_from_genomes uses, k taken from the source: dst ends up holding the slice as a finalized database.
 * dst without a taxonomy: LMAT_E_STATE; dst == e's context, a gene source, an empty slice: LMAT_E_ARG; the text is
 * lmat_export_error(e)'s. */
#define LMAT_SLICE_ANY  1   /* keep a k-mer iff at least one list entry lies in S            */
#define LMAT_SLICE_ALL  2   /* ... iff every list entry lies in S (clade-specific k-mers)    */
#define LMAT_SLICE_NONE 3   /* ... iff no list entry lies in S (e.g. S = {9606}: host-free)  */
typedef struct {
    const uint32_t* taxa; uint32_t n_taxa;  /* S = these nodes of ctx's tree and all their descendants */
    int mode;                               /* 0: no taxon test (then n_taxa must be 0)                 */
    uint32_t min_lca_depth;                 /* 0: off.  keep iff every entry has tree depth >= this     */
    uint32_t max_entries;                   /* 0: off.  keep iff the stored list has at most this many  */
} lmat_export_filter;
int lmat_export_set_filter(lmat_export* e, const lmat_export_filter* f /* NULL: clear */);
int lmat_export_filter_stats(const lmat_export* e, uint64_t out6[6], double* ms_select);
int lmat_db_from_export(lmat_ctx* dst, lmat_export* e, uint64_t table_bytes);

/* A loaded database as one more input of a merge (beside lmat_build_add_taxhisto): src is exported into host memory at the time of
 * the call and its records take the path a parsed file takes.  k must match (LMAT_E_ARG); a gene database is LMAT_E_ARG. */
int lmat_build_add_db(lmat_build* b, lmat_ctx* src);

/* ---- gene databases from gene FASTA: the id-set mode of the builder ----
 * What a gene database is, is what kmerPrefixCounter computes before tax_histo touches it (hash[kmer].insert(gid),
 * src/kmerPrefixCounter.cpp:114-147): per canonical k-mer the set of ids of the records that hold it.  lmat_genebuild_create
 * returns an lmat_build WITHOUT A TAXONOMY; every lmat_build_* entry point works on it, and the file it writes is the one
 * lmat_genedb_begin + lmat_db_add_taxhisto read (gene_label -d).
 *   result   for every canonical k-mer of the inputs the ids of the records that contain it, every id once, in ASCENDING NUMERIC
 *            order; records in ascending k-mer order.  No closure, nothing is looked up anywhere.
 *   input    FASTA as lmat_build_add_fasta reads it (">" + decimal id) or lmat_build_add_sequence.  Ids are 1 .. 2^32-1: a header
 *            of 0 (the result records' "no gene") or of a value beyond 32 bits is LMAT_E_IO naming the line, and the file adds
 *            nothing; lmat_build_add_sequence with id 0 is LMAT_E_ARG.  Records of one id are one owner.  A record shorter than
 *            k, an empty one and one without a valid base contribute nothing and are no errors.
 *   merge    lmat_build_add_taxhisto takes tax_histo-format files of gene ids (a fixture, an earlier output, an export): per
 *            k-mer the result is the union of the ids of every source that holds it, ascending -- so a one-source list is that
 *            list SORTED.  An id repeated inside one list and an id 0 are LMAT_E_IO; the other file checks are those of section
 *            10.  lmat_build_add_db takes a gene context (lmat_genedb_begin); a taxonomy context is LMAT_E_ARG, as a gene context
 *            stays for a tree-mode builder.  The inputs' entries of a prefix pass are (k-mer, owner) pairs beside the extracted
 *            ones; the derived prefix_bits accounts for them, a forced one that does not hold them is LMAT_E_CAPACITY.  Output
 *            bytes do not depend on prefix_bits, the budget, chunk_bases or the order in which inputs were added.
 *   errors   a list of more than 65535 ids: LMAT_E_CAPACITY from lmat_build_run, never cut short.
 *   stats    lmat_build_stats keeps its layout: dropped_unknown is 0, closure_ms holds the list stage, distinct_kmers counts the
 *            result's k-mers (inputs included).  lmat_merge_stats: a source is a file or the text; records_grown is 0 and only
 *            upload_ms is filled (the inputs ride in the build's own sort).  lmat_build_taxid_counts gives, per id, the number
 *            of result records whose list holds it: the gene's k-mer count.
 * lmat_genedb_build_from_genes is the counterpart of lmat_db_build_from_genomes: ctx is a fresh context (no taxonomy needed) and
 * ends holding the table lmat_genedb_begin / lmat_db_add_taxhisto / lmat_db_finalize build from the written file.  A tree-mode
 * builder passed to it, or an id-set builder passed to lmat_db_build_from_genomes, is LMAT_E_ARG. */
int lmat_genebuild_create(lmat_ctx* ctx, int k, lmat_build** out);
int lmat_genedb_build_from_genes(lmat_ctx* ctx, lmat_build* b, uint64_t table_bytes);

/* ---- per-group k-mer coverage of a set of reads (content_summ's counting, src/content_summ.cpp:113-152, 538-571) ----
 * Input: reads (ASCII, any length, 0 included) with a caller-chosen 32-bit group id each -- content_summ uses the taxid it counts
 * the read under -- and a list of k sizes in 1..31 (duplicates allowed, reported per index).
 * Per read and k: every window of k consecutive ACGTacgt bytes gives min(forward, reverse complement) over A=0 C=1 G=2 T=3; any
 * other byte and a read boundary break the run; the SET of distinct canonical k-mers of the read is what counts.
 * Per group and k: the multiplicity of a k-mer is the number of reads of the group whose set holds it; reported are `distinct`
 * (number of k-mers), `total` (sum of multiplicities) and the histogram multiplicity -> number of k-mers.  Groups without a
 * k-mer for a k are absent from that k's report.  The result is a function of the multiset of (group, read): not of the order
 * or batching of lmat_cov_add_reads, the budget or the pass split.
 *   lmat_cov_set_options   device_budget_bytes 0: half of the free device memory; prefix_bits -1: derived per k, else every k's
 *                          k-mer space is cut into 2^min(prefix_bits, 2k) passes by the top bits of the canonical k-mer
 *   lmat_cov_add_reads     read i = ascii[off[i] .. off[i+1]); a failed call adds nothing
 *   lmat_cov_run           once per object; without reads LMAT_OK and empty reports
 *   lmat_cov_summary       ascending by group id;  lmat_cov_histogram  ascending by multiplicity.  Both set *n even when cap is
 *                          too small (LMAT_E_CAPACITY): a cap of 0 asks for the size.  A group the summary does not list gives
 *                          *n = 0 and LMAT_OK from lmat_cov_histogram.
 *   errors   a k outside 1..31, n_k < 1, a NULL array with n_reads > 0, an off that does not ascend, a fetch before the run, a
 *            second run: LMAT_E_ARG.  More than 2^32 - 1 reads: LMAT_E_CAPACITY.  A pass that does not fit the budget under a
 *            forced prefix_bits, or under the finest derived split: LMAT_E_CAPACITY; nothing is ever cut short. */
typedef struct lmat_cov lmat_cov;
typedef struct {
    uint64_t reads, bases;
    uint64_t windows;        /* valid windows, summed over k */
    uint64_t runs;           /* distinct (group, k-mer), summed over k */
    uint32_t passes;         /* summed over k */
    uint32_t prefix_bits;    /* the finest split any k ran under */
    float extract_ms, sort_ms, segment_ms, histogram_ms;
} lmat_cov_stats;
int lmat_cov_create(lmat_ctx* ctx, const int* k_sizes, int n_k, lmat_cov** out);      /* no taxonomy or database needed */
void lmat_cov_destroy(lmat_cov* c);
const char* lmat_cov_error(const lmat_cov* c);
int lmat_cov_set_options(lmat_cov* c, uint64_t device_budget_bytes /* 0: half of free */, int prefix_bits /* -1: derive */);
int lmat_cov_add_reads(lmat_cov* c, const uint8_t* ascii, const uint64_t* off /* n+1 */, uint64_t n_reads, const uint32_t* group);
int lmat_cov_run(lmat_cov* c, lmat_cov_stats* out);
int lmat_cov_summary(lmat_cov* c, int k_index, uint32_t* groups, uint64_t* distinct, uint64_t* total, uint64_t cap, uint64_t* n);
int lmat_cov_histogram(lmat_cov* c, int k_index, uint32_t group, uint64_t* multiplicity, uint64_t* n_kmers, uint64_t cap, uint64_t* n);

/* ---- reads pulled by called taxon (bin/pull_reads.pl behind bin/pull_reads_mc.sh; lmat_amd/csrc/bins.hip) ----
 * Selects, on the device, the reads of a classified batch that belong to GROUPS of taxids and hands back, per group, their
 * indices, the offsets of their text and (on request) the text itself, decoded from the packed records: only the pulled reads
 * leave the GPU, and a run that did not echo its reads (-a), or whose reads have no host text at all, can still be pulled from.
 *   the rule   pull_reads.pl:76-100 on the fields of a record exactly as the .out writer prints them:
 *                status        tid                 score         third (the script's valid_kmers)   type
 *                CALL, PHIX    call_tid (none: -1) call_score    cand_kmer_cnt                     the match type word
 *                NODBHITS      read_len (sic)      k (sic)       valid_kmers                       NoDbHits
 *                SHORT_LEN     read_len            k             -1                                ReadTooShort
 *                SHORT_VALID   valid_kmers         -j min_kmer   -1                                ReadTooShort
 *              1. tid is an id of a group, score >= thresh, third >= min_kmer: that group (an id listed by two groups belongs
 *                 to the later one);  2. a LOWSCORE group exists, score < its score, third >= min_kmer: that group;  3. type
 *                 NoDbHits, third >= min_kmer, a NODBHITS group exists: that group;  4. (ReadTooShort: the script selects
 *                 nothing).  LMAT_ST_SILENT records are never selected by 1-3.  So a NoDbHits read of 202 bases is pulled by a
 *                 group that lists 202, and NoDbHits reads reach LowScore first when its score is above k -- as upstream.
 *              The score compares are made on the float the device holds; the script compares the 6-digit text.
 *   flags      LMAT_BIN_SUBTREE  the group's ids stand for their clades in ctx's tree: exact ids first (of any group), then
 *                                the nearest ancestor that a SUBTREE group owns.  Needs a loaded taxonomy (else LMAT_E_STATE);
 *                                an id the tree does not hold stays an exact id.
 *              LMAT_BIN_REST     the group takes every read no branch selected, SILENT ones included (depletion runs)
 *              LMAT_BIN_LOWSCORE the LowScore group, with low_score;  LMAT_BIN_NODBHITS  the group branch 3 selects into
 *              Of several groups with REST, LOWSCORE or NODBHITS the last one counts.  A group may have no ids and no flags.
 *   groups     at most 65534 (LMAT_E_CAPACITY); a group is known by its position in the array (file: by its line among the
 *              lines that make a group).  lmat_bins_set_from_file reads the script's grammar (pullfmt.hpp).
 *   lmat_bins_run    on the result records the most recent launch left on the device, which must have been for exactly these
 *              reads, first and count (lmat_classify, or lmat_classify_async* + lmat_sync); otherwise LMAT_E_STATE.  Blocking.
 *   lmat_bins_counts reads and bases per group.   lmat_bins_fetch  of one group: read_idx[n] ascending, indices into `reads`;
 *              base_off[n + 1] from 0; bases[base_off[n]] (ACGT, N for an invalid position) -- NULL, or a run without
 *              want_bases (then LMAT_E_STATE for a non-NULL bases): none.  Any of the three may be NULL.
 *   errors     a gene context: LMAT_E_ARG.  lmat_bins_run before lmat_bins_set, counts / fetch before a run: LMAT_E_STATE. */
#define LMAT_BIN_SUBTREE  1u
#define LMAT_BIN_REST     2u
#define LMAT_BIN_LOWSCORE 4u
#define LMAT_BIN_NODBHITS 8u
#define LMAT_BIN_NONE 0xFFFFu   /* the group of a read no group takes */
typedef struct lmat_bins lmat_bins;
typedef struct {
    const uint32_t* ids; uint32_t n_ids;   /* printed taxids (32-bit) */
    uint32_t flags;                        /* LMAT_BIN_* */
    float low_score;                       /* with LMAT_BIN_LOWSCORE */
} lmat_bin_group;
int lmat_bins_create(lmat_ctx* ctx, lmat_bins** out);
void lmat_bins_destroy(lmat_bins* b);
const char* lmat_bins_error(const lmat_bins* b);
int lmat_bins_set(lmat_bins* b, const lmat_bin_group* groups, uint32_t n_groups, float thresh, int32_t min_kmer);
int lmat_bins_set_from_file(lmat_bins* b, const char* idfile, float thresh, int32_t min_kmer);
int lmat_bins_run(lmat_bins* b, const lmat_reads* reads, uint64_t first, uint64_t count, int want_bases);
int lmat_bins_counts(lmat_bins* b, uint64_t* n_reads_per_group, uint64_t* n_bases_per_group);
int lmat_bins_fetch(lmat_bins* b, uint32_t group, uint32_t* read_idx, uint64_t* base_off, uint8_t* bases);
/* Test hook: uploads n records and runs the select kernel alone; group_out[i] = the group of record i or LMAT_BIN_NONE.
 * k and -j min_kmer are the context's. */
int lmat_debug_bins_select(lmat_bins* b, const lmat_read_result* host_results, uint64_t n, uint16_t* group_out);
/* The streamed boundary with bins (NULL clears; applies to submits made afterwards; the slots' buffers are allocated here):
 * select and partition run behind a slot's classify launches, ahead of its result copy -- also when the slot grows and the
 * batch runs again -- and lmat_stream_next_bins gives, for the batch lmat_stream_next handed out, group_off[n_groups + 1] and
 * read_idx[group_off[n_groups]] (indices into the batch, ascending per group), in pinned memory valid until the release.  No
 * bases: the submitter holds the text.  A batch submitted without bins: LMAT_E_STATE. */
int lmat_stream_set_bins(lmat_stream* st, lmat_bins* b);
int lmat_stream_next_bins(lmat_stream* st, const uint64_t** group_off, const uint32_t** read_idx);

/* ---- test hook: the decision step on given candidate tables ---------------------------------
 * Runs the decision kernels' own code -- std::sort(TCmp) (src/read_label.cpp:475-485, 892-893) and findReadLabelVer2
 * (:284-419) -- on n candidate tables given from outside instead of computed from reads: table i = the (32-bit taxid,
 * score) pairs off[i] .. off[i+1] (1..64 of them, any order) and the read's standard deviation stdev[i] (the second
 * statistic read_label prints).  Needs the taxonomy only.  results[i]: call_tid, call_score, match_type.  This is how the
 * records of the reference's own example run (tests/golden/example_records.json) are put to the GPU kernels directly. */
int lmat_debug_decide(lmat_ctx* ctx, const uint32_t* tids, const float* scores, const uint64_t* off, const float* stdev,
                      uint64_t n, lmat_read_result* results);
/* The same step on (taxid, COUNT) tables and a candidate k-mer count per table, through either decision path of the engine:
 * on_the_wave = 0 the general path (k4_part1 / k4_part2: scores = count / cand, the statistics, std::sort(TCmp) replayed,
 * findReadLabelVer2 -- the code lmat_debug_decide pins to the reference's printed records), on_the_wave = 1 k4_wave, the
 * wave-parallel form the classify kernel runs for every read of the benchmark.  A table k4_wave declines (cand above 999, the
 * heapsort turn of introsort, a lineage beyond 64 entries, two lineage entries of one depth ...) comes back with status 255.
 * results[i]: status, match_type, cand_kmer_cnt, log_avg, stdev, call_tid, call_score. */
int lmat_debug_decide_counts(lmat_ctx* ctx, const uint32_t* tids, const uint32_t* counts, const uint64_t* off, const uint32_t* cand,
                             uint64_t n, int on_the_wave, lmat_read_result* results);
/* k4_wave on tables shaped as the closure leaves a read with ONE eligible id: the first kept[i] slots of table i are the ids the
 * lists kept, eligible[i] is the slot among them whose ancestors -- registered by the closure, with its count -- fill the slots
 * behind (kept[i] = 0: nothing is said about table i).  Such a table may be decided in closed form: took[i] = 1
 * where it was, 0 where k4_wave's general code decided or declined it (status 255, as above).  with_cands != 0 attaches a
 * candidate buffer as -p does: results[i].n_cand / cand_off are then set, and no table is taken.  LMAT_K4_CHAIN=0 takes none. */
int lmat_debug_decide_chain(lmat_ctx* ctx, const uint32_t* tids, const uint32_t* counts, const uint64_t* off, const uint32_t* cand,
                            const uint32_t* kept, const uint32_t* eligible, uint64_t n, int with_cands, lmat_read_result* results,
                            uint8_t* took);
/* The same with the closure's word per table given as the classify kernel forms it: shape[i] = kept << 8 | 1 << 17 -- the closure
 * finished and kept that many slots: the closed form for ONE DOMINANT lineage among others may decide the table --, | eligible |
 * 1 << 16 when it also found one eligible id as above, or 0.  took[i] = 0 general code (or declined), 1 the closed form for one
 * lineage, 2 the one for a dominant lineage, 3 the one for TIED ids at the top, which is offered by | 1 << 18 (valid only beside bit
 * 17; the classify kernel sets the two together; a word without it behaves as before).  LMAT_K4_TIE=0 turns the last off,
 * LMAT_K4_PATH=0 the second, LMAT_K4_CHAIN=0 the first. */
int lmat_debug_decide_shape(lmat_ctx* ctx, const uint32_t* tids, const uint32_t* counts, const uint64_t* off, const uint32_t* cand,
                            const uint32_t* shape, uint64_t n, int with_cands, lmat_read_result* results, uint8_t* took);

/* ---- measurement aid ---------------------------------------------------------
 * Random 64-byte bucket gather over the loaded table with the probe kernel's access shape;
 * reports the HIP-event time and the bytes it read (the practical ceiling of the probe). */
int lmat_gather_bench(lmat_ctx* ctx, uint64_t n_probes, uint64_t seed, float* ms, uint64_t* bytes);

/* Where the compact table layout files a k-mer (forward-encoded, either strand): bucket index and 16-bit slot tag
 * for a table of about want_buckets buckets; *n_buckets = the bucket count actually used (the 16-bit tag sets a
 * minimum).  (bucket, tag) <-> canonical k-mer is a bijection; tests check exactly that.  Needs no device.
 * LMAT_E_ARG when this k has no compact layout (k < 10). */
int lmat_table_address(int k, uint64_t want_buckets, uint64_t kmer, uint64_t* n_buckets, uint32_t* bucket, uint32_t* tag);
/* The way back: the canonical k-mer filed under (bucket, tag) in that table.  LMAT_E_ARG for a bucket or tag the geometry has not. */
int lmat_table_unaddress(int k, uint64_t want_buckets, uint32_t bucket, uint32_t tag, uint64_t* kmer);

/* ---- record text -------------------------------------------------------------
 * The bytes read_label writes to a .out file for these results (prefix
 * read_label.cpp:1733-1738, body :844-848,894-937,1218,1233,1271).  Headers are
 * "r<first_index+i>"; bases/off may be NULL when prn_read == 0 ("X" is written, -a).
 * Returns the text length (excluding the terminating NUL); writes at most cap bytes. */
int64_t lmat_format_out(const lmat_ctx* ctx, const lmat_read_result* results, uint64_t n, const lmat_cand* cands,
                        const uint8_t* bases, const uint64_t* off, int prn_read, uint64_t first_index, char* buf,
                        uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LMAT_HIP_H */
