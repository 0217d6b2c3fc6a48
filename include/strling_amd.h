/*
 * strling_amd.h -- C ABI of the MI355X-native STRling extract + cluster hot path.
 *
 * The reference (quinlan-lab/STRling v0.6.0) is a single statically linked Nim program with no
 * plugin / FFI seam; its drop-in contract is CLI + files (.bin, -bounds.txt).  This header is the
 * seam a Nim (or any) host binds instead of the reference's in-process procs: each entry point
 * names the reference code it replaces (paths relative to the STRling repository root).  Plain
 * pointers and sizes only; no C++ or torch types.  All functions return 0 (STRL_OK) or a negative
 * status; strl_last_error() gives the message (thread-local).  The library has NO CPU fallback:
 * every compute entry point needs a HIP device and fails with STRL_ERR_NO_DEVICE without one.
 */
#ifndef STRLING_AMD_H
#define STRLING_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STRL_OK 0
#define STRL_ERR_NO_DEVICE (-1)
#define STRL_ERR_HIP (-2)
#define STRL_ERR_ARG (-3)
#define STRL_ERR_CAPACITY (-4)
#define STRL_ERR_IO (-5)
#define STRL_ERR_FORMAT (-6)
#define STRL_ERR_ASSERT (-7) /* a doAssert of the reference would have fired (e.g. extract.nim:72) */
#define STRL_ERR_LIMIT (-9)  /* more records than one device pass over a whole input takes (2^31 - 16: record indices travel in 31 bits);
                                * the reference has no such cap (extract.nim:308) -- the CLI routes such a file to the streaming host Cache */
#define STRL_ERR_NOMEM (-10) /* device memory exhausted (the per-read state of a whole input is resident: ~130 B per read with the device
                               * front end; 288 GB hold ~2e9 reads).  The CLI repeats the extraction with the host pair logic, which keeps
                               * nothing per read on the device. */
#define STRL_ERR_CRC (-8)    /* a BGZF block inflates, but not to the bytes its CRC-32 names (htslib stops there too) */

#define STRL_MEM_HOST 0
#define STRL_MEM_DEVICE 1

/* Longest read the KERNELS score: a lane's byte-wide class counters are exact while no class can be seen more than 255 times.
 * The reference's uint8 histograms (utils.nim:113-117) simply wrap beyond that (utils.nim:192-195), so a longer read is scored by
 * the library's host twin of the scorer with that arithmetic (csrc/host_score.cpp) and its words are merged into the device's
 * results by record index -- every scoring entry point does so by itself.  STRL_MAX_READ_LEN is what the 16-bit length
 * columns of strl_read_soa / strl_pair_rec hold; a longer record is STRL_ERR_ARG. */
#define STRL_DEVICE_READ_LEN 510
#define STRL_MAX_READ_LEN 65534

typedef struct strl_ctx strl_ctx;

int strl_version(void);
const char *strl_last_error(void);
int strl_device_count(void);

/* One context per GPU / stream (re-entrant per handle; the reference is single-threaded). */
int strl_ctx_create(int device_ordinal, strl_ctx **ctx);
void strl_ctx_destroy(strl_ctx *ctx);
/* The HIP stream (hipStream_t) all kernels of this context are launched on. */
void *strl_ctx_stream(strl_ctx *ctx);
int strl_ctx_sync(strl_ctx *ctx);
/* Free / total memory of the context's device right now (hipMemGetInfo).  No counterpart in the reference (a host program);
 * `strling extract -v` prints what the whole-file resident state takes. */
int strl_ctx_mem_info(strl_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- Options (utils.nim:119-127; extract.nim:255-256,299-300) ---- */
typedef struct {
  int32_t median_fragment_length; /* frag_dist.median, extract.nim:283 */
  double proportion_repeat;       /* -p, default 0.8 */
  uint8_t min_mapq;               /* -q, default 40 */
} strl_opts;
int strl_ctx_set_opts(strl_ctx *ctx, const strl_opts *opts);

/* ---- genome STR intervals: the table genome_repeats() returns (genome_strs.nim:107-141,
 * read_bed.nim:30-50), flattened per BAM tid.  has_chrom[tid] != 0 iff the chromosome is a key of
 * the table (extract.nim:30 `aln.chrom in genome_str`).  Intervals need not be sorted. ---- */
typedef struct {
  int32_t n_tid;
  const uint8_t *has_chrom; /* [n_tid] */
  const int64_t *iv_off;    /* [n_tid+1] */
  const int32_t *iv_start;  /* [iv_off[n_tid]] */
  const int32_t *iv_stop;
} strl_genome_str;
int strl_ctx_set_genome(strl_ctx *ctx, const strl_genome_str *g); /* g == NULL: empty table */

/* ---- BAM records as hts-nim hands them to extract.nim (tid/start/mate_*, flag, mapq, cigar,
 * 4-bit SEQ, qname).  seq_off is a byte offset and must be a multiple of 16; seq4 must have 32
 * readable bytes of slack after the last record. ---- */
typedef struct {
  int64_t n;
  const int32_t *tid, *pos, *mtid, *mpos;
  const uint16_t *flag;
  const uint8_t *mapq;
  const uint32_t *cigar_off; /* [n+1] */
  const uint32_t *cigar;     /* BAM encoding len<<4|op */
  const uint64_t *seq_off;   /* [n] */
  const int32_t *l_seq;      /* [n] */
  const uint8_t *seq4;
  const uint64_t *qname_off; /* [n+1] */
  const char *qnames;
} strl_records;

/* ---- structure-of-arrays read batch the kernels consume (24 B of metadata per read + SEQ) ---- */
#define STRL_CIG_SINGLE_M 1u /* n_cigar == 1 and op == M          (extract.nim:30) */
#define STRL_CIG_FIRST_S 2u  /* n_cigar >= 1 and cigar[0] is S     (extract.nim:98,104) */
#define STRL_CIG_LAST_S 4u   /* n_cigar >= 1 and cigar[last] is S */
#define STRL_CIG_ONE_OP 8u   /* n_cigar == 1 */
#define STRL_CIG_NONE 16u    /* n_cigar == 0 */
typedef struct {          /* == words y, z, w of a scorer queue entry */
  uint32_t seq_off;        /* 16-byte units */
  uint16_t l_seq, clip_l;
  uint16_t clip_r;
  uint8_t cig, mapq;
  uint32_t pad;
} strl_read_meta;
typedef struct {
  uint64_t n;
  const int32_t *tid;      /* [n] */
  const int32_t *pos;      /* [n] aln.start */
  const int32_t *end;      /* [n] aln.stop (bam_endpos) */
  const uint32_t *seq_off; /* [n] offset of the read's 4-bit SEQ in 16-byte units */
  const uint16_t *l_seq;   /* [n] */
  const uint16_t *clip_l;  /* [n] length of cigar[0] if it is S, or if the cigar is one single M op (the align_length of a read the
                            * skip predicate removes, extract.nim:33); else 0 */
  const uint16_t *clip_r;  /* [n] length of cigar[last] if it is S else 0 */
  const uint8_t *mapq;     /* [n] */
  const uint8_t *cig;      /* [n] STRL_CIG_* bits */
  const uint8_t *seq4;     /* BAM nibble packing; every read starts 16-byte aligned */
  uint64_t seq4_bytes;     /* including >= 32 bytes of slack */
  uint32_t max_l_seq;
  int32_t mem;             /* STRL_MEM_HOST or STRL_MEM_DEVICE: where ALL pointers above live */
  const strl_read_meta *meta; /* optional (may be NULL), same memory as the rest: seq_off | l_seq | clip_l | clip_r | cig | mapq of
                            * read i once more as ONE 16-byte row.  The skip-predicate pass removes ~90 % of the reads without
                            * looking at these six fields and gathers them for the kept ones: one row = one cache line per kept
                            * read where the five columns are five.  Host batches get their rows made on the device. */
} strl_read_soa;

/* What the pair logic (Cache.add, extract.nim:192-248 with to_tread, add_soft, adjust_by) reads of one record, as ONE
 * 32-byte row: the join touches a few per cent of the records at random, and a row is one memory transaction where the
 * column arrays of strl_read_soa would be a dozen.  Same `mem` as the read batch the rows belong to. */
typedef struct {
  int32_t tid, pos;      /* aln.tid, aln.start */
  int32_t mtid, mpos;    /* aln.mate_tid, aln.mate_pos */
  int32_t end;           /* aln.stop */
  uint16_t flag, l_seq;
  uint16_t clip_l, clip_r; /* as in strl_read_soa */
  uint8_t mapq, cig;
  uint16_t pad;
} strl_pair_rec;
typedef struct {
  const strl_pair_rec *rec; /* [n] */
  const uint64_t *qhash;    /* [n] 64-bit hash of aln.qname (strl_qname_hash); the Cache is keyed by it */
} strl_pair_soa;
/* Host: the rows of a batch from its records and the arrays strl_soa_from_records derived (out[n]). */
int strl_pair_rows(const strl_records *rec, const int32_t *end, const uint16_t *clip_l, const uint16_t *clip_r, const uint8_t *cig,
                   strl_pair_rec *out);

/* Host: derive the SoA metadata arrays from BAM-native records (replaces the hts-nim accessors
 * used at extract.nim:30-38,83-87,98-119: cigar ops, aln.stop, clip lengths).  Caller provides the
 * output arrays ([n] each); SEQ is shared with `rec` (seq_off/16). */
int strl_soa_from_records(const strl_records *rec, int32_t *end, uint32_t *seq_off16, uint16_t *l_seq, uint16_t *clip_l,
                          uint16_t *clip_r, uint8_t *cig, uint32_t *max_l_seq);

/* ---- scorer results ----
 * packed unit/count word:  bits 0-11 unit code (kmer 2-bit "CATG" code, first base in the high bits),
 * bits 12-14 unit length (0 = empty), bit 15 = read removed by the skip predicate (extract.nim:30-34),
 * bits 16-31 repeat_count (after reduce_repeat, utils.nim:271). */
#define STRL_RES_SKIPPED 0x8000u
#define STRL_RES_K(w) (((w) >> 12) & 7u)
#define STRL_RES_CODE(w) ((w) & 0xfffu)
#define STRL_RES_COUNT(w) ((w) >> 16)
typedef struct {
  uint32_t read_side; /* read index << 1 | side (0 = left clip / cigar[0], 1 = right clip / cigar[last]) */
  uint32_t res_first; /* get_repeat(soft_seq) with p - 0.07      (first-seen branch, extract.nim:241-244) */
  uint32_t res_after; /* get_repeat(soft_seq) with min(p, 0.6)   (after-mate branch,  extract.nim:207-211) */
  uint32_t seg_len;   /* c.len: number of soft-clipped bases scored */
} strl_soft_rec;

typedef struct {
  uint64_t n_reads, n_skipped, n_scored, n_soft_items;
  float ms_classify, ms_score, ms_soft; /* HIP-event kernel times on the context stream (0 if timing off) */
  uint32_t n_stage_b_whole, n_stage_b_soft; /* items whose ladder reaches k = 5 (second scorer launch) */
} strl_score_stats;

/* Score a batch: per read the skip predicate + utils.get_repeat on the whole read
 * (extract.nim:20-40 via to_tread :66), and the soft-clip repeat scan of add_soft
 * (extract.nim:93-116) for every clipped end that add_soft would look at, under both lowered
 * thresholds.  whole[n] and soft[soft_cap] live where soa->mem says.  Soft records come back in
 * unspecified order when mem == DEVICE and sorted by read_side when mem == HOST.
 * Requires strl_ctx_set_opts (and optionally strl_ctx_set_genome) first. */
int strl_score_reads(strl_ctx *ctx, const strl_read_soa *soa, uint32_t *whole, strl_soft_rec *soft, uint64_t soft_cap,
                     uint64_t *n_soft, strl_score_stats *stats);
/* `strling index` scoring (genome_strs.nim:61-92): utils.get_repeat on every window [i*step, min(n, i*step+window))
 * of one chromosome (ASCII, any case; hts-nim fai.get + toUpperAscii), with the context's proportion_repeat.
 * words[n_windows] receives the packed unit/count word of each window (host array; pass NULL to only get
 * *n_windows = ceil(n_bases / step)).  window <= 160. */
int strl_index_chrom(strl_ctx *ctx, const char *seq, uint64_t n_bases, uint32_t window, uint32_t step, uint32_t *words,
                     uint64_t *n_windows);
/* The sequential half of `strling index` (host): merge consecutive windows that carry the same unit (allowing one
 * skipped window), pad by one window on both sides and trim to the first/last unit-sized step that is a rotation of
 * the unit -- repeat_windows genome_strs.nim:76-91 and trim :22-59.  One BED row of <fasta>.str per region
 * (genome_strs.nim:137: chrom, start, stop, unit).  STRL_ERR_ASSERT where trim's doAssert would fire. */
typedef struct { uint64_t start, stop; char unit[8]; } strl_region;
int strl_index_regions(const char *seq, uint64_t n_bases, const uint32_t *words, uint64_t n_windows, uint32_t window,
                       uint32_t step, strl_region *out, uint64_t cap, uint64_t *n_out);

/* The host twin of the scorer (csrc/host_score.cpp): utils.get_repeat (utils.nim:236-271) on ONE read given as text (what
 * hts-nim's aln.sequence returns: "=ACMGRSVTWYHKDBN" letters), of any length, with the reference's own arithmetic -- uint8
 * histogram bins that wrap (utils.nim:192-195), float64 thresholds.  *word = the packed unit/count word.  No device is
 * touched.  This is what scores records of more than STRL_DEVICE_READ_LEN bases inside every scoring entry point. */
int strl_score_read_host(const char *seq, int32_t l_seq, double proportion_repeat, uint32_t *word);

/* Kernel timing with HIP events recorded on the context stream around every kernel of
 * strl_score_reads (a ring of 256 launches).  enable_timing(ctx, 1) resets the ring;
 * strl_ctx_kernel_times synchronises the stream and returns the SUM of the classify / score / soft
 * kernel durations (ms) over the launches recorded since then. */
int strl_ctx_enable_timing(strl_ctx *ctx, int on);
int strl_ctx_kernel_times(strl_ctx *ctx, double ms_sum[3], uint64_t *n_launches);
/* The same per launch of a kernel: classify | stage A, survivor compaction, stage B of the whole reads | soft-item
 * compaction | stage A, compaction, stage B of the segments. */
int strl_ctx_kernel_times_detail(strl_ctx *ctx, double ms_sum[8], uint64_t *n_launches);

/* ---- tread (cluster.nim:23-32); qname is carried as an index (record index in extract, sample
 * index in merge -- merge.nim:118-125 overwrites qname with the sample number) ---- */
#define STRL_SOFT_LEFT 0
#define STRL_SOFT_RIGHT 1
#define STRL_SOFT_BOTH 2
#define STRL_SOFT_NONE 3
#define STRL_SOFT_NONE_RIGHT 4
#define STRL_SOFT_NONE_LEFT 5
#define STRL_SOFT_TAKEN 255 /* not a Soft value: a tread strl_assign_reads_loci took out of the table (see there) */
typedef struct {
  int32_t tid;
  uint32_t position;
  char repeat[6];
  uint16_t flag;
  uint8_t split;
  uint8_t mapping_quality;
  uint8_t repeat_count;
  uint8_t align_length;
  int64_t qname_id;
} strl_tread;

/* Host pair logic: Cache.add over the record stream (extract.nim:192-248 driven by :308-329,
 * including the second visit of the unmapped tail by ibam.query("*")), fed by the scorer outputs.
 * soft must be sorted by read_side.  Writes at most cap treads; *n_out gets the total produced. */
int strl_pair_reads(const strl_records *rec, const strl_opts *opts, const uint32_t *whole, const strl_soft_rec *soft,
                    uint64_t n_soft, int64_t n_tail, strl_tread *out, uint64_t cap, uint64_t *n_out);

/* Streaming form of the pair logic: the reference's Cache (extract.nim:89-91,298) kept alive across batches fed in
 * file order.  Emitted treads accumulate inside the pairer; their qname_id indexes the pairer's own qname arena.
 * The caller replays the unmapped tail a second time itself (extract.nim:326-329). */
typedef struct strl_pairer strl_pairer;
int strl_pairer_create(const strl_opts *opts, strl_pairer **pairer);
void strl_pairer_destroy(strl_pairer *pairer);
int strl_pairer_add(strl_pairer *pairer, const strl_records *rec, const uint32_t *whole, const strl_soft_rec *soft, uint64_t n_soft);
int strl_pairer_result(strl_pairer *pairer, const strl_tread **treads, uint64_t *n, const uint64_t **qname_off,
                       const char **qnames, uint64_t *n_pending);

/* ---- the extract hot loop on the device, end to end (replaces extract.nim:308-329 for one batch that is the whole input):
 * skip predicate + scorer + soft-clip scan (strl_score_reads) and the pair logic (Cache.add with to_tread, add_soft,
 * adjust_by, unplaced_pair; the second visit of the last n_tail records, extract.nim:326-329), all as kernels on the context's
 * streams.  Asynchronous when soa->mem == STRL_MEM_DEVICE: nothing is copied to the host, the treads stay resident in the
 * context in the order of the reference's .bin file (qname_id = record index) for strl_treads_fetch / strl_cluster_resident.
 * Consecutive calls on device-resident input overlap: the pair logic of a batch runs on a side stream of the context while
 * the scorer of the next call's batch runs on the main stream (the context keeps two sets of the buffers involved); every
 * entry point that reads the results waits for the side streams first, so the caller sees the order of its calls.  The
 * input arrays of a call must stay valid and unchanged until a later synchronising call (strl_treads_fetch, strl_ctx_sync).
 * item_cap bounds the records that take part in the join (reads of qname groups with a repeat + their soft-clip records),
 * tread_cap the treads; 0 = defaults from n.  Exceeding either is reported by strl_treads_fetch (STRL_ERR_CAPACITY).
 * Qname groups are keyed by the 64-bit hash alone (two different qnames with equal hashes would be treated as one group). */
int strl_extract_device(strl_ctx *ctx, const strl_read_soa *soa, const strl_pair_soa *pair, int64_t n_tail, uint64_t item_cap,
                        uint64_t tread_cap);
/* The same for an input that arrives in chunks (a BAM file being decoded): the chunks are scored as they come, in file
 * order; per-read rows, qname hashes and scorer results of ALL chunks stay resident in HBM (44 B per read: a 30x genome is
 * ~27 GB of the 288 GB) and the pair logic runs once, at strl_extract_finish, over the whole input -- exactly the
 * reference's single Cache over the whole file (extract.nim:298), with no per-chunk state to carry.  At most 2^31 - 16
 * records.  n_reads_hint (may be 0) pre-sizes the buffers.  Then strl_treads_fetch as above (qname_id = record index over
 * all chunks). */
int strl_extract_begin(strl_ctx *ctx, uint64_t n_reads_hint);
int strl_extract_add(strl_ctx *ctx, const strl_read_soa *chunk, const strl_pair_soa *pair);
int strl_extract_finish(strl_ctx *ctx, int64_t n_tail, uint64_t item_cap, uint64_t tread_cap);
/* Wait for the last strl_extract_device call and copy its treads to the host (out may be NULL to only get the count).
 * STRL_ERR_CAPACITY: a capacity was exceeded (n_out = treads needed when known); STRL_ERR_ASSERT: the reference's
 * doAssert repeat_count < 256 (extract.nim:72) would have fired; STRL_ERR_FORMAT: more than 512 join items share the low 32
 * bits of their qname hash (one qname on hundreds of primary records), or -- checked where the device holds the qnames
 * (strl_front_*) -- two different qnames share one 64-bit hash: repeat with the host pair logic (strl_pair_reads), which
 * keys on the qname string.  Secondary / supplementary records do not take part in the join. */
int strl_treads_fetch(strl_ctx *ctx, strl_tread *out, uint64_t cap, uint64_t *n_out, strl_score_stats *stats);
/* HIP-event times (ms) of the last strl_extract_device call when timing is enabled: soft-clip join items | probe |
 * join sort | replay | order sort + gather. */
int strl_ctx_pair_times(strl_ctx *ctx, double ms[5]);

/* Stable LSD radix sort of (key, value) pairs by key bits [bit_lo, bit_lo + bits) on the device (the sort of the
 * clustering and pairing paths: call.nim:127-130 / merge.nim:132-135 `sort` by position inside a (tid, repeat) group
 * becomes one stable keyed sort).  Host arrays in, sorted in place; n_max >= n sizes the launch like a pipeline that
 * only knows an upper bound of the count would. */
int strl_sort_pairs(strl_ctx *ctx, uint64_t *keys, uint32_t *vals, uint64_t n, uint64_t n_max, int bit_lo, int bits);

/* ---- the outlier stage (scripts/strling-outliers.py, the reference's fifth step; csrc/outliers.hip) ----
 * Matrices are row-major doubles with NaN holes; `mem` (STRL_MEM_HOST / STRL_MEM_DEVICE) says where ALL array arguments of a
 * call live, so a pipeline can keep its data on the device between the stages (strl_dev_alloc / strl_copy).  fp64 throughout,
 * IEEE division and sqrt, fixed reduction orders: two runs give the same bits.  Each call returns when its results are in place. */
int strl_dev_alloc(strl_ctx *ctx, uint64_t bytes, void **p);
int strl_dev_free(strl_ctx *ctx, void *p);
/* synchronous copy of `bytes` host -> device (to_device = 1) or device -> host (0) on the context's stream */
int strl_copy(strl_ctx *ctx, void *dst, const void *src, uint64_t bytes, int to_device);
/* Medians of the rows of x (rows x cols), NaN skipped, numpy's rule for an even count (the mean of the two middle values), by
 * exact selection.  The per-sample depth medians of strling-outliers.py:247 (m_all: every value), :280-282 (m_kept: over the
 * columns with keep[c] != 0, zeros as NaN) and :296 (m_filled: the same columns with NaN / 0 filled by m_kept).  keep may be
 * NULL (every column); any of the three outputs may be NULL. */
int strl_outliers_row_medians(strl_ctx *ctx, const double *x, uint64_t rows, uint64_t cols, const uint8_t *keep, double *m_all,
                              double *m_kept, double *m_filled, int mem);
/* hubers_est (strling-outliers.py:115-136) of every row of x (rows x cols): statsmodels 0.12.2 robust.scale.Huber(maxiter=1000)
 * over the row's non-NaN values; where numpy would warn (divide by zero, invalid, overflow) or the loop does not converge, the
 * median and MAD instead (method[r] = 1 'MAD', else 0 'Huber'); sd 0 -> NaN.  Rows wider than 4096 columns take the
 * global-memory path (STRL_OUTLIERS_WIDE=1 forces it for every row). */
int strl_outliers_huber(strl_ctx *ctx, const double *x, uint64_t rows, uint64_t cols, double *mu, double *sd, uint8_t *method, int mem);
/* z = (x - mu[r]) / sd[r] (z_score :138-141, :359), p = norm.sf(z) (:395), p_adj = Benjamini-Hochberg per column over the finite p
 * (p_adj_bh :143-168 via :402), every other value passed through.  n_null control-only rows (:340-373) join each column's BH
 * with the values null_x[c] (NULL: NaN, which is what the script's :368 leaves there) against (null_mu[j], null_sd[j]); they
 * produce no output.  z, p, p_adj: rows x cols.  (rows + n_null) * cols < 2^31. */
int strl_outliers_scores(strl_ctx *ctx, const double *x, const double *mu, const double *sd, uint64_t rows, uint64_t cols,
                         const double *null_x, const double *null_mu, const double *null_sd, uint64_t n_null, double *z, double *p,
                         double *p_adj, int mem);
/* The row order of STRs.tsv (:451, sort_values(['outlier', 'allele2_est'], ascending=False), NaN last) over the cells of two
 * rows x cols matrices: order[k] = row-major index r * cols + c of the k-th output row.  Ties keep column-major order (column =
 * sample in name order, then row = locus), the order this build defines where the script's depends on Python set order. */
int strl_outliers_order(strl_ctx *ctx, const double *outlier, const double *allele2, uint64_t rows, uint64_t cols, uint32_t *order, int mem);

/* The pair rules on single treads, so that known-answer vectors (the reference's tests/test_extract.nim:7-19,
 * tests/test_strling.nim:91-107, tests/test_utils.nim:66-74) can be run through the product's own code: with a context the
 * DEVICE functions the replay kernel calls, with ctx == NULL the host twins the streaming pairer (strl_pairer_*) calls.
 * ADJUST_BY: A.adjust_by(B, opts, B_position), extract.nim:141-179 -> *result = its return value, A updated.
 * UNPLACED_PAIR: extract.nim:182-190 -> *result.  CANONICAL: A.repeat := canonical_repeat(A.repeat), utils.nim:304-316. */
#define STRL_RULE_ADJUST_BY 0
#define STRL_RULE_UNPLACED_PAIR 1
#define STRL_RULE_CANONICAL 2
int strl_pair_rule(strl_ctx *ctx, int op, strl_tread *A, const strl_tread *B, const strl_opts *opts, uint32_t B_position, int *result);

/* 64-bit hash of every record's qname (out[n]).  Qname groups never interact in the pair logic, so a multi-GPU
 * run only has to bring together the records whose hash belongs to a group that can emit (strling_amd/dist.py). */
int strl_qname_hash(const strl_records *rec, uint64_t *out);

/* The extract hot loop end to end on one batch: SoA derivation + device scoring + pair logic
 * (replaces extract.nim:308-329). */
int strl_extract(strl_ctx *ctx, const strl_records *rec, int64_t n_tail, strl_tread *out, uint64_t cap, uint64_t *n_out,
                 strl_score_stats *stats);

/* ---- clustering (cluster.nim:323-374 + :175-250, callclusters.nim:52-66) ---- */
typedef struct {
  int32_t tid;
  uint32_t left, left_most, right, right_most, center_mass;
  uint16_t n_left, n_right, n_total;
  char repeat[7];
} strl_bounds;
typedef struct {
  char repeat[7];
  int64_t count;
} strl_unplaced;
typedef struct {
  uint64_t n_treads, n_groups, n_clusters, n_bounds, n_tie_fixups;
  float ms_sort, ms_sweep, ms_bounds;
} strl_cluster_stats;

#define STRL_MODE_MERGE 0 /* merge.nim:172-187: tid<0 dropped on load, has_per_sample_reads gate, qname_id = sample in [0, 2^32) */
#define STRL_MODE_CALL 1  /* call.nim:223-235: unplaced groups reported, no per-sample gate */
/* Group treads by (tid, repeat), stable-sort by position (call.nim:118-130 / merge.nim:121-135),
 * cluster every group and derive the gated Bounds.  Output order = the reference's order (Nim Table
 * slot order of the groups, clusters in position order within a group).  treads/out are host arrays. */
int strl_cluster(strl_ctx *ctx, const strl_tread *treads, uint64_t n, int mode, uint32_t window, int32_t min_support,
                 uint16_t min_clip, uint16_t min_clip_total, uint16_t max_clip_dist, strl_bounds *out, uint64_t cap,
                 uint64_t *n_out, strl_unplaced *unplaced, uint64_t unplaced_cap, uint64_t *n_unplaced,
                 strl_cluster_stats *stats);

/* The same over the treads the last strl_extract_device call left resident in the context (extract -> call without a
 * host round trip; STRL_MODE_CALL only).  n_tid = number of contigs of the BAM header (every tid < n_tid); pos_bits: width
 * of the position field of the sort key (0 = 32; else >= 2): 1 + the bits that hold every position on a contig, e.g. 29 for
 * a genome whose longest contig is < 2^28 bases -- fewer key bits, fewer sort passes.  The upper half of the field takes
 * the positions adjust_by wrapped below zero (uint32 arithmetic, utils.nim:304-310), in the reference's uint32 order.  With out, n_out, n_unplaced and stats all NULL the call only enqueues the kernels (asynchronous, on the context's side
 * stream; see strl_cluster_collect). */
int strl_cluster_resident(strl_ctx *ctx, int mode, int32_t n_tid, int pos_bits, uint32_t window, int32_t min_support, uint16_t min_clip,
                          uint16_t min_clip_total, uint16_t max_clip_dist, strl_bounds *out, uint64_t cap, uint64_t *n_out,
                          strl_unplaced *unplaced, uint64_t unplaced_cap, uint64_t *n_unplaced, strl_cluster_stats *stats);

/* Results of the last asynchronous strl_cluster_resident (all outputs NULL there).  Such a pass runs on a side stream of the
 * context: it overlaps whatever the caller enqueues next -- typically strl_extract_device of the NEXT batch, whose VALU-bound
 * scorer hides the clustering's many small launches -- and may be collected after that call has been issued; the pair logic
 * of the next batch waits for it on the device.  Same outputs and order as strl_cluster. */
int strl_cluster_collect(strl_ctx *ctx, strl_bounds *out, uint64_t cap, uint64_t *n_out, strl_unplaced *unplaced, uint64_t unplaced_cap,
                         uint64_t *n_unplaced, strl_cluster_stats *stats);

/* ---- multi-GPU clustering (one process per GPU) ----
 * The device buffer strl_extract_device left its treads in: *treads (strl_tread[*cap]) and *count (uint32 on the device).
 * A host framework (torch.distributed over RCCL) all-gathers these buffers; nothing is copied to the host. */
int strl_ctx_treads_device(strl_ctx *ctx, void **treads, uint64_t *cap, void **count);
/* The HIP stream (hipStream_t) the tail of the last strl_extract_device call runs on -- the context's main stream, or a side
 * stream when that call overlapped its pair logic with the next batch's scorer.  Enqueue the all-gather there: it is then
 * ordered behind the batch's pair logic (and the .bin-order sort strl_ctx_treads_device adds) and before an asynchronous
 * strl_cluster_gathered, and the whole exchange step overlaps the next strl_extract_device. */
void *strl_ctx_tail_stream(strl_ctx *ctx);
/* `gathered` (device) = world x pad treads, rank-major: rank r's treads are gathered[r * pad .. r * pad + counts[r]) with
 * counts (device, uint32[world]) -- what all_gather_into_tensor over the ranks' padded tread buffers produces.  This rank
 * keeps the treads of the (tid, unit) groups it owns (a hash of the key modulo world, computed on the device), in global
 * (rank, .bin) order, and clusters them like strl_cluster_resident.  Rows of different ranks are disjoint sets of groups;
 * strl_group_order over all treads gives the reference's order of the groups. */
int strl_cluster_gathered(strl_ctx *ctx, const strl_tread *gathered, const uint32_t *counts, int world, uint32_t pad, int rank, int mode,
                          int32_t n_tid, int pos_bits, uint32_t window, int32_t min_support, uint16_t min_clip, uint16_t min_clip_total,
                          uint16_t max_clip_dist, strl_bounds *out, uint64_t cap, uint64_t *n_out, strl_unplaced *unplaced,
                          uint64_t unplaced_cap, uint64_t *n_unplaced, strl_cluster_stats *stats);

/* ---- the same exchange inside the library: RCCL over xGMI (comm.hip).  The reference is single-threaded per sample
 * (merge.nim:52,89 is its only sharding knob); this is north_star's "RCCL all-gather ... before clustering".
 * Ranks = one process per GPU: rank 0 calls strl_comm_unique_id, the bytes travel by the host framework's own means
 * (torch.distributed broadcast, MPI_Bcast), every rank calls strl_ctx_comm_init; then strl_cluster_exchange per step:
 * .bin-order sort of the resident treads, ncclAllGather of the padded tread buffers and their counts on the stream the
 * batch's tail runs on, strl_cluster_gathered.  `pad` = the most treads a rank contributes, equal on all ranks.
 * Ranks = one process, n contexts (the CLI's --gpus N): strl_ctxs_comm_init (ncclCommInitAll on n different devices; where
 * contexts share a device -- RCCL refuses two ranks per device -- the exchange is made with ordered device copies), then
 * strl_ctxs_cluster_exchange for all of them and strl_cluster_collect per context.
 * strl_exchange_treads: all ranks' treads of the last exchange in (rank, .bin) order, for strl_group_order. */
/* host treads -> the context's resident treads (as if strl_extract_device had left them): how `strling merge --gpus N`
 * hands every context its share of the .bin files' treads before strl_ctxs_cluster_exchange */
int strl_ctx_set_treads(strl_ctx *ctx, const strl_tread *treads, uint64_t n);
#define STRL_COMM_ID_BYTES 128
int strl_comm_unique_id(uint8_t id[STRL_COMM_ID_BYTES]);
int strl_ctx_comm_init(strl_ctx *ctx, int world, int rank, const uint8_t id[STRL_COMM_ID_BYTES]);
int strl_ctxs_comm_init(strl_ctx **ctxs, int n);
int strl_ctx_comm_info(strl_ctx *ctx, int *world, int *rank, int *uses_rccl);
int strl_cluster_exchange(strl_ctx *ctx, uint32_t pad, int mode, int32_t n_tid, int pos_bits, uint32_t window, int32_t min_support, uint16_t min_clip,
                          uint16_t min_clip_total, uint16_t max_clip_dist, strl_bounds *out, uint64_t cap, uint64_t *n_out, strl_unplaced *unplaced,
                          uint64_t unplaced_cap, uint64_t *n_unplaced, strl_cluster_stats *stats);
int strl_ctxs_cluster_exchange(strl_ctx **ctxs, int n, uint32_t pad, int mode, int32_t n_tid, int pos_bits, uint32_t window, int32_t min_support,
                               uint16_t min_clip, uint16_t min_clip_total, uint16_t max_clip_dist);
int strl_exchange_treads(strl_ctx *ctx, strl_tread *out, uint64_t cap, uint64_t *n_out);

/* bounds() (cluster.nim:175-250) + the gate of callclusters.nim:52-66 on one bare cluster -- reads sorted by position,
 * Cluster.left_most = right_most = 0 -- run by the device function the clustering kernels call.  *good = the gate's verdict. */
int strl_bounds_bare(strl_ctx *ctx, const uint32_t *positions, const uint8_t *splits, uint32_t n, uint16_t min_clip, uint16_t min_clip_total,
                     uint16_t max_clip_dist, strl_bounds *out, int *good);

/* HIP-event times (ms) of the last clustering pass when timing is enabled: keys + sort + group tables | ends + walk | bounds */
int strl_ctx_cluster_times(strl_ctx *ctx, double ms[3]);

/* The (tid, unit) groups of `treads` in the order the reference iterates its Table (call.nim:223, merge.nim:172) -- the
 * order strl_cluster emits the groups' rows in.  Host only.  A multi-GPU run that clusters disjoint sets of groups on
 * different ranks puts the gathered rows back into the reference's order with it (strling_amd/dist.py). */
typedef struct {
  int32_t tid;
  char repeat[8];
} strl_group_key;
int strl_group_order(const strl_tread *treads, uint64_t n, int mode, strl_group_key *out, uint64_t cap, uint64_t *n_groups);

/* The reads of every bound the last strl_cluster call on this context returned, in cluster order (position-sorted,
 * stable): bound j holds treads[members[member_off[j]]] .. treads[members[member_off[j+1] - 1]] (indices into the
 * array given to strl_cluster; c.reads of call.nim:246).  member_off is [n_bounds + 1]. */
int strl_cluster_members(strl_ctx *ctx, uint64_t *member_off, uint32_t *members, uint64_t cap, uint64_t *n_members);

/* Loci given on the command line (-l BED / -b BOUNDS) take their reads before clustering: assign_reads_locus,
 * callclusters.nim:14-50, for every locus in order.  The reads of the locus' (tid, unit) group whose position lies in
 * [left_most - 1, right_most] go to the locus (assigned[assigned_off[j] .. assigned_off[j+1]), position order), the read
 * right behind that range is lost like in the reference (:34-36), n_total/n_left/n_right of the locus are recounted.
 * Taken and lost treads get split = STRL_SOFT_TAKEN in place: strl_cluster then ignores them as reads but still
 * counts them as keys of the reference's Table, which keeps its row order.  mode as for strl_cluster. */
typedef struct {
  strl_bounds b;
  char name[128]; /* Bounds.name, column 5 of -bounds.txt */
} strl_locus;
int strl_assign_reads_loci(strl_tread *treads, uint64_t n, int mode, strl_locus *loci, uint64_t n_loci, uint64_t *assigned_off,
                           uint32_t *assigned, uint64_t cap);

/* The same on the device, for lists of many thousands of loci: one sort of the treads by (tid, unit, position, input order),
 * two binary searches per locus, and the taking itself one wave per (tid, unit) group, the groups side by side (assign.hip;
 * the rule: assign_core.h).  The contract is strl_assign_reads_loci's, field for field: `treads` (host) is marked in place,
 * the loci are recounted (the uint16 counts wrap as there), assigned_off[n_loci + 1] is filled; assigned may be NULL (no
 * lists), and STRL_ERR_CAPACITY names the entries needed when `cap` is too small (everything else is filled as on success).
 * STRL_ERR_ARG, as strl_cluster gives it and with nothing written: a tread whose unit is not a NUL-padded ACGT string, a
 * tid < -1, n > 2^31 - 16.  A locus whose unit is not made of ACGT, or whose tid no tread has, receives nothing.  After an
 * error the context goes on working.  strl_assign_info_last: the figures of the context's last call. */
typedef struct {
  uint64_t n_loci, n_groups; /* loci given; (tid, unit) groups with treads that at least one locus names */
  uint64_t n_assigned, n_lost;
  double seconds; /* the whole call on the host's clock */
} strl_assign_info;
int strl_assign_reads_loci_device(strl_ctx *ctx, strl_tread *treads, uint64_t n, int mode, strl_locus *loci, uint64_t n_loci,
                                  uint64_t *assigned_off, uint32_t *assigned, uint64_t cap);
int strl_assign_info_last(strl_ctx *ctx, strl_assign_info *info);

/* Re-run the device side of the last strl_cluster call (sorts, sweep, bounds) over the treads still resident on
 * the device, asynchronously on the context stream and without host synchronisation.  For timing. */
int strl_cluster_replay(strl_ctx *ctx);

/* ---- `strling call` evidence around one bound and the genotype record (host; collect.nim, spanning.nim,
 * genotyper.nim).  The caller performs the indexed BAM read (hts-nim `b.query(tid, start, stop)`, collect.nim:141)
 * and hands the records over; `isize` is aln.isize of each record. ---- */
#define STRL_SPANNING_FRAGMENT 0 /* collect.nim:10-13 SupportType */
#define STRL_SPANNING_READ 1
#define STRL_OVERLAPPING_READ 2
typedef struct { /* collect.nim:15-31 Support; repeat = the bound's unit, qname = qname of record `rec` */
  uint8_t type, repeat_count, cigar_ins, cigar_del;
  uint32_t fragment_length;
  double fragment_percentile;
  int64_t rec;
} strl_support;
typedef struct {
  int32_t median_depth;    /* -1: more than 20 000 read pairs in the window (collect.nim:171-174) */
  float expected_spanners;
  uint64_t n_support;
} strl_span_summary;
/* spanners(), collect.nim:132-182: out receives the Support list in the reference's order; records outside the
 * queried region [max(0, left - window), right + window) are ignored, so `r` may be a superset of the query result. */
int strl_spanners(const strl_records *r, const int32_t *isize, const strl_bounds *b, int32_t window, const uint32_t frag[4096],
                  uint8_t min_mapq, strl_support *out, uint64_t cap, strl_span_summary *sum);

typedef struct { /* the Options fields genotype() reads (utils.nim:119-127, call.nim:106-110) */
  int32_t median_fragment_length;
  int32_t min_support;
  uint16_t min_clip, min_clip_total;
} strl_call_opts;
typedef struct { /* genotyper.nim:29-52 Call */
  int32_t tid;
  uint32_t start, stop;
  char repeat[7];
  double allele1, allele2;
  uint32_t overlapping_reads, anchored_reads, spanning_reads, spanning_pairs, left_clips, right_clips, sum_str_counts;
  float expected_spanning_fragments, spanning_fragments_oe_percentile;
  int32_t unplaced_reads;
  double depth;
  int32_t is_large;
} strl_call;
/* genotype(), genotyper.nim:150-199 */
int strl_genotype(const strl_bounds *b, const strl_tread *members, uint64_t n_members, const uint64_t *qname_off, const char *qnames,
                  const strl_support *spanners, uint64_t n_spanners, const strl_call_opts *opts, double depth, strl_call *call);
/* After every bound: add_percentile (call.nim:38-48), the single-large-expansion refinement (:264-276) and the row
 * order of -genotype.txt (Table[string, seq[Call]] by canonical unit).  calls in the order they were made;
 * order[n] receives the indices in output order. */
int strl_calls_finish(strl_call *calls, uint64_t n, const strl_unplaced *unplaced, uint64_t n_unplaced, uint64_t *order);
/* Row order of -unplaced.txt (CountTable[string], call.nim:280-281) for the unplaced list strl_cluster returned */
int strl_unplaced_order(const strl_unplaced *unplaced, uint64_t n, uint64_t *order);
/* one -genotype.txt row (genotyper.nim:54-57), without newline */
int strl_call_row(char *buf, int cap, const strl_call *call, const char *chrom);
/* canonical_repeat, utils.nim:304-316 */
void strl_canonical_repeat(const char in[6], char out[6]);

/* ---- BGZF / BAM front end on the device (the reference reads the BAM through htslib on one thread, extract.nim:275,289) ----
 * Inflate n raw DEFLATE streams (the payloads of BGZF blocks: RFC 1951, <= 64 KiB inflated each) on the GPU, one wavefront
 * per stream.  comp = all compressed bytes, coff/clen = where each stream sits in it, isize = its inflated size (the BGZF
 * footer's ISIZE); out receives the streams back to back.  STRL_ERR_FORMAT for invalid data or a size mismatch. */
int strl_inflate_blocks(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen,
                        const uint32_t *isize, uint32_t n_blocks, uint8_t *out, uint64_t out_bytes);
/* HIP-event time (ms) of the inflate kernel of the last strl_inflate_blocks call (copies excluded). */
int strl_ctx_inflate_ms(strl_ctx *ctx, double *ms);

/* ---- BGZF output on the device (the reference writes its BAMs through htslib, i.e. zlib on the host) ----
 * Compress in[0, in_bytes) into BGZF members of block_bytes input bytes each (the last one shorter), written back to back
 * into out, WITHOUT the EOF block: one workgroup per member.  Every member is the 18-byte header with BSIZE, one final DEFLATE
 * block -- dynamic Huffman, or stored when that would be no smaller -- CRC-32 and ISIZE; members are compressed independently.
 * block_bytes in [1, 0xFF00], else STRL_ERR_ARG.  out_cap < strl_bgzf_deflate_bound() is STRL_ERR_CAPACITY before anything is
 * launched or written.  csize[k] = the size of member k (may be NULL), *n_stored = the members that went out stored,
 * *out_bytes = the bytes written; no byte of out behind them is touched.  in_bytes == 0: no member, STRL_OK.
 * The bytes are a function of the input alone: strl_bgzf_deflate_host gives the same ones. */
int strl_bgzf_deflate(strl_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                      uint32_t *csize, uint32_t *n_stored);
/* The output bytes that always suffice for strl_bgzf_deflate: every member stored, in_bytes + 31 bytes a member (0 for a block_bytes outside [1, 0xFF00]). */
uint64_t strl_bgzf_deflate_bound(uint64_t in_bytes, uint32_t block_bytes);
/* strl_bgzf_deflate on the calling thread, without a device: the same rule (csrc/deflate_core.h), the same bytes, the same refusals. */
int strl_bgzf_deflate_host(const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *csize,
                           uint32_t *n_stored);
/* The same calls with the match rule named.  STRL_DEFLATE_FAST is the rule of the calls above and gives their bytes: one
 * candidate per position, greedy.  STRL_DEFLATE_DENSE looks at up to 16 earlier positions with the same 4-byte hash within 16128
 * bytes and parses one step lazily (csrc/deflate_core.h: DflDense): smaller members (zlib level 5 to 6's size), more kernel time.
 * Any other mode is STRL_ERR_ARG.  Members, refusals and strl_bgzf_deflate_bound are those of the calls above; device and host
 * give the same bytes for a mode. */
#define STRL_DEFLATE_FAST 0
#define STRL_DEFLATE_DENSE 1
int strl_bgzf_deflate_mode(strl_ctx *ctx, int mode, const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap,
                           uint64_t *out_bytes, uint32_t *csize, uint32_t *n_stored);
int strl_bgzf_deflate_host_mode(int mode, const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                                uint32_t *csize, uint32_t *n_stored);
/* HIP-event time (ms) of the kernels of the last strl_bgzf_deflate / strl_bgzf_deflate_mode call (copies excluded). */
int strl_ctx_deflate_ms(strl_ctx *ctx, double *ms);

/* ---- `strling call`'s evidence reads on the device (replaces the per-bound `for aln in ibam.query(tid, left - window,
 * right + window)` of call.nim:196-218 / collect.nim:132-141, i.e. htslib's indexed iterator: bgzf seek + inflate + bam_read1
 * from the .bai linear-index offset up to the first record at or behind `end`) for many bounds at once.
 * The host looks the regions up in the index and hands over, per region, the consecutive BGZF blocks from the linear-index
 * offset on (first_block .. first_block + n_blocks - 1 of the block arrays, which are laid out as for strl_inflate_blocks;
 * crc32 = the blocks' trailers, may be NULL) and in_block = where inside the first block's inflated bytes the index points.
 * On return out[out_off[r], out_off[r] + out_len[r]) holds region r's BAM records (block_size-prefixed, back to back, file
 * order) from the first record that may reach past `beg` up to, not including, the first record with another refID or
 * pos >= end -- a superset of htslib's iterator filter (tid equal, pos < end, bam_endpos > beg), which strl_spanners applies.
 * status[r] = 0: complete; 1: the blocks handed over end before such a record (or do not parse): read that region on the host.
 * "May reach past beg": pos + 1 + the lengths of ALL its CIGAR operations > beg.  A block_size outside 32 .. 2^28 does not parse
 * (status 1); a record whose CIGAR would leave it (36 + l_read_name + 4 n_cigar_op > 4 + block_size) is kept without its CIGAR
 * being read -- whoever parses the returned bytes (strl_spanners, strl_evidence_records, the pull passes) reports it.
 * out_cap = the sum over the regions of their blocks' ISIZE + 32 bytes per region always suffices; STRL_ERR_CAPACITY leaves the
 * bytes needed in out_off[0].  STRL_ERR_FORMAT / STRL_ERR_CRC as for the front end. */
typedef struct {
  uint32_t first_block, n_blocks;
  uint32_t in_block;
  int32_t tid, beg, end;
} strl_region_req;
int strl_regions_fetch(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                       const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, uint32_t n_regions, uint8_t *out, uint64_t out_cap,
                       uint64_t *out_off, uint64_t *out_len, uint8_t *status);

/* ---- `strling call`'s evidence around a bound on the device (replaces the per-record work of spanners(), collect.nim:130-182:
 * the loop over the query's records with bam_endpos and the flag / mapq filter (:138-141), expected_spanning_probability
 * (spanning.nim:22-49), the depth array and median_depth (collect.nim:154-155, utils.nim:148-158), overlapping_read with
 * find_read_position and the unit count (collect.nim:50-119), the pair table's eligibility (:161-166); the steps that follow
 * the order of Nim's tables are finished on the host inside the call).  Bit for bit what strl_spanners returns for the same
 * records and bound.
 * Input: the records of n_regions regions as block_size-prefixed BAM records in host memory, region r at
 * bytes[off[r], off[r] + len[r]) -- what strl_regions_fetch writes to `out` (the span from the lowest to the highest region is
 * copied to the device in one piece).  bounds[r] is region r's bound; window, frag, min_mapq as for strl_spanners.
 * Output: region r's Support list at support_out[support_off[r], support_off[r + 1]) (support_off has n_regions + 1 entries;
 * `rec` = the ordinal of the record in the region's bytes) and its summary[r]; status[r] = 0: answered; 2: passed on -- more
 * than 4096 records in the region's bytes, right - left + 2 * window outside 1 .. 9190 (1000, callclusters.nim:52-66, plus
 * twice the 4095 the fragment histogram allows a window), bytes that do not parse as records, or a pair whose first record
 * starts behind its second (doAssert collect.nim:37): ask strl_spanners, which has the last word.  Nothing is answered
 * approximately.  STRL_ERR_CAPACITY when support_cap is too small: support_off[n_regions] = the entries needed.
 * STRL_ERR_ARG for a bound with left > right, like strl_spanners. */
int strl_evidence_records(strl_ctx *ctx, const uint8_t *bytes, const uint64_t *off, const uint64_t *len, const strl_bounds *bounds, uint32_t n_regions,
                          int32_t window, const uint32_t frag[4096], uint8_t min_mapq, strl_support *support_out, uint64_t support_cap,
                          uint64_t *support_off, strl_span_summary *summary, uint8_t *status);
/* The fused form `strling call` uses (replaces call.nim:196-218 from the query to the Support list: htslib's indexed iterator
 * and spanners(), collect.nim:130-182): strl_regions_fetch's inputs plus the bounds; inflate, CRC, the walk and the evidence
 * run on one stream of the context and no record bytes come back.  status[r] = 0: answered; 1: as strl_regions_fetch (read
 * the region on the host); 2: as strl_evidence_records.  Errors as for both.  kernel_ms (may be NULL): HIP-event time of the
 * evidence kernel of this call. */
int strl_regions_evidence(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                          const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, const strl_bounds *bounds, uint32_t n_regions,
                          int32_t window, const uint32_t frag[4096], uint8_t min_mapq, strl_support *support_out, uint64_t support_cap,
                          uint64_t *support_off, strl_span_summary *summary, uint8_t *status, double *kernel_ms);

/* ---- `strling extract` with the whole BAM front end on the device (replaces extract.nim:275-329: bam open / `for aln in ibam`
 * / `query("*")`, i.e. htslib's inflate + bam_read1 + the hts-nim accessors, for the whole file).  The host walks the BGZF
 * block headers and hands over compressed bytes; inflate, record boundaries, record parsing, the fragment-length words and
 * the qnames stay on the device.  Chunks are pipelined: strl_front_push(i) enqueues copy + inflate + record scan of chunk i
 * on a stream of its own, then parses and scores chunk i - 1 on the context's stream (strl_extract_add semantics: rows,
 * hashes and scorer words of ALL chunks stay resident; finish with strl_extract_finish + strl_treads_fetch).
 * A BGZF block may be handed over only once and blocks must come in file order; records may straddle blocks and chunks.
 *   n_ref                 targets in the BAM header (bounds refID / next_refID of a plausible record)
 *   first_record_offset   bytes between the start of the first pushed block's inflated data and the first record
 *   comp                  the chunk's compressed bytes; PINNED host memory (strl_pinned_alloc) makes the copy asynchronous; it
 *                         may be overwritten once the call after the next one has returned
 *   coff / clen / isize   per block: offset of its DEFLATE payload in comp, payload length, inflated size (BGZF ISIZE)
 *   crc32                 per block: the CRC-32 its BGZF trailer states (checked on the device like htslib checks it), or NULL
 *   done / n_done         summaries of chunks whose scoring has COMPLETED, in file order (push: 0 or 1, finish: up to 2)
 * Errors: STRL_ERR_FORMAT invalid DEFLATE data / ISIZE / malformed record; STRL_ERR_CRC; STRL_ERR_ARG a record's l_seq > STRL_MAX_READ_LEN (records of
 * more than STRL_DEVICE_READ_LEN bases are scored by the host twin, host_score.cpp). */
typedef struct {
  uint64_t n_records;       /* records of the chunk (secondary / supplementary included) */
  uint64_t n_primary;       /* those that are neither (the reference's progress counter, extract.nim:309,315) */
  int64_t last_placed;      /* index within the chunk of the last record with tid >= 0; -1: none */
  uint64_t tail_primary;    /* primary records behind it (the "*" region extract.nim:326 visits again) */
  uint32_t max_l_seq;
  uint32_t scan_slow_segments; /* 16 KiB segments whose guessed record start was wrong (walked again sequentially) */
} strl_front_chunk;
int strl_front_begin(strl_ctx *ctx, int32_t n_ref, uint64_t first_record_offset, uint64_t n_reads_hint);
int strl_front_push(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                    const uint32_t *crc32, uint32_t n_blocks, strl_front_chunk *done, int *n_done);
int strl_front_finish(strl_ctx *ctx, strl_front_chunk done[2], int *n_done);
/* Optional, for a caller that reads the file one chunk ahead (the CLI; the loop of extract.nim:308 has no counterpart):
 *   strl_front_reserve   (after _begin) sizes the buffers of both chunks in flight for chunks of up to max_blocks blocks and
 *                        max_comp_bytes compressed bytes, so none is reallocated in the middle of the file
 *   strl_front_stage     starts the copy to the device of the chunk the NEXT push of this context will hand over (which must
 *                        pass the same pointers and sizes) -- or, when that one is staged already, of the chunk after it: up to
 *                        two chunks may be staged, in file order.  `comp` and the tables of a staged chunk live until the
 *                        second push after its own has returned
 *   strl_front_enqueue_after + strl_front_collect = strl_front_push_after in two halves: the first queues the chunk's copy
 *                        (unless staged), inflate and record scan and returns the summary of the chunk two back; the second
 *                        waits for the PREVIOUS chunk's record scan and queues its parse + scoring.  Between them the caller
 *                        stages the chunk after this one: its copy is then in the device's queue before the wait, not behind it. */
int strl_front_reserve(strl_ctx *ctx, uint32_t max_blocks, uint64_t max_comp_bytes);
int strl_front_stage(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                     const uint32_t *crc32, uint32_t n_blocks);
int strl_front_enqueue_after(strl_ctx *ctx, strl_ctx *prev, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen,
                             const uint32_t *isize, const uint32_t *crc32, uint32_t n_blocks, strl_front_chunk *done, int *n_done);
int strl_front_collect(strl_ctx *ctx);
/* One file on several GPUs (`strling extract --gpus N`; the reference has no counterpart, extract.nim:275 is one thread): the
 * chunks go round-robin over n contexts, each with its own strl_front_begin (only the context that gets the file's first
 * chunk uses first_record_offset).  strl_front_push_after: like strl_front_push, `prev` = the context the file's previous
 * chunk went to (the partial record in front of this chunk comes from there, over xGMI when that is another device).
 * After every context's strl_front_finish, strl_ctxs_extract_gather moves what the pair logic needs of every record
 * (52 B: row, qname hash, scorer word, name reference; + soft-clip records, names, Bloom bits) to ctxs[0] in file order;
 * ctxs[0] then continues like a one-GPU run: strl_front_fragwords, strl_extract_finish, strl_treads_fetch, strl_front_qnames.
 * chunk_owner[k] / chunk_records[k]: context index and strl_front_chunk.n_records of the file's k-th chunk. */
int strl_front_push_after(strl_ctx *ctx, strl_ctx *prev, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen,
                          const uint32_t *isize, const uint32_t *crc32, uint32_t n_blocks, strl_front_chunk *done, int *n_done);
int strl_ctxs_extract_gather(strl_ctx **ctxs, int n, const uint32_t *chunk_owner, const uint64_t *chunk_records, uint64_t n_chunks);
/* The other way to spread one file (`strling extract --gpus N`, the default when the BAM has an index; extract.nim:308-329 is
 * one loop over the whole file): every context takes ONE CONTIGUOUS SHARE of the blocks, both ends at record starts the .bai
 * names, so a share is a BAM of its own -- strl_front_begin with the first record's offset in the share's first block, plain
 * strl_front_push (no `prev`, nothing carried between contexts, each context fed by its own host thread), and
 *   strl_front_trim_next   before the share's LAST chunk is handed over (strl_front_stage or the push itself): its last
 *                          tail_bytes inflated bytes -- the part of the last block behind the next share's first record --
 *                          are not the share's (the block is inflated and CRC-checked whole; the record scan ends in front of them);
 *   strl_front_tail_bytes  after strl_front_finish: bytes behind the last complete record of the last chunk.  0 for a share
 *                          that ended exactly where the next begins (anything else: the index lied; the caller repeats the
 *                          extraction chunk by chunk, strl_front_push_after).
 * strl_ctxs_extract_gather then takes the shares in order (chunk_owner non-decreasing). */
int strl_front_trim_next(strl_ctx *ctx, uint32_t tail_bytes);
int strl_front_tail_bytes(strl_ctx *ctx, uint32_t *tail_bytes);
/* Host waits of this context's front end (record scan, parse) block in the kernel instead of spinning: for N feeding threads
 * that share fewer than 2 N CPUs.  Call before strl_front_begin. */
int strl_ctx_blocking_waits(strl_ctx *ctx, int on);
/* flag | (isize in [0, 4095] ? isize : 0xffff) << 16 of records [first, first + n) of the file: what
 * fragment_length_distribution (utils.nim:86-111) reads of a record.  Synchronises the context's stream. */
int strl_front_fragwords(strl_ctx *ctx, uint64_t first, uint64_t n, uint32_t *out);
/* ... without waiting: enqueued behind the parse of every chunk handed over so far (strl_front_records of them); `out` must be
 * page-locked; *done_event is waited for (and released) with strl_event_wait, from any thread. */
int strl_front_fragwords_async(strl_ctx *ctx, uint64_t first, uint64_t n, uint32_t *out, void **done_event);
int strl_event_wait(void *event);
int strl_front_records(strl_ctx *ctx, uint64_t *n);
/* Gives up the extraction the front end fed; the context stays usable (its front-end buffers stay allocated until the context
 * goes or the next strl_front_begin).  For a caller that ran the front end over a PREFIX of a file -- `strling call`'s
 * fragment-length sample (call.nim:92, utils.nim:86-111: the first ~2.1 M records with a positive template length) -- and goes on to
 * cluster and fetch regions on the same context.  Everything the front end had in flight has completed on return. */
int strl_front_end(strl_ctx *ctx);
/* seen[tid] != 0: the contig has had a primary record so far (extract.nim:310-313 prints a line per large one) */
int strl_front_tids(strl_ctx *ctx, uint8_t *seen, int32_t n_ref);
/* qnames of the given records (a tread's qname_id) from the device's name arena: names[qname_off[i], qname_off[i + 1]).
 * STRL_ERR_CAPACITY with *need set when `cap` is too small. */
int strl_front_qnames(strl_ctx *ctx, const int64_t *record_ids, uint64_t n, uint64_t *qname_off, char *names, uint64_t cap, uint64_t *need);
/* strl_treads_fetch + strl_front_qnames in one go (no host round trips in between): the treads in .bin order (qname_id = record
 * index) and names[qname_off[i], qname_off[i + 1]) of tread i.  STRL_ERR_CAPACITY with *n_out / *names_need set when a buffer is too small. */
int strl_front_treads_named(strl_ctx *ctx, strl_tread *treads, uint64_t cap, uint64_t *n_out, uint64_t *qname_off, char *names, uint64_t names_cap,
                            uint64_t *names_need);
/* page-locked host memory for strl_front_push's compressed bytes */
void *strl_pinned_alloc(uint64_t bytes);
void strl_pinned_free(void *p);

/* ---- the BAM index (.bai) built on the device ----
 * What `samtools index` does on one thread through htslib (sam_index_build: bam_read1 + hts_idx_push per record, then
 * hts_idx_finish); the reference only consumes an index (call.nim:101-102 opens the BAM with index=true).  The chunks go through
 * the front end's copy + inflate + CRC + record scan (the same kernels as strl_front_push, and the same block tables), then one
 * lane per record computes end (CIGAR ops M, D, N, =, X; 1 for flag 0x4 or an empty CIGAR), bin (reg2bin, SAM spec 5.3) and the
 * virtual offsets of its first byte and of the byte behind it; consecutive records of one (reference, bin) collapse into a run
 * and only the runs stay resident (40 B each).  No record is parsed for the scorer and none of strl_front_begin's per-read,
 * pair-pass or name state is allocated.  Chunks are pipelined like strl_front_push: push(i) enqueues chunk i's copy + inflate +
 * scan, then indexes chunk i - 1.  Records may straddle blocks and chunks.
 *   l_ref                 [n_ref] reference lengths of the BAM header: they size the linear index (one 64-bit word per 16 KiB, and
 *                         64 windows = 1 Mbase behind l_ref: reads that hang over the end of a contig are indexed like any other)
 *   first_record_offset   bytes between the start of the first pushed block's inflated data and the first record
 *   comp .. crc32         as strl_front_push (crc32 may be NULL: not checked); blocks in file order, each once, none empty
 *   block_off             per block: file offset of its first byte (the gzip header), what a virtual offset names
 *   end_off               file offset behind the chunk's last block
 *   strl_bamindex_reserve (optional, after _begin) as strl_front_reserve
 *   strl_bamindex_finish  indexes what is in flight, sorts the runs by (reference, bin) (the library's own radix sort), merges
 *                         runs that have become neighbours and serializes: *bai_bytes = size of the .bai
 *   strl_bamindex_fetch   the bytes of the .bai file (SAM spec 5.2): bins ascending per reference, the metadata pseudo-bin 37450
 *                         (file span, mapped / placed-unmapped counts) last, n_intv = last window touched + 1, windows no
 *                         record overlaps 0, n_no_coor at the end.  A valid index for htslib-style readers; byte identity with
 *                         samtools' file is not claimed (a chunk that ends at the end of a block may name it either way).
 * Refused, never indexed wrongly: STRL_ERR_FORMAT a file that is not coordinate sorted (the message names the record), a record
 * that reaches more than 1 Mbase past its reference's l_ref or has a refID outside the header, a malformed record, invalid DEFLATE data, a file
 * that ends inside a record; STRL_ERR_LIMIT a position or end >= 2^29 (a .bai cannot hold it; strl_bamindex_begin_csi can);
 * STRL_ERR_CRC; STRL_ERR_NOMEM.
 *
 * CSI (CSIv1): the same builder with the binning scheme as a parameter -- windows of 2^min_shift bases and `depth` levels of bins
 * below bin 0; a .bai is the scheme (14, 5).  strl_bamindex_begin_csi instead of strl_bamindex_begin, everything else as above:
 *   min_shift             in [8, 24]
 *   depth                 in [0, 8]; < 0: samtools' rule, the smallest depth with 2^(min_shift + 3 depth) >= max(l_ref) + 256.
 *                         Anything else is STRL_ERR_ARG with a message (window tables and bin numbers stay small).
 *   strl_bamindex_fetch   then gives the UNCOMPRESSED CSI payload: magic CSI\1, min_shift, depth, l_aux = 0, n_ref; per reference
 *                         n_bin and per bin { bin u32, loffset u64, n_chunk i32, (beg, end) u64 x n_chunk }, bins ascending, the
 *                         pseudo-bin (8^(depth + 1) - 1) / 7 + 1 last with loffset 0; n_no_coor u64.  loffset = the scheme's linear
 *                         index at the bin's first window, empty windows filled from the next filled one (0 behind the last).
 *                         A .csi FILE is that payload in BGZF blocks: this library links nothing but the HIP runtime, so the
 *                         BGZF wrapping is the caller's job (the CLI's write_bgzf, bamio.write_csi).
 * STRL_ERR_LIMIT then is an end > min(2^(min_shift + 3 depth), 2^31 - 2): BAM positions are 32-bit and an end that left them is
 * clamped to 2^31 - 1, which is refused, not indexed. */
typedef struct {
  uint64_t n_records;  /* records of the file */
  uint64_t n_no_coor;  /* those without a reference (the index's last word) */
  uint64_t n_runs;     /* runs of consecutive records of one (reference, bin): what stayed resident */
  uint64_t n_chunks;   /* chunks written to the bins (runs merged again behind the sort) */
} strl_bamindex_info;
int strl_bamindex_begin(strl_ctx *ctx, int32_t n_ref, const int32_t *l_ref, uint64_t first_record_offset);
int strl_bamindex_begin_csi(strl_ctx *ctx, int32_t n_ref, const int32_t *l_ref, uint64_t first_record_offset, int32_t min_shift, int32_t depth);
int strl_bamindex_reserve(strl_ctx *ctx, uint32_t max_blocks, uint64_t max_comp_bytes);
int strl_bamindex_push(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                       const uint32_t *crc32, const uint64_t *block_off, uint64_t end_off, uint32_t n_blocks);
int strl_bamindex_finish(strl_ctx *ctx, uint64_t *bai_bytes, strl_bamindex_info *info);
int strl_bamindex_fetch(strl_ctx *ctx, uint8_t *out, uint64_t cap);
/* gives the builder up (also after an error): what it had in flight has completed on return, its tables are freed; the front
 * end's chunk buffers stay with the context */
int strl_bamindex_end(strl_ctx *ctx);

/* ---- `strling call --sweep`: the evidence of every bound from ONE pass over the BAM (replaces, for all bounds at once, the loop
 * call.nim:196-218 runs per bound: htslib's indexed query(tid, left - window, right + window) and spanners(), collect.nim:130-182).
 * The per-bound path (strl_regions_evidence) inflates every bound's blocks, overlapping bounds the same blocks again; here the
 * file goes through the front end's copy + inflate + CRC + record scan once, chunk by chunk like strl_bamindex_push, and behind
 * each chunk's scan the device finds, for every bound whose query ends inside the chunk, the byte range of its records --
 *   i1 = the first record with tid > b.tid, or tid == b.tid and pos >= right + window
 *   i0 = the first record of b.tid whose running maximum of bam_endpos exceeds max(0, left - window)
 * -- and runs strl_evidence_records' kernel over [i0, i1) where the records lie.  A bound is decided in the first chunk that
 * holds its i1, or in the chunk pushed with last_chunk != 0, where the end of the records closes every open bound.
 *   strl_sweep_begin    n_ref, first_record_offset as strl_bamindex_begin; bounds / window / frag / min_mapq as strl_spanners.
 *                       STRL_ERR_ARG for a bound with left > right.
 *   strl_sweep_reserve  (optional, after _begin) as strl_front_reserve
 *   strl_sweep_push     comp .. crc32 as strl_front_push (crc32 may be NULL: not checked); blocks in file order, each once, none
 *                       empty.  push(i) enqueues chunk i's copy + inflate + scan, then sweeps chunk i - 1.  last_chunk != 0: no
 *                       chunk follows; a push of no blocks with last_chunk != 0 says so of the chunk pushed before (a reader that
 *                       learns of the end of the file only behind its last chunk).
 *   strl_sweep_finish   sweeps what is in flight.  Results in the caller's order of `bounds`, laid out as strl_evidence_records'
 *                       (support_off has n_bounds + 1 entries).  status[r] = 0: answered -- the Support list and the summary are
 *                       field for field what strl_evidence_records returns for the bound and exactly the bytes of records
 *                       [i0, i1), `rec` = the ordinal counted from i0; but for `rec`, what strl_spanners returns for htslib's
 *                       query.  1: a seam -- records of the bound's reference in an earlier chunk reach past
 *                       max(0, left - window), so part of the range has left the device -- or the bound never closed (no chunk was
 *                       pushed as the last one, a reference outside the header): read the region the old way.  2: as
 *                       strl_evidence_records.  Nothing is truncated, nothing answered approximately.
 *                       STRL_ERR_CAPACITY when cap is too small: support_off[n_bounds] = the entries needed; call again.
 *   strl_sweep_end      gives the sweep up (also after an error): what it had in flight has completed on return.
 * STRL_ERR_FORMAT: a file that is not coordinate sorted (the message names the record), a refID outside the header, a malformed
 * record, invalid DEFLATE data, a file that ends inside a record; STRL_ERR_CRC; STRL_ERR_NOMEM.  After an error every later
 * push / finish repeats it; strl_sweep_end, and the context takes the next file. */
typedef struct {
  uint64_t n_answered, n_seam, n_passed_on;  /* bounds with status 0 / 1 / 2 */
  uint64_t n_chunks, n_records;              /* chunks pushed, records swept */
  double sweep_ms, evidence_ms;              /* HIP-event time of the sweep's own kernels / of the evidence kernel */
} strl_sweep_info;
int strl_sweep_begin(strl_ctx *ctx, int32_t n_ref, uint64_t first_record_offset, const strl_bounds *bounds, uint32_t n_bounds, int32_t window,
                     const uint32_t frag[4096], uint8_t min_mapq);
int strl_sweep_reserve(strl_ctx *ctx, uint32_t max_blocks, uint64_t max_comp_bytes);
int strl_sweep_push(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                    const uint32_t *crc32, uint32_t n_blocks, int last_chunk);
int strl_sweep_finish(strl_ctx *ctx, strl_support *out, uint64_t cap, uint64_t *support_off, strl_span_summary *summary, uint8_t *status,
                      strl_sweep_info *info);
int strl_sweep_end(strl_ctx *ctx);

/* ---- `strling sort`: a BAM coordinate-sorted on the device, the whole file resident (csrc/bamsort.hip) ----
 * What `samtools sort` does on the host.  The rule is csrc/bamsort_core.h's, one source for host and device:
 *   key = tid_u << 33 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1),  tid_u = refID < 0 ? n_ref : refID
 * -- (reference, position, forward before reverse), records without a reference last, the input order among equal keys (the
 * sort is stable).  The output stream is the header bytes the caller hands over followed by the records in that order, each
 * with its block_size word; it is never held whole, pieces of it are gathered on request.
 *   strl_bamsort_begin      starts a sort; the front end is set up as strl_bamindex_begin sets it up, and like every *_begin of a
 *                           pass over a file it takes the context's front end over from whatever pass had it.
 *                           arena_limit_bytes: the most the record arena may hold; 0 = what the device has free, less the
 *                           finish step's needs.  STRL_SORT_SLAB_MB (tests; default 4096): the size of an arena slab.
 *   strl_bamsort_reserve    as strl_bamindex_reserve.
 *   strl_bamsort_push       as strl_sweep_push (without last_chunk): copy, inflate, CRC and record scan of chunk i are enqueued,
 *                           then key, length and arena position of every record of chunk i - 1 are written and its complete
 *                           records copied into the arena.  STRL_ERR_NOMEM when the next slab would pass the limit or cannot
 *                           be allocated: the message gives the bytes held and the bytes needed.
 *   strl_bamsort_finish     the stable radix sort of (key, ordinal) over the 33 + bits(n_ref) key bits, and the layout: where
 *                           every record starts in the stream behind `header`'s header_bytes (strl_bamsort_header makes them).
 *                           STRL_ERR_FORMAT: a refID outside [-1, n_ref) (the message names the record's ordinal), a malformed
 *                           record, invalid DEFLATE data, a file that ends inside a record; STRL_ERR_CRC;
 *                           STRL_ERR_LIMIT: more than 2^32 - 2 records.
 *   strl_bamsort_fetch      out[0, bytes) = the stream's bytes [off, off + bytes); bytes < 4 GiB.
 *   strl_bamsort_fetch_bgzf the same bytes as BGZF members of 0xFF00 input bytes from the device compressor (the bytes
 *                           strl_bgzf_deflate gives for them), packed; off must be a multiple of 0xFF00; out_cap >=
 *                           strl_bgzf_deflate_bound(bytes, 0xFF00).  No EOF block.
 *   strl_bamsort_deflate_mode  the rule of the fetch_bgzf calls that follow on this sort (STRL_DEFLATE_FAST, where it is never
 *                           called, or STRL_DEFLATE_DENSE; else STRL_ERR_ARG); between strl_bamsort_begin and strl_bamsort_end.
 *   strl_bamsort_order      perm[j] = the input ordinal of the record of output rank j.
 *   strl_bamsort_info_now   the figures again, gather_ms summed over the fetches so far.
 *   strl_bamsort_end        gives the sort up (also after an error): what it had in flight has completed on return, arena and
 *                           tables are freed, and the context takes the next file.
 * After an error every later push / finish repeats it. */
typedef struct {
  uint64_t n_records;      /* records of the file */
  uint64_t n_no_ref;       /* those without a reference (sorted last) */
  uint64_t stream_bytes;   /* header_bytes + the bytes of all records */
  uint32_t already_sorted; /* 1: the permutation is the identity, the input was in order */
  uint32_t n_slabs;        /* slabs of the arena */
  uint64_t arena_bytes;    /* ... and their bytes */
  double sort_ms, layout_ms, gather_ms;   /* HIP-event time of the radix sort, of the layout, of the gathers of all fetches so far */
} strl_bamsort_info;
int strl_bamsort_begin(strl_ctx *ctx, int32_t n_ref, uint64_t first_record_offset, uint64_t arena_limit_bytes);
int strl_bamsort_reserve(strl_ctx *ctx, uint32_t max_blocks, uint64_t max_comp_bytes);
int strl_bamsort_push(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                      const uint32_t *crc32, uint32_t n_blocks);
int strl_bamsort_finish(strl_ctx *ctx, const uint8_t *header, uint64_t header_bytes, strl_bamsort_info *info);
int strl_bamsort_fetch(strl_ctx *ctx, uint64_t off, uint64_t bytes, uint8_t *out);
int strl_bamsort_fetch_bgzf(strl_ctx *ctx, uint64_t off, uint64_t bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *n_stored);
int strl_bamsort_deflate_mode(strl_ctx *ctx, int mode);
int strl_bamsort_order(strl_ctx *ctx, uint32_t *perm, uint64_t cap);
int strl_bamsort_info_now(strl_ctx *ctx, strl_bamsort_info *info);
int strl_bamsort_end(strl_ctx *ctx);
/* The rule without a device.  strl_bamsort_key: the key of the record whose first 20 bytes behind block_size are rec20
 * (STRL_ERR_FORMAT for a refID outside [-1, n_ref)); strl_bamsort_key_bits: 33 + bits(n_ref), the bits the sort runs over.
 * strl_bamsort_header: the output's header bytes (magic, l_text, text, reference list) from the input's -- the @HD line's SO:
 * set to coordinate (added when missing), GO: and SS: dropped, everything else byte for byte, "@HD\tVN:1.6\tSO:coordinate\n" in
 * front of a text without @HD.  `in` may hold more than the header.  *out_bytes = the bytes needed; STRL_ERR_CAPACITY when cap
 * is smaller (nothing written). */
int strl_bamsort_key(const uint8_t *rec20, int32_t n_ref, uint64_t *key);
int strl_bamsort_key_bits(int32_t n_ref);
int strl_bamsort_header(const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t cap, uint64_t *out_bytes);
/* The index of the sort's output from the sort's own pass (`strling sort --write-index`): after the last fetch and before
 * strl_bamsort_end the records, their order and their offsets in the stream are still on the device, and the index is one more
 * pass over them instead of a second read, inflate and scan of the file just written.  The stream is cut into members of exactly
 * 0xFF00 bytes, so the caller tells where it wrote them and a virtual offset is arithmetic:
 *   member_off[0 .. n_members]  file offset of every member, the last entry the EOF block's; n_members = ceil(stream_bytes / 0xFF00)
 *   voff(s) = member_off[s / 0xFF00] << 16 | s % 0xFF00, 0 <= s < stream_bytes; voff(stream_bytes) = member_off[n_members] << 16
 *   (a byte on a member boundary belongs to the member that starts there, the stream's end to the EOF block: strl_bamindex_*'s
 *   virtual offsets for the same file, so the bytes are the ones it gives)
 *   strl_bamsort_index        l_ref[n_ref] as strl_bamindex_begin; csi_min_shift < 0: a .bai, else the CSI scheme (csi_min_shift,
 *                             csi_depth), csi_depth < 0 = samtools' rule, as strl_bamindex_begin_csi.  The refusals, their words
 *                             and statuses are strl_bamindex_finish's, the ordinal the record's rank in the output; a refusal
 *                             leaves the sort as it was (fetches, another strl_bamsort_index, strl_bamsort_end).  STRL_ERR_ARG: a
 *                             table that does not ascend, does not fit 48 bits, or whose n_members is not the stream's.
 *                             STRL_SORT_INDEX_TILE (tests; default 2^22): records per launch of the per-record step.
 *   strl_bamsort_index_fetch  the bytes, as strl_bamindex_fetch gives them (a .bai, or the uncompressed CSI payload).
 * strl_bamsort_end frees the builder with the sort.  strl_bamsort_voff / strl_bamsort_members: the rule and the walk of the members
 * in a buffer of written bytes (BSIZE at byte 16; file_off = where the buffer's first byte lies in the file), without a device. */
int strl_bamsort_index(strl_ctx *ctx, const int32_t *l_ref, int32_t csi_min_shift, int32_t csi_depth, const uint64_t *member_off, uint64_t n_members,
                       uint64_t *index_bytes, strl_bamindex_info *info);
int strl_bamsort_index_fetch(strl_ctx *ctx, uint8_t *out, uint64_t cap);
int strl_bamsort_voff(const uint64_t *member_off, uint64_t n_members, uint64_t stream_bytes, uint64_t s, uint64_t *voff);
int strl_bamsort_members(const uint8_t *bytes, uint64_t n, uint64_t file_off, uint64_t *member_off, uint64_t cap, uint64_t *n_out);
/* A file larger than device memory, sorted in passes (`strling sort --windowed`).  Nothing of the records stays
 * on the device but 12 bytes each: pass 0 keeps key and length, sorts, and leaves dest[ordinal] = the record's first byte in the
 * output stream.  Every later pass reads the input again and scatters the records that touch the window [lo, hi) of the stream
 * straight to their place in a window buffer, which is then a finished piece of the stream: no temporary file, no run, no merge.
 *   strl_bamsort_begin_windowed  as strl_bamsort_begin, without an arena.  strl_bamsort_reserve / _push / _finish / _info_now /
 *                                _end work as before; strl_bamsort_info's n_slabs, arena_bytes and gather_ms stay 0.
 *   strl_bamsort_window_limit    the largest window the device can hold now: its free memory (the front end's slots are allocated
 *                                by then and so outside that figure) less the 768 MiB the resident path keeps for the piece and the
 *                                compressor.
 *   strl_bamsort_window_begin    the window [lo, hi), lo < hi <= stream_bytes, behind strl_bamsort_finish: the window buffer (never
 *                                shrunk between windows), the header's bytes inside it, the front end rewound to the file's start.
 *   strl_bamsort_window_push     the same arguments and pipelining as strl_bamsort_push, over the same file from its first chunk:
 *                                copy, inflate, CRC and record scan of chunk i, then the scatter of chunk i - 1.
 *   strl_bamsort_window_end      the last chunk's scatter, and the checks.  STRL_ERR_FORMAT "the input changed between passes:
 *                                record N" (the first record whose length is not pass 0's) or a record count that is not pass
 *                                0's; STRL_ERR_ASSERT when the bytes placed and the header's do not fill the window; and the
 *                                inflate, CRC and format errors of a push.
 * Inside the window just ended strl_bamsort_fetch / _fetch_bgzf keep their contracts and read the window buffer; outside it they
 * are STRL_ERR_ARG.  strl_bamsort_order and strl_bamsort_index are STRL_ERR_ARG in this mode (the order is given up for dest[], the
 * records are never resident in sorted order).  The 2^32 - 2 record limit stays.  STRL_SORT_GATHER_LANES = 16 / 32 / 64: lanes per
 * record of the scatter, as of the gather.  strl_bamsort_window_plan: the rule of csrc/bamsort_core.h without a device --
 * window_bytes = max(piece_bytes, limit_bytes / piece_bytes * piece_bytes), n_windows = ceil(stream_bytes / window_bytes). */
int strl_bamsort_begin_windowed(strl_ctx *ctx, int32_t n_ref, uint64_t first_record_offset);
int strl_bamsort_window_limit(strl_ctx *ctx, uint64_t *bytes);
int strl_bamsort_window_begin(strl_ctx *ctx, uint64_t lo, uint64_t hi);
int strl_bamsort_window_push(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                             const uint32_t *crc32, uint32_t n_blocks);
int strl_bamsort_window_end(strl_ctx *ctx);
int strl_bamsort_window_plan(uint64_t stream_bytes, uint64_t limit_bytes, uint64_t piece_bytes, uint64_t *window_bytes, uint64_t *n_windows);
/* SAM text as the sort's input (`strling sort IN.sam`, `strling sort -`): a second producer of what the sort
 * works from.  A chunk of whole lines is encoded to BAM records on the device (csrc/samparse.hip) by the rule of csrc/sam_core.h --
 * byte for byte the records the host's encoder of that header builds -- and key, length and arena copy run over them as over an
 * inflated chunk.  Behind the read phase nothing differs: strl_bamsort_finish, _fetch, _fetch_bgzf, _order, _index and _end.
 *   strl_bamsort_sam_begin    as strl_bamsort_begin, without a front end: names = the n_ref reference names of the @SQ lines back
 *                             to back without NULs, name_off[n_ref + 1] where each begins (strl_sam_header's list gives them).  The
 *                             host builds a hash table of the names and uploads it once.  STRL_ERR_FORMAT: a name occurs twice.
 *   strl_bamsort_sam_reserve  the slots for chunks of at most max_text_bytes (1 .. 512 MiB), before the first push.
 *   strl_bamsort_push_sam     text[0, bytes): whole alignment lines, the last byte a newline -- else STRL_ERR_ARG, which leaves the
 *                             sort as it was.  Key, length and arena copy of chunk i - 1, then the copy of chunk i, the line scan,
 *                             the size kernel and the encode are enqueued; `text` may be reused on return.  A line the rule refuses
 *                             is STRL_ERR_FORMAT "SAM line N: FIELD: ...", N counting the alignment lines from 1: the device names
 *                             the chunk's first refused line, the host's encoder says why.  Float values in spellings the kernel
 *                             does not convert exactly (more than 15 digits, a decimal exponent beyond 22, inf, nan) are the host's:
 *                             it encodes those lines and copies each record over its place.
 *   strl_bamsort_sam_info     lines, text bytes, host-finished records and chunks so far (counted when a chunk's records go into the
 *                             arena), and the HIP-event time of the copy and of the three kernels (the sums counted with the size).
 * STRL_SORT_SAM_LANES = 16 / 32 / 64: lanes per line of the size kernel and the encode.
 * Without a device: strl_sam_encode, one line (a trailing newline and a \r before it are dropped) -> one record, by the same header's
 * host function; strl_sam_header, the leading @ lines of a text -> the BAM header that text stands for (magic, l_text, the lines
 * byte for byte, n_ref, the @SQ lines' SN and LN in order), from which strl_bamsort_header makes the output's.  STRL_ERR_FORMAT: an
 * @SQ line without SN or with LN outside [1, 2^31 - 1], an SN that occurs twice.  Both follow strl_bamsort_header's capacity rule. */
typedef struct {
  uint64_t lines, text_bytes, host_finished, chunks;
  double copy_ms, scan_ms, size_ms, encode_ms;
} strl_bamsort_sam_figures;
int strl_bamsort_sam_begin(strl_ctx *ctx, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, uint64_t arena_limit_bytes);
int strl_bamsort_sam_reserve(strl_ctx *ctx, uint64_t max_text_bytes);
int strl_bamsort_push_sam(strl_ctx *ctx, const uint8_t *text, uint64_t bytes);
int strl_bamsort_sam_info(strl_ctx *ctx, strl_bamsort_sam_figures *out);
int strl_sam_encode(const uint8_t *line, uint64_t len, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, uint8_t *out, uint64_t cap, uint64_t *out_bytes);
int strl_sam_header(const uint8_t *text, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_bytes, int32_t *n_ref);
/* `strling sort --markdup` (csrc/markdup.hip, the rule in csrc/markdup_core.h): flag 0x400 set or cleared on the
 * records of a resident sort, before the first piece is gathered.  The reference drops records that carry the flag when it collects
 * spanning evidence (collect.nim:140: `if aln.flag.secondary or aln.flag.supplementary or aln.flag.dup: continue`), and an aligner
 * never sets it.  Picard's rule as `samtools markdup` applies it in template mode, without optical duplicates; mates are joined by
 * NAME on the device, so no fixmate, MC or ms tag is needed.
 *   strl_bamsort_markdup_mode  behind strl_bamsort_begin / _sam_begin and before the first push (else STRL_ERR_ARG): the pushes' arena
 *                              limit then leaves the step's 41 bytes a record free.  STRL_ERR_ARG on a windowed sort.
 *   strl_bamsort_markdup       behind strl_bamsort_finish and before the first fetch, once: the record kernel (signature, score,
 *                              name hash, class), the join by name, the pairs' and the fragments' chained sorts, and the flag bytes
 *                              written into the arena.  STRL_ERR_ARG before the finish, after a fetch, a second time, on a windowed
 *                              sort.  STRL_ERR_FORMAT: a record whose name, CIGAR, bases and qualities do not fit its block_size, or
 *                              whose unclipped end is no 32-bit position (the message names the record's ordinal).  STRL_ERR_LIMIT:
 *                              more than 512 eligible records under one name hash (the message names the count; the host path,
 *                              STRL_SORT=host, has no such limit).  After a refusal the sort is failed: only strl_bamsort_end.
 *   strl_markdup_host          the same rule without a device: records[0, bytes) = records back to back in input order, each with
 *                              its block_size word; flags[i] = the flag word record i leaves with (cap >= the number of records, else
 *                              STRL_ERR_CAPACITY with *n_records set).  The times of `info` stay 0.
 * STRL_MARKDUP_HASH_BITS = 1 .. 63 (tests; read once per process): the name hash cut to that many bits, so that different names
 * share a hash as a rule; the output does not change. */
typedef struct {
  uint64_t n_pairs, n_dup_pairs, n_fragments, n_dup_fragments, n_ineligible;
  double record_ms, join_ms, pairs_ms, fragments_ms, flag_ms;      /* HIP-event time of the step's five parts (sorts included) */
} strl_markdup_info;
int strl_bamsort_markdup_mode(strl_ctx *ctx, int on);
int strl_bamsort_markdup(strl_ctx *ctx, strl_markdup_info *info);
int strl_markdup_host(const uint8_t *records, uint64_t bytes, uint16_t *flags, uint64_t cap, uint64_t *n_records, strl_markdup_info *info);
/* `strling fastq` (csrc/fastq.hip, the rule in csrc/fastq_core.h): the reads of a resident sort back to paired
 * FASTQ, the step in front of the aligner (what `samtools collate | samtools fastq` is used for).  Mates are joined by NAME on the
 * device; three byte streams come out: 0 = p1 (R1 entries, or R1 R2 R1 R2 ... when interleaved), 1 = p2 (R2 entries; empty when
 * interleaved), 2 = s (singles; empty unless opts.singles).  Agreement with samtools is unverified.
 *   strl_bamsort_fastq_mode   behind strl_bamsort_begin / _sam_begin and before the first push (else STRL_ERR_ARG): the pushes' arena
 *                             limit then leaves the step's 57 bytes a record free.  STRL_ERR_ARG on a windowed sort and together
 *                             with strl_bamsort_markdup_mode.
 *   strl_bamsort_fastq        behind strl_bamsort_finish, once: the record kernel (field check, class, name hash, entry length), the
 *                             join by name, and one 64-bit prefix sum a stream; fills the counts and the three streams' lengths.
 *                             STRL_ERR_ARG before the finish, a second time, without the mode, on a windowed sort.  STRL_ERR_FORMAT: a
 *                             record whose name, CIGAR, bases and qualities do not fit its block_size (the message names its
 *                             ordinal).  STRL_ERR_LIMIT: more than 512 kept records under one name hash (the message names the count
 *                             and the host path, STRL_FASTQ=host, which has no such limit).
 *   strl_bamsort_fastq_fetch  behind strl_bamsort_fastq: bytes [lo, lo + len) of a stream to dst, any lo and any len inside the
 *                             stream (len < 4 GiB); nothing outside dst[0, len) is written.  STRL_ERR_ARG otherwise.
 *   strl_bamsort_fastq_info_now  the info again, text_ms and text_bytes summed over the fetches so far.
 *   strl_fastq_host           the same rule without a device: records[0, bytes) = records back to back in input order, each with its
 *                             block_size word.  info (not null) gets the counts and the streams' lengths; a stream is copied to
 *                             out[k] when cap[k] holds it, else STRL_ERR_CAPACITY (call with cap = {0, 0, 0} for the lengths).
 * STRL_FASTQ_HASH_BITS = 1 .. 63 (tests; read once per process): the name hash cut to that many bits. */
typedef struct {
  uint32_t filter;        /* -F: records with any of these flag bits are left out (default 0x900) */
  uint32_t suffix;        /* -N: /1 and /2 behind the names of reads with read number 1 and 2 */
  uint32_t default_qual;  /* -v: the quality of every base of a read without qualities (default 1) */
  uint32_t interleaved;   /* -o: each R2 behind its R1 in stream 0 */
  uint32_t singles;       /* -s: stream 2 is laid out; else singles are counted as not written */
} strl_fastq_opts;
typedef struct {
  uint64_t n_kept, n_filtered, n_empty, n_pairs, n_singles, n_singles_unwritten;
  uint64_t stream_bytes[3];
  uint64_t text_bytes;                                /* bytes the text kernel has written so far */
  double record_ms, join_ms, layout_ms, text_ms;      /* HIP-event time of the step's parts; text_ms over the fetches so far */
} strl_fastq_info;
int strl_bamsort_fastq_mode(strl_ctx *ctx, int on);
int strl_bamsort_fastq(strl_ctx *ctx, const strl_fastq_opts *opts, strl_fastq_info *info);
int strl_bamsort_fastq_fetch(strl_ctx *ctx, int stream, uint64_t lo, uint64_t len, uint8_t *dst);
int strl_bamsort_fastq_info_now(strl_ctx *ctx, strl_fastq_info *info);
int strl_fastq_host(const uint8_t *records, uint64_t bytes, const strl_fastq_opts *opts, uint8_t *const out[3], const uint64_t cap[3], strl_fastq_info *info);

/* `strling view` (csrc/view.hip, the rule in csrc/view_core.h): a BAM's records as SAM text, one line a kept
 * record, what `samtools view` is used for.  Agreement with htslib is unverified.  names / name_off[n_ref + 1]: the references' names
 * back to back, name r = names[name_off[r], name_off[r + 1]).
 *   strl_view_begin    the front end up to the record table (copy + inflate + CRC + record scan) with the view behind it; the names and
 *                      the options are uploaded once.
 *   strl_view_reserve  buffers for chunks of at most max_blocks blocks / max_comp_bytes compressed bytes.
 *   strl_view_push     a chunk of whole BGZF blocks (the block arrays of strl_bamindex_push).  The chunk is copied and its inflate is
 *                      enqueued; beside that the chunk pushed BEFORE is sized (view_size_kernel, a 64-bit prefix sum), written
 *                      (view_text_kernel) and copied to page-locked memory: *text / *text_bytes name its lines (null / 0 on the first
 *                      push and for a chunk without a kept record).  The bytes stay valid through the next call and no longer.
 *   strl_view_finish   the last chunk's lines the same way, the totals, and the check that the file does not end inside a record.
 *   strl_view_end      gives everything up.
 *                      Calls out of order (a push or finish without a begin, a push behind the finish, a second finish) are
 *                      STRL_ERR_ARG.  STRL_ERR_FORMAT: a refused record ("malformed BAM record N: FIELD ...", N its ordinal in the
 *                      file; nothing of its chunk or behind it is handed out), invalid DEFLATE data; STRL_ERR_CRC; STRL_ERR_NOMEM.
 *   strl_view_records  records[0, bytes) = records back to back in host memory, each with its block_size word, through the same two
 *                      kernels: their lines to out[0, *out_bytes).  STRL_ERR_CAPACITY leaves the bytes needed in *out_bytes and
 *                      writes nothing; nothing outside out[0, *out_bytes) is ever written.  Serves regions (opts->tid, beg, end).
 *   strl_view_records_at  the same with the ordinal of the first record given, for a caller that feeds a region in batches: refusals
 *                      name first_ordinal + the record's place in the call.  The context keeps the call's buffers for the next call.
 *   strl_view_count_only  between strl_view_begin and the first push: the pushes and the finish count (info->written) and hand out no
 *                      text -- the size kernel and the prefix sum run, the text kernel and the copy do not.
 *                      strl_view_records with out = NULL and cap = 0 does the same for records in host memory (and leaves the need
 *                      in *out_bytes, STRL_ERR_CAPACITY unless it is 0; with a hard chunk the need is the host twin's).
 *   strl_view_host     the same rule without a device (csrc/view_host.cpp): the same bytes.
 * A chunk that holds a float outside the range view_core.h's integer %g answers is formatted by the host twin (host_chunks). */
typedef struct {
  uint32_t require;       /* -f: every one of these flag bits is set */
  uint32_t exclude;       /* -F: none of these is set */
  uint32_t exclude_all;   /* -G: not all of these are set (0: no such filter) */
  uint32_t min_mapq;      /* -q */
  int32_t tid, beg, end;  /* a region, 0-based and half-open: the records that overlap it; tid = -2: no region */
} strl_view_opts;
typedef struct {
  uint64_t records, written, dropped, text_bytes;
  uint64_t chunks, host_chunks;      /* chunks (or calls) sized on the device | of those, formatted by the host twin */
  double size_ms, text_ms;           /* HIP-event time of the size kernel with its prefix sum | of the text kernel */
} strl_view_info;
int strl_view_begin(strl_ctx *ctx, int32_t n_ref, uint64_t first_record_offset, const uint8_t *names, const uint32_t *name_off, const strl_view_opts *opts);
int strl_view_reserve(strl_ctx *ctx, uint32_t max_blocks, uint64_t max_comp_bytes);
int strl_view_push(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize, const uint32_t *crc32,
                   uint32_t n_blocks, const uint8_t **text, uint64_t *text_bytes);
int strl_view_finish(strl_ctx *ctx, const uint8_t **text, uint64_t *text_bytes, strl_view_info *info);
int strl_view_end(strl_ctx *ctx);
int strl_view_records(strl_ctx *ctx, const uint8_t *records, uint64_t bytes, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, const strl_view_opts *opts,
                      uint8_t *out, uint64_t cap, uint64_t *out_bytes, strl_view_info *info);
int strl_view_records_at(strl_ctx *ctx, const uint8_t *records, uint64_t bytes, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, const strl_view_opts *opts,
                         uint64_t first_ordinal, uint8_t *out, uint64_t cap, uint64_t *out_bytes, strl_view_info *info);
int strl_view_count_only(strl_ctx *ctx, int on);
int strl_view_host(const uint8_t *records, uint64_t bytes, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, const strl_view_opts *opts, uint8_t *out,
                   uint64_t cap, uint64_t *out_bytes, strl_view_info *info);

/* ---- the .bai as a by-product of `strling extract`'s own pass (`strling extract --write-index`) ----
 * strl_front_push already copies, inflates, CRC-checks, record-scans and parses every block; the index needs of a record only
 * where it starts, refID, pos, end and flag, and the parse has just written those as dense columns.  A builder attached to the
 * context reuses strl_bamindex_*'s resident tables (runs, linear index, per-reference words) and its finish step; the per-record
 * step reads the columns instead of the records.  Nothing is added to the chunk loop that the host waits for: the base of a
 * chunk's runs is a running total on the device, the run table is sized for every record of the chunks the host has not heard
 * of yet (it looks at a copy of the device's counts a chunk late and grows the table ahead of need), and a refusal is noticed
 * late -- the chunks behind it skip the index kernels -- and reported by _finish.  A failure of the index never changes what
 * strl_extract_finish, strl_treads_fetch or strl_front_treads_named return.
 *   strl_front_index_begin   after strl_front_begin, before the first chunk, on a context that gets the whole file from its first
 *                            block (STRL_ERR_ARG on a share -- strl_front_trim_next -- and once a chunk has been handed over; a
 *                            chunk that comes with a `prev` context ends the index).  l_ref: [n_ref of strl_front_begin] as
 *                            strl_bamindex_begin; runs0: runs the table holds at first (40 B each), 0 = 2^20.
 *   strl_front_index_blocks  block_off / end_off (as strl_bamindex_push, checked the same way) of the chunk handed over NEXT:
 *                            call it before that chunk's strl_front_stage, strl_front_push or strl_front_enqueue_after; the
 *                            offsets of up to four chunks may wait, in file order.  A chunk handed over without its offsets ends
 *                            the index with a message and leaves the extraction alone.
 *   strl_front_index_finish  after strl_front_finish, before or after strl_extract_finish: the refusals of strl_bamindex_* with
 *                            the same codes and messages (record ordinal included), else sort, merge and serialization as
 *                            strl_bamindex_finish.  The bytes come out through strl_bamindex_fetch; strl_bamindex_end or the
 *                            next strl_front_begin frees the builder.
 *   strl_front_index_begin_csi  strl_front_index_begin with a CSI scheme (min_shift, depth as strl_bamindex_begin_csi): _finish and
 *                            _fetch then give the uncompressed CSI payload. */
int strl_front_index_begin(strl_ctx *ctx, const int32_t *l_ref, uint64_t runs0);
int strl_front_index_begin_csi(strl_ctx *ctx, const int32_t *l_ref, uint64_t runs0, int32_t min_shift, int32_t depth);
int strl_front_index_blocks(strl_ctx *ctx, const uint64_t *block_off, uint64_t end_off, uint32_t n_blocks);
int strl_front_index_finish(strl_ctx *ctx, uint64_t *bai_bytes, strl_bamindex_info *info);

/* ---- `strling pull`: a region's primary records and their mates (extract_region.nim:7-20,46-68) ----
 * Two batched device passes over strl_regions_fetch's inputs (the blocks of many region queries, found through the .bai), and
 * their host twins over raw record bytes (pull_logic.cpp), which need no device.
 *
 * A row describes one record; `off` is where its block_size word lies in the bytes the same call returns. */
typedef struct {
  uint64_t off;
  int32_t tid, pos, mtid, mpos; /* refID, pos, next_refID, next_pos */
  uint32_t size;                /* 4 + block_size */
  uint32_t hash;                /* Nim's murmur hash of the qname (hashes.nim), which only narrows the name compares */
  uint16_t flag;
  uint8_t l_name;               /* l_read_name: the qname's bytes + 1 */
  uint8_t found;                /* mates: 1 = the request was answered (otherwise the whole row is 0); select: 1 */
  uint32_t count;               /* select: kept records of the whole call with exactly this row's qname bytes (:50) */
} strl_pull_row;
/* A merged region [beg, end) of `tid` is cut on the 16 KiB windows of the linear index; a tile keeps the records of the region
 * (refID == tid, pos < end, bam_endpos > beg, neither 0x100 nor 0x800: :46-47 behind htslib's iterator filter) whose pos lies
 * in [own_beg, own_end).  The region's first tile has own_beg = INT32_MIN, so that it also takes the records that start before
 * `beg` and reach in; every record is therefore kept by exactly one tile.  The tile's strl_region_req is the query
 * (tid, max(beg, own_beg), own_end). */
typedef struct {
  int32_t tid, beg, end;
  int32_t own_beg, own_end;
} strl_pull_tile;
/* One kept record whose qname count is not 2 asks for its mate (:57-59, get_mate :15-19): the first record in file order of
 * next_refID that overlaps [beg, end) = [max(0, next_pos - 1), next_pos + 1), has neither 0x100 nor 0x800, differs from `flag`
 * in 0x40 and has the qname names[name_off, name_off + name_len). */
typedef struct {
  uint32_t hash;
  int32_t beg, end;
  uint32_t name_off;
  uint16_t flag;
  uint8_t name_len;
  uint8_t pad;
} strl_pull_req;
/* The select pass: inflate, CRC and walk as strl_regions_fetch (req[t] per tile), then one workgroup per tile goes through the
 * tile's records in batches of 256 (no cap on the records of a tile) and writes a row per kept record; the qname counts are
 * taken over all tiles (radix sort by hash, byte compare inside a run of equal hashes); the kept records' bytes are gathered.
 * rows[tile_rows[t], tile_rows[t + 1]) are tile t's rows in file order (tile_rows has n_tiles + 1 entries); rows[i].off indexes
 * `bytes` (every record starts at its source's offset modulo 16; *n_bytes = the bytes used).  status[t] = 0: done; 1: as
 * strl_regions_fetch; 2: bytes that do not parse -- such a tile has no rows and is read on the host.
 * STRL_ERR_CAPACITY: *n_rows / *n_bytes = what is needed (the blocks' ISIZE sum / 36 rows and twice the ISIZE sum always suffice).
 * kernel_ms (may be NULL): HIP-event time of the kernels behind the walk. */
int strl_pull_select(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                     const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, const strl_pull_tile *tiles, uint32_t n_tiles,
                     strl_pull_row *rows, uint64_t row_cap, uint64_t *n_rows, uint64_t *tile_rows, uint8_t *bytes, uint64_t bytes_cap,
                     uint64_t *n_bytes, uint8_t *status, double *kernel_ms);
/* The mate pass: the requests with a placed mate, grouped by the caller by (next_refID, 16 KiB window of `beg`): window w is
 * fetched by req[w] (tid, the window's start, the largest `end` of its requests) and holds reqs[win_off[w], win_off[w + 1]).
 * One workgroup per window enters its requests, 256 a round, in an LDS hash table keyed by the qname hash and walks the
 * window's records once per round; a record that meets a request's rule folds its place in the stream into the request's
 * answer with an integer atomicMin: the first match in file order.  rows[k] answers reqs[k] (found = 0: no mate, or its window
 * has status != 0 and is searched on the host); the mates' bytes come back like strl_pull_select's. */
int strl_pull_mates(strl_ctx *ctx, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                    const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, const uint32_t *win_off, uint32_t n_windows,
                    const strl_pull_req *reqs, const uint8_t *names, uint64_t names_bytes, strl_pull_row *rows, uint8_t *bytes,
                    uint64_t bytes_cap, uint64_t *n_bytes, uint8_t *status, double *kernel_ms);
/* The host twins (no device): `bytes` = block_size-prefixed records back to back, as BamReader's raw region read returns them.
 * strl_pull_select_host appends the tile's rows (off = base_off + the record's offset in `bytes`) behind rows[*n_rows];
 * strl_pull_counts_host fills rows[i].count, rows[i].off indexing `bytes`; strl_pull_mates_host answers the requests that are
 * not answered yet (found == 0) from the records of `bytes` in order -- use_interval = 0 leaves the overlap test out: the
 * records behind the last placed one, for the requests with next_refID == -1 (:9-13); strl_pull_order gives the stable order by
 * (tid, pos) as signed integers (:65-68).  STRL_ERR_FORMAT: bytes that are no records; STRL_ERR_CAPACITY: row_cap. */
int strl_pull_select_host(const uint8_t *bytes, uint64_t n_bytes, const strl_pull_tile *tile, uint64_t base_off, strl_pull_row *rows,
                          uint64_t row_cap, uint64_t *n_rows);
int strl_pull_counts_host(const uint8_t *bytes, strl_pull_row *rows, uint64_t n);
int strl_pull_mates_host(const uint8_t *bytes, uint64_t n_bytes, int use_interval, int32_t tid, const strl_pull_req *reqs, uint32_t n_req,
                         const uint8_t *names, uint64_t base_off, strl_pull_row *rows);
int strl_pull_order(const strl_pull_row *rows, uint64_t n, uint32_t *order);

/* ---- fragment-length statistics (utils.nim:139-146) ---- */
int strl_frag_median(const uint32_t frag[4096], double pct);

/* ---- files ---- */
/* .bin writer (extract.nim:332-348 + cluster.nim:38-50).  qname_off/qnames index by tread.qname_id. */
int strl_bin_write(const char *path, float proportion_repeat, uint8_t min_mapq, const uint32_t frag[4096],
                   const char *sam_header, int32_t header_len, const strl_tread *treads, uint64_t n,
                   const uint64_t *qname_off, const char *qnames);
/* .bin reader (unpack.nim:58-133).  Two-call protocol: with treads == NULL only the counts/sizes are
 * returned.  qname bytes are concatenated into qnames with offsets in qname_off ([n+1]). */
typedef struct {
  float proportion_repeat;
  uint8_t min_mapq;
  uint32_t frag[4096];
  int32_t header_len;
  int32_t n_reads;
  uint64_t qnames_bytes;
} strl_bin_info;
int strl_bin_read(const char *path, strl_bin_info *info, char *sam_header, strl_tread *treads, uint64_t *qname_off,
                  char *qnames);
/* The header part alone (unpack.nim:61-110 up to n_reads), without walking the records: info->qnames_bytes receives an UPPER
 * BOUND of the names' bytes (what is left of the file), so that one strl_bin_read call with buffers of these sizes reads a .bin of
 * millions of treads in a single pass. */
int strl_bin_peek(const char *path, strl_bin_info *info);
/* one -bounds.txt row (cluster.nim:262-266), without newline; returns length or <0 */
int strl_bounds_row(char *buf, int cap, const strl_bounds *b, const char *chrom);

#ifdef __cplusplus
}
#endif
#endif
