/* urcco.h -- C ABI of liburcco: MI355X-native (gfx950 / CDNA4, hand-written HIP) Correlated
 * Cross-Occurrence model build, the drop-in for the two Mahout calls the Universal Recommender makes
 * from URAlgorithm.calcAll:
 *
 *   SimilarityAnalysis.cooccurrencesIDSs(...)            reference src/main/scala/URAlgorithm.scala:323-329
 *   SimilarityAnalysis.crossOccurrenceDownsampled(...)   reference src/main/scala/URAlgorithm.scala:343-346
 *
 * (Mahout 0.13.0: math-scala/.../math/cf/SimilarityAnalysis.scala; un-vendored dependency, build.sbt:15,34-40.)
 *
 * Two levels:
 *   1. HOST level (what a JNI shim binds): host CSR in, host indicator CSR out.
 *        urcco_cooccurrences_idss / urcco_cross_occurrence_downsampled / urcco_free_indicators
 *   2. DEVICE level (what the per-GPU ranks of a multi-GPU job and bench.py drive): every pointer is a
 *      device pointer, nothing is copied, collectives between stages are the caller's (RCCL through
 *      torch.distributed).  Stage functions only enqueue on the session's HIP stream unless they say
 *      "synchronises".
 *
 * Conventions: plain C, no exceptions or aborts cross the boundary; every function returns a
 * urcco_status (0 = OK) and leaves a message for urcco_last_error() (thread local).  Matrices are
 * binary: values are implicit 1 (Preparator.scala:146,205 stores 1.0 for every event).
 * The library has no CPU fallback: without a HIP device every compute entry point returns URCCO_NO_DEVICE.
 */
#ifndef URCCO_H
#define URCCO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URCCO_VERSION 305 /* 0.3.5: urcco_dev_pack_counts, urcco_dev_cco_rows_packed (304: URCCO_BUSY, urcco_cross_occurrence_cancel_any) */

typedef enum urcco_status {
  URCCO_OK = 0,
  URCCO_BAD_ARG = 1,     /* the reference throws IllegalArgumentException for these (URAlgorithm.scala:225,232) */
  URCCO_OOM_HOST = 2,
  URCCO_OOM_DEVICE = 3,
  URCCO_HIP_ERROR = 4,
  URCCO_INTERNAL = 5,
  URCCO_NO_DEVICE = 6,
  URCCO_RCCL_ERROR = 7,  /* a collective failed, or more than one GPU was asked for and librccl could not be loaded */
  URCCO_BUSY = 8         /* the process-wide context holds ANOTHER thread's staged build (stage: not finished within the wait; cancel: not the caller's to discard) */
} urcco_status;

/* D9: how sampleDownAndBinarize's perRowSampleRate is evaluated */
#define URCCO_ROW_RATE_MAHOUT_INT_DIV 0 /* Int / Int as in Mahout 0.13.0: rows with more than max non-zeros are dropped */
#define URCCO_ROW_RATE_FRACTIONAL 1     /* min(max, n) / n in floating point */
/* The down-sampling RNG (oracle decision D10: the reference pins none -- Mahout draws from a java.util.Random per Spark partition), OR-ed
 * into row_rate_mode wherever that travels (urcco_options.row_rate_mode, urcco_dev_downsample): a stateless uniform keyed by
 * (seed, global row, column), identical in oracle/cco_oracle.{py,c} and on the device. */
#define URCCO_RNG_SPLITMIX53 0         /* 64-bit splitmix finaliser, 53-bit uniform (default) */
#define URCCO_RNG_MIX32 0x100          /* 32-bit: column xor (row, seed) key, two-round multiply-xorshift; ~10 instead of ~25 instructions per interaction.
                                        * Known structure: the seed and the row enter the key LINEARLY (key = row * C1 + seed * C2 + C3), so two seeds give the
                                        * same stream up to a constant shift of the row index, and hash(row1, col) == hash(row2, col ^ key1 ^ key2): different seeds are
                                        * relabelings of ONE sample family, not independent samples of the whole matrix.  Per-entry uniformity and the per-column keep
                                        * rates are unaffected (tests/test_oracle.py); a caller that needs independent re-samples across seeds uses the default. */

/* One IndexedDataset.matrix (user x item, binary), rows = the shared user dictionary
 * (Preparator.scala:44-87).  row_ptr has n_rows + 1 entries; col_idx is sorted and unique inside a row. */
typedef struct urcco_csr {
  int64_t n_rows;
  int64_t n_cols;
  const int64_t* row_ptr;
  const int32_t* col_idx;
} urcco_csr;

/* Mahout DownsamplableCrossOccurrenceDataset(iD, maxElementsPerRow, maxInterestingElements, minLLROpt)
 * as URAlgorithm.scala:334-341 fills it from engine.json `indicators[i]`. */
typedef struct urcco_dataset {
  urcco_csr matrix;
  int32_t max_elements_per_row;     /* indicators[i].maxItemsPerUser      (default 500, URAlgorithm.scala:54) */
  int32_t max_interesting_elements; /* indicators[i].maxCorrelatorsPerItem (default 50,  URAlgorithm.scala:56) */
  double min_llr;                   /* indicators[i].minLLR */
  int32_t has_min_llr;              /* 0 = None */
  int32_t reserved;
} urcco_dataset;

typedef struct urcco_options {
  int32_t device;        /* HIP device ordinal of the first GPU */
  int32_t row_rate_mode; /* URCCO_ROW_RATE_* | URCCO_RNG_* */
  int32_t n_gpus;        /* GPUs of THIS process to use, starting at `device`; 0 = every visible one (engine.json "numGPUs") */
  int32_t flags;         /* URCCO_FLAG_* */
  int32_t reserved[4];
} urcco_options;
#define URCCO_FLAG_SINGLE_STREAM 1  /* run the event types back to back on one HIP stream per GPU (profiling) */
#define URCCO_FLAG_FORCE_EXCHANGE 2 /* run the multi-GPU exchange path (collectives, work-balanced ranges) even with one rank */
#define URCCO_FLAG_UNORDERED_ROWS 4 /* indicator rows carry their top-k SET in unspecified (run-dependent) order: what Mahout's
                                       computeSimilarities returns -- a sparse vector has no score order, the reference sorts
                                       later (toStringMapRDD, package.scala:102) and a JNI host re-inserts by index anyway.
                                       Saves the in-kernel ranking pass.  Default off: rows ordered (llr desc, col asc). */

#define URCCO_FLAG_EMULATE_RANKS 8  /* MEASUREMENT ONLY (bench.py --emulate-ranks): the context's n_gpus ranks all run on the ONE device
                                       `device`, one after the other on a single stream (every kernel alone on the GPU), so that the per-rank
                                       critical path of a W-rank build -- user-range input phase, own-shard transposition, masks, packing,
                                       fragment merge, fused expand, item-range SpGEMM -- can be timed without W GPUs.  Needs caller-supplied
                                       collectives (urcco_comm_config.collectives; RCCL cannot put two ranks on one device) and the device
                                       level (urcco_context_build_device).  Results are the real W-rank results; xGMI time is not in them. */

/* One returned IndexedDataset: rows = items of the primary matrix A (rowIDs = A.columnIDs), columns = items
 * of B_i (columnIDs = B_i.columnIDs), values = raw LLR.  Inside a row entries are ordered (llr desc, col asc)
 * -- the order package.scala:102 (`sortBy(-score)`) produces, with the canonical tie rule.  Library-owned
 * host memory; release with urcco_free_indicators. */
typedef struct urcco_indicators {
  int64_t n_rows;
  int64_t n_cols;
  int64_t nnz;
  int64_t* row_ptr; /* n_rows + 1 */
  int32_t* col_idx;
  double* llr;
} urcco_indicators;

#define URCCO_N_BINS 7
typedef struct urcco_dataset_stats {
  int64_t nnz_raw;     /* interactions before down-sampling */
  int64_t nnz_sampled; /* after sampleDownAndBinarize */
  int64_t pairs;       /* cooccurrence pairs formed: sum_u d_A'(u) * d_B'(u) (the metric's unit) */
  int64_t nnz_out;     /* indicator entries emitted */
  int64_t rows_by_bin[7]; /* item rows per accumulator class: micro, wave, small block, block, half CU, CU, global (URCCO_N_BINS) */
  double ms_total;     /* device time of this dataset's stages (HIP events) */
} urcco_dataset_stats;

int urcco_version(void);
int urcco_device_count(void); /* 0 when no HIP device is visible */
/* Tears down the process-wide context the one-shot entry points below create on first use (streams, scratch arenas,
 * pinned staging buffers, RCCL communicators).  Safe to call when nothing was created; the next call re-creates it. */
int urcco_shutdown(void);
const char* urcco_last_error(void);
const char* urcco_status_string(int status);

/* ---- HOST level ------------------------------------------------------------------------------------- */

/* SimilarityAnalysis.cooccurrencesIDSs(indexedDatasets, randomSeed, maxInterestingItemsPerThing,
 * maxNumInteractions): datasets[0] is the primary.  out[n_datasets] receives A'A then A'B_i.
 * stats may be NULL, else stats[n_datasets]. */
int urcco_cooccurrences_idss(const urcco_csr* datasets, int32_t n_datasets, int32_t random_seed,
                             int32_t max_interesting_items_per_thing, int32_t max_num_interactions,
                             const urcco_options* options, urcco_indicators* out, urcco_dataset_stats* stats);

/* SimilarityAnalysis.crossOccurrenceDownsampled(datasets, randomSeed). */
int urcco_cross_occurrence_downsampled(const urcco_dataset* datasets, int32_t n_datasets, int32_t random_seed,
                                       const urcco_options* options, urcco_indicators* out, urcco_dataset_stats* stats);

void urcco_free_indicators(urcco_indicators* indicators, int32_t n);

/* The same call in two halves, for a caller whose input arrays are only pinned for a short while -- the JNI shim holds them
 * between Get/ReleasePrimitiveArrayCritical, which locks the JVM's garbage collector out (jni/urcco_jni.cpp):
 *   _stage   returns as soon as the library has finished READING datasets[*].matrix (every byte sits in its pinned staging ring
 *            or in HBM; the model build is already running behind the copies).  The caller may release its arrays.
 *   _finish  waits for the build and hands out the indicator matrices (n_datasets = the staged count).
 * Exactly one _finish per successful _stage, from the same thread or another; urcco_shutdown abandons a staged build.
 * urcco_cross_occurrence_downsampled == _stage followed by _finish.  out[] is zeroed on entry of every function that takes
 * it, before any fallible step: on failure the caller owns nothing and must free nothing. */
int urcco_cross_occurrence_stage(const urcco_dataset* datasets, int32_t n_datasets, int32_t random_seed, const urcco_options* options);
int urcco_cross_occurrence_finish(urcco_indicators* out, int32_t n_datasets, urcco_dataset_stats* stats);
/* The process-wide context behind these calls holds ONE build at a time: a second thread's _stage waits until the first thread's
 * _finish (at most URCCO_STAGE_WAIT_S seconds, default 600, then URCCO_BUSY -- a status of its own, so that a caller can tell "occupied"
 * from a real internal fault), the same thread staging twice is URCCO_BAD_ARG.
 * A _finish whose n_datasets differs from the staged count DISCARDS the staged build (URCCO_BAD_ARG; the context is free again).
 * _cancel discards the CALLING thread's own staged build (a caller that gave up between the halves calls it so that others do not wait);
 * nothing staged is a no-op, another thread's build is left alone (URCCO_BUSY): a thread that merely timed out in _stage must not be able
 * to throw away the owner's legitimately staged build.  _cancel_any discards whatever is staged, whoever staged it -- for a supervisor
 * that KNOWS the owner is gone (a thread that staged and died); the owner's _finish then reports "nothing staged". */
int urcco_cross_occurrence_cancel(void);
int urcco_cross_occurrence_cancel_any(void);

/* ---- CONTEXT level: the persistent form of the host level, and the multi-GPU build ------------------------------
 * A context owns, per GPU, one HIP stream + scratch arena per event type, every intermediate and output buffer (grown
 * on demand, reused by the next build), pinned staging memory and -- with more than one rank -- a communicator.  The
 * one-shot functions above run on a lazily created process-wide context (urcco_shutdown frees it); a long-lived host
 * (the Spark driver JVM) may also hold its own.  Not re-entrant: one build at a time per context, as URAlgorithm.train
 * calls it (URAlgorithm.scala:292-306, driver thread).
 *
 * Ranks: a build runs on world_size GPUs ("ranks").  Either ONE process drives them all (what a JVM does: comm = NULL,
 * n_gpus of the options, collectives through RCCL communicators created with ncclCommInitAll), or one process per GPU
 * (what bench.py does under torch.distributed.run: world_size / first_rank / nccl_unique_id filled in, n_gpus = 1).
 * Users are range-sharded over the ranks for the input phase (column counts, sampleDownAndBinarize), items of the
 * primary matrix are range-partitioned by work for the compute phase; the exchange between the two is
 * two all-reduces of column counts per event type, one all-reduce of the row-work key and one all-gather-v of the
 * down-sampled shards. */
typedef struct urcco_context urcco_context;

/* Replacement for the built-in RCCL collectives (the CPU test-suite runs the multi-rank build over `gloo` through this;
 * product callers pass NULL).  `rank` = global rank of the calling GPU; calls between group_start and group_end are
 * one collective each across all ranks and may complete at group_end -- the offset / count arrays handed to a callback stay
 * valid until that group_end returns (the data buffers until the stream has passed the collective).  stream = the HIP stream the
 * buffers are produced / consumed on.  Return 0 on success. */
typedef struct urcco_collectives {
  size_t struct_size; /* sizeof(urcco_collectives) of the header the CALLER was compiled against (since 302): a struct shorter than
                         the library's is rejected by urcco_context_create instead of being read past its end */
  void* user;
  int (*group_start)(void* user);
  int (*group_end)(void* user);
  /* in place; dtype 0 = int32, 1 = int64 */
  int (*all_reduce_sum)(void* user, int32_t rank, void* buf, int64_t count, int32_t dtype, void* stream);
  /* recv + byte_offsets[r] receives byte_counts[r] bytes = rank r's send buffer; send holds byte_counts[rank] bytes */
  int (*all_gather_v)(void* user, int32_t rank, const void* send, void* recv, const int64_t* byte_offsets,
                      const int64_t* byte_counts, void* stream);
  /* send + send_offsets[q] holds send_counts[q] bytes for rank q; recv + recv_offsets[p] receives recv_counts[p] bytes
   * from rank p (the CSC fragments of the primary).  Since 301. */
  int (*all_to_all_v)(void* user, int32_t rank, const void* send, const int64_t* send_offsets, const int64_t* send_counts,
                      void* recv, const int64_t* recv_offsets, const int64_t* recv_counts, void* stream);
} urcco_collectives;

typedef struct urcco_comm_config {
  int32_t world_size;         /* ranks of the job; 0 = the options' n_gpus (single process) */
  int32_t first_rank;         /* global rank of this process's first GPU */
  const void* nccl_unique_id; /* URCCO_UNIQUE_ID_BYTES from urcco_comm_unique_id on one rank, distributed by the caller
                                 (NULL when one process holds every rank) */
  const urcco_collectives* collectives; /* NULL = RCCL */
} urcco_comm_config;
#define URCCO_UNIQUE_ID_BYTES 128
int urcco_comm_unique_id(void* out /*[URCCO_UNIQUE_ID_BYTES]*/);

int urcco_context_create(const urcco_options* options, const urcco_comm_config* comm, urcco_context** out);
void urcco_context_destroy(urcco_context* ctx);
int32_t urcco_context_local_gpus(const urcco_context* ctx);

/* SimilarityAnalysis.crossOccurrenceDownsampled on a context: host CSR in (caller-owned, pageable is fine: staged
 * through pinned memory by a few copy threads while the GPU already works), host indicator CSR out (pinned memory of the
 * context's pool; release with urcco_free_indicators).  Single-process contexts only. */
int urcco_context_cross_occurrence(urcco_context* ctx, const urcco_dataset* datasets, int32_t n_datasets, int32_t random_seed,
                                   urcco_indicators* out, urcco_dataset_stats* stats);
/* ... and its two halves (see urcco_cross_occurrence_stage): out[n_datasets of the stage call] */
int urcco_context_stage(urcco_context* ctx, const urcco_dataset* datasets, int32_t n_datasets, int32_t random_seed);
int urcco_context_finish(urcco_context* ctx, urcco_indicators* out, urcco_dataset_stats* stats);

/* The same build with the matrices already resident in HBM -- what bench.py times.  Per event type and per local GPU
 * one user-range shard (rows [row_base, row_base + n_rows) of the n_users_total x n_cols matrix). */
typedef struct urcco_dev_shard {
  int64_t n_rows;
  int64_t row_base;
  const int64_t* row_ptr; /* device, n_rows + 1, starts at 0 */
  const int32_t* col_idx; /* device */
  int64_t nnz;            /* == row_ptr[n_rows] (known to the host) */
} urcco_dev_shard;
typedef struct urcco_dev_dataset {
  int64_t n_cols;
  int32_t max_elements_per_row;
  int32_t max_interesting_elements;
  double min_llr;
  int32_t has_min_llr;
  int32_t reserved;
  const urcco_dev_shard* shards; /* [urcco_context_local_gpus] */
} urcco_dev_dataset;
/* One indicator matrix slice: rows = items [item_lo, item_hi) of A.  Device memory owned by the context, valid until
 * its next build or destruction. */
typedef struct urcco_dev_result {
  int32_t item_lo, item_hi;
  const int64_t* row_ptr;  /* item_hi - item_lo + 1 */
  const int32_t* col_idx;
  const double* llr;
  const int64_t* stats;    /* URCCO_STATS_LEN, see urcco_dev_cco_rows */
  /* The down-sampled B this GPU multiplied with, sampled_rows + 1 row pointers.  One rank: the whole matrix.  Several ranks: a row per
   * user of the job, but (row-filtered exchange, the default) only the rows of users holding an item of THIS rank's item range are
   * filled -- every other row is empty, and sampled_row_ptr[sampled_rows] is this rank's filtered entry count, not the matrix's.  Debug
   * bit 16384 (urcco_context_set_debug) exchanges every row instead.  The exchange is also unfiltered when the job has more than 64
   * ranks or runs on caller-supplied collectives without all_to_all_v. */
  const int64_t* sampled_row_ptr;
  const int32_t* sampled_col_idx;
  int64_t sampled_rows;
  /* entries of the WHOLE down-sampled matrix, over all ranks (host-known after the exchange); -1 on a one-rank build, where the host
   * never reads a size back: there it equals sampled_row_ptr[sampled_rows] on the device */
  int64_t sampled_nnz_total;
  /* ABI 305: sampled_col_idx[e] & sampled_col_mask is the column index.  -1 (every bit) on a one-rank build.  On a sharded build the rows a rank received
   * travelled with their column's post-sampling count in the bits above the column (the words the row kernels consume: see urcco_dev_pack_counts) whenever
   * every count fits; the mask then keeps the column's bits. */
  int32_t sampled_col_mask;
} urcco_dev_result;
/* input_stream (nullable hipStream_t): the stream the shards were produced on -- the build waits for it on the device.
 * out[d * local_gpus + g].  Returns after ENQUEUEING (except for the one blocking read of range bounds / shard sizes
 * with more than one rank); follow with urcco_context_wait_stream or urcco_context_synchronize. */
int urcco_context_build_device(urcco_context* ctx, const urcco_dev_dataset* datasets, int32_t n_datasets, int64_t n_users_total,
                               int32_t random_seed, void* input_stream, urcco_dev_result* out);
int urcco_context_wait_stream(urcco_context* ctx, void* stream); /* `stream` waits (on the device) for the last build */
int urcco_context_synchronize(urcco_context* ctx);               /* the host waits */
/* per-stage timing of every session of the context (see urcco_session_set_timing) */
int urcco_context_set_timing(urcco_context* ctx, int32_t enable);
int urcco_context_get_timings(urcco_context* ctx, double* ms, int64_t* launches);
/* the same for ONE local GPU (rank first_rank + local_gpu): what bench.py --emulate-ranks reads per rank */
int urcco_context_get_timings_gpu(urcco_context* ctx, int32_t local_gpu, double* ms, int64_t* launches);
/* Debug bits of every session of the context (urcco_context_set_debug) or of one session (urcco_session_set_debug); 0 in production.
 * The names are those of cco_kernels.h (urcco::DBG_*).
 * SpGEMM row phases switched off, for profiling (results are meaningless):
 *   1 GATHER_ONLY, 2 NO_LLR, 4 NO_TOPK, 8 NO_SELECT, 16 NO_RANK (no ranking / output), 512 NO_COUNT_GATHER (every cB = 100).
 * A/B paths, results unchanged:
 *   4096 UNFUSED_EXPAND       every event type prepares its own expand operands (no fused pass over the CSC of A')
 *   8192 GATHERED_PRIMARY     several ranks: the primary's CSC from a pass over the whole gathered A' instead of fragments
 *   16384 UNFILTERED_EXCHANGE several ranks: every row of B is exchanged (see urcco_dev_result::sampled_row_ptr)
 *   1048576 UNPACKED_COUNTS   B' travels as plain column indices and the row kernels gather the counts (the form of rounds 1-5)
 *   8388608 NO_PREFILTER      the packed row kernels score every distinct candidate (no k11 = 1 prefilter: cco_rows.hip)
 *   16777216 COUNT_SCORED     with stage timing on, stats[30] counts the candidates that were scored, not the distinct ones
 *   33554432 NO_DIRECT_RANK   the packed row kernels send every row with more than k valid candidates through the select (no direct ranking: cco_rows.hip)
 *   67108864 COUNT_DIRECT     with stage timing on, stats[30] counts the rows that were ranked directly, not candidates
 *   134217728 NO_SMALL_WAVE   the one-wave class's rows of <= 64 users and <= 256 pairs stay in its general kernel (no micro-shaped body: cco_rows.hip)
 *   268435456 COUNT_SMALL_WAVE with stage timing on, stats[30] counts the rows that ran in that body, plus 2^32 per row that took its fallback
 *   536870912 NO_BLOCK_SMALL_WAVE the rows of <= 128 users and <= 512 pairs that the same body takes with two users per lane -- the rest of the one-wave class,
 *                             the first list of the small-block class -- stay in the general kernels
 *   1073741824 COUNT_BLOCK_SMALL_WAVE with stage timing on, stats[30] counts the rows of those lists that ran in the body, plus 2^32 per row that took its fallback
 * Test hook: 131072 SELECT_DELAY = the first wave of every multi-wave team sleeps before it reads the select histogram
 * (tests/test_gpu_parity.py::test_select_overlay_race_fixed).
 * The row-kernel bits (1..16, 512, 131072) run the rows on separate instantiations that carry the switches. */
int urcco_context_set_debug(urcco_context* ctx, int32_t flags);
int urcco_context_set_flags(urcco_context* ctx, int32_t flags); /* URCCO_FLAG_* */

/* ---- DEVICE level ----------------------------------------------------------------------------------- */

typedef struct urcco_session urcco_session;

/* stream: a hipStream_t (NULL = the library creates its own).  The session owns a scratch arena that grows on
 * demand and is reused by every stage. */
int urcco_session_create(int32_t device, void* stream, urcco_session** out);
void urcco_session_destroy(urcco_session* s);
int urcco_session_synchronize(urcco_session* s);
/* Per-stage device timing with HIP events on the session's stream (what bench.py's roofline numbers are made of).
 * set_timing resets the accumulators; get_timings synchronises and returns, per stage id, the summed event time
 * in ms and the number of timed launches. */
#define URCCO_N_STAGES 17
enum {
  URCCO_STAGE_COLUMN_COUNTS = 0,
  URCCO_STAGE_DOWNSAMPLE_FLAGS = 1,
  URCCO_STAGE_DOWNSAMPLE_SCAN = 2,
  URCCO_STAGE_DOWNSAMPLE_COMPACT = 3,
  URCCO_STAGE_TRANSPOSE = 4,
  URCCO_STAGE_ROW_WORK = 5,
  URCCO_STAGE_BINNING = 6,
  URCCO_STAGE_ENTROPY = 7,
  URCCO_STAGE_CCO_BIN0 = 8,  /* micro rows (<= 64 pairs)    */
  URCCO_STAGE_CCO_BIN1 = 9,  /* wave-LDS accumulator rows   */
  URCCO_STAGE_CCO_BIN2 = 10, /* small block-LDS rows        */
  URCCO_STAGE_CCO_BIN3 = 11, /* block-LDS accumulator rows  */
  URCCO_STAGE_CCO_BIN4 = 12, /* half-CU-LDS rows            */
  URCCO_STAGE_CCO_BIN5 = 13, /* CU-LDS accumulator rows     */
  URCCO_STAGE_CCO_BIN6 = 14, /* global accumulator rows     */
  URCCO_STAGE_COMPACT_INDICATORS = 15,
  URCCO_STAGE_EXCHANGE = 16 /* several ranks only: row lengths, need masks, masked lengths, packing per destination, row_ptr rebuild of what was received */
};
int urcco_session_set_timing(urcco_session* s, int32_t enable);
/* the debug bits of urcco_context_set_debug, for this session only */
int urcco_session_set_debug(urcco_session* s, int32_t flags);
/* The expand tables of urcco_dev_cco_rows* (per CSC entry of A': the start of the user's B' row, and the prefix of the rows' lengths) are built in a
 * NARROW form -- 32-bit starts, the prefix modulo 2^32 -- whenever the device finds that exact: B' holds fewer than 2^32 entries, no scan tile of the
 * prefix sums to `limit` = 2^32 or more (a tile = 2048 consecutive CSC entries of A' in the order of a_row_idx; its sum = the B' row lengths of those
 * entries' users), and the packed-count instantiations of the row kernels run.  Otherwise they are built wide
 * (64-bit), as before.  Results do not depend on the form.
 * urcco_session_expand_form: synchronises; *form_host = 0 when the session's last urcco_dev_cco_rows* call ran on narrow tables, else the reasons for
 * the wide form: 1 | 2 (B' too large) | 4 (a tile sum reached the limit) | 8 (counts do not fit the packed words) | 16 (no packed B', or debug row kernels).
 * urcco_session_set_expand_test: test hook -- lowers `limit` so that the wide form can be driven at toy size (0 restores 2^32), and starts the
 * prefix at prefix_seed instead of 0 (just below 2^32: toy rows straddle the wrap of the narrow form).  (0, 0) is production.
 * ABI: both entries are additions within ABI 305 (no existing entry changed a signature, an array's element type or a stride: the expand tables are
 * internal scratch).  urcco_session_expand_form is a stable diagnostic; urcco_session_set_expand_test is TEST-ONLY and may change or go without notice. */
int urcco_session_expand_form(urcco_session* s, int32_t* form_host);
int urcco_session_set_expand_test(urcco_session* s, int64_t limit, int64_t prefix_seed);
int urcco_session_get_timings(urcco_session* s, double* ms /*[URCCO_N_STAGES]*/, int64_t* launches /*[URCCO_N_STAGES]*/);
/* bytes of device scratch currently held */
int64_t urcco_session_scratch_bytes(const urcco_session* s);
/* Fault-hunting aid.  With URCCO_DEBUG_MARKS=1 in the environment every launch group of every session leaves "begun" /
 * "finished" marks in pinned host memory (stream-ordered); this prints them to stderr (the library's own SIGABRT handler does
 * the same when the HSA runtime aborts the process on a GPU memory fault).  Without the variable it prints nothing. */
void urcco_debug_dump_marks(void);

/* numNonZeroElementsPerColumn: counts[n_cols] = occurrences of each column id in col_idx[0..nnz).
 * counts is overwritten. */
int urcco_dev_column_counts(urcco_session* s, int64_t nnz, const int32_t* col_idx, int32_t n_cols, int32_t* counts);

/* sampleDownAndBinarize on a row shard.  raw_counts are the column counts of the WHOLE raw matrix (all shards
 * summed).  row_base = global index of local row 0 (keys the stateless RNG so results do not depend on
 * sharding).  out_row_ptr[n_rows+1], out_col_idx[capacity >= nnz], post_counts[n_cols] (nullable) is
 * overwritten with the kept entries' column counts of THIS shard.  nnz_out (device int64, nullable) receives
 * the kept total (it is also out_row_ptr[n_rows]). */
int urcco_dev_downsample(urcco_session* s, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx,
                         int64_t nnz, int32_t n_cols, const int32_t* raw_counts, int32_t seed,
                         int32_t max_elements_per_row, int32_t row_rate_mode, int64_t row_base,
                         int64_t* out_row_ptr, int32_t* out_col_idx, int32_t* post_counts);

/* CSR -> CSC of a (down-sampled) matrix.  counts[n_cols] = its column counts.  out_col_ptr[n_cols+1],
 * out_row_idx[nnz]; order inside a column is unspecified (only integer sums are formed from it).  Only columns in
 * [col_lo, col_hi) are materialised (the others get empty CSC columns): a rank of a multi-GPU job transposes just the
 * item range it owns. */
int urcco_dev_transpose(urcco_session* s, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx,
                        int64_t nnz, int32_t n_cols, const int32_t* counts, int32_t col_lo, int32_t col_hi,
                        int64_t* out_col_ptr, int32_t* out_row_idx);

/* Upper-bound work per item row of A'B: work[i - item_lo] = sum over users u of item i of d_B(u)
 * (= the cooccurrence pairs row i forms).  Used for accumulator binning and for work-balanced item ranges. */
int urcco_dev_row_work(urcco_session* s, int32_t item_lo, int32_t item_hi, int32_t n_items_a, const int64_t* a_col_ptr,
                       const int32_t* a_row_idx, int64_t nnz_a_bound, const int64_t* b_row_ptr, int64_t* work);

/* The same per-item work from a USER shard, before any rank holds the whole matrix: work[i] = sum over the shard's
 * users u that hold item i (rows of a_*) of d_B(u) (rows of b_row_ptr, same users).  Summed over the ranks it equals
 * urcco_dev_row_work's result.  work[n_items_a] is overwritten. */
int urcco_dev_row_work_csr(urcco_session* s, int64_t n_rows, const int64_t* a_row_ptr, const int32_t* a_col_idx,
                           int64_t nnz_a, const int64_t* b_row_ptr, int32_t n_items_a, int64_t* work);

/* Splits items [0, n_items) into n_parts contiguous ranges of ~equal summed work.  bounds_host[n_parts+1]
 * (host memory).  Synchronises. */
int urcco_dev_partition(urcco_session* s, int32_t n_items, const int64_t* work, int32_t n_parts,
                        int32_t* bounds_host);

/* Multi-GPU: the CSC of the item range [item_lo, item_hi) of the primary from the fragments of `world` user shards.  Rank p
 * transposed its own shard (urcco_dev_transpose over all columns: shard-local user ids) and sent the slice of that CSC
 * that belongs to the range: lens[p * (item_hi - item_lo) + j] = length of column item_lo + j in shard p (uint16 when
 * wire16, else int32), entries = the W slices one behind the other in rank order (n_entries in all).
 * sizes[URCCO_EXCH_SIZES * p] = rows of shard p (the record of the exchange, ABI 305: rows, nnz, rows longer than 65535, counts that do not fit a
 * packed B' word -- four int64 per shard, three before 305); counts[n_items] = the
 * all-reduced column counts.  out_col_ptr[n_items + 1] (columns outside the range are empty), out_row_idx = global
 * user ids, ascending inside a column when the fragments were.  Replaces the pass every rank used to make over the
 * whole gathered A' to pick its columns out (Spark: the shuffle inside `A.t %*% B`, URAlgorithm.scala:323-346). */
int urcco_dev_merge_fragments(urcco_session* s, int32_t world, int32_t item_lo, int32_t item_hi, int32_t n_items,
                              const void* lens, int32_t wire16, const int32_t* entries, int64_t n_entries,
                              const int64_t* sizes, const int32_t* counts, int64_t* out_col_ptr, int32_t* out_row_idx);

/* Rows [item_lo, item_hi) of A'B, LLR scored, cut to the top k (computeSimilarities fused onto the SpGEMM).
 *   a_col_ptr/a_row_idx   CSC of down-sampled A (nnz_a_bound >= its nnz: sizes scratch, no host sync needed)
 *   b_row_ptr/b_col_idx   CSR of down-sampled B
 *   counts_a/counts_b     post-sampling column counts     n_users               nrow of the DRMs (N)
 *   exclude_self          1 for A'A (crossCooccurrence = false)
 * Outputs (strided, row r = item_lo + r): out_count[r] entries at out_idx/out_llr[r*k ..], sorted
 * (llr desc, col asc).  stats_dev (nullable, device int64[URCCO_STATS_LEN]): [0] pairs, then URCCO_N_BINS entries each
 * of rows / pairs / users (sum of cA) / emitted entries per accumulator bin (the last group only while timing is
 * enabled), then [1 + 4 * URCCO_N_BINS] accumulator-table overflows (an internal invariant: must be 0).
 * [URCCO_STATS_LEN - 1]: rows of the first accumulator bin (the micro class: <= 64 pairs and users) that were binned into its two
 * shared-wave sub-lists (<= 16 / <= 32 pairs and users: four / two rows per wave) -- 0 when the build kept the class as one list
 * (fewer item rows than URCCO_MICRO_SPLIT_ROWS, default 1,000,000): the word names the form of the micro class that ran. */
#define URCCO_STATS_LEN 32
#define URCCO_EXCH_SIZES 4 /* int64 words of a shard's record in urcco_dev_merge_fragments' sizes */
int urcco_dev_cco_rows(urcco_session* s, int32_t item_lo, int32_t item_hi, int32_t n_items_a,
                       const int64_t* a_col_ptr, const int32_t* a_row_idx, int64_t nnz_a_bound,
                       const int64_t* b_row_ptr, const int32_t* b_col_idx, int32_t n_cols_b, const int32_t* counts_a,
                       const int32_t* counts_b, int64_t n_users, int32_t exclude_self, int32_t k,
                       int32_t has_min_llr, double min_llr, int32_t* out_count, int32_t* out_idx,
                       double* out_llr, int64_t* stats_dev);

/* B' with the columns' counts aboard (round 6): out_packed[e] = b_col_idx[e] | counts_b[b_col_idx[e]] << key_bits for the entries of B' (b_row_ptr[n_rows_b] of
 * them, read on the device; nnz_b_bound >= that sizes the launch; out_packed holds nnz_b_bound words), key_bits = the bits of the value n_cols_b.
 * out_bad[0] = number of entries whose count does not fit the word's 32 - key_bits spare bits or 16 bits.  urcco_dev_cco_rows_packed is
 * urcco_dev_cco_rows for a B' that comes with such a copy: while out_bad[0] == 0 the row kernels read a candidate's cB off the word that claims its
 * accumulator slot instead of gathering counts_b[col] once per candidate -- more than half of the SpGEMM's cache-line fills; otherwise,
 * or with b_packed == pack_bad == NULL, it IS urcco_dev_cco_rows.  The context level packs every B' itself.  Results are identical either way. */
int urcco_dev_pack_counts(urcco_session* s, int64_t n_rows_b, const int64_t* b_row_ptr, const int32_t* b_col_idx, int64_t nnz_b_bound, const int32_t* counts_b,
                          int32_t n_cols_b, int32_t* out_packed, int32_t* out_bad);
int urcco_dev_cco_rows_packed(urcco_session* s, int32_t item_lo, int32_t item_hi, int32_t n_items_a,
                              const int64_t* a_col_ptr, const int32_t* a_row_idx, int64_t nnz_a_bound,
                              const int64_t* b_row_ptr, const int32_t* b_col_idx, int32_t n_cols_b, const int32_t* counts_a,
                              const int32_t* counts_b, int64_t n_users, int32_t exclude_self, int32_t k,
                              int32_t has_min_llr, double min_llr, int32_t* out_count, int32_t* out_idx,
                              double* out_llr, int64_t* stats_dev, const int32_t* b_packed, const int32_t* pack_bad);

/* Strided top-k rows -> CSR.  out_row_ptr[n_rows+1]; out_col_idx/out_llr capacity n_rows*k. */
int urcco_dev_compact_indicators(urcco_session* s, int32_t n_rows, int32_t k, const int32_t* count,
                                 const int32_t* idx, const double* llr, int64_t* out_row_ptr,
                                 int32_t* out_col_idx, double* out_llr);

/* PopModel.calcPopular / calcTrending / calcHot (reference src/main/scala/PopModel.scala:113-179, consumed by
 * URAlgorithm.getRanksRDD, URAlgorithm.scala:537-560): per-item counts of the events whose time (ms since the epoch) lies in
 * one of n_intervals (1..3) consecutive half-open intervals [bounds_host[b], bounds_host[b + 1]) -- PEventStore.find's
 * startTime (inclusive) / untilTime (exclusive).  item_ids[e] < 0 = no target item / other event name: skipped.
 * counts (device): int32[n_intervals * n_items], overwritten; counts[b * n_items + i].  The host derives the ranks:
 * popular = counts, trending = newer - older, hot = (newer - middle) - (middle - older), each over the items present in
 * every interval it joins (universal-recommender_amd/pop_model.py). */
int urcco_dev_pop_counts(urcco_session* s, int64_t n_events, const int32_t* item_ids, const int64_t* times_ms, int32_t n_items,
                         int32_t n_intervals, const int64_t* bounds_host, int32_t* counts);

/* Batch recommendations from a built model, where the indicator matrices already sit in HBM (the query half of the reference: URAlgorithm.predict /
 * buildQuery, URAlgorithm.scala:484-953, minus Elasticsearch; DESIGN.md decision D15).  For query row q and item i of the primary's item dictionary
 *   m_c(q, i)   = | T_c(q) ^ I_c(i) |                        exact integer, per should-clause c
 *   score(q, i) = ((0.0 + boost_0 m_0) + boost_1 m_1) + ...  f64, clauses in call order, no contraction
 * -- the reference's bool query (:594-603) with Elasticsearch's per-term weight replaced by 1: an item has a positive score exactly when ES gives it one.
 * An item is eligible when it is not in the query's exclusion row (must_not ids, :715) and item_mask[i] != 0 (the available / expire date filter, :888-953,
 * evaluated by the host).  Row q of the result = the eligible items in the total order (score desc, backfill position asc), cut to num: out_count[q] entries
 * at out_idx / out_score[q * num ..] (the rest of a row is not written).  The backfill position of an item is its place in fill_order, a permutation of the
 * items, strongest rank first (`sort: [_score desc, popRank desc]`, :730-738) -- without fill_order the item index.  Items nothing hit take part with score 0
 * (the match_all clause of :668-681) unless URCCO_REC_NO_BACKFILL is set.  Ids and scores are reproducible bit for bit.
 * Enqueues on the session's stream, does not synchronise; scratch from the session's arena.  URCCO_BAD_ARG: num outside 1..URCCO_REC_MAX_NUM, n_clauses
 * outside 0..URCCO_REC_MAX_CLAUSES (0 = pure backfill), a boost that is not positive and finite, a NULL half of a pointer pair. */
#define URCCO_REC_MAX_CLAUSES 16
#define URCCO_REC_MAX_NUM 256
#define URCCO_REC_NO_BACKFILL 1
#define URCCO_REC_STATS_LEN 8   /* [0] queries served by the LDS class, [1] by the global-accumulator class,
                                   [2] candidate-table overflows (invariant: 0), [3] sum of candidates,
                                   [4] backfill steps (urcco_dev_recommend_rules with rules only, else 0), rest 0 */
typedef struct urcco_rec_clause {
  int32_t n_cols;               /* columns of I_c = items of the clause's event type */
  int32_t reserved;
  double boost;                 /* > 0, finite */
  const int64_t* ind_col_ptr;   /* device: CSC of I_c (n_items x n_cols), n_cols + 1 -- what urcco_dev_transpose makes of an indicator CSR */
  const int32_t* ind_row_idx;   /* device: order inside a column unspecified */
  const int64_t* q_row_ptr;     /* device: CSR of T_c (n_queries x n_cols), sorted unique columns */
  const int32_t* q_col_idx;
} urcco_rec_clause;

int urcco_dev_recommend(urcco_session* s, int64_t n_queries, int32_t n_items, const urcco_rec_clause* clauses, int32_t n_clauses,
                        const int64_t* excl_row_ptr, const int32_t* excl_col_idx,  /* nullable pair: CSR n_queries x n_items */
                        const uint8_t* item_mask,    /* nullable, [n_items] */
                        const int32_t* fill_order,   /* nullable, [n_items], a permutation (caller's duty) */
                        int32_t num, int32_t flags,
                        int32_t* out_count, int32_t* out_idx, double* out_score,   /* strided by num, like urcco_dev_cco_rows */
                        int64_t* stats_dev /* nullable, [URCCO_REC_STATS_LEN] */);

/* urcco_dev_recommend under business rules (the reference's must / must_not clauses: buildQueryMust / buildQueryMustNot / getFilteringDateRange,
 * URAlgorithm.scala:684-727, :841-953; DESIGN.md decision D16).  score(q, i) is the one above.  An item is eligible when it is not in the exclusion row,
 * item_mask[i] != 0 AND every rule of the call holds for (q, i); the rules are conjunctive:
 *   URCCO_RULE_ANY    row i of M and row q of the query matrix share at least one column   (`terms` in must: fields with bias < 0, user history or
 *                     similar items as a filter, :688-708, :854) -- an empty query row matches no item, as an empty `terms` query does
 *   URCCO_RULE_NONE   they share no column                                                   (fields with bias == 0 in must_not, :717-726, :863-864)
 *   URCCO_RULE_RANGE  q_lo[q] <= item_value[i] < q_hi[q]; an item without a value (INT64_MIN) fails   (`range` in must: dateRange, available / expire
 *                     dates, :872-953; gt x is lo = x + 1, an open side is INT64_MIN / INT64_MAX)
 * M is a CSR over the items (an item x value property matrix, or an indicator matrix as the build leaves it): order inside a row unspecified, duplicates
 * allowed, a column outside 0..n_cols never matches; the query rows have sorted unique columns.  The rules are evaluated on the device once per distinct
 * item a query touches and once per walked backfill position; the backfill is the ELIGIBLE zero-score items in fill_order, so a rule that few items pass
 * makes the walk long: stats[4] = backfill steps taken (256 positions each), summed over the queries -- only counted by this entry point with n_rules > 0.
 * n_rules == 0 is urcco_dev_recommend itself (results and statistics).  URCCO_BAD_ARG, in addition: n_rules outside 0..URCCO_REC_MAX_RULES, an unknown
 * kind, a NULL array that the kind needs, n_cols < 0. */
#define URCCO_REC_MAX_RULES 16
#define URCCO_RULE_ANY 0
#define URCCO_RULE_NONE 1
#define URCCO_RULE_RANGE 2
typedef struct urcco_rec_rule {
  int32_t kind, n_cols;
  const int64_t* m_row_ptr; const int32_t* m_col_idx;   /* ANY/NONE: device CSR n_items x n_cols, row order unspecified */
  const int64_t* q_row_ptr; const int32_t* q_col_idx;   /* ANY/NONE: device CSR n_queries x n_cols, sorted unique */
  const int64_t* item_value;                            /* RANGE: device [n_items], INT64_MIN = none */
  const int64_t* q_lo; const int64_t* q_hi;             /* RANGE: device [n_queries], lo <= v < hi */
} urcco_rec_rule;

int urcco_dev_recommend_rules(urcco_session* s, int64_t n_queries, int32_t n_items, const urcco_rec_clause* clauses, int32_t n_clauses,
                              const int64_t* excl_row_ptr, const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order,
                              int32_t num, int32_t flags, int32_t* out_count, int32_t* out_idx, double* out_score, int64_t* stats_dev,
                              const urcco_rec_rule* rules, int32_t n_rules);

/* urcco_dev_recommend_rules with per-term weights (DESIGN.md decision D20).  A clause c may carry a weight array w_c[h], one unsigned 32-bit integer per
 * column h of I_c, in units of 2^-15; valid values are 1 .. URCCO_REC_WEIGHT_MAX (32.0), URCCO_REC_WEIGHT_ONE is 1.0.
 *   M_c(q, i)   = sum over h in T_c(q) ^ I_c(i) of w_c[h]                                      exact integer
 *   score(q, i) = ((0.0 + boost_0 ((double)M_0 2^-15)) + boost_1 ((double)M_1 2^-15)) + ...    f64, clauses in call order, no contraction
 * The weights are accumulated with integer atomics and folded into the f64 score once per clause: ids and score bits stay reproducible bit for bit whatever
 * the order of the hits.  A clause without an array (a NULL entry) behaves as w = URCCO_REC_WEIGHT_ONE throughout, and (double)(m 2^15) 2^-15 == m exactly:
 * clause_weights == NULL, all entries NULL, or arrays that hold URCCO_REC_WEIGHT_ONE alone give the counts, ids, score bits and statistics of
 * urcco_dev_recommend_rules.  Weights are >= 1, so an item has a positive score exactly when it has one there: eligibility, exclusions, the mask, the rules,
 * the backfill, URCCO_REC_NO_BACKFILL and the total order (score desc, backfill position asc) are those of urcco_dev_recommend_rules.
 * No counter overflows: a query whose work bound w(q) is at most 3072 runs on 32-bit counters and has at most 3072 hits, so M <= 3072 * 2^20 < 2^32; every
 * other query counts in 64 bits (24 instead of 20 bytes of scratch per item and resident block).  That the values lie in 1 .. URCCO_REC_WEIGHT_MAX is the
 * caller's duty, like fill_order being a permutation; the kernel clamps every weight it loads into that range (0 counts as 1, anything larger as the
 * maximum), so a bad array gives other scores but cannot overflow a counter.  URCCO_BAD_ARG: as urcco_dev_recommend_rules. */
#define URCCO_REC_WEIGHT_ONE (1 << 15)
#define URCCO_REC_WEIGHT_MAX (1 << 20)
int urcco_dev_recommend_weighted(urcco_session* s, int64_t n_queries, int32_t n_items, const urcco_rec_clause* clauses, int32_t n_clauses,
                                 const int64_t* excl_row_ptr, const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order,
                                 int32_t num, int32_t flags, int32_t* out_count, int32_t* out_idx, double* out_score, int64_t* stats_dev,
                                 const urcco_rec_rule* rules, int32_t n_rules,
                                 const uint32_t* const* clause_weights /* nullable: HOST array [n_clauses] of device pointers [clause.n_cols], entries nullable */);

/* Term weights by rarity for urcco_dev_recommend_weighted: for column h of a CSC, df = ind_col_ptr[h + 1] - ind_col_ptr[h] (a df above n_docs counts as n_docs),
 *   idf = log(1 + (n_docs - df + 0.5) / (df + 0.5))   in f64 -- Lucene's BM25 idf, the term-rarity half of what the reference's Elasticsearch index computes;
 *   out_weight[h] = clamp(llrint(idf * 2^15), 1, URCCO_REC_WEIGHT_MAX); a column nothing lists (df == 0) gets 1.
 * BM25's length norm and per-shard statistics are not part of it.  n_docs is the caller's document count (Elasticsearch's: the items whose field is not empty).
 * Enqueues on the session's stream.  URCCO_BAD_ARG: n_cols < 0, n_docs < 1, a NULL array with n_cols > 0. */
int urcco_dev_idf_weights(urcco_session* s, int32_t n_cols, const int64_t* ind_col_ptr /* device, n_cols + 1 */, int64_t n_docs,
                          uint32_t* out_weight /* device, [n_cols] */);

/* Hold-out evaluation of a table of recommendations: hits, average precision and NDCG at up to URCCO_EVAL_MAX_KS cut-offs per query, and their sums over
 * the queries -- the arithmetic of the reference's MAP@k tool (the query key `eventNames` exists "for indicator predictiveness testing with the MAP@k
 * tool"; URAlgorithm.scala:401), without leaving the device.  DESIGN.md decision D19.  For query q:
 *   c = min(max(rec_count[q], 0), num), r_j = rec_idx[q * num + j] for j < c -- nothing at or behind c is read; the entries are distinct (the caller's
 *       duty, urcco_dev_recommend's guarantee), a repeated entry counts each time
 *   T = the truth row (sorted unique, e.g. a history term row), t = |T|; rel_j = 1 iff r_j is in T (binary search); H(j) = rel_0 + ... + rel_j
 *   for each k of ks, m = min(k, c):
 *     hits[q, k] = H(m - 1), 0 when m = 0
 *     ap[q, k]   = (sum over j < m with rel_j = 1 of (double)H(j) / (double)(j + 1)) / (double)min(k, t)
 *     dcg[q, k]  = sum over j < m with rel_j = 1 of discount[j];   ideal[n] = discount[0] + ... + discount[n - 1];   ndcg[q, k] = dcg / ideal[min(k, t)]
 *   every sum starts at 0.0 and runs in ascending j: one rounding per division and per add, no contraction.  The caller supplies the position weights
 *   (1 / log2(j + 2) for the usual NDCG); the library never evaluates a logarithm.
 *   t = 0: the query is NOT evaluated -- its outputs are 0 / 0.0 and it is counted in out_sums_i[1].
 * Sums, kappa = the index of k in ks:
 *   out_sums_i = [queries evaluated, queries not evaluated, sum_q hits[q, kappa] per kappa, #{q: hits[q, kappa] > 0} per kappa]
 *   out_sums_f = [tree(ap[., kappa]) per kappa, tree(ndcg[., kappa]) per kappa]  (the second half zeros without discount)
 *   tree(x) over all n_queries positions (not-evaluated ones hold +0.0): pad with +0.0 to the next power of two, then x[i] = x[2i] + x[2i + 1] until one
 *   value is left -- in numpy `while x.size > 1: x = x[0::2] + x[1::2]`.  Every number is reproducible bit for bit; no float atomics are used.
 * urcco_dev_tree_sum: out[c] = tree(x[., c]) for a row-major x [n, n_cols] -- the sums of per-query values gathered over several calls do not depend
 *   on how the queries were split into calls.  n = 0 gives 0.0.
 * Both enqueue on the session's stream and do not synchronise; scratch from the session's arena.  URCCO_BAD_ARG (rank_metrics): num outside
 * 1..URCCO_REC_MAX_NUM, n_ks outside 1..URCCO_EVAL_MAX_KS, ks not strictly ascending or a k outside 1..num, n_queries * n_ks >= 2^31, a NULL array the call
 * needs, discount / out_ndcg or out_sums_i / out_sums_f not both NULL or both non-NULL; (tree_sum): n < 0, n_cols outside 1..1024, n * n_cols >= 2^31, a NULL.
 * n_queries == 0 is legal and writes zero sums.  ABI: additions within ABI 305 -- the presence of the symbols is the feature test. */
#define URCCO_EVAL_MAX_KS 8
int urcco_dev_rank_metrics(urcco_session* s, int64_t n_queries, int32_t num,
                           const int32_t* rec_count, const int32_t* rec_idx,             /* device, as urcco_dev_recommend leaves them: rows strided by num */
                           const int64_t* truth_row_ptr, const int32_t* truth_col_idx,   /* device CSR, n_queries rows, sorted unique */
                           const int32_t* ks_host, int32_t n_ks,                         /* host: strictly ascending, each in 1..num */
                           const double* discount,                                       /* device [num], nullable */
                           int32_t* out_hits, double* out_ap, double* out_ndcg,          /* device [n_queries * n_ks], row-major by query; out_ndcg NULL iff discount NULL */
                           int64_t* out_sums_i, double* out_sums_f);                     /* device, nullable pair: [2 + 2 * n_ks], [2 * n_ks] */
int urcco_dev_tree_sum(urcco_session* s, int64_t n, int32_t n_cols, const double* x /* device [n * n_cols] */, double* out /* device [n_cols] */);

/* Device-resident user history: the event-store half of a batch of queries (getBiasedRecentUserActions, URAlgorithm.scala:795-839; getExcludedItems,
 * :741-767), from event streams that already sit in HBM -- (user id, column id, time) per event and event type, dense ids as urcco_dev_dictionary_lookup
 * yields them.  DESIGN.md decision D17.  For a query user u and event type e with cap max_items (the indicator's maxItemsPerUser):
 *   events of u    the stream positions p of e's stream with users[p] == u; positions with users[p] < 0 (or >= n_users) belong to nobody
 *   recency        the order (times_ms[p] desc, p desc): of two events with equal time the later stream position is the more recent (the reference
 *                  leaves ties to the event store, `latest = true`, :809 -- this tie-break is this library's); times_ms == NULL: stream order is time order
 *   window         the first min(n_u, max_items) events in that order.  Events with items[p] < 0 (an item outside the column dictionary) COUNT toward the
 *                  cap and contribute no column: the reference counts `items.size` before any lookup (:830)
 *   term row       the distinct items[p] of the window, ascending -- the form urcco_rec_clause.q_col_idx and the ANY / NONE rule rows need; duplicates
 *                  inside the window make the row shorter than the cap (`distinct` after the cut)
 *   exclusion row  of a query: the union over the event types flagged `blacklist` of col_map_e[items[p]] over ALL events of u (no cap, :743-752), united with
 *                  the query's row of the caller's extra exclusion CSR (blacklistItems, the query item, the item set); ascending, distinct; entries outside
 *                  0..n_items are dropped.  col_map_e (NULL = identity) maps e's column ids to the primary's item ids, -1 where the primary has none
 *   unknown user   q_users[q] < 0 or >= n_users: empty term rows, the exclusion row is the extra row alone
 * Everything is integer and the order is total: the rows are bit-identical from run to run, whatever order the index build's scatter produced.
 *
 * urcco_dev_history_index: out_pos[out_row_ptr[u] .. out_row_ptr[u + 1]) = the stream positions p with users[p] == u, order unspecified.
 * urcco_dev_history_append (DESIGN.md decision D21): the index of a stream that grew by a batch, from the old index and the batch's users alone.  The old
 *   index (old_row_ptr [n_users_old + 1], old_pos) covers the stream positions 0 .. n_old; new_users[p] is the user of position n_old + p, p = 0 .. n_new;
 *   n_users >= n_users_old is the user id space after the append.  The result is an index of the concatenated stream in the sense of _index: for every
 *   user u the segment out_pos[out_row_ptr[u] .. out_row_ptr[u + 1]) holds FIRST u's old segment in its old order (empty for u >= n_users_old), THEN the
 *   positions n_old + p with new_users[p] == u in unspecified order.  new_users[p] < 0 or >= n_users belongs to nobody.  out_row_ptr / out_pos must not
 *   overlap old_row_ptr / old_pos (the old segments are copied at their new offsets; nothing else of the old index is read, no `users` array of the old
 *   stream is needed).  n_new == 0 with n_users > n_users_old extends the id space only; n_old == 0, n_users_old == 0 with NULL old arrays is _index of
 *   the batch.  old_row_ptr is needed when n_users_old > 0, old_pos when also n_old > 0, new_users when n_new > 0, out_pos when anything is written.
 *   URCCO_BAD_ARG: n_old + n_new >= 2^31, n_users < n_users_old, a negative count, a NULL the call needs.
 * urcco_dev_history_trim (DESIGN.md decision D22): a stream and its index without the events older than a cut-off and without the events of listed users,
 *   from the stream and the index alone.
 *   dropped by time   the event at stream position p when times_ms != NULL and times_ms[p] < min_time_ms: a signed compare, equality keeps the event,
 *                     INT64_MIN keeps everything; min_time_ms is read only when times_ms != NULL
 *   dropped by user   an event that an index entry of a user listed in drop_users names.  The ids may come in any order and may repeat; an id < 0 or
 *                     >= n_users is ignored
 *   nobody's events   a position that no index entry names is kept or dropped by the time rule alone: nothing reads it, and no `users` array exists to
 *                     decide otherwise
 *   stream output     K = the number of kept events, new_of[p] = the number of kept positions below p: out_items[0 .. K) and out_times[0 .. K) are the
 *                     kept events in stream order
 *   index output      KE = the number of kept index entries among the n_e = min(idx_row_ptr[n_users], n_events) entries (n_e is read on the device):
 *                     out_pos[0 .. KE) are the kept entries in their old order, each renumbered to new_of[idx_pos[e]]; out_row_ptr[u] = the number of
 *                     kept entries below idx_row_ptr[u].  So every user's segment is its old segment with the dropped entries removed and the order
 *                     kept; the id space does not change, a dropped user keeps its id and has an empty segment
 *   counts            out_counts[0] = K, out_counts[1] = KE
 *   capacities        nothing is written at or past out_items[K], out_times[K], out_pos[KE] or out_row_ptr[n_users + 1]; a caller that does not know K
 *                     sizes the three arrays by n_events.  out_* must not overlap the inputs: the compaction is not in place
 *   malformed index   entries of idx_pos outside 0 .. n_events count as dropped, row starts are clamped into 0 .. n_e; whatever idx_row_ptr and idx_pos
 *                     hold, the result may be wrong, but no access leaves the arrays
 *   URCCO_BAD_ARG: n_events >= 2^31, a negative count, n_users > 0x7ffffff0, a NULL the call needs, out_times and times_ms not NULL together.  Needed:
 *   items, idx_pos, out_items and out_pos only when n_events > 0; idx_row_ptr when n_users > 0; drop_users when n_drop > 0; out_row_ptr and out_counts always.
 * urcco_dev_history_cap (DESIGN.md decision D27): urcco_dev_history_trim with a bound on the events a user keeps.  The arguments are the trim's plus
 *   max_per_user; every rule, output, capacity and malformed-index guarantee of the trim holds unchanged, and one rule is added:
 *   dropped by cap    the valid index entries of user u are those of its segment (row starts clamped as the trim clamps them) with
 *                     0 <= idx_pos[e] < n_events.  The recency key of an entry is the rows': (times_ms[p] ^ sign bit, p) compared as unsigned, p alone
 *                     when times_ms == NULL.  The event an entry names is dropped when the entry's key is not among the max_per_user largest keys of
 *                     u's valid entries.  Keys are unique, so the order is total: the result is reproducible bit for bit and does not depend on the
 *                     order inside a segment
 *   kept events       an event is kept iff it passes the time rule, is not a listed user's and passes the cap rule.  The three rules are independent:
 *                     each is decided on the stream as it is passed in.  The time rule removes a suffix of every user's recency order, so cap-then-time
 *                     equals time-then-cap: one call with all three rules gives what a call with the cap alone and a call with the other two give,
 *                     in either order
 *   nobody's events   a position that no index entry names follows the time rule alone, as in the trim
 *   no cap            max_per_user == INT32_MAX: the outputs are bit-identical to urcco_dev_history_trim's with the same other arguments (the same
 *                     kernels are launched)
 *   classes           by the entries m of the user's segment, chosen on the device: m <= max_per_user nothing (two row starts are read); m <= 64 one
 *                     wave ranking the keys in registers; m <= 4096 one block, the threshold = the max_per_user-th largest key by a radix select
 *                     over keys in LDS; larger the same with the keys re-read from global memory per discriminating digit.  No sort of a user's events
 *   malformed index   entries outside 0 .. n_events take no part in the ranking and drop nothing; duplicated positions may give a wrong result; no
 *                     access leaves the arrays
 *   URCCO_BAD_ARG: max_per_user < 1, and the trim's refusals.
 * urcco_dev_history_users /urcco_dev_history_matrix (DESIGN.md decision D23): the Preparator's output -- which users train, and one event type's user x
 *   column matrix with sorted, duplicate-free rows -- from the stream and the index alone; no `users` array exists after an append or a trim.
 *   window            the event at stream position p is in the window when times_ms == NULL, or when t_lo <= times_ms[p] and (t_hi == INT64_MAX or
 *                     times_ms[p] < t_hi): signed compares, the start inclusive, the end exclusive as in urcco_dev_pop_counts, INT64_MAX = no end.  With
 *                     times_ms == NULL any window other than (INT64_MIN, INT64_MAX) is URCCO_BAD_ARG
 *   _users            c[u] = the number of u's index entries whose position is in the window, whatever item the event carries (the Preparator's
 *                     minEventsPerUser counts events).  out_row_of[u] = the number of users v < u with c[v] >= min_events when c[u] >= min_events, else
 *                     -1; out_n_rows[0] = the number of kept users.  The counting is balanced by index entries, not by users: one user may own a
 *                     quarter of the stream
 *   _matrix           row row_of[u] of the result holds the distinct items[p], ascending, with 0 <= items[p] < n_cols, over u's index entries whose p is
 *                     in the window.  row_of == NULL is the identity and needs n_rows == n_users.  A user with row_of[u] < 0 contributes nothing, one
 *                     with row_of[u] >= n_rows is ignored; a row that no user names is empty.  That row_of ascends over the users it keeps and names no
 *                     row twice is the caller's duty (_users' output does).  out_row_ptr and out_col_idx[0 .. nnz) are then, bit for bit, the arrays
 *                     urcco_dev_csr_from_pairs gives for the pairs (row_of[user], item) of the kept events; out_nnz[0] = nnz = out_row_ptr[n_rows]
 *   capacity          the raw entries of a user are its index segment, so idx_row_ptr is the prefix of the rows' upper bounds: user u's row is written iff
 *                     idx_row_ptr[u + 1] <= capacity (the bound of its END, over ALL users below it, kept or not); every other row is left empty.
 *                     Nothing is written at or past out_col_idx[capacity] or out_row_ptr[n_rows + 1].  A caller that sizes by n_events never loses a row
 *   classes           by the raw entries m of the user: m <= 64 one wave, m <= 4096 one block sorting in LDS, larger a column bitmap of ceil(n_cols / 32)
 *                     words in arena scratch per block of that class -- one atomic bit set per kept entry, one walk over the words, no sort.  The
 *                     bitmaps of one call take at most 8 MiB (64 blocks at most; one block when a single bitmap is larger than that)
 *   malformed index   entries of idx_pos outside 0 .. n_events are dropped, row starts are clamped into 0 .. min(idx_row_ptr[n_users], n_events); whatever
 *                     idx_row_ptr, idx_pos and row_of hold, the result may be wrong, but no access leaves the arrays
 *   URCCO_BAD_ARG: n_events >= 2^31, a negative count or capacity, n_users or n_rows > 0x7ffffff0, min_events < 1, n_cols < 1, a window without times_ms,
 *   row_of == NULL with n_rows != n_users, a NULL the call needs.  Needed: idx_pos (and items) only when n_events > 0; idx_row_ptr (and out_row_of) when
 *   n_users > 0; out_col_idx when capacity > 0; out_n_rows, out_row_ptr and out_nnz always.
 * urcco_dev_history_bounds: term_row_ptr of every type and excl_row_ptr receive the exclusive scans of upper bounds of the rows' lengths (min(n_u, max_items);
 *   blacklist events + extra row).  The caller reads the 1 + n_types totals (term_row_ptr[n_queries], excl_row_ptr[n_queries]: its one synchronisation),
 *   allocates term_col_idx / excl_col_idx of at least that many entries and states the sizes in term_capacity / excl_capacity.
 * urcco_dev_history_rows: the same arguments, the row_ptr arrays as _bounds left them; on return they hold the final row starts and the col_idx arrays
 *   the rows.  A capacity below a bound total: a row is written iff its bound ENDS within the capacity (row_ptr[q + 1] as _bounds left it <= capacity);
 *   every other row of that array -- all rows behind the first one cut, those of bound 0 included -- is left empty and counted in stats[6], and
 *   stats[0..5] count the written rows only.  Nothing is written at or past col_idx[capacity].
 * stats_dev (nullable, int64[URCCO_HIST_STATS_LEN]): (query, type) pairs served by [0] the wave class (<= 64 events), [1] the block class (<= 4096, keys in
 *   LDS), [2] the global class; [3] pairs that ran the select (n_u > max_items); exclusion rows built by [4] one wave, [5] one block; [6] rows dropped
 *   for lack of capacity (0 when the caller sized its buffers by the bounds); [7] 0.
 * All eight enqueue on the session's stream and do not synchronise; scratch from the session's arena.  URCCO_BAD_ARG: n_events >= 2^31, n_types outside
 * 1..URCCO_REC_MAX_CLAUSES, max_items < 1, n_queries * (n_types + 1) >= 2^31, a NULL the call needs, a half-NULL extra pair, a negative capacity.
 * ABI: additions within ABI 305 -- the presence of the symbols is the feature test. */
#define URCCO_HIST_STATS_LEN 8
int urcco_dev_history_index(urcco_session* s, int64_t n_events, const int32_t* users, int64_t n_users,
                            int64_t* out_row_ptr /* [n_users + 1] */, int32_t* out_pos /* capacity n_events */);
int urcco_dev_history_append(urcco_session* s,
                             int64_t n_old,                      /* events the old index covers: stream positions 0 .. n_old */
                             int64_t n_users_old, const int64_t* old_row_ptr /* [n_users_old + 1] */, const int32_t* old_pos,
                             int64_t n_new, const int32_t* new_users,        /* users of stream positions n_old .. n_old + n_new */
                             int64_t n_users,                                /* >= n_users_old: the id space after the append */
                             int64_t* out_row_ptr /* [n_users + 1] */, int32_t* out_pos /* capacity n_old + n_new */);
int urcco_dev_history_trim(urcco_session* s,
                           int64_t n_events, const int32_t* items, const int64_t* times_ms /* nullable */,
                           int64_t n_users, const int64_t* idx_row_ptr /* [n_users + 1] */, const int32_t* idx_pos,
                           int64_t min_time_ms,                          /* read only when times_ms != NULL */
                           int64_t n_drop, const int32_t* drop_users,    /* device; nullable iff n_drop == 0 */
                           int32_t* out_items, int64_t* out_times /* NULL iff times_ms NULL */,
                           int64_t* out_row_ptr /* [n_users + 1] */, int32_t* out_pos,
                           int64_t* out_counts /* device [2] */);
int urcco_dev_history_cap(urcco_session* s,
                          int64_t n_events, const int32_t* items, const int64_t* times_ms /* nullable */,
                          int64_t n_users, const int64_t* idx_row_ptr /* [n_users + 1] */, const int32_t* idx_pos,
                          int64_t min_time_ms,                          /* read only when times_ms != NULL */
                          int64_t n_drop, const int32_t* drop_users,    /* device; nullable iff n_drop == 0 */
                          int32_t max_per_user,                         /* >= 1; INT32_MAX = no cap */
                          int32_t* out_items, int64_t* out_times /* NULL iff times_ms NULL */,
                          int64_t* out_row_ptr /* [n_users + 1] */, int32_t* out_pos,
                          int64_t* out_counts /* device [2] */);
/* which users train, and under which row number */
int urcco_dev_history_users(urcco_session* s, int64_t n_events, const int64_t* times_ms /* nullable */,
                            int64_t n_users, const int64_t* idx_row_ptr /* [n_users + 1] */, const int32_t* idx_pos,
                            int64_t t_lo, int64_t t_hi, int32_t min_events,
                            int32_t* out_row_of /* [n_users] */, int64_t* out_n_rows /* device [1] */);
/* one event type's user x column matrix */
int urcco_dev_history_matrix(urcco_session* s, int64_t n_events, const int32_t* items, const int64_t* times_ms /* nullable */,
                             int64_t n_users, const int64_t* idx_row_ptr /* [n_users + 1] */, const int32_t* idx_pos,
                             int64_t t_lo, int64_t t_hi, int32_t n_cols,
                             const int32_t* row_of /* nullable: identity, n_rows == n_users */, int64_t n_rows,
                             int64_t* out_row_ptr /* [n_rows + 1] */, int32_t* out_col_idx, int64_t capacity,
                             int64_t* out_nnz /* device [1] */);

typedef struct urcco_hist_event {
  int32_t n_cols, max_items;          /* max_items >= 1 */
  int32_t blacklist, reserved;        /* != 0: this type's events feed the exclusion rows */
  const int64_t* idx_row_ptr; const int32_t* idx_pos;   /* urcco_dev_history_index of this stream */
  const int32_t* items;               /* the stream: dense column id per event, < 0 = no column */
  const int64_t* times_ms;            /* nullable: stream order is time order */
  const int32_t* col_map;             /* nullable (identity): [n_cols] -> primary item id or -1 */
  int64_t* term_row_ptr;              /* [n_queries + 1]: bounds after _bounds, final after _rows */
  int32_t* term_col_idx;              /* _rows: capacity term_capacity; _bounds does not read it */
  int64_t term_capacity;              /* _rows: entries of term_col_idx, >= the bound total the caller read after _bounds */
} urcco_hist_event;

int urcco_dev_history_bounds(urcco_session* s, int64_t n_queries, const int32_t* q_users, int64_t n_users, urcco_hist_event* events, int32_t n_types,
                             const int64_t* extra_row_ptr, const int32_t* extra_col_idx /* nullable pair */, int64_t* excl_row_ptr /* [n_queries + 1] */);
int urcco_dev_history_rows(urcco_session* s, int64_t n_queries, const int32_t* q_users, int64_t n_users, urcco_hist_event* events, int32_t n_types,
                           const int64_t* extra_row_ptr, const int32_t* extra_col_idx, int32_t n_items,
                           int64_t* excl_row_ptr, int32_t* excl_col_idx, int64_t excl_capacity, int64_t* stats_dev /* nullable */);

/* Backfill ranks from the resident history (DESIGN.md decision D24): PopModel.calcPopular / calcTrending / calcHot (PopModel.scala:113-179) over event streams
 * that sit in HBM instead of PEventStore.find, and the order the reference's query sort gives the backfill (buildQuerySort, URAlgorithm.scala:730-738).
 *
 * urcco_dev_history_ranks: out_rank[i] for every item i of the primary's dictionary.  With D = t_end - t_start the intervals are
 *   popular    one,   [t_start, t_end)
 *   trending   two,   [t_start, t_start + D / 2) and [t_start + D / 2, t_end)                                           D / 2: integer division
 *   hot        three, [t_start, t_start + D / 3), [t_start + D / 3, t_start + 2 (D / 3)) and [t_start + 2 (D / 3), t_end)
 *   -- what urcco_dev_pop_counts is given by universal-recommender_amd/pop_model.py.  Signed compares, the start inclusive, the end exclusive;
 *   t_end == INT64_MAX: the last interval has no end, as in urcco_dev_history_users.
 *   counted    position p of a stream counts for item i when c = items[p] lies in 0 .. n_cols and i = col_map ? col_map[c] : c lies in 0 .. n_items, in the
 *              interval b that holds times_ms[p].  The counts add over all streams (one stream listed twice counts twice).  No index is read: every stream
 *              position counts, whoever its user is, as every event of the store does in the reference.  times_ms == NULL: every position is in interval 0
 *   ranks      popular  c0 > 0 ? c0 : URCCO_RANK_NONE;  trending  c0 > 0 && c1 > 0 ? c1 - c0 : NONE;  hot  c0, c1, c2 > 0 ? (c2 - c1) - (c1 - c0) : NONE
 *              (c0 the oldest interval): the reference's joins; exact integers, the values its doubles hold
 *   out_counts nullable: counts[b * n_items + i], n_intervals = type
 *   URCCO_BAD_ARG: type outside 1..3; n_streams outside 0..URCCO_RANK_MAX_STREAMS (0 is legal: every item NONE); t_end < t_start; trending or hot with a D
 *   beyond 64 bits; a stream without times_ms unless the call is popular over the open window (INT64_MIN, INT64_MAX); streams whose n_events sum to 2^31 or
 *   more; 3 * n_items (or 3 * n_cols of a stream with a col_map) beyond what urcco_dev_pop_counts accepts; a negative size; NULL items with n_events > 0;
 *   NULL out_rank with n_items > 0.
 * urcco_dev_fill_order: out_order = the permutation of 0 .. n_items sorted by the tuple (field 0, field 1, ..., item id ascending); within a field the larger
 *   rank first and URCCO_RANK_NONE last (Elasticsearch sorts a missing field last).  Every int64 other than INT64_MIN is a rank.  One field: the order
 *   DeviceModel.from_indicators(ranks=...) builds.  n_fields == 0: the identity.  n_items == 0: nothing is done.  The same pointer may be given twice.
 *   A stable radix sort, reproducible bit for bit (csrc/cco_ranks.h).  URCCO_BAD_ARG: n_fields outside 0..URCCO_RANK_MAX_FIELDS, a NULL field, NULL out_order
 *   with n_items > 0, a negative n_items.
 * Both enqueue on the session's stream and do not synchronise; scratch from the session's arena.
 * ABI: additions within ABI 305 -- the presence of the symbols is the feature test. */
#define URCCO_RANK_POPULAR 1
#define URCCO_RANK_TRENDING 2
#define URCCO_RANK_HOT 3
#define URCCO_RANK_NONE INT64_MIN        /* the item has no rank in this field */
#define URCCO_RANK_MAX_STREAMS 16
#define URCCO_RANK_MAX_FIELDS 4
typedef struct urcco_rank_stream {
  int64_t n_events;
  const int32_t* items;      /* device: column id per stream position, as urcco_hist_event.items */
  const int64_t* times_ms;   /* device, nullable */
  const int32_t* col_map;    /* device, nullable (identity): [n_cols] -> primary item id or -1, as urcco_hist_event.col_map */
  int32_t n_cols, reserved;
} urcco_rank_stream;
int urcco_dev_history_ranks(urcco_session* s, const urcco_rank_stream* streams /* host */, int32_t n_streams, int32_t n_items, int32_t type, int64_t t_start, int64_t t_end,
                            int64_t* out_rank /* device [n_items] */, int32_t* out_counts /* device, nullable: [n_intervals * n_items] */);
int urcco_dev_fill_order(urcco_session* s, int32_t n_items, const int64_t* const* ranks /* host array of n_fields device pointers, each [n_items] */, int32_t n_fields,
                         int32_t* out_order /* device [n_items] */);

/* Device-resident item queries: the model half of a batch of item queries ("people who liked this also liked": getBiasedSimilarItems,
 * URAlgorithm.scala:770-792), cut from the indicator matrices where the build left them in HBM.  DESIGN.md decision D18.  For query q with item
 * i = q_items[q] and event type e with cap max_terms (the reference's maxQueryEvents):
 *   row            ind_col_idx[ind_row_ptr[i] .. ind_row_ptr[i + 1]) in stored order (strongest first for an ordered build), of length n
 *   window         all n entries when n <= max_terms, otherwise the first max_terms - 1 (the reference's `slice(0, maxQueryEvents - 1)`, :782);
 *                  max_terms == 1 with n > 1 therefore gives an empty window.  An entry outside 0..n_cols COUNTS toward the cut and contributes no column
 *   term row       the distinct columns of the window, ascending -- the form urcco_rec_clause.q_col_idx and the ANY / NONE rule rows need; duplicates
 *                  inside a row are legal (a model may be loaded from a caller's matrix) and make the term row shorter than the window
 *   unknown item   q_items[q] < 0 or >= n_items: empty rows
 * Exclusion rows stay with the caller: the query item (unless returnSelf) and blacklistItems are known on the host.
 * Everything is integer: the rows are bit-identical from run to run.
 *
 * urcco_dev_item_bounds: term_row_ptr of every type receives the exclusive scan of the window lengths, upper bounds of the rows' lengths.  The caller reads
 *   the n_types totals (term_row_ptr[n_queries]: its one synchronisation), allocates term_col_idx of at least that many entries and states the size in
 *   term_capacity.
 * urcco_dev_item_rows: the same arguments, the row_ptr arrays as _bounds left them; on return they hold the final row starts and the col_idx arrays
 *   the rows.  A capacity below a bound total: a row is written iff its bound ENDS within the capacity (row_ptr[q + 1] as _bounds left it <= capacity);
 *   every other row of that array -- all rows behind the first one cut, those of bound 0 included -- is left empty and counted in stats[6], and
 *   stats[0..5] count the written rows only.  Nothing is written at or past col_idx[capacity].
 * stats_dev (nullable, int64[URCCO_HIST_STATS_LEN]): (query, type) pairs served by [0] the wave class (window <= 64 entries), [1] the block class
 *   (<= 4096, sorted in LDS), [2] the global class; [3] pairs whose row was cut (n > max_terms); [6] rows dropped for lack of capacity (0 when the caller
 *   sized its buffers by the bounds); every other entry 0.
 * Both enqueue on the session's stream and do not synchronise; scratch from the session's arena.  URCCO_BAD_ARG: n_types outside
 * 1..URCCO_REC_MAX_CLAUSES, max_terms < 1, n_cols < 0, n_queries * n_types >= 2^31, a NULL the call needs, a negative capacity.
 * ABI: additions within ABI 305 -- the presence of the symbols is the feature test. */
typedef struct urcco_item_event {
  int32_t n_cols, max_terms;          /* max_terms >= 1: the reference's maxQueryEvents */
  const int64_t* ind_row_ptr;         /* device: indicator CSR of this event type, n_items rows, as the build leaves it */
  const int32_t* ind_col_idx;         /* order inside a row = stored order (strongest first for an ordered build) */
  int64_t* term_row_ptr;              /* [n_queries + 1]: bounds after _bounds, final after _rows */
  int32_t* term_col_idx;              /* _rows: capacity term_capacity; _bounds does not read it */
  int64_t term_capacity;              /* _rows: entries of term_col_idx, >= the bound total the caller read after _bounds */
} urcco_item_event;

int urcco_dev_item_bounds(urcco_session* s, int64_t n_queries, const int32_t* q_items, int32_t n_items, urcco_item_event* events, int32_t n_types);
int urcco_dev_item_rows(urcco_session* s, int64_t n_queries, const int32_t* q_items, int32_t n_items, urcco_item_event* events, int32_t n_types,
                        int64_t* stats_dev /* nullable */);

/* Device-resident item properties (DESIGN.md decision D25): what the reference reads with PEventStore.aggregateProperties(entityType = "item")
 * (DataSource.scala:93-97) and indexes next to the indicators -- here aggregated on the device from the $set / $unset / $delete events where they arrive,
 * so that a serving model takes an inventory change without a rebuild.  One property is one stream of $set and $unset events (item, time, and per $set a
 * value: a slice of value ids for a list of strings, an int64 for a date); the $delete events of all items are one more stream.
 *
 * THE RULE (the contract: PredictionIO's per-key comparison of set, unset and delete times).  Per item i and property p, over all events applied so far:
 *   S        the $set of (i, p) with the largest (time, stream position): of two sets with equal time the later one in the stream wins
 *   U, D     the largest time of an $unset of (i, p); the largest time of a $delete of i
 *   alive    S exists and time(S) > U and time(S) > D.  An $unset or a $delete at the millisecond of the set wins the tie
 *   value    that of S alone: a $set replaces the value, lists are not merged
 *   deleted  a $delete of i exists and no property of i has a set later than D.  A later $set of one key revives that key only
 * The rule does not depend on the order of the events: it is exact under any batching and reproducible bit for bit.  An event with time INT64_MIN is
 * ignored (INT64_MIN is "no value", and "nothing seen" below).
 *
 * State, caller-owned, zero-initialised; per property three arrays of n_items words, per store one:
 *   t_set  (uint64)   time of S as (uint64)t ^ 2^63 -- unsigned words that order as the signed times do -- 0 = no $set seen
 *   pos_set (uint32)  stream position of S + 1, 0 = none          t_unset (uint64)  U, biased alike, 0 = none          t_del (uint64)  D, alike
 * All-zero is "nothing seen": a new store is zeros, a grown catalogue is the old state extended by zeros.
 *
 * urcco_dev_props_apply: the events at stream positions pos_base .. pos_base + n_new of one property.  kinds[j] URCCO_PROP_SET or URCCO_PROP_UNSET (any
 *   other value: the event is ignored; kinds == NULL: all SET).  Two launches: t_set / t_unset = max(., time); then every SET whose time equals t_set of
 *   its item: pos_set = max(., pos_base + j + 1).  Each reads the word first and issues the atomic only when the event would raise it.  Stream positions
 *   only grow, so a stream applied in any number of batches leaves the bits one call over the whole stream leaves.  Items outside 0 .. n_items are ignored.
 * urcco_dev_props_delete: t_del = max(., time) over n $delete events.
 * urcco_dev_props_bounds / _rows: a list-of-strings property as an item x value matrix, by the two-call protocol of urcco_dev_history_bounds / _rows.
 *   val_ptr (int64 [state.n_events + 1]) and values (int32 [n_values] value ids) hold the value slice of every stream position (an $unset's is empty).
 *   _bounds  row_ptr = the exclusive scan of the bounds; the bound of item i = the length of S's slice when the property is alive, else 0.  The caller reads
 *            the total row_ptr[n_items] and allocates col_idx.
 *   _rows    row_ptr as _bounds left it; on return row_ptr / col_idx are the CSR whose row i holds the distinct value ids of S's slice, ascending, ids outside
 *            0 .. n_cols dropped: bit for bit what urcco_dev_csr_from_pairs gives for the (item, value id) pairs of the alive winners.  An alive property
 *            set to [] is an empty row.  A row is written iff its bound ENDS within the capacity (row_ptr[i + 1] as _bounds left it <= capacity); every
 *            other row is left empty.  Nothing is written at or past col_idx[capacity].  state.t_del == NULL: no deletes.
 *   Contents of pos_set or val_ptr that name no position / no slice (positions beyond n_events, slice ends outside 0 .. n_values) may give wrong rows,
 *   never an access outside the arrays.  The CSC for boost clauses comes from urcco_dev_column_counts + urcco_dev_transpose.
 * urcco_dev_props_dates: out[i] = date_values[position of S] when the property is alive, else INT64_MIN.  date_values: int64 per stream position.
 * urcco_dev_props_exists: out_mask[i] = 0 iff item i is deleted by the rule over the n_props properties whose t_set arrays are given, else 1; an item
 *   without any event gets 1.  The mask is urcco_dev_recommend's item_mask.
 * urcco_dev_props_compact (DESIGN.md decision D28): one property's stream without the values that no item's state names any more.
 *   winners         the positions pos_set[i] - 1 that lie in 0 .. state.n_events, one per item; K = their number.  Numbered in ascending old position they
 *                   are the new stream: positions keep their relative order, so a later urcco_dev_props_apply with pos_base = K breaks equal-time ties
 *                   exactly as it would have on the uncompacted stream
 *   out_pos_set     [n_items]: the new position + 1; 0 where pos_set[i] was 0 or named no position
 *   out_old_pos     [0 .. K): the old position of every new position -- what the caller gathers its own per-position arrays by
 *   lists           val_ptr != NULL: out_val_ptr[0 .. K] and out_values[0 .. V) hold the winners' slices in new order.  A winner whose property is not
 *                   alive by THE RULE (time(S) <= U or <= D) gets an empty slice: it can never become alive again, because a maximum only grows; its
 *                   position is kept, so that t_set and pos_set stay consistent.  V = out_val_ptr[K]
 *   dates           date_values != NULL: out_date_values[0 .. K) is gathered.  val_ptr and date_values are not given together; with neither, the
 *                   positions alone are compacted
 *   out_counts      device int64 [2] = {K, V} (V = 0 without val_ptr)
 *   untouched       t_set, t_unset and t_del are read to decide "alive" and never written; pos_set is read only
 *   capacities      nothing is written at or past out_old_pos[K], out_val_ptr[K + 1], out_values[V] or out_date_values[K].  K <= min(n_items,
 *                   state.n_events) and V <= n_values: a caller that does not know them sizes by those bounds.  Outputs must not overlap inputs
 *   malformed input slice ends are clamped into 0 .. n_values as _rows clamps them, and the new slice starts into 0 .. n_values (slices that overlap cannot
 *                   make V exceed n_values); two items that name one position keep it once.  The result may be wrong, no access leaves the arrays
 *   The slices are copied balanced by entries, not by items: one winner may hold 8193 values while a million hold two.  Atomics only to mark the winners.
 *   URCCO_BAD_ARG: the state's refusals (below), a negative n_values, val_ptr and date_values together, a NULL the call needs.  Needed: out_counts always;
 *   out_pos_set when n_items > 0; out_old_pos when n_items > 0 and state.n_events > 0; out_val_ptr with val_ptr; values and out_values with val_ptr when
 *   also n_values > 0, n_items > 0 and state.n_events > 0; out_date_values with date_values when n_items > 0 and state.n_events > 0.
 * All seven enqueue on the session's stream and do not synchronise; scratch from the session's arena.  URCCO_BAD_ARG: a negative n_items, n_new, n, n_values,
 * n_cols, capacity or state.n_events; pos_base < 0 or pos_base + n_new >= 2^31; state.n_events >= 2^31; n_props outside 0..URCCO_PROP_MAX; a NULL the call
 * needs.  Needed: items and times_ms when n_new (n) > 0; the state arrays the call names when n_items > 0 (apply: also with n_new == 0); val_ptr when
 * n_items > 0 and state.n_events > 0; values when n_values > 0; col_idx when capacity > 0; date_values when state.n_events > 0; row_ptr always; t_sets and
 * each of its pointers when n_props > 0 and n_items > 0; out / out_mask when n_items > 0.
 * ABI: additions within ABI 305 -- the presence of the symbols is the feature test. */
#define URCCO_PROP_SET 0
#define URCCO_PROP_UNSET 1
#define URCCO_PROP_MAX 16
typedef struct urcco_prop_state {
  const uint64_t* t_set;      /* device [n_items] */
  const uint32_t* pos_set;    /* device [n_items] */
  const uint64_t* t_unset;    /* device [n_items] */
  const uint64_t* t_del;      /* device [n_items], the store's; nullable: no $delete was ever applied */
  int64_t n_events;           /* stream positions of the property applied so far */
} urcco_prop_state;
int urcco_dev_props_apply(urcco_session* s, int32_t n_items, int64_t n_new, const int32_t* items, const int64_t* times_ms, const uint8_t* kinds /* nullable: all SET */,
                          int64_t pos_base, uint64_t* t_set, uint32_t* pos_set, uint64_t* t_unset);
int urcco_dev_props_delete(urcco_session* s, int32_t n_items, int64_t n, const int32_t* items, const int64_t* times_ms, uint64_t* t_del);
int urcco_dev_props_bounds(urcco_session* s, int32_t n_items, const urcco_prop_state* state /* host */, const int64_t* val_ptr, int64_t n_values,
                           int64_t* row_ptr /* [n_items + 1] */);
int urcco_dev_props_rows(urcco_session* s, int32_t n_items, const urcco_prop_state* state /* host */, const int64_t* val_ptr, const int32_t* values, int64_t n_values,
                         int32_t n_cols, int64_t* row_ptr /* [n_items + 1]: bounds on entry, final on return */, int32_t* col_idx, int64_t capacity);
int urcco_dev_props_dates(urcco_session* s, int32_t n_items, const urcco_prop_state* state /* host */, const int64_t* date_values, int64_t* out /* [n_items] */);
int urcco_dev_props_exists(urcco_session* s, int32_t n_items, const uint64_t* t_del, const uint64_t* const* t_sets /* host array of n_props device pointers */,
                           int32_t n_props, uint8_t* out_mask /* [n_items] */);
int urcco_dev_props_compact(urcco_session* s, int32_t n_items, const urcco_prop_state* state /* host */,
                            const int64_t* val_ptr /* nullable: [state.n_events + 1] of a list property */, const int32_t* values, int64_t n_values,
                            const int64_t* date_values /* nullable: [state.n_events] of a date property */,
                            uint32_t* out_pos_set /* [n_items] */, int32_t* out_old_pos /* [K] */,
                            int64_t* out_val_ptr /* [K + 1] */, int32_t* out_values /* [V] */, int64_t* out_date_values /* [K] */,
                            int64_t* out_counts /* device [2]: K, V */);

/* Test hooks (device level): LLR of SimilarityAnalysis.logLikelihoodRatio evaluated by the device code for
 * n argument tuples; u01 of the down-sampling RNG.  All pointers device. */
int urcco_dev_llr(urcco_session* s, int64_t n, const int64_t* with_a, const int64_t* with_b, const int64_t* with_ab,
                  const int64_t* n_users, double* out);
int urcco_dev_u01(urcco_session* s, int64_t n, int32_t seed, const int32_t* row, const int32_t* col, double* out);
int urcco_dev_u01_rng(urcco_session* s, int64_t n, int32_t seed, const int32_t* row, const int32_t* col, int32_t rng /* URCCO_RNG_* */, double* out);

/* ---- DEVICE level: Preparator (reference src/main/scala/Preparator.scala:44-87, :102-158, :160-214) -------------
 * Dictionaries and binary CSR matrices from event streams of 64-bit keys resident in HBM (the host hashes its id
 * strings or passes integer ids; the value ~0, i.e. the integer id -1, is reserved).  Dense ids follow FIRST APPEARANCE in the stream
 * (oracle decision D8), so the host recovers the id -> string dictionary from `first_pos` alone. */
typedef struct urcco_key_table urcco_key_table;

/* Host helper: keys[i] = XXH64(bytes[offsets[i] .. offsets[i + 1]), seed) for n strings laid end to end (UTF-8); the value ~0
 * is remapped to 0 (reserved by the device dictionary).  A few host threads for large n.  The same function with a
 * second seed gives the independent check keys of urcco_dev_dictionary_verify. */
int urcco_hash_strings(const uint8_t* bytes, const int64_t* offsets, int64_t n, uint64_t seed, uint64_t* keys);

/* BiDictionary over keys[0..n): id = rank of the key's first position among the first positions of the keys that
 * occur at least min_count times (`minEventsPerUser` counts RAW events, Preparator.scala:129-132); other keys get no id.
 * select (nullable, device int32[n]): positions with select[p] < 0 do not take part (events of dropped users,
 * Preparator.scala:173-179).  first_pos (device int64, capacity n): first_pos[id] = stream position of the id's first
 * occurrence.  *n_ids is written on the host (the call synchronises the stream).
 * The key ~0 (2^64 - 1: the integer id -1) marks an empty slot of the table and is not a key: if a position that takes part holds it the
 * call returns URCCO_BAD_ARG, the message names the reserved key, no table is handed out and *table stays NULL.  A position masked by
 * select may hold it.  (urcco_dev_dictionary_lookup answers -1 for it, the verify calls skip it.) */
int urcco_dev_dictionary_build(urcco_session* s, int64_t n, const uint64_t* keys, const int32_t* select, int32_t min_count,
                               int64_t* first_pos, urcco_key_table** table, int64_t* n_ids);
/* ids[p] = dense id of keys[p], or -1 (key without id, or select[p] < 0).  No host synchronisation. */
int urcco_dev_dictionary_lookup(urcco_session* s, const urcco_key_table* table, int64_t n, const uint64_t* keys,
                                const int32_t* select, int32_t* ids);
/* Collision check of a dictionary built from 64-bit hashes: check_keys[p] = a SECOND, independent hash of the same string
 * (another seed).  Counts the positions whose check key differs from the check key of their id's first occurrence, i.e. two
 * different strings that the first hash merged into one id (probability ~n^2 / 2^65 per dictionary); *n_mismatch is written
 * on the host (synchronises).  first_pos = the array urcco_dev_dictionary_build filled. */
int urcco_dev_dictionary_verify(urcco_session* s, const urcco_key_table* table, int64_t n, const uint64_t* keys, const int32_t* select,
                                const uint64_t* check_keys, const int64_t* first_pos, int64_t* n_mismatch);
/* The same check for ANOTHER stream looked up in the dictionary (Preparator.scala:173-179: the user keys of a secondary event
 * type against the user dictionary of the primary): dict_check_keys = the check keys of the stream the dictionary was built
 * from (first_pos indexes it).  A secondary-event user string whose 64-bit key collides with a primary user's would otherwise
 * be merged into that user silently. */
int urcco_dev_dictionary_verify_against(urcco_session* s, const urcco_key_table* table, int64_t n, const uint64_t* keys, const int32_t* select,
                                        const uint64_t* check_keys, const uint64_t* dict_check_keys, const int64_t* first_pos, int64_t* n_mismatch);
/* A batch of keys against a LIVE table (DESIGN.md decision D26): the keys the table knows keep their ids, the others get the next ids in order of
 * first appearance in the batch.  The table after build(S0), extend(B1), ..., extend(Bk) answers every lookup as the table of ONE
 * urcco_dev_dictionary_build over S0 ++ B1 ++ ... ++ Bk with min_count = 1; a build with n = 0 yields the empty table to start from.  The table keeps
 * its own id count and the min_count it was built with; an addition within the ABI number: the presence of the symbol is the feature test.
 *   ids       device out [n], nullable: ids[p] = the id of keys[p] after the call, -1 where select[p] < 0
 *   new_pos   device out, capacity n: new_pos[j] = the position within this batch of the first appearance of id n_before + j, for the
 *             *n_ids - n_before new ids -- with the batch's strings the host extends its id -> string list
 *   n_ids     host out: the number of ids after the call (the call synchronises the stream, as the build does)
 * Capacity: before a batch is inserted the table has the smallest power of two >= max(1024, 2 (n_ids + n)) slots, the build's rule over what it could
 * hold afterwards; a table that is too small is rehashed into fresh arrays (device memory for both while the call runs).
 * URCCO_BAD_ARG, the message names the cause, and the table is exactly as it was -- every later lookup and extend behave as if the call had not
 * happened: a selected position holds the reserved key ~0; the table was built with min_count > 1 (its keys without an id cannot be told from new
 * keys); n_ids + n exceeds 2^31 - 1, or n >= 2^32 - 1; a NULL or negative argument.  ids and new_pos are undefined after a refused call.
 * Not served: removing keys. */
int urcco_dev_dictionary_extend(urcco_session* s, urcco_key_table* table, int64_t n, const uint64_t* keys, const int32_t* select, int32_t* ids,
                                int64_t* new_pos, int64_t* n_ids);
/* Frees the table (hipFree: waits for device work still using it). */
void urcco_key_table_destroy(urcco_key_table* table);
/* IndexedDatasetSpark's row assembly: (row id, column id) pairs (pairs with a negative id are skipped) -> binary CSR
 * with sorted, duplicate-free columns (`setQuick(col, 1.0)`, Preparator.scala:146, :205).  out_row_ptr: int64[n_rows + 1],
 * out_col_idx: capacity >= n.  nnz (nullable, host): written after a stream synchronisation when not NULL. */
int urcco_dev_csr_from_pairs(urcco_session* s, int64_t n, const int32_t* rows, const int32_t* cols, int64_t n_rows,
                             int64_t* out_row_ptr, int32_t* out_col_idx, int64_t* nnz);

#ifdef __cplusplus
}
#endif
#endif /* URCCO_H */
