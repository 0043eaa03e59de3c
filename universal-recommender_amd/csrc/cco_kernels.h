// Host-callable launchers of the gfx950 CCO kernels (cco_counts / cco_rowscan / cco_transpose / cco_expand / cco_rows / cco_misc .hip).  Every pointer is a device pointer;
// every launcher only enqueues on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace urcco {

constexpr int NBINS = 7;  // accumulator classes: 0 micro (one wave, <= 64 pairs), 1 wave-LDS (64 thr, 1024 words),
                          // 2 small-block-LDS (256 thr, 4096 words), 3 block-LDS (256 thr, 8192 words),
                          // 4 half-CU-LDS (512 thr, 16384 words), 5 CU-LDS (1024 thr, 32768 words),
                          // 6 multi-pass CU-LDS (rows no single table holds; dense global counters when k > MP_KMAX_HOST)
constexpr int MP_KMAX_HOST = 256;  // largest k the multi-pass class serves (== MP_KMAX in cco_rows.hip)

// Geometry the host side needs for scratch sizing.
constexpr int SCAN_TILE = 2048;          // elements per scan tile (256 threads x 8)
constexpr int DS_TILE = 4096;            // entries per down-sample tile (256 threads x 4 x 4)
constexpr int GLOBAL_BIN_BLOCKS = 128;    // persistent blocks of the global-accumulator kernel (upper bound)
constexpr int BIN_TILE = 1024;           // items per binning tile
constexpr int XLX_TABLE_HOST = 4096;     // entries of the small-integer xLogX table (== XLX_TABLE in cco_device.h)
// The ROW LISTS, in the order they lie in bin_rows: a class (public bin) is one list or a run of consecutive ones, each with a kernel body of its own
// (cco_rows.hip: the binning pass fills them, launch_cco_rows_bin names the kernel of each).  A build that is not split keeps a class in its last list.
enum RowList : int {
  NO_LIST = -1,                                               // an empty indicator row
  LIST_MICRO16, LIST_MICRO32, LIST_MICRO,                     // bin 0: <= 16 / <= 32 pairs and users (four / two rows share a wave), the rest of the class
  LIST_WAVE_P128, LIST_WAVE_P256, LIST_WAVE_U128, LIST_WAVE,  // bin 1: <= 64 users and <= 128 / <= 256 pairs, <= 128 users (the small-row body), the rest
  LIST_BLOCKS_U128, LIST_BLOCKS,                              // bin 2: <= 128 users and <= 512 pairs (the small-row body), the rest
  LIST_BLOCK, LIST_HALF_CU, LIST_CU, LIST_MULTI_PASS,         // bins 3 .. 6
  N_ROW_LISTS
};
// the first list of every public bin: bin b is the lists [first_list(b), first_list(b + 1))
__host__ __device__ constexpr int first_list(int bin) {
  constexpr int first[NBINS + 1] = {LIST_MICRO16, LIST_WAVE_P128, LIST_BLOCKS_U128, LIST_BLOCK, LIST_HALF_CU, LIST_CU, LIST_MULTI_PASS, N_ROW_LISTS};
  return first[bin];
}
constexpr int BIN_COLS_HOST = N_ROW_LISTS + 2 * NBINS + 1;  // int64 per binning tile: rows per list, pairs and users per bin, total pairs
constexpr int BIN_OFF_LEN = N_ROW_LISTS + 1;                // bin_off: the exclusive prefix of the lists' lengths -- list l is bin_rows[bin_off[l] .. bin_off[l + 1])
constexpr int CAND_SLOTS = 64;           // words the row kernels spread their candidate counts over (see CcoArgs::cand)
constexpr int STATS_LEN = 32;            // [0] pairs, then NBINS each of rows / pairs / users / out entries per bin, [1 + 4 NBINS] table overflows,
                                         // [STATS_LEN - 1] rows binned into the micro class's two shared-wave sub-lists (0: the class ran as one list)

// Bits of urcco_session_set_debug / urcco_context_set_debug (include/urcco.h documents them; _lib.py carries the same names and values for the tests, bench.py passes the values).
// SpGEMM row phases switched off (profiling only, results meaningless): the DBG instantiations of the row kernels.
constexpr int32_t DBG_GATHER_ONLY = 1;
constexpr int32_t DBG_NO_LLR = 2;
constexpr int32_t DBG_NO_TOPK = 4;
constexpr int32_t DBG_NO_SELECT = 8;
constexpr int32_t DBG_NO_RANK = 16;
constexpr int32_t DBG_NO_COUNT_GATHER = 512;
// A/B paths of the host level
constexpr int32_t DBG_UNFUSED_EXPAND = 4096;        // every event type prepares its own expand operands
constexpr int32_t DBG_GATHERED_PRIMARY = 8192;      // the primary's CSC from a pass over the whole gathered A' instead of fragments
constexpr int32_t DBG_UNFILTERED_EXCHANGE = 16384;  // several ranks: every row of B is exchanged
constexpr int32_t DBG_SELECT_DELAY = 131072;        // test hook: the first wave of a multi-wave team dawdles before the select histogram
constexpr int32_t DBG_UNPACKED_COUNTS = 1048576;    // B' travels as plain columns, the row kernels gather the counts
// The k11 = 1 prefilter of the packed row kernels (cco_rows.hip).  Neither bit selects the DBG instantiations: the production kernels take them as arguments.
constexpr int32_t DBG_NO_PREFILTER = 8388608;       // every distinct candidate is scored (A/B, and the tests' bit-for-bit comparison)
constexpr int32_t DBG_COUNT_SCORED = 16777216;      // with stage timing on: stats[2 + 4 * NBINS] counts the candidates that were SCORED instead of the distinct ones
// The direct ranking of the packed row kernels (cco_rows.hip, direct_limit).  As above: arguments of the production kernels.
constexpr int32_t DBG_NO_DIRECT_RANK = 33554432;    // every row with more than k valid candidates goes through the select (A/B, and the tests' bit-for-bit comparison)
constexpr int32_t DBG_COUNT_DIRECT = 67108864;      // with stage timing on: stats[2 + 4 * NBINS] counts the ROWS that were ranked directly instead of the candidates
// The micro-shaped body of the one-wave class's small rows (cco_rows.hip, cco_rows_small_kernel).  As above: arguments of the production kernels.
constexpr int32_t DBG_NO_SMALL_WAVE = 134217728;    // the class's sub-lists of small rows stay in the general kernel (A/B, and the tests' bit-for-bit comparison)
constexpr int32_t DBG_COUNT_SMALL_WAVE = 268435456; // with stage timing on: stats[2 + 4 * NBINS] counts the ROWS that ran in that body, + 2^32 per row that took its fallback
// The same body with eight pairs and two users per lane: the one-wave class's rows of <= 128 users that those sub-lists leave, and the small-block class's rows
// of <= 128 users and <= 512 pairs.  As above: arguments of the production kernels.
constexpr int32_t DBG_NO_BLOCK_SMALL_WAVE = 536870912;     // these sub-lists run in the general kernels (A/B, and the tests' bit-for-bit comparison)
constexpr int32_t DBG_COUNT_BLOCK_SMALL_WAVE = 1073741824; // with stage timing on: stats[2 + 4 * NBINS] counts the ROWS of these sub-lists that ran in that body, + 2^32 per row that took its fallback
constexpr int32_t DBG_ROW_KERNELS = DBG_GATHER_ONLY | DBG_NO_LLR | DBG_NO_TOPK | DBG_NO_SELECT | DBG_NO_RANK | DBG_NO_COUNT_GATHER | DBG_SELECT_DELAY;

// The form of a build's expand tables, decided on the device by the scan of the work prefix (launch_expand_prepare / launch_expand_scan).
// *word == 0: narrow.  Otherwise wide, and the bits say why.
constexpr int32_t FORM_WIDE = 1;        // set with every other bit
constexpr int32_t FORM_PS64 = 2;        // B' holds 2^32 entries or more (or no 32-bit row pointers were made): expand_prepare wrote pstart64 itself
constexpr int32_t FORM_TILE = 4;        // a scan tile's sum reached `limit`: the 64-bit prefix cannot be rebuilt from tile bases + low words
constexpr int32_t FORM_PACK = 8;        // *pack_bad != 0: the plain instantiations run, and they read wide tables
constexpr int32_t FORM_HOST = 16;       // the host asked for the plain instantiations (no packed B', or the DBG ones)
constexpr unsigned long long NARROW_LIMIT = 1ull << 32;
struct ExpandForm {
  int32_t* word;               // [1]
  const int32_t* pack_bad;     // nullable: the verdict of launch_pack_counts, final on the stream by the time the scan runs
  int32_t host_wide;           // 1: FORM_HOST
  int32_t host_narrow;         // 1: the host knows every condition of the narrow form holds (cco_rows_impl): the word is set to 0 without the device-side tests
  unsigned long long limit;    // NARROW_LIMIT in production; a test lowers it to drive the wide form at toy size
  long long seed;              // 0 in production: the prefix starts here (a test starts it just below 2^32, so that toy rows straddle the wrap of the narrow form)
};

struct CcoArgs {
  // row lists per bin
  const int32_t* bin_rows;   // item ids grouped by bin
  const int32_t* bin_off;    // [BIN_OFF_LEN] offsets into bin_rows
  // matrices
  const int64_t* a_col_ptr;  // CSC of A': users of item i are entries [a_col_ptr[i], a_col_ptr[i+1])
  // The expand tables come in two forms; *form (ExpandForm) names the one this build holds, and with it the instantiation whose turn it is:
  //   narrow (*form == 0, the PK instantiations): pstart32[p] and the work prefix as 32-bit words modulo 2^32 (wp read as unsigned[cap + 1])
  //   wide   (*form != 0, the plain ones):        pstart64[p] and the work prefix as int64[cap + 1]
  // (pstart64 and work are appended at the end: the fields ahead of them keep the offsets they had)
  const unsigned* pstart32;  // per CSC entry: start of that user's B' row in b_col_idx
  const int64_t* wp;         // per CSC entry (+1): exclusive prefix of B' row lengths over the CSC (a row kernel only ever takes differences inside one item row)
  const int32_t* b_col_idx;
  // Round 6: B' with the column's post-sampling count riding in the spare bits of the column word -- word = col | cB << (32 - count_bits) -- so that a
  // candidate's cB arrives with the pair that claims its accumulator slot instead of through one scattered 2-byte gather per candidate (more than half
  // of the SpGEMM classes' line fills: profiles/r06_fetch_by_phase.txt).  Nullable; used while *form == 0 (every count fits its 32 - key bits -- the
  // pack verdict is folded into the form word -- and the expand tables are narrow).
  const int32_t* b_packed;
  const int32_t* form;       // [1] see ExpandForm
  int32_t pk_known;          // 1: the HOST knows the verdict -- packed words that are good AND narrow tables (cco_rows_impl): *form is not read, one instantiation is launched
  uint32_t b_col_mask;       // b_col_idx[e] & b_col_mask = the column (0xffffffff unless b_col_idx itself holds packed words: the rows a sharded build received)
  const int32_t* cnt_a;
  const int32_t* cnt_b;
  const double* ent_a;       // rowEntropy per item of A
  const unsigned short* cnt_b16;  // 16-bit copy of cnt_b (a quarter of the bytes behind the one gather per candidate); valid while *cnt16_bad == 0
  const int32_t* cnt16_bad;  // [1] number of counts beyond 16 bits (then cnt_b is gathered)
  const double* xlx_n;       // [1] xLogX(N)
  const double* xlx_tab;     // [XLX_TABLE_HOST] xLogX of small integers
  const double* xlx_hi;      // [XLX_TABLE_HOST] xLogX(n_users - d): the k22 term without a logarithm
  const double* col_ent;     // [XLX_TABLE_HOST] columnEntropy of a column with d interactions, for the N of the build (behind xlx_hi in the same allocation)
  int32_t debug;             // DBG_* bits (0 in production); the row kernels read those of DBG_ROW_KERNELS
  long long n_users;
  int32_t n_cols_b;
  int32_t item_lo;
  int32_t exclude_self;
  int32_t k;
  int32_t has_min_llr;
  double min_llr;
  int32_t count_bits;        // packed LDS entry = ((col+1) << count_bits) | count
  int32_t col_bytes;         // bytes needed for a column index of B (1..4): digits of the top-k tie break
  int32_t g_log2;            // lanes cooperating on one user's B row = 1 << g_log2
  int32_t unordered;         // 1: rows carry their top-k set in arbitrary order (no ranking pass)
  // outputs (strided by k)
  int32_t* out_count;
  int32_t* out_idx;
  double* out_llr;
  unsigned long long* err;   // stats[1 + 4 * NBINS]: LDS table overflows (must stay 0)
  unsigned long long* cand;  // nullable [CAND_SLOTS], zero on entry: distinct (row, column) candidates scored, spread over the slots (statistics)
  // global-accumulator scratch (bin 6 when k is beyond the multi-pass class: g_blocks > 0)
  int32_t* g_counts;         // [GLOBAL_BIN_BLOCKS][n_cols_b] zero on entry, zero on exit
  unsigned long long* g_cand_key;  // [GLOBAL_BIN_BLOCKS][n_cols_b]
  int32_t* g_cand_col;       // [GLOBAL_BIN_BLOCKS][n_cols_b]
  int32_t g_blocks;          // > 0: bin 6 runs on the dense global-accumulator kernel with this many resident blocks; 0: multi-pass LDS class
  const int64_t* pstart64;   // the wide form's starts
  const int64_t* work;       // [item_hi - item_lo] the rows' pairs in full (launch_row_work): what the multi-pass class sizes its passes by
  const unsigned short* pf_limit;  // nullable [n_items_a]: mono_limit[cA[i]] (launch_mono_limit, launch_item_entropy) -- the k11 = 1 prefilter of the packed row kernels; null: off
};

hipError_t launch_column_counts(hipStream_t st, int n_cu, const int32_t* col_idx, int64_t nnz, int32_t n_cols, int32_t* counts);
// Atomic-free variant for large matrices: returns 0 scratch bytes when the plain kernel should be used instead
// (small nnz or more than 1024 buckets of 8192 columns).  nnz_dev (nullable): device-side nnz <= nnz.
constexpr int64_t PH_MIN_NNZ = 1 << 20;
int64_t column_counts_scratch_bytes(int64_t nnz, int32_t n_cols);
hipError_t launch_column_counts_partitioned(hipStream_t st, const int32_t* col_idx, int64_t nnz, const int64_t* nnz_dev, int32_t n_cols,
                                            int32_t* counts, char* scratch);

// scans: out[i] = sum_{t<i} in[t], out[n] = total.  tile_sums scratch: ceil(n / SCAN_TILE) + 1 int64.
hipError_t launch_scan_i32(hipStream_t st, const int32_t* in, int64_t n, int64_t* out, int64_t* tile_sums);
// part-local layouts (column counts, transposition): weight[b] = entries of bucket b over all parts, from the transposed slice table loc_t[(n_buckets + 1) x n_parts]
hipError_t launch_slice_weights(hipStream_t st, const unsigned short* loc_t, int n_buckets, int64_t n_parts, long long* weight);

// CSR row scan.  Scratch: thresholds [n_cols + n_cols / 8 + 2] u64 (the 8-byte thresholds, then their one-byte prefixes), tile_rows [tiles + 1] i64, flags [tiles * DS_TILE / 64] u64,
// tile_count [tiles + 1] i64 (exclusive offsets after launch_downsample_scan), tiles = ceil(nnz / DS_TILE)
hipError_t launch_downsample_flags(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, int64_t nnz,
                                   int32_t n_cols, const int32_t* raw_counts, unsigned long long* thresholds, uint32_t seed, int32_t max_n,
                                   int row_rate_mode, int64_t row_base, int64_t* tile_rows, unsigned long long* flags, int64_t* tile_count,
                                   int32_t* post_counts);
hipError_t launch_downsample_scan(hipStream_t st, int64_t nnz, int64_t* tile_count);
hipError_t launch_downsample_compact(hipStream_t st, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, int64_t nnz,
                                     const int64_t* tile_rows, const unsigned long long* flags, const int64_t* tile_off, int64_t* out_row_ptr,
                                     int32_t* out_col_idx);

// only columns in [col_lo, col_hi) are transposed (col_ptr must come from launch_scan_i32_range with the same range)
hipError_t launch_scan_i32_range(hipStream_t st, const int32_t* in, int64_t n, int32_t lo, int32_t hi, int64_t* out, int64_t* tile_sums);
hipError_t launch_transpose(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, int g_log2,
                            const int64_t* col_ptr, int32_t* cursor, int32_t* out_row_idx, int32_t col_lo, int32_t col_hi);
// two-level counting sort for large matrices (part-local partition + placement): returns 0 scratch bytes when the cursor-atomic kernel should be used
int64_t transpose_scratch_bytes(int64_t n_rows, int64_t nnz, int32_t n_cols);
hipError_t launch_transpose_partitioned(hipStream_t st, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, int64_t nnz, int32_t n_cols,
                                        const int64_t* col_ptr, int32_t* cursor /* [n_cols] zero */, int32_t* out_row_idx, int32_t col_lo, int32_t col_hi, char* scratch);
hipError_t launch_row_work_csr(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* a_row_ptr, const int32_t* a_col_idx,
                               const int64_t* b_row_ptr, int g_log2, int32_t n_items_a, int64_t* work);

// ---- device-side Preparator (ingest_kernels.hip) ------------------------------------------------------
// open-addressing dictionary of 64-bit keys: capacity = mask + 1 (power of two, >= 2 x keys), ~0 = empty slot
struct KeyTable {
  unsigned long long* keys;  // [capacity] initialised to ~0
  unsigned* minpos;          // [capacity] smallest stream position of the key, initialised to ~0
  unsigned* count;           // [capacity] occurrences, initialised to 0
  int32_t* id;               // [capacity] dense id (first-appearance order), -1 = none
  unsigned long long mask;
};
// flag: int32[n] scratch, prefix: int64[n + 1] scratch (prefix[n] = number of ids), first_pos: int64[>= ids] out,
// reserved: one word out = selected positions holding the reserved key ~0 (nothing was inserted for them: the caller refuses the build)
hipError_t launch_dictionary_build(hipStream_t st, int n_cu, KeyTable t, int64_t n, const unsigned long long* keys, const int32_t* select,
                                   int32_t min_count, int32_t* flag, int64_t* prefix, int64_t* tile_sums, int64_t* first_pos, unsigned* reserved);
hipError_t launch_dictionary_lookup(hipStream_t st, int n_cu, KeyTable t, int64_t n, const unsigned long long* keys, const int32_t* select,
                                    int32_t* ids);
hipError_t launch_dictionary_verify(hipStream_t st, int n_cu, KeyTable t, int64_t n, const unsigned long long* keys, const int32_t* select,
                                    const unsigned long long* check, const unsigned long long* ref_check, const int64_t* first_pos, unsigned long long* err);
// ---- growable dictionary (cco_dictionary.h, compiled into ingest_kernels.hip behind cco_props.h; decision D26) ----
// One batch against a live table built with min_count = 1 whose capacity is at least 2 x (n_before + n).  gate[0] (out) = selected positions holding the
// reserved key ~0: when it is not 0 the table was not touched and every other output is undefined.  prefix[n] = the number of new ids.
struct DictExtend {
  KeyTable t;
  int64_t n;
  const unsigned long long* keys;  // [n]
  const int32_t* select;           // nullable [n]: positions with a negative entry take no part
  int64_t n_before;                // ids of the table before the call
  int32_t* ids;                    // nullable out [n]: the id of keys[p] after the call, -1 where select[p] < 0
  int64_t* new_pos;                // out [n]: new_pos[j] = the batch position of the first appearance of id n_before + j
  int32_t* flag;                   // scratch [n]
  int64_t* prefix;                 // scratch [n + 1]
  int64_t* tile_sums;              // scratch: ceil(n / SCAN_TILE) + 1 words
  unsigned* gate;                  // out [1]
};
hipError_t launch_dictionary_extend(hipStream_t st, int n_cu, const DictExtend& a);
// every (key, id) pair with id >= 0 of `from` into `to`: keys ~0, minpos ~0 and id -1 throughout, at least twice as many slots as pairs.  `to.count` is not touched.
hipError_t launch_dictionary_rehash(hipStream_t st, int n_cu, KeyTable from, KeyTable to);
// Raw rows on their way to sorted, duplicate-free rows (cco_sorted_rows.h): the scratch of the CSR build, of every history and of every item event type
struct RawRows {
  int64_t* raw_ptr;  // [n_rows + 1]: the raw row starts (scan of the bounds)
  int32_t* tmp;      // [capacity]: the raw rows
  int32_t* len;      // [n_rows]: the rows' final lengths
  int64_t capacity;  // entries of tmp (and of the caller's col_idx)
};
// cnt: int32[n_rows] scratch, raw_ptr: int64[n_rows + 1] scratch, tmp: int32[n] scratch
hipError_t launch_csr_from_pairs(hipStream_t st, int n_cu, int64_t n, const int32_t* rows, const int32_t* cols, int64_t n_rows, int32_t* cnt,
                                 int64_t* raw_ptr, int32_t* tmp, int64_t* tile_sums, int64_t* out_row_ptr, int32_t* out_col_idx);

// len[n_rows] = row lengths, len16 (nullable) = the same as uint16; sizes (nullable) = {n_rows, nnz, rows longer than 65535}
constexpr int EXCH_SIZES = 4;  // == URCCO_EXCH_SIZES of include/urcco.h (checked in urcco_internal.h)  // (round 6: [3] = columns whose count does not fit a packed B' word -- launch_counts_over_limit)
hipError_t launch_row_lengths(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* row_ptr, int32_t* len, unsigned short* len16, int64_t* sizes);
// out[0] = number of counts that a B' word of a matrix with these counts cannot carry (>= 2^min(count_bits, 16)): a fact of the count TABLE, the same on
// every rank of a sharded build once the counts are all-reduced -- so every rank decides alike whether the rows it sends travel with their counts aboard
hipError_t launch_counts_over_limit(hipStream_t st, int n_cu, const int32_t* counts, int64_t n, int32_t count_bits, int64_t* out);
// row-filtered exchange (cco_misc.hip): per-user masks of the ranks whose item range a row of A' touches, per-destination masked row
// lengths + their scan + the totals per destination, and the packing of the rows per destination
hipError_t launch_need_mask(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* a_row_ptr, const int32_t* a_col_idx, const int32_t* bounds, int world,
                            unsigned long long* mask);
hipError_t launch_masked_lengths(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* row_ptr, const unsigned long long* mask, int world, int32_t* mlen, int64_t* off,
                                 int64_t* tile_sums, int64_t* to_nnz);
hipError_t launch_pack_rows(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, const unsigned long long* mask, int world,
                            const int64_t* off, int32_t* pack);
hipError_t launch_scan_u16(hipStream_t st, const unsigned short* in, int64_t n, int64_t* out, int64_t* tile_sums);
// CSC fragments of the primary (multi-GPU): the record a rank publishes ((2 * world + 3) int64) and the merge of received fragments
hipError_t launch_frag_record(hipStream_t st, int32_t world, const int32_t* bounds, const int64_t* l_cp, const int32_t* bad, int64_t* rec);
hipError_t launch_frag_place(hipStream_t st, int n_cu, int32_t world, int32_t lo, int32_t n_range, const void* lens, int wire16, const int64_t* src_off,
                             const int32_t* ents, const int64_t* a_cp, const int64_t* sizes, int32_t* a_ri);

// boundary checks of a caller-supplied CSR (rp0 = value of row_ptr[0] of the slice); err[0] += violations
hipError_t launch_validate_csr(hipStream_t st, int n_cu, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, int64_t nnz, int32_t n_cols,
                               int g_log2, int64_t rp0, unsigned long long* err);
hipError_t launch_rebase_i64(hipStream_t st, int n_cu, int64_t* p, int64_t n, int64_t delta);
// *dst_mapped = *src, dst_mapped = the device address of host-mapped pinned memory (no copy engine involved)
hipError_t launch_publish_word(hipStream_t st, const unsigned long long* src, unsigned long long* dst_mapped);

// PopModel interval histograms: counts[b * n_items + i] = events of item i with bounds[b] <= t < bounds[b + 1], b < n_buckets <= 3
hipError_t launch_pop_counts(hipStream_t st, int n_cu, int64_t n, const int32_t* item, const int64_t* t_ms, int32_t n_items, int n_buckets,
                             const int64_t* bounds, int32_t* counts);

// ---- backfill ranks from a resident history (decision D24; include/urcco.h urcco_dev_history_ranks / urcco_dev_fill_order) ----------------------
constexpr int RANK_MAX_STREAMS = 16;            // == URCCO_RANK_MAX_STREAMS ... of include/urcco.h (checked in urcco_internal.h)
constexpr int RANK_MAX_FIELDS = 4;
constexpr long long RANK_NONE = INT64_MIN;      // the item has no rank in the field
struct RankStream {
  int64_t n_events;
  const int32_t* items;      // column id per stream position
  const int64_t* times_ms;   // nullable: only the open popular call
  const int32_t* col_map;    // nullable (identity): [n_cols] -> item id or -1
  int32_t n_cols;
};
// The interval histograms of launch_pop_counts summed over the streams (cco_counts.hip), then the ranks.  counts [n_buckets * n_items], col_counts
// [n_buckets * the largest n_cols of a stream with a col_map]: scratch.  open_end: the last interval has no end.  out_counts: nullable.
hipError_t launch_rank_counts(hipStream_t st, int n_cu, const RankStream* streams, int n_streams, int32_t n_items, int n_buckets, const int64_t* bounds, bool open_end,
                              int32_t* counts, int32_t* col_counts, int64_t* out_rank, int32_t* out_counts);
// The backfill order (cco_ranks.h, compiled into cco_misc.hip behind cco_eval.h): a stable LSD radix sort of (key, item) pairs, 8-bit digits.
constexpr int RK_TILE = 2048;                   // pairs one block counts and places per pass
inline int64_t fill_order_tiles(int32_t n_items) { return ((int64_t)n_items + RK_TILE - 1) / RK_TILE; }
struct FillOrderScratch {
  unsigned long long* keys[2];   // [n_items] each: the two sides the passes alternate between
  int32_t* ids[2];               // [n_items] each
  unsigned long long* differ;    // [2 * RANK_MAX_FIELDS]: per field the bits in which two keys differ, then per field the smallest key
  int32_t* hist;                 // [256 * fill_order_tiles]: digit-major per-tile digit counts
  int64_t* offsets;              // [256 * fill_order_tiles + 1]: their exclusive scan
  int64_t* tile_sums;            // scan_tile_words(256 * fill_order_tiles)
};
// ranks: host array of n_fields device pointers
hipError_t launch_fill_order(hipStream_t st, int32_t n_items, const int64_t* const* ranks, int n_fields, const FillOrderScratch& s, int32_t* out_order);

// out[e] = col_idx[e] | counts16[col_idx[e]] << (32 - count_bits) for e < *nnz_dev (<= nnz_bound); counts16 / bad16 as launch_narrow_counts leaves them;
// bad[0] (zeroed here) = counts that do not fit (or 1 when *bad16 != 0: nothing packed)
hipError_t launch_pack_counts(hipStream_t st, int n_cu, const int32_t* col_idx, const int64_t* nnz_dev, int64_t nnz_bound, const unsigned short* counts16,
                              const int32_t* bad16, int32_t count_bits, int32_t* out, int32_t* bad);
hipError_t launch_xlx_table(hipStream_t st, double* tab);
hipError_t launch_xlx_hi_table(hipStream_t st, double* tab /*[2 * XLX_TABLE_HOST]: xlx_hi, then col_ent*/, const double* xlx_tab, long long n_users);
// mono (nullable): the monotone-limit table; then lim[i] = mono[counts[i]] (0 beyond the table) is written too
hipError_t launch_item_entropy(hipStream_t st, const int32_t* counts, int32_t n, long long n_users, double* ent, double* xlx_n, const unsigned short* mono = nullptr,
                               unsigned short* lim = nullptr);
// mono[cA], cA < XLX_TABLE_HOST: up to which cB the LLR of a k11 = 1 candidate is verified to fall strictly and stay positive (cco_rows.hip, mono_limit_kernel); after launch_xlx_hi_table
hipError_t launch_mono_limit(hipStream_t st, unsigned short* mono, const double* xlx_tab, const double* hi_tab, long long n_users);
// out16[i] = counts[i] (low 16 bits); bad[0] = number of counts that do not fit
hipError_t launch_narrow_counts(hipStream_t st, int n_cu, const int32_t* counts, int64_t n, unsigned short* out16, int32_t* bad);  // n: 64-bit (world x shard rows)

// pstart[cap], plen[cap] (scratch), wp[cap + 1]; cap >= nnz(A'); tile_sums scratch as for scans over cap elements
hipError_t launch_expand_prepare(hipStream_t st, int n_cu, const int64_t* a_col_ptr, int32_t n_items_a, const int32_t* a_row_idx,
                                 const int64_t* b_row_ptr, unsigned* b_rp32_scratch /* nullable: n_rows_b + 1 words */, int64_t n_rows_b, int64_t cap,
                                 unsigned* pstart32, int64_t* pstart64, int32_t* plen, int64_t* wp, int64_t* tile_sums, ExpandForm form);
// the same for up to EXPAND_MULTI_MAX event types with ONE gather per CSC entry: T = scratch of n_rows_b * n * 8 bytes
constexpr int EXPAND_MULTI_MAX = 8;
hipError_t launch_expand_prepare_multi(hipStream_t st, int n_cu, const int64_t* a_col_ptr, int32_t n_items_a, const int32_t* a_row_idx, int n,
                                       const int64_t* const* b_row_ptr, int64_t n_rows_b, int64_t cap, unsigned* const* pstart, int32_t* const* plen, void* T,
                                       int64_t* const* tsum /* nullable; tsum[d]: ceil(cap / 2048) + 2 words: the scan-tile sums of plen[d] */);
// (pstart32: the starts the multi form left; pstart64: cap words of scratch they are widened into when the verdict is the wide form)
hipError_t launch_expand_scan(hipStream_t st, const int64_t* a_col_ptr, int32_t n_items_a, const int32_t* plen, int64_t cap, int64_t* wp, int64_t* tile_sums,
                              bool tile_sums_ready, const unsigned* pstart32, int64_t* pstart64, ExpandForm form);
// wp / tile_sums / form as the expand scan left them: in the narrow form a row's 64-bit work is rebuilt from the scan's tile bases and the low words
hipError_t launch_row_work(hipStream_t st, int n_cu, int32_t item_lo, int32_t item_hi, const int64_t* a_col_ptr, const int64_t* wp, const int64_t* tile_sums,
                           const int32_t* form, int64_t* work);

// binning: tile_counts scratch [(ceil(n/BIN_TILE)+1) * BIN_COLS_HOST] int64;
// bin_off[BIN_OFF_LEN] int32, bin_rows[n] int32, stats[STATS_LEN] int64.
hipError_t launch_binning(hipStream_t st, int32_t item_lo, int32_t n, const int64_t* work, const int32_t* cnt_a, int32_t n_cols_b,
                          int32_t count_bits, int32_t k, int64_t* tile_counts, int32_t* bin_off, int32_t* bin_rows, int64_t* stats);

// Which instantiations of the row kernels one A'B call enqueues per LDS class, decided once on the host (cco_rows_impl); the kernels' first-line guard
// states the same rule on the device.  The two host verdicts follow from it: ExpandForm::host_wide = no PK instantiation runs, ExpandForm::host_narrow =
// CcoArgs::pk_known = PACKED.
//   DEBUG           DBG_ROW_KERNELS: the DBG instantiations (they exist for the plain form only), b_packed = NULL
//   PLAIN           no packed words (no copy, or DBG_UNPACKED_COUNTS on a plain B'): the plain instantiations
//   DEVICE_DECIDES  packed words whose verdict -- do the counts fit, are the tables narrow -- is a device-side fact: the PK, then the plain instantiations; the
//                   one whose turn it is not returns at once
//   PACKED          words known good AND tables known narrow (cco_rows_impl): the PK instantiations alone
enum class RowsPlan { DEBUG, PLAIN, DEVICE_DECIDES, PACKED };
constexpr bool plan_runs_pk(RowsPlan p) { return p == RowsPlan::DEVICE_DECIDES || p == RowsPlan::PACKED; }
constexpr bool plan_runs_plain(RowsPlan p) { return p == RowsPlan::PLAIN || p == RowsPlan::DEVICE_DECIDES; }
hipError_t launch_cco_rows_bin(hipStream_t st, int n_cu, const CcoArgs& args, RowsPlan plan, int bin, int32_t n_rows /* item rows of the build: bounds the grids */);
hipError_t launch_bin_out_stats(hipStream_t st, const int32_t* bin_rows, const int32_t* bin_off, int32_t item_lo, const int32_t* out_count,
                                const unsigned long long* cand, int64_t* stats);

hipError_t launch_compact_indicators(hipStream_t st, int32_t n_rows, int32_t k, const int32_t* count, const int32_t* idx,
                                     const double* llr, const int64_t* row_ptr, int32_t* out_idx, double* out_llr);

// splits: bounds[p] = first item whose exclusive work prefix >= p * total / n_parts (prefix = scan of work)
hipError_t launch_partition(hipStream_t st, int32_t n_items, const int64_t* work_prefix, int32_t n_parts, int32_t* bounds);
hipError_t launch_scan_i64(hipStream_t st, const int64_t* in, int64_t n, int64_t* out, int64_t* tile_sums);

// ---- batch recommendations from a built model (cco_recommend.h, compiled into cco_misc.hip) ----------------------
constexpr int REC_MAX_CLAUSES = 16;   // == URCCO_REC_MAX_CLAUSES ... of include/urcco.h (checked in urcco_internal.h)
constexpr int REC_MAX_NUM = 256;
constexpr int REC_NO_BACKFILL = 1;
constexpr int REC_STATS_LEN = 8;
constexpr int REC_LDS_LIMIT = 3072;   // a query whose work bound w(q) (candidate touches + exclusions) is larger runs in the global-accumulator class
constexpr int REC_WEIGHT_ONE = 1 << 15;  // term weights of urcco_dev_recommend_weighted (decision D20): unsigned integers in units of 2^-15 ...
constexpr int REC_WEIGHT_MAX = 1 << 20;  // ... from 1 to 32.0
struct RecClause {
  const int64_t* ind_col_ptr;  // CSC of the indicator matrix I_c (n_items x n_cols)
  const int32_t* ind_row_idx;
  const int64_t* q_row_ptr;    // CSR of the query terms T_c (n_queries x n_cols)
  const int32_t* q_col_idx;
  double boost;
  int32_t n_cols;
  int32_t reserved;
};
// ---- eligibility rules of urcco_dev_recommend_rules (decision D16): every rule of a call must hold for (query, item) ----
constexpr int REC_MAX_RULES = 16;
constexpr int REC_RULE_ANY = 0;     // row `item` of M and the query's row share a column
constexpr int REC_RULE_NONE = 1;    // they share none
constexpr int REC_RULE_RANGE = 2;   // q_lo[q] <= item_value[item] < q_hi[q]; INT64_MIN = the item has no value and fails
struct RecRule {
  const int64_t* m_row_ptr;    // ANY / NONE: CSR of M (n_items x n_cols), order inside a row unspecified, duplicates allowed
  const int32_t* m_col_idx;
  const int64_t* q_row_ptr;    // ANY / NONE: CSR of the query rows (n_queries x n_cols), sorted unique columns
  const int32_t* q_col_idx;
  const int64_t* item_value;   // RANGE: [n_items]
  const int64_t* q_lo;         // RANGE: [n_queries]
  const int64_t* q_hi;
  int32_t kind, n_cols;
};
struct RecArgs;  // cco_recommend.h
int32_t recommend_global_blocks(int64_t n_queries, int32_t n_items, int n_cu, bool weighted = false);
// ctr[5], list[n_queries], pos[n_items] (only with fill_order), g_state / g_m / g_list [g_blocks * n_items] words, g_score [g_blocks * n_items] doubles: scratch.
// weights != NULL (host array [n_clauses] of device pointers, entries nullable): the weighted kernels; g_m64 [g_blocks * n_items] 64-bit words then takes g_m's place
hipError_t launch_recommend(hipStream_t st, int n_cu, int64_t n_queries, int32_t n_items, const RecClause* clauses, int32_t n_clauses, const int64_t* excl_row_ptr,
                            const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order, int32_t num, int32_t flags, int32_t* out_count,
                            int32_t* out_idx, double* out_score, int64_t* stats_dev, unsigned long long* ctr, int32_t* list, int32_t* pos, int32_t g_blocks,
                            unsigned* g_state, unsigned* g_m, int32_t* g_list, double* g_score, int32_t lds_limit = REC_LDS_LIMIT, const RecRule* rules = nullptr,
                            int32_t n_rules = 0, const uint32_t* const* weights = nullptr, unsigned long long* g_m64 = nullptr);
hipError_t launch_idf_weights(hipStream_t st, int n_cu, int32_t n_cols, const int64_t* col_ptr, int64_t n_docs, uint32_t* out);

// ---- hold-out evaluation (cco_eval.h, compiled into cco_misc.hip behind cco_recommend.h; decision D19) ----------------------
constexpr int EVAL_MAX_KS = 8;        // == URCCO_EVAL_MAX_KS of include/urcco.h
void tree_sum_scratch(int64_t n, int32_t n_cols, size_t* pa, size_t* pb);
// pa, pb: scratch doubles as tree_sum_scratch sizes them
hipError_t launch_tree_sum(hipStream_t st, const double* x, int64_t n, int32_t n_cols, double* out, double* pa, double* pb);
// ks: host; ideal [num + 1] (only with discount), pa / pb (only with the sums; sized for n_queries x n_ks): scratch
hipError_t launch_rank_metrics(hipStream_t st, int n_cu, int64_t n_queries, int32_t num, const int32_t* rec_count, const int32_t* rec_idx, const int64_t* truth_row_ptr,
                               const int32_t* truth_col_idx, const int32_t* ks, int32_t n_ks, const double* discount, double* ideal, int32_t* out_hits, double* out_ap,
                               double* out_ndcg, int64_t* out_sums_i, double* out_sums_f, double* pa, double* pb);

// ---- device-resident user history (cco_history.h, compiled into ingest_kernels.hip; decision D17) ----------------------
constexpr int HIST_STATS_LEN = 8;   // == URCCO_HIST_STATS_LEN of include/urcco.h
enum { HIST_STAT_WAVE = 0, HIST_STAT_BLOCK = 1, HIST_STAT_GLOBAL = 2, HIST_STAT_SELECT = 3, HIST_STAT_EXCL_WAVE = 4, HIST_STAT_EXCL_BLOCK = 5, HIST_STAT_OVERFLOW = 6 };
struct HistEvent {
  const int64_t* idx_row_ptr;  // the stream's positions by user (launch_history_index)
  const int32_t* idx_pos;
  const int32_t* items;        // the stream: column id per event, < 0 = none
  const int64_t* times_ms;     // nullable: stream order is time order
  const int32_t* col_map;      // nullable (identity): column id -> item id of the primary or -1
  RawRows raw;                 // scratch, n_queries rows; capacity = entries of the caller's term_col_idx
  int32_t n_cols, max_items, blacklist, reserved;
};
struct HistArgs {
  HistEvent ev[REC_MAX_CLAUSES];
  int64_t n_queries, n_users;
  const int32_t* q_users;
  const int64_t* extra_row_ptr;  // nullable pair: the caller's own exclusions per query
  const int32_t* extra_col_idx;
  RawRows excl;                  // scratch, as in HistEvent
  int32_t* big_list;             // scratch [n_queries * (n_types + 1)]: jobs of more than one wave
  unsigned long long* ctr;       // scratch [1 + HIST_STATS_LEN]
  int32_t n_types, n_items;
};
// cnt [n_users], tile_sums: scratch
hipError_t launch_history_index(hipStream_t st, int n_cu, int64_t n, const int32_t* users, int64_t n_users, int32_t* cnt, int64_t* tile_sums, int64_t* out_row_ptr,
                                int32_t* out_pos);
// the index of the stream grown by n_new events (decision D21): cnt [n_users], add [n_users + 1], tile_sums: scratch; out_* must not overlap old_*
hipError_t launch_history_append(hipStream_t st, int n_cu, int64_t n_old, int64_t n_users_old, const int64_t* old_row_ptr, const int32_t* old_pos, int64_t n_new,
                                 const int32_t* new_users, int64_t n_users, int32_t* cnt, int64_t* add, int64_t* tile_sums, int64_t* out_row_ptr, int32_t* out_pos);
// a stream and its index without the events before min_time_ms and those of drop_users (decision D22; include/urcco.h urcco_dev_history_trim)
struct TrimArgs {
  int64_t n_events, n_users, n_drop, min_time_ms;
  const int32_t* items;
  const int64_t* times_ms;       // nullable: no time rule
  const int64_t* idx_row_ptr;    // [n_users + 1]
  const int32_t* idx_pos;
  const int32_t* drop_users;     // [n_drop]
  int32_t* out_items;
  int64_t* out_times;            // NULL iff times_ms is
  int64_t* out_row_ptr;          // [n_users + 1]
  int32_t* out_pos;
  int64_t* out_counts;           // [2]: kept events, kept index entries
  unsigned long long *s_bits, *i_bits;  // scratch [ceil(n_events / 64)]: one bit per stream position / per index entry
  int32_t *s_cnt, *i_cnt;               // scratch [ceil(n_events / 64)]: the words' popcounts
  int64_t *s_base, *i_base;             // scratch [ceil(n_events / 64) + 1]: their exclusive scans
  int64_t* tile_sums;                   // scratch: scan_tile_words(ceil(n_events / 64))
};
hipError_t launch_history_trim(hipStream_t st, int n_cu, const TrimArgs& a);
// the trim with a per-user cap on the stored events (decision D27; include/urcco.h urcco_dev_history_cap)
struct CapArgs {
  TrimArgs trim;
  int32_t max_per_user;          // INT32_MAX: no cap, the launches of launch_history_trim
  int32_t* list;                 // scratch [n_users]: users above the cap of more than a wave's entries
  unsigned long long* ctr;       // scratch [1]: their number
};
hipError_t launch_history_cap(hipStream_t st, int n_cu, const CapArgs& c);
// the users that train and their row numbers, one event type's user x column matrix (decision D23; include/urcco.h urcco_dev_history_users / _matrix)
constexpr int64_t HM_BITMAP_BUDGET = 8ll << 20;  // bytes of arena the column bitmaps of one _matrix launch may take
constexpr int HM_BITMAP_BLOCKS = 64;             // blocks of the bitmap class at most: one bitmap each
int32_t history_bitmap_blocks(int32_t n_cols, int64_t budget_bytes);  // min(HM_BITMAP_BLOCKS, budget / bytes of one bitmap), at least 1
struct UsersArgs {
  int64_t n_events, n_users, t_lo, t_hi;
  const int64_t* times_ms;       // nullable: every event is in the window
  const int64_t* idx_row_ptr;    // [n_users + 1]
  const int32_t* idx_pos;
  int32_t min_events;
  int32_t* out_row_of;           // [n_users]
  int64_t* out_n_rows;           // [1]
  unsigned long long* i_bits;    // scratch [ceil(n_events / 64)]: one bit per index entry, "its position is in the window"
  int32_t* i_cnt;                // scratch [ceil(n_events / 64)]: the words' popcounts
  int64_t* i_base;               // scratch [ceil(n_events / 64) + 1]: their exclusive scan
  int32_t* keep;                 // scratch [n_users]: 1 = the user trains
  int64_t* prefix;               // scratch [n_users + 1]: its exclusive scan
  int64_t* tile_sums;            // scratch: scan_tile_words(max(ceil(n_events / 64), n_users))
};
hipError_t launch_history_users(hipStream_t st, int n_cu, const UsersArgs& a);
struct MatrixArgs {
  int64_t n_events, n_users, n_rows, t_lo, t_hi, capacity;
  const int32_t* items;
  const int64_t* times_ms;       // nullable
  const int64_t* idx_row_ptr;    // [n_users + 1]: also the raw row starts
  const int32_t* idx_pos;
  const int32_t* row_of;         // nullable: identity
  int32_t n_cols, bm_blocks;     // bm_blocks: blocks of the bitmap class; 0 = no user can be that heavy (n_events <= 4096)
  int64_t* out_row_ptr;          // [n_rows + 1]
  int32_t* out_col_idx;          // [capacity]
  int64_t* out_nnz;              // [1]
  int32_t* tmp;                  // scratch [n_events]: the raw rows, user u's at its clamped index segment
  int32_t* len;                  // scratch [n_rows]: the rows' final lengths
  int32_t* raw_start;            // scratch [n_rows]: where in tmp the row lies
  int32_t* list;                 // scratch [n_users]: users of 65 .. 4096 raw entries from the front, heavier ones from the back
  unsigned long long* ctr;       // scratch [2]: their numbers
  unsigned* bitmaps;             // scratch [bm_blocks * ceil(n_cols / 32)]
  int64_t* tile_sums;            // scratch: scan_tile_words(n_rows)
};
hipError_t launch_history_matrix(hipStream_t st, int n_cu, const MatrixArgs& a);
// bnd [(n_types + 1) * n_queries]: scratch; only the inputs of `a` are read
hipError_t launch_history_bounds(hipStream_t st, int n_cu, const HistArgs& a, int32_t* bnd, int64_t* tile_sums, int64_t* const* term_row_ptr, int64_t* excl_row_ptr);
hipError_t launch_history_rows(hipStream_t st, int n_cu, const HistArgs& a, int64_t* tile_sums, int64_t* const* term_row_ptr, int32_t* const* term_col_idx,
                               int64_t* excl_row_ptr, int32_t* excl_col_idx, int64_t* stats_dev);

// ---- device-resident item queries (cco_items.h, compiled into ingest_kernels.hip behind cco_history.h; decision D18) ----
struct ItemEvent {
  const int64_t* ind_row_ptr;  // the indicator CSR of the event type, n_items rows, as the build leaves it
  const int32_t* ind_col_idx;
  RawRows raw;                 // scratch, n_queries rows; capacity = entries of the caller's term_col_idx
  int32_t n_cols, max_terms;
};
struct ItemArgs {
  ItemEvent ev[REC_MAX_CLAUSES];
  int64_t n_queries;
  const int32_t* q_items;
  int32_t* big_list;             // scratch [n_queries * n_types]: jobs of more than one wave
  unsigned long long* ctr;       // scratch [1]: the cursor of big_list
  int32_t n_types, n_items;
};
// bnd [n_types * n_queries]: scratch; only the inputs of `a` are read
hipError_t launch_item_bounds(hipStream_t st, int n_cu, const ItemArgs& a, int32_t* bnd, int64_t* tile_sums, int64_t* const* term_row_ptr);
hipError_t launch_item_rows(hipStream_t st, int n_cu, const ItemArgs& a, int64_t* tile_sums, int64_t* const* term_row_ptr, int32_t* const* term_col_idx, int64_t* stats_dev);

// ---- device-resident item properties (cco_props.h, compiled into ingest_kernels.hip behind cco_items.h; decision D25) ----
constexpr unsigned PROP_SET = 0, PROP_UNSET = 1;  // include/urcco.h URCCO_PROP_*
constexpr int PROP_MAX = 16;                      // URCCO_PROP_MAX: properties per urcco_dev_props_exists call
struct PropState {
  const unsigned long long* t_set;    // [n_items]: biased time of the latest $set, 0 = none
  const unsigned* pos_set;            // [n_items]: its stream position + 1
  const unsigned long long* t_unset;  // [n_items]: biased time of the latest $unset
  const unsigned long long* t_del;    // nullable [n_items]: biased time of the item's latest $delete
  int64_t n_events;                   // positions the property's stream holds
};
struct PropRows {
  PropState st;
  const int64_t* val_ptr;   // [n_events + 1]: the value slice of every stream position
  const int32_t* values;    // [n_values] value ids
  int64_t n_values;
  RawRows raw;              // scratch, n_items rows; capacity = entries of the caller's col_idx
  int32_t n_items, n_cols;
};
struct PropSets {
  const unsigned long long* t_set[PROP_MAX];
  int32_t n_props;
};
hipError_t launch_props_apply(hipStream_t st, int n_cu, int32_t n_items, int64_t n, const int32_t* items, const int64_t* times, const uint8_t* kinds, int64_t pos_base,
                              unsigned long long* t_set, unsigned* pos_set, unsigned long long* t_unset);
hipError_t launch_props_delete(hipStream_t st, int n_cu, int32_t n_items, int64_t n, const int32_t* items, const int64_t* times, unsigned long long* t_del);
// bnd [n_items]: scratch
hipError_t launch_props_bounds(hipStream_t st, int n_cu, const PropRows& a, int32_t* bnd, int64_t* tile_sums, int64_t* row_ptr);
hipError_t launch_props_rows(hipStream_t st, int n_cu, const PropRows& a, int64_t* tile_sums, int64_t* row_ptr, int32_t* col_idx);
hipError_t launch_props_dates(hipStream_t st, int n_cu, int32_t n_items, const PropState& s, const int64_t* date_values, int64_t* out);
hipError_t launch_props_exists(hipStream_t st, int n_cu, int32_t n_items, const unsigned long long* t_del, const PropSets& sets, uint8_t* mask);
// one property's stream without the superseded values (decision D28; include/urcco.h urcco_dev_props_compact)
struct CompactArgs {
  PropState st;
  const int64_t* val_ptr;        // nullable: not a list property
  const int32_t* values;
  int64_t n_values;
  const int64_t* date_values;    // nullable: not a date property
  int32_t n_items;
  unsigned* out_pos_set;         // [n_items]
  int32_t* out_old_pos;          // [K]
  int64_t* out_val_ptr;          // [K + 1]
  int32_t* out_values;           // [V]
  int64_t* out_date_values;      // [K]
  int64_t* out_counts;           // [2]: K, V
  unsigned long long* bits;      // scratch [ceil(n_events / 64)]: one bit per stream position, "an item's winner"
  int32_t* cnt;                  // scratch [ceil(n_events / 64)]: the words' popcounts
  int64_t* base;                 // scratch [ceil(n_events / 64) + 1]: their exclusive scan
  int32_t* len;                  // scratch [min(n_items, n_events)]: the new positions' slice lengths
  int64_t* src;                  // scratch [min(n_items, n_events)]: where in `values` their slices start
  int64_t* val_base;             // scratch [min(n_items, n_events) + 1]: the scan of len
  int64_t* tile_sums;            // scratch: scan_tile_words(max(ceil(n_events / 64), min(n_items, n_events)))
};
hipError_t launch_props_compact(hipStream_t st, int n_cu, const CompactArgs& a);

hipError_t launch_llr_test(hipStream_t st, int64_t n, const int64_t* a, const int64_t* b, const int64_t* ab, const int64_t* nu, double* out);
hipError_t launch_u01_test(hipStream_t st, int64_t n, uint32_t seed, const int32_t* row, const int32_t* col, double* out, int rng32 = 0);

}  // namespace urcco
