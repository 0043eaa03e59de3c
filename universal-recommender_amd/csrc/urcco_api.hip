// C ABI of liburcco (include/urcco.h): session / scratch management, the device-level stage functions and the
// host-level one-shot entry points that stand in for Mahout's SimilarityAnalysis.cooccurrencesIDSs and
// crossOccurrenceDownsampled (reference call sites: src/main/scala/URAlgorithm.scala:323-329, :343-346).
// No CPU fallback: without a HIP device the compute entry points return URCCO_NO_DEVICE.
#include "urcco_internal.h"

using namespace urcco_detail;

#include <signal.h>
#include <unistd.h>

#include <mutex>

namespace urcco_detail {
char* err_buf() {
  static thread_local char buf[512] = "";
  return buf;
}

// ---- fault-hunting aids (urcco_internal.h: URCCO_DEBUG_MARKS / URCCO_DEBUG_POISON) ----------------------------------
const DebugCfg& debug_cfg() {
  static const DebugCfg cfg = [] {
    DebugCfg c;
    const char* m = getenv("URCCO_DEBUG_MARKS");
    const char* p = getenv("URCCO_DEBUG_POISON");
    c.marks = m && *m && *m != '0';
    c.poison = p && *p && *p != '0';
    return c;
  }();
  return cfg;
}

namespace {
__global__ void debug_mark_kernel(unsigned* slot, unsigned value) {
  __hip_atomic_store(slot, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
constexpr int MARK_SESSIONS = 64;
struct MarkSlot { unsigned* marks; void* stream; int device; };
MarkSlot g_mark_slots[MARK_SESSIONS];  // read by the signal handler: plain array, entries published by their `marks` pointer
std::mutex g_mark_mu;
struct sigaction g_prev_abrt;
void put(const char* s) { (void)!write(2, s, strlen(s)); }
void put_u(unsigned long long v, int base = 10) {
  char b[24];
  int n = 0;
  do { const int d = (int)(v % (unsigned)base); b[n++] = (char)(d < 10 ? '0' + d : 'a' + d - 10); v /= (unsigned)base; } while (v && n < 23);
  char o[24];
  for (int i = 0; i < n; ++i) o[i] = b[n - 1 - i];
  o[n] = 0;
  put(o);
}
const char* const STAGE_NAME[URCCO_N_STAGES] = {"column_counts", "downsample_flags", "downsample_scan", "downsample_compact", "transpose", "row_work", "binning",
                                               "entropy", "cco_bin0", "cco_bin1", "cco_bin2", "cco_bin3", "cco_bin4", "cco_bin5", "cco_bin6", "compact_indicators", "exchange"};
void dump_marks(const char* why) {  // async-signal-safe: write(2) only
  put("[urcco marks] "); put(why); put(": last launch groups per session (ordinal:stage begun / finished)\n");
  for (int i = 0; i < MARK_SESSIONS; ++i) {
    unsigned* m = g_mark_slots[i].marks;
    if (!m) continue;
    const unsigned b = __atomic_load_n(&m[0], __ATOMIC_RELAXED), f = __atomic_load_n(&m[1], __ATOMIC_RELAXED);
    put("[urcco marks]   session "); put_u((unsigned)i); put(" dev "); put_u((unsigned)g_mark_slots[i].device);
    put(" stream 0x"); put_u((unsigned long long)(uintptr_t)g_mark_slots[i].stream, 16);
    put(": begun "); put_u(b >> 8); put(":"); put((b & 255u) < URCCO_N_STAGES ? STAGE_NAME[b & 255u] : "?");
    put("  finished "); put_u(f >> 8); put(":"); put((f & 255u) < URCCO_N_STAGES ? STAGE_NAME[f & 255u] : "?");
    put(b == f ? "  (idle)\n" : "  <-- IN FLIGHT\n");
  }
}
void on_abort(int sig) {
  dump_marks("SIGABRT");
  sigaction(SIGABRT, &g_prev_abrt, nullptr);
  raise(sig);
}
}  // namespace

void debug_register(urcco_session* s) {
  if (!debug_cfg().marks) return;
  std::lock_guard<std::mutex> g(g_mark_mu);
  static bool installed = false;
  if (!installed) {
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_handler = on_abort;
    sigaction(SIGABRT, &sa, &g_prev_abrt);
    installed = true;
  }
  unsigned* m = nullptr;
  if (hipHostMalloc((void**)&m, 64, 0) != hipSuccess || !m) return;
  m[0] = m[1] = 0u;
  for (int i = 0; i < MARK_SESSIONS; ++i)
    if (!g_mark_slots[i].marks) {
      g_mark_slots[i].stream = (void*)s->stream;
      g_mark_slots[i].device = s->device;
      __atomic_store_n(&g_mark_slots[i].marks, m, __ATOMIC_RELEASE);
      s->marks = m;
      return;
    }
  (void)hipHostFree(m);
}
void debug_unregister(urcco_session* s) {
  if (!s->marks) return;
  std::lock_guard<std::mutex> g(g_mark_mu);
  for (int i = 0; i < MARK_SESSIONS; ++i)
    if (g_mark_slots[i].marks == s->marks) __atomic_store_n(&g_mark_slots[i].marks, (unsigned*)nullptr, __ATOMIC_RELEASE);
  (void)hipHostFree(s->marks);
  s->marks = nullptr;
}
void debug_mark(urcco_session* s, int which, int stage) {
  if (which == 0) ++s->mark_seq;
  hipLaunchKernelGGL(debug_mark_kernel, dim3(1), dim3(1), 0, s->stream, s->marks + which, (s->mark_seq << 8) | (unsigned)(stage & 255));
}
void debug_poison(void* p, size_t bytes, hipStream_t st, bool async) {
#ifdef HIPSIM_HOST_BUILD
  if (hipsim::guard_on()) return;  // the simulator's own guard mode poisons (and keeps PROT_NONE pages inside the arena)
#endif
  if (!p || !bytes) return;
  if (async) (void)hipMemsetAsync(p, 0x7f, bytes, st);
  else (void)hipMemset(p, 0x7f, bytes);
}
}  // namespace urcco_detail

extern "C" {

int urcco_version(void) { return URCCO_VERSION; }

int urcco_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* urcco_last_error(void) { return err_buf(); }

const char* urcco_status_string(int status) {
  switch (status) {
    case URCCO_OK: return "OK";
    case URCCO_BAD_ARG: return "BAD_ARG";
    case URCCO_OOM_HOST: return "OOM_HOST";
    case URCCO_OOM_DEVICE: return "OOM_DEVICE";
    case URCCO_HIP_ERROR: return "HIP_ERROR";
    case URCCO_INTERNAL: return "INTERNAL";
    case URCCO_NO_DEVICE: return "NO_DEVICE";
    case URCCO_RCCL_ERROR: return "RCCL_ERROR";
    default: return "UNKNOWN";
  }
}

void urcco_debug_dump_marks(void) {
  if (debug_cfg().marks) dump_marks("dump");
}

int urcco_session_create(int32_t device, void* stream, urcco_session** out) {
  if (!out) return fail(URCCO_BAD_ARG, "urcco_session_create: out is NULL");
  *out = nullptr;
  const int n = urcco_device_count();
  if (n <= 0) return fail(URCCO_NO_DEVICE, "no HIP device visible (liburcco has no CPU fallback)");
  if (device < 0 || device >= n) return fail(URCCO_BAD_ARG, "device %d out of range [0,%d)", device, n);
  HIPC(hipSetDevice(device));
  urcco_session* s = new (std::nothrow) urcco_session();
  if (!s) return fail(URCCO_OOM_HOST, "session alloc");
  s->device = device;
  if (stream) {
    s->stream = (hipStream_t)stream;
  } else {
    hipError_t e = hipStreamCreate(&s->stream);
    if (e != hipSuccess) { delete s; return hip_fail(e, "hipStreamCreate"); }
    s->own_stream = true;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cu = prop.multiProcessorCount;
  debug_register(s);
  *out = s;
  return URCCO_OK;
}

void urcco_session_destroy(urcco_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->stream);
  debug_unregister(s);
  s->collect();
  for (hipEvent_t e : s->free_events) (void)hipEventDestroy(e);
  if (s->own_stream) (void)hipStreamDestroy(s->stream);
  delete s;  // its device is current and its stream drained: the device buffers it owns free themselves
}

int urcco_session_synchronize(urcco_session* s) {
  if (!s) return fail(URCCO_BAD_ARG, "session is NULL");
  HIPC(hipStreamSynchronize(s->stream));
  return URCCO_OK;
}

int urcco_session_set_debug(urcco_session* s, int32_t flags) {
  if (!s) return fail(URCCO_BAD_ARG, "session is NULL");
  s->debug = flags;
  return URCCO_OK;
}

int urcco_session_set_expand_test(urcco_session* s, int64_t limit, int64_t prefix_seed) {
  if (!s || limit < 0 || prefix_seed < 0) return fail(URCCO_BAD_ARG, "urcco_session_set_expand_test: bad argument");
  s->narrow_limit = limit == 0 ? urcco::NARROW_LIMIT : (unsigned long long)limit;
  s->prefix_seed = prefix_seed;
  return URCCO_OK;
}

int urcco_session_expand_form(urcco_session* s, int32_t* form_host) {
  if (!s || !form_host) return fail(URCCO_BAD_ARG, "urcco_session_expand_form: bad argument");
  if (!s->form_word.p || !s->form_valid) return fail(URCCO_BAD_ARG, "urcco_session_expand_form: no rows were built on this session");
  HIPC(hipMemcpyAsync(form_host, s->form_word.p, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  HIPC(hipStreamSynchronize(s->stream));
  return URCCO_OK;
}

int urcco_session_set_timing(urcco_session* s, int32_t enable) {
  if (!s) return fail(URCCO_BAD_ARG, "session is NULL");
  s->collect();
  s->timing = enable != 0;
  for (int i = 0; i < URCCO_N_STAGES; ++i) { s->acc_ms[i] = 0; s->acc_n[i] = 0; }
  return URCCO_OK;
}

int urcco_session_get_timings(urcco_session* s, double* ms, int64_t* launches) {
  if (!s || !ms || !launches) return fail(URCCO_BAD_ARG, "urcco_session_get_timings: bad argument");
  s->collect();
  for (int i = 0; i < URCCO_N_STAGES; ++i) { ms[i] = s->acc_ms[i]; launches[i] = s->acc_n[i]; }
  return URCCO_OK;
}

int64_t urcco_session_scratch_bytes(const urcco_session* s) {
  if (!s) return 0;
  return (int64_t)s->arena.cap + (int64_t)s->g_cap * 16;
}

int urcco_dev_column_counts(urcco_session* s, int64_t nnz, const int32_t* col_idx, int32_t n_cols, int32_t* counts) {
  if (!s || nnz < 0 || n_cols < 0 || (nnz > 0 && !col_idx) || (n_cols > 0 && !counts)) return fail(URCCO_BAD_ARG, "urcco_dev_column_counts: bad argument");
  if (n_cols == 0) return URCCO_OK;
  const int64_t ph_bytes = urcco::column_counts_scratch_bytes(nnz, n_cols);
  char* ph = nullptr;
  if (ph_bytes > 0) URC(ArenaLayout(s).add(&ph, (size_t)ph_bytes).commit());
  s->begin(URCCO_STAGE_COLUMN_COUNTS);
  if (ph_bytes > 0)
    HIPC(urcco::launch_column_counts_partitioned(s->stream, col_idx, nnz, nullptr, n_cols, counts, ph));
  else
    HIPC(urcco::launch_column_counts(s->stream, s->n_cu, col_idx, nnz, n_cols, counts));
  s->end();
  return URCCO_OK;
}

int urcco_dev_downsample(urcco_session* s, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, int64_t nnz, int32_t n_cols,
                         const int32_t* raw_counts, int32_t seed, int32_t max_elements_per_row, int32_t row_rate_mode, int64_t row_base,
                         int64_t* out_row_ptr, int32_t* out_col_idx, int32_t* post_counts) {
  if (!s || n_rows < 0 || nnz < 0 || n_cols < 0 || !row_ptr || !out_row_ptr || (nnz > 0 && (!col_idx || !raw_counts || !out_col_idx)))
    return fail(URCCO_BAD_ARG, "urcco_dev_downsample: bad argument");
  if (max_elements_per_row <= 0) return fail(URCCO_BAD_ARG, "maxElementsPerRow must be positive, got %d", max_elements_per_row);
  if ((row_rate_mode & ~URCCO_RNG_MIX32) != URCCO_ROW_RATE_MAHOUT_INT_DIV && (row_rate_mode & ~URCCO_RNG_MIX32) != URCCO_ROW_RATE_FRACTIONAL)
    return fail(URCCO_BAD_ARG, "unknown row_rate_mode %d", row_rate_mode);
  if (post_counts && n_cols > 0) HIPC(hipMemsetAsync(post_counts, 0, sizeof(int32_t) * (size_t)n_cols, s->stream));
  if (nnz == 0) {
    HIPC(hipMemsetAsync(out_row_ptr, 0, sizeof(int64_t) * (size_t)(n_rows + 1), s->stream));
    return URCCO_OK;
  }
  // post-sampling column counts: large matrices are counted after compaction by the atomic-free partitioned histogram
  // (its length is read on the device: out_row_ptr[n_rows]); small ones by L2 atomics inside the scan kernel
  const int64_t ph_bytes = post_counts ? urcco::column_counts_scratch_bytes(nnz, n_cols) : 0;
  const int64_t ds_tiles = (nnz + urcco::DS_TILE - 1) / urcco::DS_TILE;
  const size_t n_words = (size_t)ds_tiles * (urcco::DS_TILE / 64);
  const size_t thr_words = (size_t)n_cols + (size_t)n_cols / 8 + 2;  // 8-byte thresholds + their one-byte prefixes
  ArenaLayout L(s);
  unsigned long long *thresholds, *flags;
  int64_t *tile_rows, *tile_count;
  char* ph = nullptr;
  L.add(&thresholds, thr_words).add(&tile_rows, (size_t)ds_tiles + 1).add(&tile_count, (size_t)ds_tiles + 1).add(&flags, n_words);
  if (ph_bytes > 0) L.add(&ph, (size_t)ph_bytes);
  URC(L.commit());
  s->begin(URCCO_STAGE_DOWNSAMPLE_FLAGS);
  HIPC(urcco::launch_downsample_flags(s->stream, s->n_cu, n_rows, row_ptr, col_idx, nnz, n_cols, raw_counts, thresholds, (uint32_t)seed,
                                      max_elements_per_row, row_rate_mode, row_base, tile_rows, flags, tile_count,
                                      ph_bytes > 0 ? nullptr : post_counts));
  s->end();
  s->begin(URCCO_STAGE_DOWNSAMPLE_SCAN);
  HIPC(urcco::launch_downsample_scan(s->stream, nnz, tile_count));
  s->end();
  s->begin(URCCO_STAGE_DOWNSAMPLE_COMPACT);
  HIPC(urcco::launch_downsample_compact(s->stream, n_rows, row_ptr, col_idx, nnz, tile_rows, flags, tile_count, out_row_ptr, out_col_idx));
  s->end();
  if (ph_bytes > 0) {
    s->begin(URCCO_STAGE_COLUMN_COUNTS);
    HIPC(urcco::launch_column_counts_partitioned(s->stream, out_col_idx, nnz, out_row_ptr + n_rows, n_cols, post_counts, ph));
    s->end();
  }
  return URCCO_OK;
}

int urcco_dev_transpose(urcco_session* s, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_idx, int64_t nnz, int32_t n_cols,
                        const int32_t* counts, int32_t col_lo, int32_t col_hi, int64_t* out_col_ptr, int32_t* out_row_idx) {
  if (!s || n_rows < 0 || nnz < 0 || n_cols < 0 || !row_ptr || !out_col_ptr || (n_cols > 0 && !counts) || (nnz > 0 && (!col_idx || !out_row_idx)) ||
      col_lo < 0 || col_hi < col_lo || col_hi > n_cols)
    return fail(URCCO_BAD_ARG, "urcco_dev_transpose: bad argument");
  const int64_t tr_bytes = urcco::transpose_scratch_bytes(n_rows, nnz, n_cols);
  ArenaLayout L(s);
  int32_t* cursor;
  int64_t* tile_sums;
  char* tr = nullptr;  // the partitioned form's block, carved by its launcher
  L.add(&cursor, (size_t)n_cols).add(&tile_sums, scan_tile_words(n_cols));
  if (tr_bytes > 0) L.add(&tr, (size_t)tr_bytes);
  URC(L.commit());
  s->begin(URCCO_STAGE_TRANSPOSE);
  HIPC(urcco::launch_scan_i32_range(s->stream, counts, n_cols, col_lo, col_hi, out_col_ptr, tile_sums));
  if (nnz > 0 && n_rows > 0) {
    int g = ceil_log2_i64((nnz + n_rows - 1) / n_rows);
    if (g < 1) g = 1;
    if (g > 6) g = 6;
    HIPC(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)n_cols, s->stream));
    if (tr_bytes > 0) {
      HIPC(urcco::launch_transpose_partitioned(s->stream, n_rows, row_ptr, col_idx, nnz, n_cols, out_col_ptr, cursor, out_row_idx, col_lo, col_hi, tr));
    } else {
      HIPC(urcco::launch_transpose(s->stream, s->n_cu, n_rows, row_ptr, col_idx, g, out_col_ptr, cursor, out_row_idx, col_lo, col_hi));
    }
  }
  s->end();
  return URCCO_OK;
}

int urcco_dev_row_work_csr(urcco_session* s, int64_t n_rows, const int64_t* a_row_ptr, const int32_t* a_col_idx, int64_t nnz_a, const int64_t* b_row_ptr,
                           int32_t n_items_a, int64_t* work) {
  if (!s || n_rows < 0 || nnz_a < 0 || n_items_a < 0 || !a_row_ptr || !b_row_ptr || (nnz_a > 0 && !a_col_idx) || (n_items_a > 0 && !work))
    return fail(URCCO_BAD_ARG, "urcco_dev_row_work_csr: bad argument");
  int g = n_rows > 0 ? ceil_log2_i64((nnz_a + n_rows - 1) / n_rows) : 1;
  if (g < 1) g = 1;
  if (g > 6) g = 6;
  s->begin(URCCO_STAGE_ROW_WORK);
  HIPC(urcco::launch_row_work_csr(s->stream, s->n_cu, n_rows, a_row_ptr, a_col_idx, b_row_ptr, g, n_items_a, work));
  s->end();
  return URCCO_OK;
}

int urcco_dev_row_work(urcco_session* s, int32_t item_lo, int32_t item_hi, int32_t n_items_a, const int64_t* a_col_ptr, const int32_t* a_row_idx,
                       int64_t nnz_a_bound, const int64_t* b_row_ptr, int64_t* work) {
  if (!s || item_lo < 0 || item_hi < item_lo || item_hi > n_items_a || nnz_a_bound < 0 || !a_col_ptr || !b_row_ptr || (item_hi > item_lo && !work))
    return fail(URCCO_BAD_ARG, "urcco_dev_row_work: bad argument");
  const int64_t cap = nnz_a_bound;
  int32_t* plen;
  int64_t *wp, *tile_sums;
  URC(ArenaLayout(s).add(&plen, (size_t)cap).add(&wp, (size_t)cap + 1).add(&tile_sums, scan_tile_words(cap)).commit());
  if (!s->form_word.p) URC(s->form_word.alloc(1));
  s->form_valid = false;
  int32_t* form = s->form_word.p;
  s->begin(URCCO_STAGE_ROW_WORK);
  // (no row kernel follows: the lengths and their prefix alone, no starts -- the prefix in the narrow form unless a tile sum forbids it)
  HIPC(urcco::launch_expand_prepare(s->stream, s->n_cu, a_col_ptr, n_items_a, a_row_idx, b_row_ptr, nullptr, 0, cap, nullptr, nullptr, plen, wp, tile_sums,
                                    urcco::ExpandForm{form, nullptr, 0, 0, s->narrow_limit, s->prefix_seed}));
  HIPC(urcco::launch_row_work(s->stream, s->n_cu, item_lo, item_hi, a_col_ptr, wp, tile_sums, form, work));
  s->form_valid = true;
  s->end();
  return URCCO_OK;
}

int urcco_dev_partition(urcco_session* s, int32_t n_items, const int64_t* work, int32_t n_parts, int32_t* bounds_host) {
  if (!s || n_items < 0 || n_parts <= 0 || n_parts > 4096 || !bounds_host || (n_items > 0 && !work)) return fail(URCCO_BAD_ARG, "urcco_dev_partition: bad argument");
  int32_t* bounds = nullptr;
  URC(urcco_detail::partition_dev(s, n_items, work, n_parts, nullptr, &bounds));
  HIPC(hipMemcpyAsync(bounds_host, bounds, sizeof(int32_t) * (size_t)(n_parts + 1), hipMemcpyDeviceToHost, s->stream));
  HIPC(hipStreamSynchronize(s->stream));
  return URCCO_OK;
}

int urcco_dev_merge_fragments(urcco_session* s, int32_t world, int32_t item_lo, int32_t item_hi, int32_t n_items, const void* lens, int32_t wire16,
                              const int32_t* entries, int64_t n_entries, const int64_t* sizes, const int32_t* counts, int64_t* out_col_ptr,
                              int32_t* out_row_idx) {
  if (!s || world <= 0 || item_lo < 0 || item_hi < item_lo || item_hi > n_items || n_entries < 0 || !sizes || !out_col_ptr || (n_items > 0 && !counts) ||
      (item_hi > item_lo && !lens) || (n_entries > 0 && (!entries || !out_row_idx)))
    return fail(URCCO_BAD_ARG, "urcco_dev_merge_fragments: bad argument");
  const int32_t n_range = item_hi - item_lo;
  const int64_t n_runs = (int64_t)world * n_range;
  int64_t *src_off, *tile_sums;
  ArenaLayout L(s);
  L.add(&src_off, (size_t)n_runs + 1);
  L.add(&tile_sums, scan_tile_words(n_items > n_runs ? n_items : n_runs));  // shared by the scan over the items and the one over the runs
  URC(L.commit());
  s->begin(URCCO_STAGE_TRANSPOSE);
  HIPC(urcco::launch_scan_i32_range(s->stream, counts, n_items, item_lo, item_hi, out_col_ptr, tile_sums));
  if (wire16) {
    HIPC(urcco::launch_scan_u16(s->stream, static_cast<const unsigned short*>(lens), n_runs, src_off, tile_sums));
  } else {
    HIPC(urcco::launch_scan_i32(s->stream, static_cast<const int32_t*>(lens), n_runs, src_off, tile_sums));
  }
  HIPC(urcco::launch_frag_place(s->stream, s->n_cu, world, item_lo, n_range, lens, wire16, src_off, entries, out_col_ptr, sizes, out_row_idx));
  s->end();
  return URCCO_OK;
}

int urcco_dev_cco_rows(urcco_session* s, int32_t item_lo, int32_t item_hi, int32_t n_items_a, const int64_t* a_col_ptr,
                       const int32_t* a_row_idx, int64_t nnz_a_bound, const int64_t* b_row_ptr, const int32_t* b_col_idx, int32_t n_cols_b,
                       const int32_t* counts_a, const int32_t* counts_b, int64_t n_users, int32_t exclude_self, int32_t k,
                       int32_t has_min_llr, double min_llr, int32_t* out_count, int32_t* out_idx, double* out_llr, int64_t* stats_dev) {
  return urcco_dev_cco_rows_packed(s, item_lo, item_hi, n_items_a, a_col_ptr, a_row_idx, nnz_a_bound, b_row_ptr, b_col_idx, n_cols_b, counts_a, counts_b, n_users, exclude_self,
                                   k, has_min_llr, min_llr, out_count, out_idx, out_llr, stats_dev, nullptr, nullptr);
}

int urcco_dev_pack_counts(urcco_session* s, int64_t n_rows_b, const int64_t* b_row_ptr, const int32_t* b_col_idx, int64_t nnz_b_bound, const int32_t* counts_b,
                          int32_t n_cols_b, int32_t* out_packed, int32_t* out_bad) {
  return urcco_detail::pack_counts(s, BPrime(b_row_ptr, b_col_idx, n_rows_b, nnz_b_bound, n_cols_b, counts_b, false), out_packed, out_bad);
}

int urcco_dev_cco_rows_packed(urcco_session* s, int32_t item_lo, int32_t item_hi, int32_t n_items_a, const int64_t* a_col_ptr,
                              const int32_t* a_row_idx, int64_t nnz_a_bound, const int64_t* b_row_ptr, const int32_t* b_col_idx, int32_t n_cols_b,
                              const int32_t* counts_a, const int32_t* counts_b, int64_t n_users, int32_t exclude_self, int32_t k,
                              int32_t has_min_llr, double min_llr, int32_t* out_count, int32_t* out_idx, double* out_llr, int64_t* stats_dev,
                              const int32_t* b_packed, const int32_t* pack_bad) {
  if ((b_packed == nullptr) != (pack_bad == nullptr)) return fail(URCCO_BAD_ARG, "urcco_dev_cco_rows_packed: b_packed and pack_bad come together");
  RowsCall c;
  c.item_lo = item_lo; c.item_hi = item_hi; c.n_items_a = n_items_a;
  c.a_col_ptr = a_col_ptr; c.a_row_idx = a_row_idx; c.nnz_a_bound = nnz_a_bound; c.counts_a = counts_a;
  c.b = BPrime(b_row_ptr, b_col_idx, n_users, -1, n_cols_b, counts_b, false);
  if (b_packed) c.b = c.b.with_copy(b_packed, pack_bad);
  c.n_users = n_users; c.exclude_self = exclude_self; c.k = k; c.has_min_llr = has_min_llr; c.min_llr = min_llr;
  c.out_count = out_count; c.out_idx = out_idx; c.out_llr = out_llr; c.stats_dev = stats_dev;
  return urcco_detail::cco_rows_impl(s, c);
}

}  // extern "C"

namespace urcco_detail {

// bounds stay on the device: `bounds_dev` if given, else arena scratch returned through *bounds_out (valid until the session's next scratch layout)
int partition_dev(urcco_session* s, int32_t n_items, const int64_t* work, int32_t n_parts, int32_t* bounds_dev, int32_t** bounds_out) {
  ArenaLayout L(s);
  int64_t *prefix, *tile_sums;
  int32_t* bounds = bounds_dev;
  L.add(&prefix, (size_t)n_items + 1).add(&tile_sums, scan_tile_words(n_items));
  if (!bounds_dev) L.add(&bounds, (size_t)n_parts + 1);
  URC(L.commit());
  HIPC(urcco::launch_scan_i64(s->stream, work, n_items, prefix, tile_sums));
  HIPC(urcco::launch_partition(s->stream, n_items, prefix, n_parts, bounds));
  if (bounds_out) *bounds_out = bounds;
  return URCCO_OK;
}

int cco_rows_impl(urcco_session* s, const RowsCall& c) {
  const int32_t item_lo = c.item_lo, item_hi = c.item_hi, n_items_a = c.n_items_a, n_cols_b = c.b.n_cols, k = c.k;
  const int64_t n_users = c.n_users;  // (the rows of B': c.b.n_rows)
  if (!s || item_lo < 0 || item_hi < item_lo || item_hi > n_items_a || n_cols_b < 0 || n_users < 0 || c.nnz_a_bound < 0 || !c.a_col_ptr || !c.b.row_ptr)
    return fail(URCCO_BAD_ARG, "urcco_dev_cco_rows: bad argument");
  if (k <= 0) return fail(URCCO_BAD_ARG, "maxInterestingElements must be positive, got %d", k);
  const int32_t n = item_hi - item_lo;
  if (n == 0) {
    if (c.stats_dev) HIPC(hipMemsetAsync(c.stats_dev, 0, sizeof(int64_t) * URCCO_STATS_LEN, s->stream));
    return URCCO_OK;
  }
  if (!c.out_count || !c.out_idx || !c.out_llr || !c.counts_a || (n_cols_b > 0 && !c.b.counts)) return fail(URCCO_BAD_ARG, "urcco_dev_cco_rows: NULL buffer");
  HIPC(hipMemsetAsync(c.out_count, 0, sizeof(int32_t) * (size_t)n, s->stream));
  if (n_cols_b == 0 || n_users == 0) {
    if (c.stats_dev) HIPC(hipMemsetAsync(c.stats_dev, 0, sizeof(int64_t) * URCCO_STATS_LEN, s->stream));
    return URCCO_OK;
  }
  int key_bits = 0;  // packed LDS entry: key = col + 1 in the high bits, count in the low bits
  URC(packed_key_bits(n_cols_b, &key_bits));
  const int count_bits = 32 - key_bits;
  // bin 6 = the multi-pass LDS class; only a k beyond its running lists (or beyond any LDS table) falls back to the dense
  // global-accumulator kernel and pays for its n_cols x 16 B of scratch per resident block
  const bool dense_bin6 = k > urcco::MP_KMAX_HOST || 3ll * k + 5 > 32768ll;
  if (dense_bin6) URC(s->ensure_global_bin(n_cols_b));
  if (!s->xlx_tab.p) {
    URC(s->xlx_tab.alloc(urcco::XLX_TABLE_HOST));
    HIPC(urcco::launch_xlx_table(s->stream, s->xlx_tab.p));
  }
  if (!s->xlx_hi.p) URC(s->xlx_hi.alloc(2 * urcco::XLX_TABLE_HOST + urcco::XLX_TABLE_HOST / 4));  // xLogX(N - d), then columnEntropy(c), then the 16-bit monotone limits
  unsigned short* mono = reinterpret_cast<unsigned short*>(s->xlx_hi.p + 2 * urcco::XLX_TABLE_HOST);
  if (s->xlx_hi_n != n_users) {
    HIPC(urcco::launch_xlx_hi_table(s->stream, s->xlx_hi.p, s->xlx_tab.p, n_users));
    HIPC(urcco::launch_mono_limit(s->stream, mono, s->xlx_tab.p, s->xlx_hi.p, n_users));
    s->xlx_hi_n = n_users;
  }
  const int64_t n_tiles = ((int64_t)n + urcco::BIN_TILE - 1) / urcco::BIN_TILE;
  const int64_t cap = c.nnz_a_bound;
  if (!s->form_word.p) URC(s->form_word.alloc(1));
  s->form_valid = false;
  // the expand tables in the narrow form (32-bit starts; the work prefix as 32-bit words in the front half of wp) or, when the scan's verdict says so, in
  // the wide one (pstart64; wp whole): cco_kernels.h, ExpandForm.  pstart64 is touched by the wide form alone.
  ArenaLayout L(s);
  int64_t *pstart64, *wp, *p_tile_sums, *work, *tile_counts, *stats = c.stats_dev;
  unsigned *own_pstart = nullptr, *b_rp32;
  int32_t *own_plen, *bin_off, *bin_rows, *cnt16_bad;
  double *ent_a, *xlx_n;
  unsigned short *cnt_b16, *pf_limit;
  unsigned long long* cand;
  L.add(&pstart64, (size_t)cap);
  if (!c.pre_pstart) L.add(&own_pstart, (size_t)cap);
  L.add(&own_plen, (size_t)cap).add(&wp, (size_t)cap + 1).add(&p_tile_sums, scan_tile_words(cap));
  L.add(&work, (size_t)n).add(&tile_counts, (size_t)(n_tiles + 1) * urcco::BIN_COLS_HOST);  // binning
  L.add(&bin_off, urcco::BIN_OFF_LEN).add(&bin_rows, (size_t)n);
  L.add(&ent_a, (size_t)n_items_a).add(&cnt_b16, (size_t)n_cols_b).add(&cnt16_bad, 1).add(&pf_limit, (size_t)n_items_a);
  L.add(&cand, urcco::CAND_SLOTS).add(&xlx_n, 1);
  if (!c.stats_dev) L.add(&stats, URCCO_STATS_LEN);
  L.add(&b_rp32, (size_t)n_users + 1);
  URC(L.commit());
  const unsigned* pstart32 = c.pre_pstart ? c.pre_pstart : own_pstart;
  int32_t* form = s->form_word.p;  // (the session's own word, not arena scratch: urcco_session_expand_form reads it after the call)

  // The plan (urcco::RowsPlan), decided here once for the expand scan and for every class's launch.
  // The packed words: B' itself when it is known good -- no plain copy exists, every reader masks -- else its packed copy, unless DBG_UNPACKED_COUNTS asks for
  // the count gather of rounds 1-5 (A/B, tests).
  const int32_t* packed = c.b.known_good() ? c.b.words : ((s->debug & urcco::DBG_UNPACKED_COUNTS) ? nullptr : c.b.packed());
  // Known-good words: the host can know the whole verdict.  B' holds fewer than 2^32 entries (the shard sizes), and a row of B' holds distinct columns, so no
  // tile of 2048 lengths sums to more than 2048 * n_cols_b.  (maxElementsPerRow is no bound: the down-sampling keeps entries at a RATE.)  Then only the packed
  // instantiation of every class is enqueued and the scan sets the word without its tests.
  const bool narrow_known = c.b.known_good() && c.b.nnz_bound >= 0 && c.b.nnz_bound < ((int64_t)1 << 32) &&
                            (unsigned long long)n_cols_b * (unsigned long long)urcco::SCAN_TILE < s->narrow_limit;
  using urcco::RowsPlan;
  const RowsPlan plan = (s->debug & urcco::DBG_ROW_KERNELS) ? RowsPlan::DEBUG : !packed ? RowsPlan::PLAIN : narrow_known ? RowsPlan::PACKED : RowsPlan::DEVICE_DECIDES;
  const urcco::ExpandForm ef{form, c.b.pack_bad(), urcco::plan_runs_pk(plan) ? 0 : 1, plan == RowsPlan::PACKED ? 1 : 0, s->narrow_limit, s->prefix_seed};
  int64_t* tile_sums = c.pre_pstart ? c.pre_tile_sums : p_tile_sums;
  s->begin(URCCO_STAGE_ROW_WORK);
  if (c.pre_pstart)
    HIPC(urcco::launch_expand_scan(s->stream, c.a_col_ptr, n_items_a, c.pre_plen, cap, wp, tile_sums, true, c.pre_pstart, pstart64, ef));
  else
    HIPC(urcco::launch_expand_prepare(s->stream, s->n_cu, c.a_col_ptr, n_items_a, c.a_row_idx, c.b.row_ptr, b_rp32, n_users, cap, own_pstart, pstart64, own_plen, wp, tile_sums, ef));
  HIPC(urcco::launch_row_work(s->stream, s->n_cu, item_lo, item_hi, c.a_col_ptr, wp, tile_sums, form, work));
  s->form_valid = true;
  s->end();
  s->begin(URCCO_STAGE_BINNING);
  HIPC(hipMemsetAsync(stats, 0, sizeof(int64_t) * URCCO_STATS_LEN, s->stream));
  HIPC(urcco::launch_binning(s->stream, item_lo, n, work, c.counts_a, n_cols_b, count_bits, k, tile_counts, bin_off, bin_rows, stats));
  s->end();
  s->begin(URCCO_STAGE_ENTROPY);
  HIPC(urcco::launch_item_entropy(s->stream, c.counts_a, n_items_a, n_users, ent_a, xlx_n, mono, pf_limit));
  HIPC(urcco::launch_narrow_counts(s->stream, s->n_cu, c.b.counts, n_cols_b, cnt_b16, cnt16_bad));
  s->end();

  urcco::CcoArgs a;
  a.bin_rows = bin_rows; a.bin_off = bin_off;
  a.a_col_ptr = c.a_col_ptr; a.pstart32 = pstart32; a.pstart64 = pstart64; a.wp = wp; a.form = form; a.work = work; a.b_col_idx = c.b.words;
  a.b_packed = urcco::plan_runs_pk(plan) ? packed : nullptr; a.pk_known = ef.host_narrow; a.b_col_mask = c.b.col_mask();
  a.cnt_a = c.counts_a; a.cnt_b = c.b.counts; a.ent_a = ent_a; a.cnt_b16 = cnt_b16; a.cnt16_bad = cnt16_bad; a.xlx_n = xlx_n; a.xlx_tab = s->xlx_tab.p; a.xlx_hi = s->xlx_hi.p; a.col_ent = s->xlx_hi.p + urcco::XLX_TABLE_HOST; a.debug = s->debug;
  a.pf_limit = (s->debug & urcco::DBG_NO_PREFILTER) ? nullptr : pf_limit;
  a.n_users = n_users; a.n_cols_b = n_cols_b; a.item_lo = item_lo; a.exclude_self = c.exclude_self ? 1 : 0; a.k = k;
  a.has_min_llr = c.has_min_llr ? 1 : 0; a.min_llr = c.min_llr; a.count_bits = count_bits;
  a.col_bytes = n_cols_b <= (1 << 8) ? 1 : (n_cols_b <= (1 << 16) ? 2 : (n_cols_b <= (1 << 24) ? 3 : 4));
  a.unordered = s->unordered_rows ? 1 : 0;
  a.g_log2 = 4;  // 16 lanes stream one user's B' row: 64 B segments, matches the ~10-40 item rows the cut leaves
  a.out_count = c.out_count; a.out_idx = c.out_idx; a.out_llr = c.out_llr;
  a.err = reinterpret_cast<unsigned long long*>(stats + 1 + 4 * urcco::NBINS);
  a.cand = s->timing ? cand : nullptr;
  if (s->timing) HIPC(hipMemsetAsync(cand, 0, sizeof(unsigned long long) * urcco::CAND_SLOTS, s->stream));
  a.g_counts = s->g_counts.p; a.g_cand_key = s->g_cand_key.p; a.g_cand_col = s->g_cand_col.p; a.g_blocks = dense_bin6 ? s->g_blocks : 0;
  // Heaviest classes first (global, whole-CU, half-CU, ...): they have few, long rows and end raggedly; the fine-grained
  // one-wave and micro classes run last and finish sharply -- and, with a stream per event type, fill the heavy classes'
  // tails of the other event types instead of leaving a tail of their own.
  for (int step = 0; step < urcco::NBINS; ++step) {
    const int bin = urcco::NBINS - 1 - step;
    s->begin(URCCO_STAGE_CCO_BIN0 + bin);
    HIPC(urcco::launch_cco_rows_bin(s->stream, s->n_cu, a, plan, bin, n));
    s->end();
  }
  if (s->timing) HIPC(urcco::launch_bin_out_stats(s->stream, bin_rows, bin_off, item_lo, c.out_count, cand, stats));
  return URCCO_OK;
}

int pack_counts(urcco_session* s, const BPrime& b, int32_t* out, int32_t* bad) {
  if (!s || !b.row_ptr || b.n_rows < 0 || b.nnz_bound < 0 || !out || !bad || (b.nnz_bound > 0 && (!b.words || !b.counts))) return fail(URCCO_BAD_ARG, "pack_counts: bad argument");
  int key_bits = 0;
  URC(packed_key_bits(b.n_cols, &key_bits));
  const int count_bits = 32 - key_bits;
  // the gathers read the 16-bit copy of the counts (half the table: 4 MB for a 2M-item catalogue) -- arena scratch, needed until the pack kernel has run
  unsigned short* c16;
  int32_t* bad16;
  URC(ArenaLayout(s).add(&c16, (size_t)b.n_cols + 8).add(&bad16, 1).commit());
  s->begin(URCCO_STAGE_ENTROPY);
  HIPC(urcco::launch_narrow_counts(s->stream, s->n_cu, b.counts, b.n_cols, c16, bad16));
  HIPC(urcco::launch_pack_counts(s->stream, s->n_cu, b.words, b.row_ptr + b.n_rows, b.nnz_bound, c16, bad16, count_bits, out, bad));
  s->end();
  return URCCO_OK;
}

// Expand preparation of n secondaries in one pass over the CSC of A' (cco_expand.hip, expand_prepare_multi): pstart[d] / plen[d] hold
// cap entries each.  The interleaved (start, length) table lives in the session's arena for the duration of the launch.
int expand_multi(urcco_session* s, int n, const int64_t* a_col_ptr, int32_t n_items_a, const int32_t* a_row_idx, int64_t cap, const int64_t* const* b_row_ptr,
                 int64_t n_users, unsigned* const* pstart, int32_t* const* plen, int64_t* const* tile_sums) {
  if (!s || n < 1 || n > urcco::EXPAND_MULTI_MAX || !a_col_ptr || cap < 0) return fail(URCCO_BAD_ARG, "expand_multi: bad argument");
  unsigned* T;
  // n_users + 1 records of n starts (+ one record of slack: the last user's 2 n-word read)
  URC(ArenaLayout(s).add(&T, ((size_t)n_users + 2) * (size_t)n).commit());
  s->begin(URCCO_STAGE_ROW_WORK);
  HIPC(urcco::launch_expand_prepare_multi(s->stream, s->n_cu, a_col_ptr, n_items_a, a_row_idx, n, b_row_ptr, n_users, cap, pstart, plen, T, tile_sums));
  s->end();
  return URCCO_OK;
}

}  // namespace urcco_detail

extern "C" {

int urcco_dev_compact_indicators(urcco_session* s, int32_t n_rows, int32_t k, const int32_t* count, const int32_t* idx, const double* llr,
                                 int64_t* out_row_ptr, int32_t* out_col_idx, double* out_llr) {
  if (!s || n_rows < 0 || k <= 0 || !out_row_ptr || (n_rows > 0 && (!count || !idx || !llr || !out_col_idx || !out_llr)))
    return fail(URCCO_BAD_ARG, "urcco_dev_compact_indicators: bad argument");
  int64_t* tile_sums;
  URC(ArenaLayout(s).add(&tile_sums, scan_tile_words(n_rows)).commit());
  s->begin(URCCO_STAGE_COMPACT_INDICATORS);
  HIPC(urcco::launch_scan_i32(s->stream, count, n_rows, out_row_ptr, tile_sums));
  HIPC(urcco::launch_compact_indicators(s->stream, n_rows, k, count, idx, llr, out_row_ptr, out_col_idx, out_llr));
  s->end();
  return URCCO_OK;
}

struct urcco_key_table {
  DBuf<unsigned long long> keys;
  DBuf<unsigned> minpos, count;
  DBuf<int32_t> id;
  urcco::KeyTable t{};  // the kernels' view of the four arrays above
  int64_t capacity = 0;
  int device = 0;
  int64_t n_ids = 0;      // ids handed out so far: set by the build, raised by urcco_dev_dictionary_extend
  int32_t min_count = 1;  // what the table was built with: only a table of min_count 1 can be extended (cco_dictionary.h, the invariant)
};

void urcco_key_table_destroy(urcco_key_table* table) {
  if (!table) return;
  (void)hipSetDevice(table->device);
  delete table;
}

int urcco_dev_dictionary_build(urcco_session* s, int64_t n, const uint64_t* keys, const int32_t* select, int32_t min_count,
                               int64_t* first_pos, urcco_key_table** table, int64_t* n_ids) {
  if (!s || n < 0 || (n > 0 && (!keys || !first_pos)) || !table || !n_ids) return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_build: bad argument");
  if (n >= ((int64_t)1 << 32) - 1) return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_build: at most 2^32 - 2 events per stream, got %lld", (long long)n);
  *table = nullptr;
  std::unique_ptr<urcco_key_table, void (*)(urcco_key_table*)> tab(new (std::nothrow) urcco_key_table(), urcco_key_table_destroy);
  if (!tab) return fail(URCCO_OOM_HOST, "key table alloc");
  tab->device = s->device;
  int64_t cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  tab->capacity = cap;
  tab->t.mask = (unsigned long long)cap - 1ull;
  URC(tab->keys.alloc((size_t)cap));
  URC(tab->minpos.alloc((size_t)cap));
  URC(tab->count.alloc((size_t)cap));
  URC(tab->id.alloc((size_t)cap));
  tab->t.keys = tab->keys.p; tab->t.minpos = tab->minpos.p; tab->t.count = tab->count.p; tab->t.id = tab->id.p;
  HIPC(hipMemsetAsync(tab->t.keys, 0xFF, sizeof(unsigned long long) * (size_t)cap, s->stream));
  HIPC(hipMemsetAsync(tab->t.minpos, 0xFF, sizeof(unsigned) * (size_t)cap, s->stream));
  HIPC(hipMemsetAsync(tab->t.count, 0, sizeof(unsigned) * (size_t)cap, s->stream));
  HIPC(hipMemsetAsync(tab->t.id, 0xFF, sizeof(int32_t) * (size_t)cap, s->stream));
  int32_t* flag;
  int64_t *prefix, *tile_sums;
  unsigned* reserved;
  URC(ArenaLayout(s).add(&flag, (size_t)n).add(&prefix, (size_t)n + 1).add(&tile_sums, scan_tile_words(n)).add(&reserved, 1).commit());
  HIPC(urcco::launch_dictionary_build(s->stream, s->n_cu, tab->t, n, reinterpret_cast<const unsigned long long*>(keys), select, min_count, flag, prefix,
                                      tile_sums, first_pos, reserved));
  int64_t ids = 0;
  unsigned n_reserved = 0;
  HIPC(hipMemcpyAsync(&ids, prefix + n, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
  HIPC(hipMemcpyAsync(&n_reserved, reserved, sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
  HIPC(hipStreamSynchronize(s->stream));
  if (n_reserved)  // (the table goes with `tab`; *table stays NULL)
    return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_build: %u selected position(s) hold the reserved key ~0 (2^64 - 1, the integer id -1): it marks an empty slot",
                n_reserved);
  *n_ids = ids;
  tab->n_ids = ids;
  tab->min_count = min_count < 1 ? 1 : min_count;
  *table = tab.release();
  return URCCO_OK;
}

// A batch against a live table (cco_dictionary.h, decision D26).  Nothing of `table` changes before the one synchronisation at the end has shown that the
// batch is accepted: a table that has to grow is rehashed into fresh arrays that replace the old ones only then -- the old arrays are released after the
// stream has passed the rehash, and a refused call leaves them as they were.
int urcco_dev_dictionary_extend(urcco_session* s, urcco_key_table* table, int64_t n, const uint64_t* keys, const int32_t* select, int32_t* ids,
                                int64_t* new_pos, int64_t* n_ids) {
  if (!s || !table || n < 0 || !n_ids || (n > 0 && (!keys || !new_pos))) return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_extend: bad argument");
  if (table->min_count > 1)
    return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_extend: the table was built with min_count %d: its keys without an id cannot be told from new keys",
                table->min_count);
  if (n >= ((int64_t)1 << 32) - 1) return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_extend: at most 2^32 - 2 events per batch, got %lld", (long long)n);
  if (table->n_ids + n > (int64_t)INT32_MAX)
    return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_extend: %lld ids and a batch of %lld could exceed the 2^31 - 1 ids a table holds", (long long)table->n_ids,
                (long long)n);
  if (n == 0) {
    *n_ids = table->n_ids;
    HIPC(hipStreamSynchronize(s->stream));
    return URCCO_OK;
  }
  int64_t need = 1024;  // the build's rule over what the table could hold afterwards: the load never exceeds one half
  while (need < 2 * (table->n_ids + n)) need <<= 1;
  DBuf<unsigned long long> g_keys;
  DBuf<unsigned> g_minpos;
  DBuf<int32_t> g_id;
  urcco::KeyTable t = table->t;
  const bool grow = need > table->capacity;
  if (grow) {
    URC(g_keys.alloc((size_t)need));
    URC(g_minpos.alloc((size_t)need));
    URC(g_id.alloc((size_t)need));
    t.keys = g_keys.p; t.minpos = g_minpos.p; t.id = g_id.p;
    t.count = nullptr;  // only a build with min_count > 1 reads counts
    t.mask = (unsigned long long)need - 1ull;
    HIPC(hipMemsetAsync(t.keys, 0xFF, sizeof(unsigned long long) * (size_t)need, s->stream));
    HIPC(hipMemsetAsync(t.minpos, 0xFF, sizeof(unsigned) * (size_t)need, s->stream));
    HIPC(hipMemsetAsync(t.id, 0xFF, sizeof(int32_t) * (size_t)need, s->stream));
    HIPC(urcco::launch_dictionary_rehash(s->stream, s->n_cu, table->t, t));
  }
  urcco::DictExtend a{};
  a.t = t; a.n = n; a.keys = reinterpret_cast<const unsigned long long*>(keys); a.select = select; a.n_before = table->n_ids; a.ids = ids; a.new_pos = new_pos;
  URC(ArenaLayout(s).add(&a.flag, (size_t)n).add(&a.prefix, (size_t)n + 1).add(&a.tile_sums, scan_tile_words(n)).add(&a.gate, 1).commit());
  HIPC(urcco::launch_dictionary_extend(s->stream, s->n_cu, a));
  int64_t fresh = 0;
  unsigned n_reserved = 0;
  HIPC(hipMemcpyAsync(&fresh, a.prefix + n, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
  HIPC(hipMemcpyAsync(&n_reserved, a.gate, sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
  HIPC(hipStreamSynchronize(s->stream));
  if (n_reserved)  // (the grown arrays go with this frame; the table's own were only read)
    return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_extend: %u selected position(s) hold the reserved key ~0 (2^64 - 1, the integer id -1): it marks an empty slot",
                n_reserved);
  if (grow) {  // the stream has passed the rehash: the move-assignments release the old arrays
    table->keys = std::move(g_keys);
    table->minpos = std::move(g_minpos);
    table->id = std::move(g_id);
    (void)table->count.release();
    table->t = t;
    table->capacity = need;
  }
  table->n_ids += fresh;
  *n_ids = table->n_ids;
  return URCCO_OK;
}

int urcco_dev_dictionary_lookup(urcco_session* s, const urcco_key_table* table, int64_t n, const uint64_t* keys, const int32_t* select,
                                int32_t* ids) {
  if (!s || !table || n < 0 || (n > 0 && (!keys || !ids))) return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_lookup: bad argument");
  HIPC(urcco::launch_dictionary_lookup(s->stream, s->n_cu, table->t, n, reinterpret_cast<const unsigned long long*>(keys), select, ids));
  return URCCO_OK;
}

int urcco_dev_dictionary_verify_against(urcco_session* s, const urcco_key_table* table, int64_t n, const uint64_t* keys, const int32_t* select,
                                        const uint64_t* check_keys, const uint64_t* dict_check_keys, const int64_t* first_pos, int64_t* n_mismatch) {
  if (!s || !table || n < 0 || !n_mismatch || (n > 0 && (!keys || !check_keys || !dict_check_keys || !first_pos)))
    return fail(URCCO_BAD_ARG, "urcco_dev_dictionary_verify: bad argument");
  unsigned long long* err;
  URC(ArenaLayout(s).add(&err, 1).commit());
  HIPC(urcco::launch_dictionary_verify(s->stream, s->n_cu, table->t, n, reinterpret_cast<const unsigned long long*>(keys), select,
                                       reinterpret_cast<const unsigned long long*>(check_keys), reinterpret_cast<const unsigned long long*>(dict_check_keys),
                                       first_pos, err));
  unsigned long long bad = 0;
  HIPC(hipMemcpyAsync(&bad, err, sizeof(bad), hipMemcpyDeviceToHost, s->stream));
  HIPC(hipStreamSynchronize(s->stream));
  *n_mismatch = (int64_t)bad;
  return URCCO_OK;
}

int urcco_dev_dictionary_verify(urcco_session* s, const urcco_key_table* table, int64_t n, const uint64_t* keys, const int32_t* select,
                                const uint64_t* check_keys, const int64_t* first_pos, int64_t* n_mismatch) {
  return urcco_dev_dictionary_verify_against(s, table, n, keys, select, check_keys, check_keys, first_pos, n_mismatch);
}

int urcco_dev_csr_from_pairs(urcco_session* s, int64_t n, const int32_t* rows, const int32_t* cols, int64_t n_rows, int64_t* out_row_ptr,
                             int32_t* out_col_idx, int64_t* nnz) {
  if (!s || n < 0 || n_rows < 0 || !out_row_ptr || (n > 0 && (!rows || !cols || !out_col_idx)))
    return fail(URCCO_BAD_ARG, "urcco_dev_csr_from_pairs: bad argument");
  int32_t *cnt, *tmp;
  int64_t *raw_ptr, *tile_sums;
  ArenaLayout L(s);
  L.add(&cnt, (size_t)n_rows).add(&raw_ptr, (size_t)n_rows + 1).add(&tmp, (size_t)n).add(&tile_sums, scan_tile_words(n_rows));
  URC(L.commit());
  HIPC(urcco::launch_csr_from_pairs(s->stream, s->n_cu, n, rows, cols, n_rows, cnt, raw_ptr, tmp, tile_sums, out_row_ptr, out_col_idx));
  if (nnz) {
    HIPC(hipMemcpyAsync(nnz, out_row_ptr + n_rows, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
    HIPC(hipStreamSynchronize(s->stream));
  }
  return URCCO_OK;
}

int urcco_dev_pop_counts(urcco_session* s, int64_t n_events, const int32_t* item_ids, const int64_t* times_ms, int32_t n_items, int32_t n_intervals,
                         const int64_t* bounds_host, int32_t* counts) {
  if (!s || n_events < 0 || n_items < 0 || n_intervals < 1 || n_intervals > 3 || !bounds_host || (n_events > 0 && (!item_ids || !times_ms)) ||
      (n_items > 0 && !counts))
    return fail(URCCO_BAD_ARG, "urcco_dev_pop_counts: bad argument");
  for (int k = 0; k < n_intervals; ++k)
    if (bounds_host[k + 1] < bounds_host[k]) return fail(URCCO_BAD_ARG, "urcco_dev_pop_counts: interval bounds must not decrease");
  if ((int64_t)n_items * n_intervals > 0x7ffffff0ll) return fail(URCCO_BAD_ARG, "urcco_dev_pop_counts: too many items");
  if (n_items == 0) return URCCO_OK;
  HIPC(urcco::launch_pop_counts(s->stream, s->n_cu, n_events, item_ids, times_ms, n_items, n_intervals, bounds_host, counts));
  return URCCO_OK;
}

}  // extern "C"

// the scratch of n_rows raw rows (cco_sorted_rows.h) of `capacity` entries in all
static void add_raw_rows(ArenaLayout& L, urcco::RawRows* r, size_t n_rows, int64_t capacity) {
  L.add(&r->raw_ptr, n_rows + 1).add(&r->len, n_rows).add(&r->tmp, (size_t)capacity);
  r->capacity = capacity;
}

// urcco_dev_history_bounds / _rows: argument checks and the launch arguments; rows: also the output arrays
static int history_args(const char* who, urcco_session* s, int64_t n_queries, const int32_t* q_users, int64_t n_users, const urcco_hist_event* events, int32_t n_types,
                        const int64_t* extra_row_ptr, const int32_t* extra_col_idx, const int64_t* excl_row_ptr, bool rows, urcco::HistArgs* a) {
  if (!s || n_queries < 0 || n_users < 0 || (n_queries > 0 && !q_users) || !excl_row_ptr) return fail(URCCO_BAD_ARG, "%s: bad argument", who);
  if (n_types < 1 || n_types > URCCO_REC_MAX_CLAUSES || !events) return fail(URCCO_BAD_ARG, "%s: between 1 and %d event types, got %d", who, URCCO_REC_MAX_CLAUSES, n_types);
  if (n_queries * (int64_t)(n_types + 1) > 0x7ffffff0ll) return fail(URCCO_BAD_ARG, "%s: too many queries", who);
  if ((extra_row_ptr == nullptr) != (extra_col_idx == nullptr)) return fail(URCCO_BAD_ARG, "%s: the extra exclusion CSR needs both of its arrays", who);
  *a = urcco::HistArgs{};
  for (int t = 0; t < n_types; ++t) {
    const urcco_hist_event& in = events[t];
    if (in.max_items < 1) return fail(URCCO_BAD_ARG, "%s: event type %d: max_items must be >= 1, got %d", who, t, in.max_items);
    if (in.n_cols < 0 || !in.idx_row_ptr || !in.idx_pos || !in.items || !in.term_row_ptr || (rows && (!in.term_col_idx || in.term_capacity < 0)))
      return fail(URCCO_BAD_ARG, "%s: event type %d: bad argument", who, t);
    urcco::HistEvent& e = a->ev[t];
    e.idx_row_ptr = in.idx_row_ptr; e.idx_pos = in.idx_pos; e.items = in.items; e.times_ms = in.times_ms; e.col_map = in.col_map;
    e.n_cols = in.n_cols; e.max_items = in.max_items; e.blacklist = in.blacklist != 0;
  }
  a->n_queries = n_queries; a->n_users = n_users; a->q_users = q_users; a->extra_row_ptr = extra_row_ptr; a->extra_col_idx = extra_col_idx; a->n_types = n_types;
  return URCCO_OK;
}

extern "C" {

int urcco_dev_history_index(urcco_session* s, int64_t n_events, const int32_t* users, int64_t n_users, int64_t* out_row_ptr, int32_t* out_pos) {
  if (!s || n_events < 0 || n_events > 0x7fffffffll || n_users < 0 || n_users > 0x7ffffff0ll || !out_row_ptr || (n_events > 0 && (!users || !out_pos)))
    return fail(URCCO_BAD_ARG, "urcco_dev_history_index: bad argument (a stream holds fewer than 2^31 events)");
  int32_t* cnt;
  int64_t* tile_sums;
  URC(ArenaLayout(s).add(&cnt, (size_t)n_users).add(&tile_sums, scan_tile_words(n_users)).commit());
  HIPC(urcco::launch_history_index(s->stream, s->n_cu, n_events, users, n_users, cnt, tile_sums, out_row_ptr, out_pos));
  return URCCO_OK;
}

int urcco_dev_history_append(urcco_session* s, int64_t n_old, int64_t n_users_old, const int64_t* old_row_ptr, const int32_t* old_pos, int64_t n_new,
                             const int32_t* new_users, int64_t n_users, int64_t* out_row_ptr, int32_t* out_pos) {
  if (!s || n_old < 0 || n_new < 0 || n_users_old < 0 || n_old > 0x7fffffffll - n_new || n_users < n_users_old || n_users > 0x7ffffff0ll)
    return fail(URCCO_BAD_ARG, "urcco_dev_history_append: bad argument (a stream holds fewer than 2^31 events, the user id space does not shrink)");
  const bool copies = n_users_old > 0 && n_old > 0;
  if (!out_row_ptr || (n_users_old > 0 && !old_row_ptr) || (copies && !old_pos) || (n_new > 0 && !new_users) || ((copies || n_new > 0) && !out_pos))
    return fail(URCCO_BAD_ARG, "urcco_dev_history_append: NULL argument");
  int32_t* cnt;
  int64_t *add, *tile_sums;
  URC(ArenaLayout(s).add(&cnt, (size_t)n_users).add(&add, (size_t)n_users + 1).add(&tile_sums, scan_tile_words(n_users)).commit());
  HIPC(urcco::launch_history_append(s->stream, s->n_cu, n_old, n_users_old, old_row_ptr, old_pos, n_new, new_users, n_users, cnt, add, tile_sums, out_row_ptr, out_pos));
  return URCCO_OK;
}

int urcco_dev_history_trim(urcco_session* s, int64_t n_events, const int32_t* items, const int64_t* times_ms, int64_t n_users, const int64_t* idx_row_ptr,
                           const int32_t* idx_pos, int64_t min_time_ms, int64_t n_drop, const int32_t* drop_users, int32_t* out_items, int64_t* out_times,
                           int64_t* out_row_ptr, int32_t* out_pos, int64_t* out_counts) {
  if (!s || n_events < 0 || n_events > 0x7fffffffll || n_users < 0 || n_users > 0x7ffffff0ll || n_drop < 0)
    return fail(URCCO_BAD_ARG, "urcco_dev_history_trim: bad argument (a stream holds fewer than 2^31 events)");
  if (!out_row_ptr || !out_counts || (n_events > 0 && (!items || !idx_pos || !out_items || !out_pos)) || (n_users > 0 && !idx_row_ptr) || (n_drop > 0 && !drop_users))
    return fail(URCCO_BAD_ARG, "urcco_dev_history_trim: NULL argument");
  if ((times_ms == nullptr) != (out_times == nullptr)) return fail(URCCO_BAD_ARG, "urcco_dev_history_trim: times_ms and out_times are both NULL or both given");
  urcco::TrimArgs a{};
  a.n_events = n_events; a.n_users = n_users; a.n_drop = n_drop; a.min_time_ms = min_time_ms;
  a.items = items; a.times_ms = times_ms; a.idx_row_ptr = idx_row_ptr; a.idx_pos = idx_pos; a.drop_users = drop_users;
  a.out_items = out_items; a.out_times = out_times; a.out_row_ptr = out_row_ptr; a.out_pos = out_pos; a.out_counts = out_counts;
  const size_t n_words = (size_t)((n_events + 63) >> 6);
  URC(ArenaLayout(s).add(&a.s_bits, n_words).add(&a.i_bits, n_words).add(&a.s_cnt, n_words).add(&a.i_cnt, n_words).add(&a.s_base, n_words + 1).add(&a.i_base, n_words + 1)
          .add(&a.tile_sums, scan_tile_words((int64_t)n_words)).commit());
  HIPC(urcco::launch_history_trim(s->stream, s->n_cu, a));
  return URCCO_OK;
}

int urcco_dev_history_cap(urcco_session* s, int64_t n_events, const int32_t* items, const int64_t* times_ms, int64_t n_users, const int64_t* idx_row_ptr,
                          const int32_t* idx_pos, int64_t min_time_ms, int64_t n_drop, const int32_t* drop_users, int32_t max_per_user, int32_t* out_items,
                          int64_t* out_times, int64_t* out_row_ptr, int32_t* out_pos, int64_t* out_counts) {
  if (!s || n_events < 0 || n_events > 0x7fffffffll || n_users < 0 || n_users > 0x7ffffff0ll || n_drop < 0)
    return fail(URCCO_BAD_ARG, "urcco_dev_history_cap: bad argument (a stream holds fewer than 2^31 events)");
  if (max_per_user < 1) return fail(URCCO_BAD_ARG, "urcco_dev_history_cap: max_per_user must be >= 1, got %d", max_per_user);
  if (!out_row_ptr || !out_counts || (n_events > 0 && (!items || !idx_pos || !out_items || !out_pos)) || (n_users > 0 && !idx_row_ptr) || (n_drop > 0 && !drop_users))
    return fail(URCCO_BAD_ARG, "urcco_dev_history_cap: NULL argument");
  if ((times_ms == nullptr) != (out_times == nullptr)) return fail(URCCO_BAD_ARG, "urcco_dev_history_cap: times_ms and out_times are both NULL or both given");
  urcco::CapArgs c{};
  urcco::TrimArgs& a = c.trim;
  c.max_per_user = max_per_user;
  a.n_events = n_events; a.n_users = n_users; a.n_drop = n_drop; a.min_time_ms = min_time_ms;
  a.items = items; a.times_ms = times_ms; a.idx_row_ptr = idx_row_ptr; a.idx_pos = idx_pos; a.drop_users = drop_users;
  a.out_items = out_items; a.out_times = out_times; a.out_row_ptr = out_row_ptr; a.out_pos = out_pos; a.out_counts = out_counts;
  const size_t n_words = (size_t)((n_events + 63) >> 6);
  URC(ArenaLayout(s).add(&a.s_bits, n_words).add(&a.i_bits, n_words).add(&a.s_cnt, n_words).add(&a.i_cnt, n_words).add(&a.s_base, n_words + 1).add(&a.i_base, n_words + 1)
          .add(&a.tile_sums, scan_tile_words((int64_t)n_words)).add(&c.list, (size_t)n_users).add(&c.ctr, 1).commit());
  HIPC(urcco::launch_history_cap(s->stream, s->n_cu, c));
  return URCCO_OK;
}

// the window of urcco_dev_history_users / _matrix: without times only the open one
static bool history_window_ok(const int64_t* times_ms, int64_t t_lo, int64_t t_hi) { return times_ms || (t_lo == INT64_MIN && t_hi == INT64_MAX); }

int urcco_dev_history_users(urcco_session* s, int64_t n_events, const int64_t* times_ms, int64_t n_users, const int64_t* idx_row_ptr, const int32_t* idx_pos, int64_t t_lo,
                            int64_t t_hi, int32_t min_events, int32_t* out_row_of, int64_t* out_n_rows) {
  if (!s || n_events < 0 || n_events > 0x7fffffffll || n_users < 0 || n_users > 0x7ffffff0ll)
    return fail(URCCO_BAD_ARG, "urcco_dev_history_users: bad argument (a stream holds fewer than 2^31 events)");
  if (min_events < 1) return fail(URCCO_BAD_ARG, "urcco_dev_history_users: min_events must be >= 1, got %d", min_events);
  if (!history_window_ok(times_ms, t_lo, t_hi)) return fail(URCCO_BAD_ARG, "urcco_dev_history_users: a window needs times_ms");
  if (!out_n_rows || (n_users > 0 && (!idx_row_ptr || !out_row_of)) || (n_events > 0 && !idx_pos)) return fail(URCCO_BAD_ARG, "urcco_dev_history_users: NULL argument");
  urcco::UsersArgs a{};
  a.n_events = n_events; a.n_users = n_users; a.t_lo = t_lo; a.t_hi = t_hi; a.times_ms = times_ms; a.idx_row_ptr = idx_row_ptr; a.idx_pos = idx_pos;
  a.min_events = min_events; a.out_row_of = out_row_of; a.out_n_rows = out_n_rows;
  const size_t n_words = (size_t)((n_events + 63) >> 6);
  URC(ArenaLayout(s).add(&a.i_bits, n_words).add(&a.i_cnt, n_words).add(&a.i_base, n_words + 1).add(&a.keep, (size_t)n_users).add(&a.prefix, (size_t)n_users + 1)
          .add(&a.tile_sums, scan_tile_words(std::max((int64_t)n_words, n_users))).commit());
  HIPC(urcco::launch_history_users(s->stream, s->n_cu, a));
  return URCCO_OK;
}

int urcco_dev_history_matrix(urcco_session* s, int64_t n_events, const int32_t* items, const int64_t* times_ms, int64_t n_users, const int64_t* idx_row_ptr,
                             const int32_t* idx_pos, int64_t t_lo, int64_t t_hi, int32_t n_cols, const int32_t* row_of, int64_t n_rows, int64_t* out_row_ptr,
                             int32_t* out_col_idx, int64_t capacity, int64_t* out_nnz) {
  if (!s || n_events < 0 || n_events > 0x7fffffffll || n_users < 0 || n_users > 0x7ffffff0ll || n_rows < 0 || n_rows > 0x7ffffff0ll || capacity < 0)
    return fail(URCCO_BAD_ARG, "urcco_dev_history_matrix: bad argument (a stream holds fewer than 2^31 events)");
  if (n_cols < 1) return fail(URCCO_BAD_ARG, "urcco_dev_history_matrix: n_cols must be >= 1, got %d", n_cols);
  if (!row_of && n_rows != n_users) return fail(URCCO_BAD_ARG, "urcco_dev_history_matrix: without row_of every user has a row: n_rows must be n_users");
  if (!history_window_ok(times_ms, t_lo, t_hi)) return fail(URCCO_BAD_ARG, "urcco_dev_history_matrix: a window needs times_ms");
  if (!out_row_ptr || !out_nnz || (n_users > 0 && !idx_row_ptr) || (n_events > 0 && (!items || !idx_pos)) || (capacity > 0 && !out_col_idx))
    return fail(URCCO_BAD_ARG, "urcco_dev_history_matrix: NULL argument");
  urcco::MatrixArgs a{};
  a.n_events = n_events; a.n_users = n_users; a.n_rows = n_rows; a.t_lo = t_lo; a.t_hi = t_hi; a.capacity = capacity;
  a.items = items; a.times_ms = times_ms; a.idx_row_ptr = idx_row_ptr; a.idx_pos = idx_pos; a.row_of = row_of; a.n_cols = n_cols;
  a.out_row_ptr = out_row_ptr; a.out_col_idx = out_col_idx; a.out_nnz = out_nnz;
  // URCCO_HM_BITMAP_BUDGET lowers the bytes the bitmaps of the heavy-row class may take (read per call): with few bytes one block serves many heavy rows
  int64_t budget = urcco::HM_BITMAP_BUDGET;
  if (const char* e = getenv("URCCO_HM_BITMAP_BUDGET")) {
    const long long v = atoll(e);
    if (v >= 0 && v < budget) budget = v;
  }
  a.bm_blocks = n_events > 4096 && n_users > 0 ? urcco::history_bitmap_blocks(n_cols, budget) : 0;  // 4096 = SR_LDS: no raw row of a shorter stream is heavy
  const size_t bm_words = (size_t)a.bm_blocks * (size_t)(((int64_t)n_cols + 31) >> 5);
  URC(ArenaLayout(s).add(&a.tmp, (size_t)n_events).add(&a.len, (size_t)n_rows).add(&a.raw_start, (size_t)n_rows).add(&a.list, (size_t)n_users).add(&a.ctr, 2)
          .add(&a.bitmaps, bm_words).add(&a.tile_sums, scan_tile_words(n_rows)).commit());
  HIPC(urcco::launch_history_matrix(s->stream, s->n_cu, a));
  return URCCO_OK;
}

int urcco_dev_history_ranks(urcco_session* s, const urcco_rank_stream* streams, int32_t n_streams, int32_t n_items, int32_t type, int64_t t_start, int64_t t_end,
                            int64_t* out_rank, int32_t* out_counts) {
  if (!s || n_items < 0 || (n_items > 0 && !out_rank)) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: bad argument");
  if (type < URCCO_RANK_POPULAR || type > URCCO_RANK_HOT) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: type must be popular (1), trending (2) or hot (3), got %d", type);
  if (n_streams < 0 || n_streams > URCCO_RANK_MAX_STREAMS || (n_streams > 0 && !streams))
    return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: between 0 and %d streams, got %d", URCCO_RANK_MAX_STREAMS, n_streams);
  if (t_end < t_start) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: t_end lies before t_start");
  const int n_int = type;  // popular 1, trending 2, hot 3 intervals
  int64_t bounds[4] = {t_start, t_end, t_end, t_end};
  if (n_int > 1) {
    int64_t d;
    if (__builtin_sub_overflow(t_end, t_start, &d)) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: t_end - t_start does not fit 64 bits");
    const int64_t step = d / n_int;  // the reference's integer division (PopModel.scala:133, :158)
    for (int k = 1; k < n_int; ++k) bounds[k] = t_start + k * step;
    bounds[n_int] = t_end;
  }
  if ((int64_t)n_items * 3 > 0x7ffffff0ll) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: too many items");
  const bool open = type == URCCO_RANK_POPULAR && t_start == INT64_MIN && t_end == INT64_MAX;
  urcco::RankStream rs[URCCO_RANK_MAX_STREAMS];
  int64_t total = 0;
  int32_t map_cols = 0;  // the widest stream that is counted in its own column space
  for (int k = 0; k < n_streams; ++k) {
    const urcco_rank_stream& in = streams[k];
    if (in.n_events < 0 || in.n_cols < 0 || (in.n_events > 0 && !in.items)) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: stream %d: bad argument", k);
    if (!in.times_ms && !open) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: stream %d: only the popular ranking over the open window needs no times_ms", k);
    if (in.col_map && (int64_t)in.n_cols * 3 > 0x7ffffff0ll) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: stream %d: too many columns", k);
    total += in.n_events;
    if (total > 0x7fffffffll) return fail(URCCO_BAD_ARG, "urcco_dev_history_ranks: the streams hold 2^31 events or more: the counts are 32-bit");
    if (in.col_map && in.n_events > 0 && in.n_cols > map_cols) map_cols = in.n_cols;
    rs[k] = urcco::RankStream{in.n_events, in.items, in.times_ms, in.col_map, in.n_cols};
  }
  if (n_items == 0) return URCCO_OK;
  int32_t *counts, *col_counts;
  URC(ArenaLayout(s).add(&counts, (size_t)n_items * (size_t)n_int).add(&col_counts, (size_t)map_cols * (size_t)n_int).commit());
  HIPC(urcco::launch_rank_counts(s->stream, s->n_cu, rs, n_streams, n_items, n_int, bounds, t_end == INT64_MAX, counts, col_counts, out_rank, out_counts));
  return URCCO_OK;
}

int urcco_dev_fill_order(urcco_session* s, int32_t n_items, const int64_t* const* ranks, int32_t n_fields, int32_t* out_order) {
  if (!s || n_items < 0 || (n_items > 0 && !out_order)) return fail(URCCO_BAD_ARG, "urcco_dev_fill_order: bad argument");
  if (n_fields < 0 || n_fields > URCCO_RANK_MAX_FIELDS || (n_fields > 0 && !ranks))
    return fail(URCCO_BAD_ARG, "urcco_dev_fill_order: between 0 and %d rank fields, got %d", URCCO_RANK_MAX_FIELDS, n_fields);
  for (int f = 0; f < n_fields; ++f)
    if (!ranks[f]) return fail(URCCO_BAD_ARG, "urcco_dev_fill_order: rank field %d is NULL", f);
  if (n_items == 0) return URCCO_OK;
  urcco::FillOrderScratch w{};
  if (n_fields > 0) {
    const size_t n = (size_t)n_items, m = 256 * (size_t)urcco::fill_order_tiles(n_items);
    URC(ArenaLayout(s).add(&w.keys[0], n).add(&w.keys[1], n).add(&w.ids[0], n).add(&w.ids[1], n).add(&w.differ, 2 * urcco::RANK_MAX_FIELDS).add(&w.hist, m)
            .add(&w.offsets, m + 1).add(&w.tile_sums, scan_tile_words((int64_t)m)).commit());
  }
  HIPC(urcco::launch_fill_order(s->stream, n_items, ranks, n_fields, w, out_order));
  return URCCO_OK;
}

int urcco_dev_history_bounds(urcco_session* s, int64_t n_queries, const int32_t* q_users, int64_t n_users, urcco_hist_event* events, int32_t n_types,
                             const int64_t* extra_row_ptr, const int32_t* extra_col_idx, int64_t* excl_row_ptr) {
  urcco::HistArgs a;
  URC(history_args("urcco_dev_history_bounds", s, n_queries, q_users, n_users, events, n_types, extra_row_ptr, extra_col_idx, excl_row_ptr, false, &a));
  int32_t* bnd;
  int64_t* tile_sums;
  URC(ArenaLayout(s).add(&bnd, (size_t)n_queries * (size_t)(n_types + 1)).add(&tile_sums, scan_tile_words(n_queries)).commit());
  int64_t* rp[URCCO_REC_MAX_CLAUSES];
  for (int t = 0; t < n_types; ++t) rp[t] = events[t].term_row_ptr;
  HIPC(urcco::launch_history_bounds(s->stream, s->n_cu, a, bnd, tile_sums, rp, excl_row_ptr));
  return URCCO_OK;
}

int urcco_dev_history_rows(urcco_session* s, int64_t n_queries, const int32_t* q_users, int64_t n_users, urcco_hist_event* events, int32_t n_types,
                           const int64_t* extra_row_ptr, const int32_t* extra_col_idx, int32_t n_items, int64_t* excl_row_ptr, int32_t* excl_col_idx,
                           int64_t excl_capacity, int64_t* stats_dev) {
  urcco::HistArgs a;
  URC(history_args("urcco_dev_history_rows", s, n_queries, q_users, n_users, events, n_types, extra_row_ptr, extra_col_idx, excl_row_ptr, true, &a));
  if (n_items < 0 || !excl_col_idx || excl_capacity < 0) return fail(URCCO_BAD_ARG, "urcco_dev_history_rows: bad argument");
  const size_t nq = (size_t)n_queries, n_jobs = nq * (size_t)(n_types + 1);
  ArenaLayout L(s);
  int64_t* tile_sums;
  L.add(&tile_sums, scan_tile_words(n_queries)).add(&a.big_list, n_jobs).add(&a.ctr, 1 + URCCO_HIST_STATS_LEN);
  int64_t* rp[URCCO_REC_MAX_CLAUSES];
  int32_t* ci[URCCO_REC_MAX_CLAUSES];
  for (int t = 0; t < n_types; ++t) {
    add_raw_rows(L, &a.ev[t].raw, nq, events[t].term_capacity);
    rp[t] = events[t].term_row_ptr;
    ci[t] = events[t].term_col_idx;
  }
  add_raw_rows(L, &a.excl, nq, excl_capacity);
  URC(L.commit());
  a.n_items = n_items;
  HIPC(urcco::launch_history_rows(s->stream, s->n_cu, a, tile_sums, rp, ci, excl_row_ptr, excl_col_idx, stats_dev));
  return URCCO_OK;
}

}  // extern "C"

// urcco_dev_item_bounds / _rows: argument checks and the launch arguments
static int item_args(const char* who, urcco_session* s, int64_t n_queries, const int32_t* q_items, int32_t n_items, const urcco_item_event* events, int32_t n_types,
                     bool rows, urcco::ItemArgs* a) {
  if (!s || n_queries < 0 || n_items < 0 || (n_queries > 0 && !q_items)) return fail(URCCO_BAD_ARG, "%s: bad argument", who);
  if (n_types < 1 || n_types > URCCO_REC_MAX_CLAUSES || !events) return fail(URCCO_BAD_ARG, "%s: between 1 and %d event types, got %d", who, URCCO_REC_MAX_CLAUSES, n_types);
  if (n_queries * (int64_t)n_types > 0x7ffffff0ll) return fail(URCCO_BAD_ARG, "%s: too many queries", who);
  *a = urcco::ItemArgs{};
  for (int t = 0; t < n_types; ++t) {
    const urcco_item_event& in = events[t];
    if (in.max_terms < 1) return fail(URCCO_BAD_ARG, "%s: event type %d: max_terms must be >= 1, got %d", who, t, in.max_terms);
    if (in.n_cols < 0 || !in.ind_row_ptr || !in.ind_col_idx || !in.term_row_ptr || (rows && (!in.term_col_idx || in.term_capacity < 0)))
      return fail(URCCO_BAD_ARG, "%s: event type %d: bad argument", who, t);
    urcco::ItemEvent& e = a->ev[t];
    e.ind_row_ptr = in.ind_row_ptr; e.ind_col_idx = in.ind_col_idx; e.n_cols = in.n_cols; e.max_terms = in.max_terms;
  }
  a->n_queries = n_queries; a->q_items = q_items; a->n_types = n_types; a->n_items = n_items;
  return URCCO_OK;
}

extern "C" {

int urcco_dev_item_bounds(urcco_session* s, int64_t n_queries, const int32_t* q_items, int32_t n_items, urcco_item_event* events, int32_t n_types) {
  urcco::ItemArgs a;
  URC(item_args("urcco_dev_item_bounds", s, n_queries, q_items, n_items, events, n_types, false, &a));
  int32_t* bnd;
  int64_t* tile_sums;
  URC(ArenaLayout(s).add(&bnd, (size_t)n_queries * (size_t)n_types).add(&tile_sums, scan_tile_words(n_queries)).commit());
  int64_t* rp[URCCO_REC_MAX_CLAUSES];
  for (int t = 0; t < n_types; ++t) rp[t] = events[t].term_row_ptr;
  HIPC(urcco::launch_item_bounds(s->stream, s->n_cu, a, bnd, tile_sums, rp));
  return URCCO_OK;
}

int urcco_dev_item_rows(urcco_session* s, int64_t n_queries, const int32_t* q_items, int32_t n_items, urcco_item_event* events, int32_t n_types, int64_t* stats_dev) {
  urcco::ItemArgs a;
  URC(item_args("urcco_dev_item_rows", s, n_queries, q_items, n_items, events, n_types, true, &a));
  const size_t nq = (size_t)n_queries;
  ArenaLayout L(s);
  int64_t* tile_sums;
  L.add(&tile_sums, scan_tile_words(n_queries)).add(&a.big_list, nq * (size_t)n_types).add(&a.ctr, 1);
  int64_t* rp[URCCO_REC_MAX_CLAUSES];
  int32_t* ci[URCCO_REC_MAX_CLAUSES];
  for (int t = 0; t < n_types; ++t) {
    add_raw_rows(L, &a.ev[t].raw, nq, events[t].term_capacity);
    rp[t] = events[t].term_row_ptr;
    ci[t] = events[t].term_col_idx;
  }
  URC(L.commit());
  HIPC(urcco::launch_item_rows(s->stream, s->n_cu, a, tile_sums, rp, ci, stats_dev));
  return URCCO_OK;
}

}  // extern "C"

// urcco_dev_props_bounds / _rows / _dates: the state's checks and its device form
static int props_state(const char* who, urcco_session* s, int32_t n_items, const urcco_prop_state* state, urcco::PropState* out) {
  if (!s || n_items < 0 || !state || state->n_events < 0 || state->n_events > 0x7fffffffll)
    return fail(URCCO_BAD_ARG, "%s: bad argument (a property's stream holds fewer than 2^31 events)", who);
  if (n_items > 0 && (!state->t_set || !state->pos_set || !state->t_unset)) return fail(URCCO_BAD_ARG, "%s: NULL state array", who);
  *out = urcco::PropState{reinterpret_cast<const unsigned long long*>(state->t_set), state->pos_set, reinterpret_cast<const unsigned long long*>(state->t_unset),
                          reinterpret_cast<const unsigned long long*>(state->t_del), state->n_events};
  return URCCO_OK;
}

static int props_rows_args(const char* who, urcco_session* s, int32_t n_items, const urcco_prop_state* state, const int64_t* val_ptr, const int32_t* values,
                           int64_t n_values, int32_t n_cols, const int64_t* row_ptr, bool rows, urcco::PropRows* a) {
  *a = urcco::PropRows{};
  URC(props_state(who, s, n_items, state, &a->st));
  if (n_values < 0 || n_cols < 0 || !row_ptr || (n_items > 0 && state->n_events > 0 && !val_ptr) || (rows && n_values > 0 && !values))
    return fail(URCCO_BAD_ARG, "%s: bad argument", who);
  a->val_ptr = val_ptr; a->values = values; a->n_values = n_values; a->n_items = n_items; a->n_cols = n_cols;
  return URCCO_OK;
}

extern "C" {

int urcco_dev_props_apply(urcco_session* s, int32_t n_items, int64_t n_new, const int32_t* items, const int64_t* times_ms, const uint8_t* kinds, int64_t pos_base,
                          uint64_t* t_set, uint32_t* pos_set, uint64_t* t_unset) {
  if (!s || n_items < 0 || n_new < 0 || pos_base < 0 || n_new > 0x7fffffffll || pos_base > 0x7fffffffll - n_new)
    return fail(URCCO_BAD_ARG, "urcco_dev_props_apply: bad argument (pos_base + n_new stays below 2^31)");
  if ((n_new > 0 && (!items || !times_ms)) || (n_items > 0 && (!t_set || !pos_set || !t_unset))) return fail(URCCO_BAD_ARG, "urcco_dev_props_apply: NULL argument");
  HIPC(urcco::launch_props_apply(s->stream, s->n_cu, n_items, n_new, items, times_ms, kinds, pos_base, reinterpret_cast<unsigned long long*>(t_set), pos_set,
                                 reinterpret_cast<unsigned long long*>(t_unset)));
  return URCCO_OK;
}

int urcco_dev_props_delete(urcco_session* s, int32_t n_items, int64_t n, const int32_t* items, const int64_t* times_ms, uint64_t* t_del) {
  if (!s || n_items < 0 || n < 0 || n > 0x7fffffffll) return fail(URCCO_BAD_ARG, "urcco_dev_props_delete: bad argument (fewer than 2^31 events a call)");
  if ((n > 0 && (!items || !times_ms)) || (n_items > 0 && !t_del)) return fail(URCCO_BAD_ARG, "urcco_dev_props_delete: NULL argument");
  HIPC(urcco::launch_props_delete(s->stream, s->n_cu, n_items, n, items, times_ms, reinterpret_cast<unsigned long long*>(t_del)));
  return URCCO_OK;
}

int urcco_dev_props_bounds(urcco_session* s, int32_t n_items, const urcco_prop_state* state, const int64_t* val_ptr, int64_t n_values, int64_t* row_ptr) {
  urcco::PropRows a;
  URC(props_rows_args("urcco_dev_props_bounds", s, n_items, state, val_ptr, nullptr, n_values, 0, row_ptr, false, &a));
  int32_t* bnd;
  int64_t* tile_sums;
  URC(ArenaLayout(s).add(&bnd, (size_t)n_items).add(&tile_sums, scan_tile_words(n_items)).commit());
  HIPC(urcco::launch_props_bounds(s->stream, s->n_cu, a, bnd, tile_sums, row_ptr));
  return URCCO_OK;
}

int urcco_dev_props_rows(urcco_session* s, int32_t n_items, const urcco_prop_state* state, const int64_t* val_ptr, const int32_t* values, int64_t n_values, int32_t n_cols,
                         int64_t* row_ptr, int32_t* col_idx, int64_t capacity) {
  urcco::PropRows a;
  URC(props_rows_args("urcco_dev_props_rows", s, n_items, state, val_ptr, values, n_values, n_cols, row_ptr, true, &a));
  if (capacity < 0 || (capacity > 0 && !col_idx)) return fail(URCCO_BAD_ARG, "urcco_dev_props_rows: a capacity needs col_idx, and is not negative");
  ArenaLayout L(s);
  int64_t* tile_sums;
  L.add(&tile_sums, scan_tile_words(n_items));
  add_raw_rows(L, &a.raw, (size_t)n_items, capacity);
  URC(L.commit());
  HIPC(urcco::launch_props_rows(s->stream, s->n_cu, a, tile_sums, row_ptr, col_idx));
  return URCCO_OK;
}

int urcco_dev_props_dates(urcco_session* s, int32_t n_items, const urcco_prop_state* state, const int64_t* date_values, int64_t* out) {
  urcco::PropState st;
  URC(props_state("urcco_dev_props_dates", s, n_items, state, &st));
  if (n_items > 0 && (!out || (state->n_events > 0 && !date_values))) return fail(URCCO_BAD_ARG, "urcco_dev_props_dates: NULL argument");
  HIPC(urcco::launch_props_dates(s->stream, s->n_cu, n_items, st, date_values, out));
  return URCCO_OK;
}

int urcco_dev_props_exists(urcco_session* s, int32_t n_items, const uint64_t* t_del, const uint64_t* const* t_sets, int32_t n_props, uint8_t* out_mask) {
  if (!s || n_items < 0) return fail(URCCO_BAD_ARG, "urcco_dev_props_exists: bad argument");
  if (n_props < 0 || n_props > URCCO_PROP_MAX) return fail(URCCO_BAD_ARG, "urcco_dev_props_exists: between 0 and %d properties, got %d", URCCO_PROP_MAX, n_props);
  if (n_items > 0 && (!t_del || !out_mask || (n_props > 0 && !t_sets))) return fail(URCCO_BAD_ARG, "urcco_dev_props_exists: NULL argument");
  urcco::PropSets sets{};
  sets.n_props = n_items > 0 ? n_props : 0;
  for (int p = 0; p < sets.n_props; ++p) {
    if (!t_sets[p]) return fail(URCCO_BAD_ARG, "urcco_dev_props_exists: t_set array %d is NULL", p);
    sets.t_set[p] = reinterpret_cast<const unsigned long long*>(t_sets[p]);
  }
  HIPC(urcco::launch_props_exists(s->stream, s->n_cu, n_items, reinterpret_cast<const unsigned long long*>(t_del), sets, out_mask));
  return URCCO_OK;
}

int urcco_dev_props_compact(urcco_session* s, int32_t n_items, const urcco_prop_state* state, const int64_t* val_ptr, const int32_t* values, int64_t n_values,
                            const int64_t* date_values, uint32_t* out_pos_set, int32_t* out_old_pos, int64_t* out_val_ptr, int32_t* out_values,
                            int64_t* out_date_values, int64_t* out_counts) {
  urcco::CompactArgs a{};
  URC(props_state("urcco_dev_props_compact", s, n_items, state, &a.st));
  if (n_values < 0 || !out_counts) return fail(URCCO_BAD_ARG, "urcco_dev_props_compact: bad argument");
  if (val_ptr && date_values) return fail(URCCO_BAD_ARG, "urcco_dev_props_compact: a property holds lists (val_ptr) or dates (date_values), not both");
  const bool any = n_items > 0 && state->n_events > 0;  // a winner may exist
  if ((n_items > 0 && !out_pos_set) || (any && !out_old_pos) || (val_ptr && !out_val_ptr) || (val_ptr && any && n_values > 0 && (!values || !out_values)) ||
      (date_values && any && !out_date_values))
    return fail(URCCO_BAD_ARG, "urcco_dev_props_compact: NULL argument");
  a.val_ptr = val_ptr; a.values = values; a.n_values = val_ptr ? n_values : 0; a.date_values = date_values; a.n_items = n_items;
  a.out_pos_set = out_pos_set; a.out_old_pos = out_old_pos; a.out_val_ptr = out_val_ptr; a.out_values = out_values; a.out_date_values = out_date_values;
  a.out_counts = out_counts;
  const size_t n_words = (size_t)((state->n_events + 63) >> 6);
  const size_t k_max = (size_t)((int64_t)n_items < state->n_events ? (int64_t)n_items : state->n_events);
  URC(ArenaLayout(s).add(&a.bits, n_words).add(&a.cnt, n_words).add(&a.base, n_words + 1).add(&a.len, k_max).add(&a.src, k_max).add(&a.val_base, k_max + 1)
          .add(&a.tile_sums, scan_tile_words((int64_t)(n_words > k_max ? n_words : k_max))).commit());
  HIPC(urcco::launch_props_compact(s->stream, s->n_cu, a));
  return URCCO_OK;
}

}  // extern "C"

// urcco_dev_recommend (n_rules == 0), urcco_dev_recommend_rules and urcco_dev_recommend_weighted (clause_weights != NULL)
static int recommend_call(urcco_session* s, int64_t n_queries, int32_t n_items, const urcco_rec_clause* clauses, int32_t n_clauses, const int64_t* excl_row_ptr,
                          const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order, int32_t num, int32_t flags, int32_t* out_count,
                          int32_t* out_idx, double* out_score, int64_t* stats_dev, const urcco_rec_rule* rules, int32_t n_rules,
                          const uint32_t* const* clause_weights) {
  if (!s || n_queries < 0 || n_queries > 0x7fffffffll || n_items < 0 || n_items == 0x7fffffff) return fail(URCCO_BAD_ARG, "urcco_dev_recommend: bad argument");
  if (num < 1 || num > URCCO_REC_MAX_NUM) return fail(URCCO_BAD_ARG, "urcco_dev_recommend: num must lie in 1..%d, got %d", URCCO_REC_MAX_NUM, num);
  if (n_clauses < 0 || n_clauses > URCCO_REC_MAX_CLAUSES || (n_clauses > 0 && !clauses))
    return fail(URCCO_BAD_ARG, "urcco_dev_recommend: between 0 and %d clauses, got %d", URCCO_REC_MAX_CLAUSES, n_clauses);
  if ((excl_row_ptr == nullptr) != (excl_col_idx == nullptr)) return fail(URCCO_BAD_ARG, "urcco_dev_recommend: the exclusion CSR needs both of its arrays");
  if (flags & ~URCCO_REC_NO_BACKFILL) return fail(URCCO_BAD_ARG, "urcco_dev_recommend: unknown flags %d", flags);
  if (n_queries > 0 && (!out_count || !out_idx || !out_score)) return fail(URCCO_BAD_ARG, "urcco_dev_recommend: output arrays missing");
  urcco::RecClause cl[URCCO_REC_MAX_CLAUSES];
  for (int c = 0; c < n_clauses; ++c) {
    const urcco_rec_clause& in = clauses[c];
    if (!(in.boost > 0.0) || in.boost > 1.7976931348623157e308) return fail(URCCO_BAD_ARG, "urcco_dev_recommend: clause %d: the boost must be positive and finite", c);
    if (in.n_cols < 0 || (in.ind_col_ptr == nullptr) != (in.ind_row_idx == nullptr) || (in.q_row_ptr == nullptr) != (in.q_col_idx == nullptr) || !in.ind_col_ptr || !in.q_row_ptr)
      return fail(URCCO_BAD_ARG, "urcco_dev_recommend: clause %d: bad matrix", c);
    cl[c] = urcco::RecClause{in.ind_col_ptr, in.ind_row_idx, in.q_row_ptr, in.q_col_idx, in.boost, in.n_cols, 0};
  }
  if (n_rules < 0 || n_rules > URCCO_REC_MAX_RULES || (n_rules > 0 && !rules))
    return fail(URCCO_BAD_ARG, "urcco_dev_recommend_rules: between 0 and %d rules, got %d", URCCO_REC_MAX_RULES, n_rules);
  urcco::RecRule rl[URCCO_REC_MAX_RULES];
  for (int j = 0; j < n_rules; ++j) {
    const urcco_rec_rule& in = rules[j];
    if (in.kind == URCCO_RULE_ANY || in.kind == URCCO_RULE_NONE) {
      if (in.n_cols < 0 || !in.m_row_ptr || !in.m_col_idx || !in.q_row_ptr || !in.q_col_idx) return fail(URCCO_BAD_ARG, "urcco_dev_recommend_rules: rule %d: bad matrix", j);
    } else if (in.kind == URCCO_RULE_RANGE) {
      if (in.n_cols < 0 || !in.item_value || !in.q_lo || !in.q_hi) return fail(URCCO_BAD_ARG, "urcco_dev_recommend_rules: rule %d: a range needs item_value, q_lo and q_hi", j);
    } else {
      return fail(URCCO_BAD_ARG, "urcco_dev_recommend_rules: rule %d: unknown kind %d", j, in.kind);
    }
    rl[j] = urcco::RecRule{in.m_row_ptr, in.m_col_idx, in.q_row_ptr, in.q_col_idx, in.item_value, in.q_lo, in.q_hi, in.kind, in.n_cols};
  }
  // URCCO_REC_LDS_LIMIT lowers the work bound up to which a query runs in the LDS class (read per call): small test shapes reach the global class with it
  int32_t lds_limit = urcco::REC_LDS_LIMIT;
  if (const char* e = getenv("URCCO_REC_LDS_LIMIT")) {
    const long v = atol(e);
    if (v >= 0 && v < lds_limit) lds_limit = (int32_t)v;
  }
  // the weighted kernels run when a clause carries an array: without one every weight is WEIGHT_ONE, which the unweighted kernels compute bit for bit
  bool weighted = false;
  for (int c = 0; clause_weights && c < n_clauses; ++c) weighted = weighted || clause_weights[c] != nullptr;
  const int32_t g_blocks = urcco::recommend_global_blocks(n_queries, n_items, s->n_cu, weighted);
  const size_t slice = (size_t)g_blocks * (size_t)(n_items > 0 ? n_items : 1);
  ArenaLayout L(s);
  unsigned long long* ctr;
  int32_t *list, *pos, *g_list;
  unsigned *g_state, *g_m;
  double* g_score;
  unsigned long long* g_m64;
  L.add(&ctr, 8).add(&list, (size_t)n_queries).add(&pos, (size_t)n_items);
  L.add(&g_state, slice).add(&g_m, weighted ? 1 : slice).add(&g_list, slice).add(&g_score, slice);  // the global class's per-block slices
  L.add(&g_m64, weighted ? slice : 1);                                                               // ... the weighted call counts in 64 bits instead of g_m
  URC(L.commit());
  HIPC(urcco::launch_recommend(s->stream, s->n_cu, n_queries, n_items, cl, n_clauses, excl_row_ptr, excl_col_idx, item_mask, fill_order, num, flags, out_count, out_idx,
                               out_score, stats_dev, ctr, list, pos, g_blocks, g_state, g_m, g_list, g_score, lds_limit, rl, n_rules, weighted ? clause_weights : nullptr,
                               g_m64));
  return URCCO_OK;
}

extern "C" {

int urcco_dev_recommend(urcco_session* s, int64_t n_queries, int32_t n_items, const urcco_rec_clause* clauses, int32_t n_clauses, const int64_t* excl_row_ptr,
                        const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order, int32_t num, int32_t flags, int32_t* out_count,
                        int32_t* out_idx, double* out_score, int64_t* stats_dev) {
  return recommend_call(s, n_queries, n_items, clauses, n_clauses, excl_row_ptr, excl_col_idx, item_mask, fill_order, num, flags, out_count, out_idx, out_score, stats_dev,
                        nullptr, 0, nullptr);
}

int urcco_dev_recommend_rules(urcco_session* s, int64_t n_queries, int32_t n_items, const urcco_rec_clause* clauses, int32_t n_clauses, const int64_t* excl_row_ptr,
                              const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order, int32_t num, int32_t flags, int32_t* out_count,
                              int32_t* out_idx, double* out_score, int64_t* stats_dev, const urcco_rec_rule* rules, int32_t n_rules) {
  return recommend_call(s, n_queries, n_items, clauses, n_clauses, excl_row_ptr, excl_col_idx, item_mask, fill_order, num, flags, out_count, out_idx, out_score, stats_dev,
                        rules, n_rules, nullptr);
}

int urcco_dev_recommend_weighted(urcco_session* s, int64_t n_queries, int32_t n_items, const urcco_rec_clause* clauses, int32_t n_clauses, const int64_t* excl_row_ptr,
                                 const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order, int32_t num, int32_t flags, int32_t* out_count,
                                 int32_t* out_idx, double* out_score, int64_t* stats_dev, const urcco_rec_rule* rules, int32_t n_rules,
                                 const uint32_t* const* clause_weights) {
  return recommend_call(s, n_queries, n_items, clauses, n_clauses, excl_row_ptr, excl_col_idx, item_mask, fill_order, num, flags, out_count, out_idx, out_score, stats_dev,
                        rules, n_rules, clause_weights);
}

int urcco_dev_idf_weights(urcco_session* s, int32_t n_cols, const int64_t* ind_col_ptr, int64_t n_docs, uint32_t* out_weight) {
  if (!s || n_cols < 0 || n_docs < 1) return fail(URCCO_BAD_ARG, "urcco_dev_idf_weights: n_cols must be >= 0 and n_docs >= 1");
  if (n_cols > 0 && (!ind_col_ptr || !out_weight)) return fail(URCCO_BAD_ARG, "urcco_dev_idf_weights: an array is missing");
  HIPC(urcco::launch_idf_weights(s->stream, s->n_cu, n_cols, ind_col_ptr, n_docs, out_weight));
  return URCCO_OK;
}

int urcco_dev_rank_metrics(urcco_session* s, int64_t n_queries, int32_t num, const int32_t* rec_count, const int32_t* rec_idx, const int64_t* truth_row_ptr,
                           const int32_t* truth_col_idx, const int32_t* ks_host, int32_t n_ks, const double* discount, int32_t* out_hits, double* out_ap, double* out_ndcg,
                           int64_t* out_sums_i, double* out_sums_f) {
  if (!s || n_queries < 0) return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: bad argument");
  if (num < 1 || num > URCCO_REC_MAX_NUM) return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: num must lie in 1..%d, got %d", URCCO_REC_MAX_NUM, num);
  if (n_ks < 1 || n_ks > URCCO_EVAL_MAX_KS || !ks_host) return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: between 1 and %d cut-offs, got %d", URCCO_EVAL_MAX_KS, n_ks);
  for (int x = 0; x < n_ks; ++x)
    if (ks_host[x] < 1 || ks_host[x] > num || (x > 0 && ks_host[x] <= ks_host[x - 1]))
      return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: the cut-offs must ascend strictly inside 1..num");
  if (n_queries * (int64_t)n_ks > 0x7fffffffll) return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: too many queries");
  if ((discount == nullptr) != (out_ndcg == nullptr)) return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: discount and out_ndcg go together");
  if ((out_sums_i == nullptr) != (out_sums_f == nullptr)) return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: the sums need both of their arrays");
  if (n_queries > 0 && (!rec_count || !rec_idx || !truth_row_ptr || !truth_col_idx || !out_hits || !out_ap))
    return fail(URCCO_BAD_ARG, "urcco_dev_rank_metrics: an array is missing");
  double *ideal, *pa, *pb;
  size_t na = 0, nb = 0;
  if (out_sums_f) urcco::tree_sum_scratch(n_queries, n_ks, &na, &nb);
  URC(ArenaLayout(s).add(&ideal, (size_t)num + 1).add(&pa, na).add(&pb, nb).commit());
  HIPC(urcco::launch_rank_metrics(s->stream, s->n_cu, n_queries, num, rec_count, rec_idx, truth_row_ptr, truth_col_idx, ks_host, n_ks, discount, ideal, out_hits, out_ap,
                                  out_ndcg, out_sums_i, out_sums_f, pa, pb));
  return URCCO_OK;
}

int urcco_dev_tree_sum(urcco_session* s, int64_t n, int32_t n_cols, const double* x, double* out) {
  if (!s || n < 0 || n_cols < 1 || n_cols > 1024 || !out || (n > 0 && !x) || n * (int64_t)n_cols > 0x7fffffffll)
    return fail(URCCO_BAD_ARG, "urcco_dev_tree_sum: bad argument");
  double *pa, *pb;
  size_t na, nb;
  urcco::tree_sum_scratch(n, n_cols, &na, &nb);
  URC(ArenaLayout(s).add(&pa, na).add(&pb, nb).commit());
  HIPC(urcco::launch_tree_sum(s->stream, x, n, n_cols, out, pa, pb));
  return URCCO_OK;
}

int urcco_dev_llr(urcco_session* s, int64_t n, const int64_t* with_a, const int64_t* with_b, const int64_t* with_ab, const int64_t* n_users,
                  double* out) {
  if (!s || n < 0) return fail(URCCO_BAD_ARG, "urcco_dev_llr: bad argument");
  HIPC(urcco::launch_llr_test(s->stream, n, with_a, with_b, with_ab, n_users, out));
  return URCCO_OK;
}

int urcco_dev_u01(urcco_session* s, int64_t n, int32_t seed, const int32_t* row, const int32_t* col, double* out) {
  if (!s || n < 0) return fail(URCCO_BAD_ARG, "urcco_dev_u01: bad argument");
  HIPC(urcco::launch_u01_test(s->stream, n, (uint32_t)seed, row, col, out));
  return URCCO_OK;
}

int urcco_dev_u01_rng(urcco_session* s, int64_t n, int32_t seed, const int32_t* row, const int32_t* col, int32_t rng, double* out) {
  if (!s || n < 0 || (rng != URCCO_RNG_SPLITMIX53 && rng != URCCO_RNG_MIX32)) return fail(URCCO_BAD_ARG, "urcco_dev_u01_rng: bad argument");
  HIPC(urcco::launch_u01_test(s->stream, n, (uint32_t)seed, row, col, out, rng == URCCO_RNG_MIX32 ? 1 : 0));
  return URCCO_OK;
}

}  // extern "C"
