// Internals shared by the C-ABI translation units of liburcco (urcco_api.hip: sessions + device-level stages;
// urcco_context.hip: persistent contexts, the host level, the multi-GPU build).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/urcco.h"
#include "cco_kernels.h"
static_assert(urcco::EXCH_SIZES == URCCO_EXCH_SIZES && urcco::STATS_LEN == URCCO_STATS_LEN, "include/urcco.h and cco_kernels.h agree");
static_assert(urcco::REC_MAX_CLAUSES == URCCO_REC_MAX_CLAUSES && urcco::REC_MAX_NUM == URCCO_REC_MAX_NUM && urcco::REC_NO_BACKFILL == URCCO_REC_NO_BACKFILL &&
                  urcco::REC_STATS_LEN == URCCO_REC_STATS_LEN && urcco::REC_MAX_RULES == URCCO_REC_MAX_RULES && urcco::REC_RULE_ANY == URCCO_RULE_ANY &&
                  urcco::REC_RULE_NONE == URCCO_RULE_NONE && urcco::REC_RULE_RANGE == URCCO_RULE_RANGE &&
                  urcco::REC_WEIGHT_ONE == URCCO_REC_WEIGHT_ONE && urcco::REC_WEIGHT_MAX == URCCO_REC_WEIGHT_MAX,
              "include/urcco.h and cco_kernels.h agree on the recommendation call");
static_assert(urcco::HIST_STATS_LEN == URCCO_HIST_STATS_LEN, "include/urcco.h and cco_kernels.h agree on the history calls");
static_assert(urcco::EVAL_MAX_KS == URCCO_EVAL_MAX_KS, "include/urcco.h and cco_kernels.h agree on the evaluation call");
static_assert(urcco::RANK_MAX_STREAMS == URCCO_RANK_MAX_STREAMS && urcco::RANK_MAX_FIELDS == URCCO_RANK_MAX_FIELDS && urcco::RANK_NONE == URCCO_RANK_NONE,
              "include/urcco.h and cco_kernels.h agree on the rank calls");

struct urcco_session;
namespace urcco_detail {

char* err_buf();  // thread-local message buffer of urcco_last_error (512 bytes)

inline int fail(int status, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return status;
}

inline int hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? URCCO_OOM_DEVICE : URCCO_HIP_ERROR, "%s: %s", what, hipGetErrorString(e));
}

#define HIPC(expr)                                                  \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) return urcco_detail::hip_fail(_e, #expr); \
  } while (0)

#define URC(expr)                  \
  do {                             \
    int _s = (expr);               \
    if (_s != URCCO_OK) return _s; \
  } while (0)

// No C++ exception crosses the C ABI: every extern "C" entry point that can allocate runs its body through this.
template <typename F>
inline int guarded(F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(URCCO_OOM_HOST, "out of host memory");
  } catch (const std::exception& e) {
    return fail(URCCO_INTERNAL, "unexpected exception: %s", e.what());
  } catch (...) {
    return fail(URCCO_INTERNAL, "unexpected exception");
  }
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Fault-hunting aids, off unless the environment asks (read once; urcco_api.hip):
//   URCCO_DEBUG_MARKS=1   flight recorder: every launch group of every session writes "begun" / "finished" marks (build ordinal, stage)
//                         into pinned host memory, in stream order; a SIGABRT handler (the HSA runtime aborts the process on a GPU
//                         memory fault) prints every session's last marks, so the launch groups in flight at the fault are known
//   URCCO_DEBUG_POISON=1  every fresh device allocation of the library and the WHOLE scratch arena at every ArenaLayout::commit() are filled with
//                         0x7f bytes (stream-ordered): a kernel that consumes memory nobody wrote meets an index ~2^31 elements away
//                         (or a 64-bit offset beyond the address space) instead of a stale but plausible value
struct DebugCfg { bool marks = false, poison = false; };
const DebugCfg& debug_cfg();
void debug_mark(urcco_session* s, int which /*0: begun, 1: finished*/, int stage);
void debug_register(urcco_session* s);
void debug_unregister(urcco_session* s);
void debug_poison(void* p, size_t bytes, hipStream_t st, bool async);

inline int ceil_log2_i64(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

// words of scan-tile sums a tiled scan over n elements needs (the launch_scan_* family of cco_kernels.h)
inline size_t scan_tile_words(int64_t n) { return (size_t)((n + urcco::SCAN_TILE - 1) / urcco::SCAN_TILE + 2); }

// packed accumulator entry: key = column + 1 in the high bits, count in the low ones.  *key_bits = the bits of a key (values 1..n_cols_b; the column
// itself fits them too), the count keeps the other 32 - *key_bits
inline int key_bits_of(int64_t n_cols_b) {
  int b = 1;
  while (((int64_t)1 << b) <= n_cols_b) ++b;
  return b;
}
inline int packed_key_bits(int32_t n_cols_b, int* key_bits) {
  const int b = key_bits_of(n_cols_b);
  if (32 - b < 1) return fail(URCCO_BAD_ARG, "n_cols_b %d too large for the packed accumulator", n_cols_b);
  *key_bits = b;
  return URCCO_OK;
}

// B': the matrix a GPU multiplies A' with, as the row kernels take it.  What `words` hold comes in exactly three forms, and only the two members below set one:
//   plain (the constructor, packed_good = false): column indices; the row kernels gather the columns' counts
//   plain + packed copy (with_copy() of a plain one): column indices, and beside them the copy with the counts aboard that launch_pack_counts made (`packed`)
//       with its device-side verdict (`pack_bad`): the device decides which of the two is read
//   packed, known good (the constructor, packed_good = true): col | cB << key bits, and the HOST knows that every count fits (the rows a sharded build
//       received travelled in that form); no plain copy exists, every reader masks.  nnz_bound is then one the host trusts (< 0: none)
struct BPrime {
  const int64_t* row_ptr = nullptr;
  const int32_t *words = nullptr, *counts = nullptr;  // counts: the columns' post-sampling counts
  int64_t n_rows = 0, nnz_bound = -1;
  int32_t n_cols = 0;
  BPrime() = default;
  BPrime(const int64_t* rp, const int32_t* w, int64_t rows, int64_t bound, int32_t cols, const int32_t* cnt, bool packed_good)
      : row_ptr(rp), words(w), counts(cnt), n_rows(rows), nnz_bound(bound), n_cols(cols), good_(packed_good) {}
  BPrime with_copy(const int32_t* packed, const int32_t* pack_bad) const {  // (both non-NULL; a copy never comes with known-good words)
    BPrime b(row_ptr, words, n_rows, nnz_bound, n_cols, counts, false);
    b.packed_ = packed; b.pack_bad_ = pack_bad;
    return b;
  }
  bool known_good() const { return good_; }
  const int32_t* packed() const { return packed_; }      // NULL unless with_copy()
  const int32_t* pack_bad() const { return pack_bad_; }  // ... and so is this
  // words[e] & col_mask() = the column (CcoArgs::b_col_mask, urcco_dev_result::sampled_col_mask)
  uint32_t col_mask() const { return good_ ? (1u << key_bits_of(n_cols)) - 1u : 0xffffffffu; }  // (a 32-bit n_cols has at most 31 key bits)

 private:
  bool good_ = false;
  const int32_t *packed_ = nullptr, *pack_bad_ = nullptr;
};

// ---- owners of device objects: move-only, released by their destructors, so a struct that holds them needs no release list.  What it does need:
// its device is current and its streams are drained when it goes away (urcco_session_destroy, urcco_context_destroy) ----
template <typename T>
struct DBuf {  // device buffer that only grows (hipFree synchronises the device: growth happens on the first builds only)
  T* p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(DBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DBuf& operator=(DBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }  // (o frees what this held)
  ~DBuf() { (void)release(); }
  int release() {  // with hipFree's status, for the paths that can report it
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr; cap = 0;
    return e == hipSuccess ? URCCO_OK : hip_fail(e, "hipFree");
  }
  // Exactly n elements, whatever it held before; no growth slack and NO poison fill (fixed-size tables their owner sizes itself): else use ensure().
  int alloc(size_t n) {
    URC(release());
    HIPC(hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
    return URCCO_OK;
  }
  int ensure(size_t n) {
    if (n <= cap && p) return URCCO_OK;
    size_t want = n + n / 16 + 64;
#ifdef HIPSIM_HOST_BUILD  // test-only host simulator: no slack, so that an overrun meets the guard page
    if (hipsim::guard_on()) want = n ? n : 1;
#endif
    URC(alloc(want));
    if (debug_cfg().poison) debug_poison(p, want * sizeof(T), nullptr, false);
    return URCCO_OK;
  }
};

struct Event {  // an event without timing, created on first use under the device that is current then
  struct Destroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
  std::unique_ptr<std::remove_pointer<hipEvent_t>::type, Destroy> e;
  int ensure() {
    hipEvent_t raw = nullptr;
    if (!e) { HIPC(hipEventCreateWithFlags(&raw, hipEventDisableTiming)); e.reset(raw); }
    return URCCO_OK;
  }
  operator hipEvent_t() const { return e.get(); }
};

struct MappedWord {  // one host-mapped, coherent pinned word the GPU stores to: `word` is the CPU's address of it, `dev` the GPU's
  struct Free { void operator()(unsigned long long* p) const { (void)hipHostFree(p); } };
  std::unique_ptr<unsigned long long, Free> word;
  unsigned long long* dev = nullptr;
  int ensure() {
    unsigned long long* raw = nullptr;
    if (word) return URCCO_OK;
    HIPC(hipHostMalloc((void**)&raw, sizeof(*raw), hipHostMallocMapped | hipHostMallocCoherent));
    word.reset(raw);
    HIPC(hipHostGetDevicePointer((void**)&dev, raw, 0));
    return URCCO_OK;
  }
};

}  // namespace urcco_detail

namespace urcco_detail {
// One A'B call: urcco_dev_cco_rows, urcco_dev_cco_rows_packed and the contexts' stage_rows fill it by name.
struct RowsCall {
  int32_t item_lo = 0, item_hi = 0, n_items_a = 0;  // the item range of A', its CSC and its post-sampling counts
  const int64_t* a_col_ptr = nullptr;
  const int32_t *a_row_idx = nullptr, *counts_a = nullptr;
  int64_t nnz_a_bound = 0, n_users = 0;
  BPrime b;
  int32_t exclude_self = 0, k = 0, has_min_llr = 0;
  double min_llr = 0.0;
  int32_t *out_count = nullptr, *out_idx = nullptr;  // strided by k
  double* out_llr = nullptr;
  int64_t* stats_dev = nullptr;  // nullable
  // this event type's share of a fused expand preparation (expand_multi), with the scan-tile sums of plen: all three, or none (it prepares its own)
  const unsigned* pre_pstart = nullptr; const int32_t* pre_plen = nullptr; int64_t* pre_tile_sums = nullptr;
};
int cco_rows_impl(urcco_session* s, const RowsCall& c);
// The copy of a plain B' with the counts aboard (BPrime::with_copy): out[e] = words[e] | counts[words[e]] << key bits, e < row_ptr[n_rows] (<= nnz_bound); bad[0] = counts that do not fit
int pack_counts(urcco_session* s, const BPrime& b, int32_t* out, int32_t* bad);
int partition_dev(urcco_session* s, int32_t n_items, const int64_t* work, int32_t n_parts, int32_t* bounds_dev, int32_t** bounds_out);
int expand_multi(urcco_session* s, int n, const int64_t* a_col_ptr, int32_t n_items_a, const int32_t* a_row_idx, int64_t cap, const int64_t* const* b_row_ptr,
                 int64_t n_users, unsigned* const* pstart, int32_t* const* plen, int64_t* const* tile_sums = nullptr /* [d]: scan_tile_words(cap) words */);
}  // namespace urcco_detail

using namespace urcco_detail;

struct urcco_session {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 256;
  DBuf<char> arena;  // stage scratch: laid out, grown and carved by ArenaLayout alone (below)
  // persistent zeroed dense counters + candidate scratch of the global-accumulator kernel
  DBuf<int32_t> g_counts;
  DBuf<unsigned long long> g_cand_key;
  DBuf<int32_t> g_cand_col;
  int64_t g_cols = 0;
  DBuf<double> xlx_tab;  // xLogX of small integers (N-independent), filled once
  DBuf<double> xlx_hi;   // xLogX(N - d) for the N of the last build
  long long xlx_hi_n = -1;
  int debug = 0;              // urcco::DBG_* bits (urcco_session_set_debug)
  unsigned long long narrow_limit = urcco::NARROW_LIMIT;  // urcco_session_set_expand_test (test hook): the tile sum from which the expand tables take the wide form
  long long prefix_seed = 0;                              // ... and where the work prefix starts
  DBuf<int32_t> form_word;                                // [1] the form of the expand tables of the session's last build (urcco::ExpandForm), allocated on first use
  bool form_valid = false;                                // a cco_rows_impl has written it
  unsigned* marks = nullptr;  // URCCO_DEBUG_MARKS: pinned host words [0] last launch group begun, [1] last finished ((ordinal << 8) | stage)
  unsigned mark_seq = 0;
  int unordered_rows = 0;     // URCCO_FLAG_UNORDERED_ROWS of the owning context
  // optional per-stage HIP-event timing (bench.py's roofline numbers)
  bool timing = false;
  struct Rec { int stage; hipEvent_t e0, e1; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> free_events;
  double acc_ms[URCCO_N_STAGES] = {0};
  int64_t acc_n[URCCO_N_STAGES] = {0};

  // Timing bookkeeping never throws across the C ABI: an allocation failure just drops the sample.
  hipEvent_t get_event() noexcept {
    if (!free_events.empty()) { hipEvent_t e = free_events.back(); free_events.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  void begin(int stage) noexcept {
    cur_stage = stage;
    if (marks) debug_mark(this, 0, stage);
    if (!timing) return;
    try {
      recs.reserve(recs.size() + 1);
      free_events.reserve(free_events.size() + 2 * (recs.size() + 1));
    } catch (...) {
      open_rec = false;
      return;
    }
    Rec r{stage, get_event(), get_event()};
    if (!r.e0 || !r.e1) { open_rec = false; return; }
    (void)hipEventRecord(r.e0, stream);
    recs.push_back(r);
    open_rec = true;
  }
  bool open_rec = false;
  int cur_stage = 0;
  void end() noexcept {
    if (marks) debug_mark(this, 1, cur_stage);
    if (!timing || !open_rec || recs.empty()) return;
    (void)hipEventRecord(recs.back().e1, stream);
    open_rec = false;
  }
  void collect() {
    (void)hipStreamSynchronize(stream);
    for (const Rec& r : recs) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { acc_ms[r.stage] += ms; acc_n[r.stage] += 1; }
      free_events.push_back(r.e0);
      free_events.push_back(r.e1);
    }
    recs.clear();
  }

  // Dense per-block counters of the global-accumulator class: g_blocks x n_cols_b x 16 B.  The block count shrinks with
  // the width of B so that the scratch stays within 1 GiB per session (4 GiB from 1M columns on: 128 blocks at 2M, 26 at 10M, never fewer
  // than 2): the class serves the rows no LDS table can hold -- a handful under a Zipf catalogue, thousands under config
  // 5's hot head, where the number of resident blocks is what its throughput scales with.
  int g_blocks = 0;
  size_t g_cap = 0;  // elements allocated
  int ensure_global_bin(int64_t n_cols_b) {
    // wide column spaces (>= 1M columns: the 10M x 2M configurations) are where thousands of rows land in this class
    const int64_t budget = n_cols_b >= (1 << 20) ? ((int64_t)4096 << 20) : ((int64_t)1024 << 20);
    int64_t blocks = budget / ((n_cols_b > 0 ? n_cols_b : 1) * 16);
    if (blocks > urcco::GLOBAL_BIN_BLOCKS) blocks = urcco::GLOBAL_BIN_BLOCKS;
    if (blocks < 2) blocks = 2;
    const size_t n = (size_t)blocks * (size_t)n_cols_b;
    if (n <= g_cap && g_counts.p) {
      // the counters are zero between launches whatever the geometry (every claim walk restores them)
      g_blocks = (int)(g_cap / (size_t)(n_cols_b > 0 ? n_cols_b : 1) < (size_t)urcco::GLOBAL_BIN_BLOCKS ? g_cap / (size_t)(n_cols_b > 0 ? n_cols_b : 1)
                                                                                                         : (size_t)urcco::GLOBAL_BIN_BLOCKS);
      g_cols = n_cols_b;
      return URCCO_OK;
    }
    HIPC(hipStreamSynchronize(stream));
    URC(g_counts.release()); URC(g_cand_key.release()); URC(g_cand_col.release());  // all three first: the new ones may not fit beside the old
    g_cols = 0; g_cap = 0;
    URC(g_counts.alloc(n));
    URC(g_cand_key.alloc(n));
    URC(g_cand_col.alloc(n));
    HIPC(hipMemsetAsync(g_counts.p, 0, n * sizeof(int32_t), stream));
    g_cols = n_cols_b;
    g_cap = n;
    g_blocks = (int)blocks;
    return URCCO_OK;
  }
};

// The scratch of one stage, declared once: every buffer gives add() the pointer it will live in and its element count; commit() sums the entries, reserves
// the session's arena for them -- what the previous stage carved is gone -- and only then hands out the addresses, in the order of the add() calls.  Until
// commit() has returned URCCO_OK every declared pointer is NULL.  No heap allocation: CAPACITY entries, one more makes commit() fail with URCCO_INTERNAL.
class ArenaLayout {
 public:
  static constexpr int CAPACITY = 64;
  // the largest user is urcco_dev_history_rows: three buffers per event type, three for the exclusions, three shared ones
  static_assert(CAPACITY >= 3 * URCCO_REC_MAX_CLAUSES + 6, "more event types need a larger ArenaLayout::CAPACITY (urcco_dev_history_rows)");

  explicit ArenaLayout(urcco_session* s) : s_(s) {}
  template <typename T>
  ArenaLayout& add(T** out, size_t n) {
    *out = nullptr;
    if (n_ < CAPACITY) e_[n_] = Entry{out, (n ? n : 1) * sizeof(T), [](void* slot, char* p) { *static_cast<T**>(slot) = reinterpret_cast<T*>(p); }};
    ++n_;
    return *this;
  }

  // The arena is reused when it is large enough; else the stream is drained and a quarter more than asked, rounded up to 1 MiB, replaces it (URCCO_DEBUG_POISON: filled whole).
  int commit() {
    if (n_ > CAPACITY) return fail(URCCO_INTERNAL, "scratch layout: %d buffers, room for %d", n_, CAPACITY);
    size_t bytes = 0, off = 0;
    for (int i = 0; i < n_; ++i) bytes += slot_bytes(e_[i].bytes);
    DBuf<char>& arena = s_->arena;
#ifdef HIPSIM_HOST_BUILD
    if (hipsim::guard_on()) hipsim::arena_unguard(arena.p, arena.cap);
#endif
    if (bytes > arena.cap) {
      if (arena.p) HIPC(hipStreamSynchronize(s_->stream));
      URC(arena.alloc(align_up(bytes + bytes / 4, (size_t)1 << 20)));
    }
    if (debug_cfg().poison) debug_poison(arena.p, arena.cap, s_->stream, true);
    for (int i = 0; i < n_; ++i) e_[i].set(e_[i].slot, place(arena, &off, e_[i].bytes));
    return URCCO_OK;
  }

 private:
  struct Entry { void* slot; size_t bytes; void (*set)(void* slot, char* p); };
  // Sub-buffers start 256-byte aligned.  Test-only host simulator (tests/hostsim) under HIPSIM_GUARD: each ends at a PROT_NONE page (mode 3: starts behind one).
  static size_t slot_bytes(size_t bytes) {
#ifdef HIPSIM_HOST_BUILD
    if (hipsim::guard_on()) return align_up(bytes, hipsim::GUARD_PAGE) + 2 * hipsim::GUARD_PAGE;
#endif
    return align_up(bytes, 256);
  }
  static char* place(DBuf<char>& arena, size_t* off, size_t bytes) {
#ifdef HIPSIM_HOST_BUILD
    if (hipsim::guard_on()) {
      char* q = hipsim::arena_place(arena.p, *off, bytes, off);
      if (*off > arena.cap) { fprintf(stderr, "hipsim guard: arena overflow (%zu > %zu)\n", *off, arena.cap); abort(); }
      return q;
    }
#endif
    char* p = arena.p + *off;
    *off += align_up(bytes, 256);
    return p;
  }
  urcco_session* s_;
  Entry e_[CAPACITY];
  int n_ = 0;
};
