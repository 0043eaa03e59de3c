// Hand-written gfx950 kernels of the device-side Preparator: dictionaries and
// binary CSR matrices straight from (user key, item key) event streams in HBM.
//
// Replaces what UR's own IndexedDatasetSpark builders do with three `distinct().collect()` + broadcast round trips and a
// string-keyed `groupByKey` per event type (reference src/main/scala/Preparator.scala:102-158, :160-214):
//   dictionary   key -> dense id, ids in order of FIRST APPEARANCE in the stream (decision D8), optionally only keys that
//                occur at least min_count times (`minEventsPerUser`, raw events, duplicates included: :129-132)
//   lookup       ids of a stream against an existing dictionary (-1 = not in it: :173-179 drop such events)
//   CSR build    (row id, column id) pairs -> rows with sorted, duplicate-free columns (`setQuick(col, 1.0)`: :146, :205)
// Keys are 64-bit (the host hashes its strings, or passes integer ids); ~0 is reserved for "empty slot": the insert pass counts
// the selected positions that hold it and leaves the table alone for them, and the build is refused (urcco_api.hip).
// First-appearance ids need no sort: every slot keeps the smallest position of its key (atomicMin); an event is a
// "first" iff its position equals that minimum; the id of a key is the number of firsts before its own first -- one
// exclusive scan over the stream.
// Wave = 64 lanes.  Wave-level primitives only under wave-uniform control flow.
#include "cco_kernels.h"

namespace urcco {

namespace {
constexpr unsigned long long IG_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long ig_mix(unsigned long long x) {  // splitmix64 finaliser
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// slot of `key`, or the empty slot where its probe sequence ends
__device__ __forceinline__ unsigned long long ig_find(const KeyTable& t, unsigned long long key) {
  unsigned long long slot = ig_mix(key) & t.mask;
  for (;;) {
    const unsigned long long cur = t.keys[slot];
    if (cur == key || cur == IG_EMPTY) return slot;
    slot = (slot + 1) & t.mask;
  }
}
}  // namespace

// Popular keys are hit by millions of events (the top item of a Zipf catalogue by ~1 % of the stream): three atomics per event
// on the key's slot -- claim, position minimum, count -- serialise on one L2 address each (measured: 6.2 ms per dictionary,
// two thirds of the whole ingest).  A key never changes once written, the position minimum only decreases and the count only
// matters up to `need` (min_count), so each of the three is read first and the atomic issued only if it can still change
// something; a stale read (L1 is not coherent with other CUs' atomics) costs one unnecessary atomic, never a wrong result.
// reserved[0] counts the selected positions that hold IG_EMPTY itself: such a key cannot be told from a free slot (its CAS would "claim" the slot
// without changing it, and the next real key to probe there would inherit its position minimum), so the table is not touched for it.
__global__ __launch_bounds__(256) void ig_insert_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys,
                                                        const int32_t* __restrict__ select, unsigned need, unsigned* __restrict__ reserved) {
  unsigned n_reserved = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    if (select && select[p] < 0) continue;
    const unsigned long long key = keys[p];
    if (key == IG_EMPTY) {
      ++n_reserved;
      continue;
    }
    unsigned long long slot = ig_mix(key) & t.mask;
    for (;;) {
      unsigned long long cur = t.keys[slot];
      if (cur == IG_EMPTY) cur = atomicCAS(&t.keys[slot], IG_EMPTY, key);
      if (cur == IG_EMPTY || cur == key) {
        if ((unsigned)p < t.minpos[slot]) atomicMin(&t.minpos[slot], (unsigned)p);
        if (need > 1u && t.count[slot] < need) atomicAdd(&t.count[slot], 1u);  // exact below `need`, at least `need` from there on
        break;
      }
      slot = (slot + 1) & t.mask;
    }
  }
  if (n_reserved) atomicAdd(reserved, n_reserved);
}

// flag[p] = 1 iff event p is the first appearance of a key that occurs at least min_count times
__global__ __launch_bounds__(256) void ig_first_flags_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys,
                                                             const int32_t* __restrict__ select, unsigned min_count, int32_t* __restrict__ flag) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    int f = 0;
    if (!(select && select[p] < 0)) {
      const unsigned long long slot = ig_find(t, keys[p]);
      f = t.minpos[slot] == (unsigned)p && (min_count <= 1u || t.count[slot] >= min_count);
    }
    flag[p] = f;
  }
}

__global__ __launch_bounds__(256) void ig_assign_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys,
                                                        const int32_t* __restrict__ flag, const int64_t* __restrict__ prefix,
                                                        int64_t* __restrict__ first_pos) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    if (!flag[p]) continue;
    const int64_t id = prefix[p];
    t.id[ig_find(t, keys[p])] = (int32_t)id;
    first_pos[id] = p;
  }
}

__global__ __launch_bounds__(256) void ig_lookup_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys,
                                                        const int32_t* __restrict__ select, int32_t* __restrict__ ids) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    int32_t id = -1;
    if (!(select && select[p] < 0)) {
      const unsigned long long key = keys[p];
      const unsigned long long slot = ig_find(t, key);
      if (t.keys[slot] == key) id = t.id[slot];
    }
    ids[p] = id;
  }
}

static unsigned ig_grid(int64_t n, int n_cu) {
  int64_t b = (n + 255) / 256;
  const int64_t cap = (int64_t)n_cu * 16;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

hipError_t launch_dictionary_build(hipStream_t st, int n_cu, KeyTable t, int64_t n, const unsigned long long* keys, const int32_t* select,
                                   int32_t min_count, int32_t* flag, int64_t* prefix, int64_t* tile_sums, int64_t* first_pos, unsigned* reserved) {
  hipError_t e = hipMemsetAsync(reserved, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  if (n == 0) return hipMemsetAsync(prefix, 0, sizeof(int64_t), st);
  hipLaunchKernelGGL(ig_insert_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, t, n, keys, select, (unsigned)(min_count < 1 ? 1 : min_count), reserved);
  hipLaunchKernelGGL(ig_first_flags_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, t, n, keys, select, (unsigned)(min_count < 1 ? 1 : min_count), flag);
  e = launch_scan_i32(st, flag, n, prefix, tile_sums);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ig_assign_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, t, n, keys, flag, prefix, first_pos);
  return hipGetLastError();
}

// collision check: the check key (a second, independent hash of the same string) of every position must equal the check key
// of its id's first occurrence; err[0] counts the positions where it does not
__global__ __launch_bounds__(256) void ig_verify_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys, const int32_t* __restrict__ select,
                                                        const unsigned long long* __restrict__ check, const unsigned long long* __restrict__ ref_check,
                                                        const int64_t* __restrict__ first_pos, unsigned long long* __restrict__ err) {
  unsigned bad = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    if (select && select[p] < 0) continue;
    const unsigned long long key = keys[p];
    const unsigned long long slot = ig_find(t, key);
    if (t.keys[slot] != key) continue;
    const int32_t id = t.id[slot];
    if (id >= 0 && check[p] != ref_check[first_pos[id]]) ++bad;  // ref_check: check keys of the stream the dictionary was built from
  }
  if (bad) atomicAdd(err, (unsigned long long)bad);
}
hipError_t launch_dictionary_verify(hipStream_t st, int n_cu, KeyTable t, int64_t n, const unsigned long long* keys, const int32_t* select,
                                    const unsigned long long* check, const unsigned long long* ref_check, const int64_t* first_pos, unsigned long long* err) {
  hipError_t e = hipMemsetAsync(err, 0, sizeof(unsigned long long), st);
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(ig_verify_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, t, n, keys, select, check, ref_check, first_pos, err);
  return hipGetLastError();
}

hipError_t launch_dictionary_lookup(hipStream_t st, int n_cu, KeyTable t, int64_t n, const unsigned long long* keys, const int32_t* select,
                                    int32_t* ids) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ig_lookup_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, t, n, keys, select, ids);
  return hipGetLastError();
}

}  // namespace urcco

#include "cco_sorted_rows.h"  // raw rows -> sorted, duplicate-free rows: the unit of the CSR build below, of cco_history.h and of cco_items.h

namespace urcco {

// ============================================================================================
// (row, col) pairs -> binary CSR.  count per row (L2 atomics) -> scan -> scatter by cursor -> per row: sort ascending,
// drop duplicates (cco_sorted_rows.h: one wave for rows of <= 64 raw entries, one block for longer ones) -> scan of the
// final lengths -> compaction.
// ============================================================================================
__global__ __launch_bounds__(256) void ig_count_rows_kernel(int64_t n, const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                            int32_t* __restrict__ cnt) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256)
    if (rows[p] >= 0 && cols[p] >= 0) atomicAdd(&cnt[rows[p]], 1);
}

__global__ __launch_bounds__(256) void ig_scatter_rows_kernel(int64_t n, const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                              const int64_t* __restrict__ raw_ptr, int32_t* __restrict__ cursor,
                                                              int32_t* __restrict__ tmp) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const int r = rows[p], c = cols[p];
    if (r >= 0 && c >= 0) tmp[raw_ptr[r] + atomicAdd(&cursor[r], 1)] = c;
  }
}

// one wave per row with <= 64 raw entries: sort, unique, write back to the row's start, len[r] = distinct columns.
// Rows with more entries get len[r] = -1 (the block kernel takes them).
__global__ __launch_bounds__(256) void ig_sort_rows_wave_kernel(int64_t n_rows, const int64_t* __restrict__ raw_ptr, int32_t* __restrict__ tmp,
                                                                int32_t* __restrict__ len) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t r = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; r < n_rows; r += n_waves) {  // wave-uniform
    const int64_t s = raw_ptr[r];
    const int64_t L = raw_ptr[r + 1] - s;
    if (L > SR_WAVE) {
      if (lane == 0) len[r] = -1;
      continue;
    }
    const int n = sr_wave_tail<false>(lane < L ? tmp[s + lane] : SR_SENT, lane, (int)L, tmp + s);
    if (lane == 0) len[r] = n;
  }
}

// one block per row with > 64 raw entries (grid-stride over all rows; the test is block-uniform)
__global__ __launch_bounds__(256) void ig_sort_rows_block_kernel(int64_t n_rows, const int64_t* __restrict__ raw_ptr, int32_t* __restrict__ tmp,
                                                                 int32_t* __restrict__ len) {
  __shared__ int s_v[SR_LDS];
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int64_t s = raw_ptr[r];
    const int64_t L = raw_ptr[r + 1] - s;
    if (L <= SR_WAVE) continue;  // block-uniform
    const int n = sr_block_tail(tmp + s, L, s_v);
    if (threadIdx.x == 0) len[r] = n;
    __syncthreads();
  }
}

hipError_t launch_csr_from_pairs(hipStream_t st, int n_cu, int64_t n, const int32_t* rows, const int32_t* cols, int64_t n_rows, int32_t* cnt,
                                 int64_t* raw_ptr, int32_t* tmp, int64_t* tile_sums, int64_t* out_row_ptr, int32_t* out_col_idx) {
  hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(n_rows > 0 ? n_rows : 1), st);
  if (e != hipSuccess) return e;
  if (n > 0) hipLaunchKernelGGL(ig_count_rows_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, rows, cols, cnt);
  e = launch_scan_i32(st, cnt, n_rows, raw_ptr, tile_sums);
  if (e != hipSuccess) return e;
  if (n_rows == 0) return hipMemsetAsync(out_row_ptr, 0, sizeof(int64_t), st);
  e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n_rows, st);  // now the scatter cursors
  if (e != hipSuccess) return e;
  if (n > 0) hipLaunchKernelGGL(ig_scatter_rows_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, rows, cols, raw_ptr, cnt, tmp);
  const RowsOut out{RawRows{raw_ptr, tmp, cnt, n}, out_row_ptr, out_col_idx};  // cnt becomes the final lengths
  hipLaunchKernelGGL(ig_sort_rows_wave_kernel, dim3(ig_grid(n_rows * SR_WAVE, n_cu)), dim3(256), 0, st, n_rows, raw_ptr, tmp, cnt);
  int64_t bgrid = n_rows < (int64_t)n_cu * 8 ? n_rows : (int64_t)n_cu * 8;
  hipLaunchKernelGGL(ig_sort_rows_block_kernel, dim3((unsigned)(bgrid < 1 ? 1 : bgrid)), dim3(256), 0, st, n_rows, raw_ptr, tmp, cnt);
  return sr_finish_rows(st, n_cu, &out, 1, n_rows, tile_sums);
}

}  // namespace urcco

#include "cco_select.h"   // the k-th largest key by one block: the select of cco_history.h
#include "cco_history.h"  // device-resident user history: uses ig_grid, cco_sorted_rows.h and cco_select.h
#include "cco_items.h"    // device-resident item queries: the same over the model's own indicator rows
#include "cco_props.h"    // device-resident item properties: $set / $unset / $delete aggregated in place; the winners' value lists through cco_sorted_rows.h
#include "cco_dictionary.h"  // growable dictionary: a batch of keys against a live table, new keys get the next ids; uses ig_mix, ig_find, ig_grid
