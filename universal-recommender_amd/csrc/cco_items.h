// Device-resident item queries (decision D18 of DESIGN.md 7a; include/urcco.h urcco_dev_item_*): the term rows of a batch of item queries, cut from
// the indicator matrices where the build left them.  Compiled into ingest_kernels.hip behind cco_sorted_rows.h: it uses that header's sort + unique
// tails, in their sentinel-dropping forms, and its host helpers, and ingest_kernels.hip's grid helper.
//
// What the reference does per query item and event type (getBiasedSimilarItems, URAlgorithm.scala:770-792: the item's own indicator list from the
// model, cut to maxQueryEvents) is here
//   bounds  per (query, type) the window length: the row's n entries when n <= max_terms, else max_terms - 1; scans = raw row starts
//   rows    per (query, type): the window's columns, those outside 0..n_cols dropped, sorted, distinct -> the raw row
//   compact raw rows -> final CSR
// Three classes by the window length w, chosen on the device:
//   <= 64     one wave: a lane per entry, bitonic network + ballot unique in registers
//   <= 4096   one block: the window copied into LDS (the row is contiguous: a straight coalesced copy), sorted and made distinct there
//   larger    one block: the window copied into its raw row and sorted there in global memory
// The row kernels' only atomic is the cursor of the list of jobs the wave kernel leaves to the block kernel; the statistics are recomputed from the
// inputs by a kernel of their own (one integer add per wave and counter), launched only when the caller asks for them.  Everything is integer: the
// rows are bit-identical from run to run.
namespace urcco {

namespace {
// the window of (item of query q, type e): its start in ind_col_idx and its length; cut = the row is longer than max_terms
__device__ __forceinline__ int it_window(const ItemEvent& e, const int32_t* q_items, int n_items, int64_t q, int64_t& seg, bool& cut) {
  const int i = q_items[q];
  seg = 0;
  cut = false;
  if (i < 0 || i >= n_items) return 0;
  seg = e.ind_row_ptr[i];
  int64_t n = e.ind_row_ptr[i + 1] - seg;
  if (n < 0) n = 0;
  cut = n > e.max_terms;
  if (cut) n = e.max_terms - 1;
  return n > 0x7fffffffll ? 0x7fffffff : (int)n;
}
}  // namespace

// bnd[t * n_queries + q] = the window length of (q, t)
__global__ __launch_bounds__(256) void it_bounds_kernel(ItemArgs a, int32_t* __restrict__ bnd) {
  const int64_t n_jobs = a.n_queries * a.n_types;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_jobs; j += (int64_t)gridDim.x * 256) {
    const int t = (int)(j / a.n_queries);
    int64_t seg;
    bool cut;
    bnd[j] = it_window(a.ev[t], a.q_items, a.n_items, j - (int64_t)t * a.n_queries, seg, cut);
  }
}

hipError_t launch_item_bounds(hipStream_t st, int n_cu, const ItemArgs& a, int32_t* bnd, int64_t* tile_sums, int64_t* const* term_row_ptr) {
  if (a.n_queries == 0) {
    for (int t = 0; t < a.n_types; ++t) {
      const hipError_t e = hipMemsetAsync(term_row_ptr[t], 0, sizeof(int64_t), st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  hipLaunchKernelGGL(it_bounds_kernel, dim3(ig_grid(a.n_queries * a.n_types, n_cu)), dim3(256), 0, st, a, bnd);
  for (int t = 0; t < a.n_types; ++t) {
    const hipError_t e = launch_scan_i32(st, bnd + (int64_t)t * a.n_queries, a.n_queries, term_row_ptr[t], tile_sums);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

// job j = t * n_queries + q.  One wave per job whose window holds <= 64 entries; the others go on big_list (ctr[0] = their number).
__global__ __launch_bounds__(256) void it_rows_wave_kernel(ItemArgs a) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  const int64_t n_jobs = a.n_queries * a.n_types;
  for (int64_t j = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; j < n_jobs; j += n_waves) {  // wave-uniform
    const int t = (int)(j / a.n_queries);
    const int64_t q = j - (int64_t)t * a.n_queries;
    const ItemEvent& e = a.ev[t];
    if (e.raw.raw_ptr[q + 1] > e.raw.capacity) {  // the caller's buffer is smaller than the bounds: an empty row
      if (lane == 0) e.raw.len[q] = 0;
      continue;
    }
    int64_t seg;
    bool cut;
    const int w = it_window(e, a.q_items, a.n_items, q, seg, cut);
    if (w > SR_WAVE) {
      if (lane == 0) a.big_list[atomicAdd(&a.ctr[0], 1ull)] = (int32_t)j;
      continue;
    }
    int v = SR_SENT;
    if (lane < w) {
      const int c = e.ind_col_idx[seg + lane];
      if (c >= 0 && c < e.n_cols) v = c;
    }
    const int len = sr_wave_tail<true>(v, lane, SR_WAVE, e.raw.tmp + e.raw.raw_ptr[q]);
    if (lane == 0) e.raw.len[q] = len;
  }
}

// One block per job of big_list.
__global__ __launch_bounds__(256) void it_rows_block_kernel(ItemArgs a) {
  __shared__ int s_v[SR_LDS];
  const int64_t n_big = (int64_t)a.ctr[0];
  for (int64_t li = blockIdx.x; li < n_big; li += gridDim.x) {  // block-uniform
    const int64_t j = a.big_list[li];
    const int t = (int)(j / a.n_queries);
    const int64_t q = j - (int64_t)t * a.n_queries;
    const ItemEvent& e = a.ev[t];
    int64_t seg;
    bool cut;
    const int w = it_window(e, a.q_items, a.n_items, q, seg, cut);  // == raw_ptr[q + 1] - raw_ptr[q]: the raw row holds the whole window
    const int32_t* __restrict__ src = e.ind_col_idx + seg;
    int32_t* row = e.raw.tmp + e.raw.raw_ptr[q];
    const int n_cols = e.n_cols;
    if (w <= SR_LDS) {
      int P = 2;
      while (P < w) P <<= 1;
      for (int i = threadIdx.x; i < P; i += 256) {
        int v = SR_SENT;
        if (i < w) {
          const int c = src[i];
          if (c >= 0 && c < n_cols) v = c;
        }
        s_v[i] = v;
      }
    } else {
      for (int i = threadIdx.x; i < w; i += 256) {
        const int c = src[i];
        row[i] = c >= 0 && c < n_cols ? c : SR_SENT;
      }
    }
    __syncthreads();  // the staged window is complete
    const int len = sr_block_tail<true>(row, w, s_v);
    if (threadIdx.x == 0) e.raw.len[q] = len;
    __syncthreads();
  }
}

// the statistics of include/urcco.h, recomputed from the bounds (raw_ptr) and the capacities: the row kernels keep no counter.  stats: zeroed.
__global__ __launch_bounds__(256) void it_stats_kernel(ItemArgs a, unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_jobs = a.n_queries * a.n_types;
  int c[5] = {0, 0, 0, 0, 0};  // wave, block, global, cut, dropped: < 2^31 jobs in all
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_jobs; j += (int64_t)gridDim.x * 256) {
    const int t = (int)(j / a.n_queries);
    const int64_t q = j - (int64_t)t * a.n_queries;
    const ItemEvent& e = a.ev[t];
    if (e.raw.raw_ptr[q + 1] > e.raw.capacity) { ++c[4]; continue; }
    int64_t seg;
    bool cut;
    const int w = it_window(e, a.q_items, a.n_items, q, seg, cut);
    c[0] += w <= SR_WAVE;
    c[1] += w > SR_WAVE && w <= SR_LDS;
    c[2] += w > SR_LDS;
    c[3] += cut;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {  // every lane of the wave is here
    int v = c[k];
    for (int o = SR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0 && v) atomicAdd(&stats[k < 4 ? k : HIST_STAT_OVERFLOW], (unsigned long long)v);
  }
}

// a.ev[t].raw, a.big_list, a.ctr: scratch.  term_row_ptr[t] holds the bounds' scan on entry, the final row starts on return.
hipError_t launch_item_rows(hipStream_t st, int n_cu, const ItemArgs& a, int64_t* tile_sums, int64_t* const* term_row_ptr, int32_t* const* term_col_idx, int64_t* stats_dev) {
  const int64_t nq = a.n_queries, n_jobs = nq * a.n_types;
  RowsOut out[REC_MAX_CLAUSES];
  for (int t = 0; t < a.n_types; ++t) out[t] = RowsOut{a.ev[t].raw, term_row_ptr[t], term_col_idx[t]};
  hipError_t e = sr_seed_raw_ptr(st, out, a.n_types, nq);
  if (e != hipSuccess) return e;
  if (nq > 0) {
    e = hipMemsetAsync(a.ctr, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(it_rows_wave_kernel, dim3(ig_grid(n_jobs * SR_WAVE, n_cu)), dim3(256), 0, st, a);
    const int64_t bgrid = n_jobs < (int64_t)n_cu * 8 ? n_jobs : (int64_t)n_cu * 8;
    hipLaunchKernelGGL(it_rows_block_kernel, dim3((unsigned)bgrid), dim3(256), 0, st, a);
    e = sr_finish_rows(st, n_cu, out, a.n_types, nq, tile_sums);
    if (e != hipSuccess) return e;
  }
  if (stats_dev) {
    e = hipMemsetAsync(stats_dev, 0, sizeof(int64_t) * HIST_STATS_LEN, st);
    if (e != hipSuccess) return e;
    if (nq > 0) hipLaunchKernelGGL(it_stats_kernel, dim3(ig_grid(n_jobs, n_cu)), dim3(256), 0, st, a, reinterpret_cast<unsigned long long*>(stats_dev));
  }
  return hipGetLastError();
}

}  // namespace urcco
