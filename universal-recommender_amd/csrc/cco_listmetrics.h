// cco_listmetrics.h -- list metrics of a recommendation table (urcco_dev_list_exposure, urcco_dev_exposure_stats, urcco_dev_list_links; DESIGN.md, decision
// D35): how often every item is shown inside each cut-off, the integers behind coverage, Gini, Herfindahl and novelty, and per row the ordered pairs of
// listed items that the similarity matrix links.  Included once, from cco_misc.hip, behind cco_ranks.h (whose launch_fill_order orders the exposures).
// Every output is an exact integer that does not depend on the grid or on how the rows were split into calls; the floats are formed by the caller.
//
//   lm_exposure_kernel   a block takes tiles of LM_TILE_ENTRIES / num rows.  Every table position below the row's count and the last cut-off is one counted
//                        increment of the key bucket * n_items + item in an LDS open-addressing table (atomicCAS claims the slot, atomicAdd counts); after the
//                        tile one global atomic per occupied slot flushes it.  A recommendation table is head-heavy -- a popular or backfilled item sits in
//                        most rows -- so the tile's thousands of increments fall on a few hundred keys.  A key that finds no slot within LM_PROBES probes
//                        goes straight to a global atomic: the result never depends on the table's size (URCCO_EXPO_LDS_SLOTS lowers it for the tests).
//   lm_expo_kernel       a thread per item: the running sums over the buckets are expo [n_ks, n_items]; covered, total and the sum of squares collect per
//                        lane, then per wave by xor-shuffles, per block in LDS, and reach the output by one integer atomic per block and cut-off.
//   lm_rank_sum_kernel   R = sum over the positions of launch_fill_order's descending stable order of (n_items - position) * expo[item at position]: the
//                        ascending rank times the exposure, ties interchangeable.  Same reduction shape.
//   lm_links_kernel      a wave per table row, four rows a block, grid-striding.  The wave stages the row's valid items in a 512-slot LDS set, item -> first
//                        position (atomicCAS, atomicMin).  Every first position is a source: the length and start of its similarity row go to LDS, the
//                        exclusive prefix of the lengths is formed by wave scans with a carry between the rounds of 64.  Then the FLATTENED (source, entry)
//                        pairs are walked 64 at a time; a lane finds its source by a binary search of the prefix, loads its entry and probes the set.  A row of
//                        300 correlators next to rows of 3 costs ceil(303 / 64) rounds, not 300: no lane idles on a short row.  A hit at first position b
//                        raises the lane's counter of every cut-off above max(a, b) -- the comparison itself is the running sum over the buckets; no array is
//                        indexed by a lane's value.  Xor-shuffles add the lanes' counters, lane kappa writes linked[q][kappa].
// No float arithmetic, no float atomics, no waiting between blocks.  Wave primitives under wave-uniform control flow only, one per source line.
#pragma once

namespace urcco {

constexpr int LM_THREADS = 256;
constexpr int LM_NW = LM_THREADS / WAVE;
constexpr int LM_TILE_ENTRIES = 8192;      // table positions a block counts into its LDS table before it flushes
constexpr int LM_PROBES = 32;              // probes after which a key goes to global memory
constexpr unsigned LM_EMPTY = 0xffffffffu; // no key: a key lies below 2^31
constexpr int LM_SET_SLOTS = 512;          // a wave's item set: REC_MAX_NUM items at load 1/2
static_assert((LM_EXPO_SLOTS & (LM_EXPO_SLOTS - 1)) == 0 && LM_SET_SLOTS >= 2 * REC_MAX_NUM && (LM_SET_SLOTS & (LM_SET_SLOTS - 1)) == 0, "power-of-two tables");
static_assert(REC_MAX_NUM == 4 * WAVE && LM_NW == 4, "four rounds of 64 positions a row; four waves a block");

__device__ __forceinline__ unsigned lm_hash(unsigned key) {
  const unsigned x = key * 2654435761u;
  return x ^ (x >> 15);
}
// the smallest x with j < ks[x]; n_ks when there is none
__device__ __forceinline__ int lm_bucket(const ListArgs& a, int j) {
  int x = 0;
#pragma unroll
  for (int t = 0; t < EVAL_MAX_KS; ++t) x += (t < a.n_ks && j >= a.ks[t]) ? 1 : 0;
  return x;
}
__device__ __forceinline__ int lm_row_len(const ListArgs& a, int64_t q) {
  const int c = a.rec_count[q];
  return c < 0 ? 0 : c > a.num ? a.num : c;
}
__device__ __forceinline__ unsigned long long lm_wave_sum(unsigned long long v) {
  for (int o = WAVE / 2; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
  return v;
}

__global__ __launch_bounds__(LM_THREADS) void lm_exposure_kernel(ListArgs a) {
  __shared__ unsigned s_key[LM_EXPO_SLOTS];
  __shared__ unsigned s_cnt[LM_EXPO_SLOTS];
  const int tid = threadIdx.x;
  const unsigned slots = (unsigned)a.slots, mask = slots - 1u;
  const unsigned probes = slots < (unsigned)LM_PROBES ? slots : (unsigned)LM_PROBES;
  const unsigned num = (unsigned)a.num;
  const int64_t n_tiles = (a.n_rows + a.tile_rows - 1) / a.tile_rows;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    for (unsigned h = (unsigned)tid; h < slots; h += LM_THREADS) {
      s_key[h] = LM_EMPTY;
      s_cnt[h] = 0u;
    }
    __syncthreads();
    const int64_t r0 = tile * a.tile_rows;
    const unsigned rows = (unsigned)(a.n_rows - r0 < a.tile_rows ? a.n_rows - r0 : a.tile_rows);
    for (unsigned e = (unsigned)tid; e < rows * num; e += LM_THREADS) {
      const unsigned r = e / num, j = e - r * num;
      const int64_t q = r0 + r;
      int m = lm_row_len(a, q);
      m = m < a.k_max ? m : a.k_max;
      if ((int)j >= m) continue;
      const int32_t item = a.rec_idx[q * num + j];
      if ((unsigned)item >= (unsigned)a.n_items) continue;
      const unsigned key = (unsigned)lm_bucket(a, (int)j) * (unsigned)a.n_items + (unsigned)item;  // < n_ks * n_items < 2^31
      unsigned h = lm_hash(key) & mask;
      bool placed = false;
      for (unsigned p = 0; p < probes; ++p) {
        const unsigned k = atomicCAS(&s_key[h], LM_EMPTY, key);
        if (k == LM_EMPTY || k == key) {
          atomicAdd(&s_cnt[h], 1u);
          placed = true;
          break;
        }
        h = (h + 1u) & mask;
      }
      if (!placed) atomicAdd(&a.bucket[key], 1u);
    }
    __syncthreads();
    for (unsigned h = (unsigned)tid; h < slots; h += LM_THREADS)
      if (s_key[h] != LM_EMPTY) atomicAdd(&a.bucket[s_key[h]], s_cnt[h]);
    __syncthreads();
  }
}

// s_acc[slot] += the wave's sum of v; every lane of the wave arrives
__device__ __forceinline__ void lm_block_add(unsigned long long* s_acc, int slot, unsigned long long v, int lane) {
  v = lm_wave_sum(v);
  if (lane == 0 && v) atomicAdd(&s_acc[slot], v);
}

__global__ __launch_bounds__(LM_THREADS) void lm_expo_kernel(int32_t n_items, int32_t n_ks, const unsigned* __restrict__ bucket, long long* __restrict__ expo,
                                                            unsigned long long* __restrict__ stats /* [n_ks * 4], zero before the launch */) {
  __shared__ unsigned long long s_acc[EVAL_MAX_KS * 4];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  if (tid < EVAL_MAX_KS * 4) s_acc[tid] = 0ull;
  __syncthreads();
  unsigned long long covered[EVAL_MAX_KS], total[EVAL_MAX_KS], sq[EVAL_MAX_KS];
#pragma unroll
  for (int x = 0; x < EVAL_MAX_KS; ++x) covered[x] = total[x] = sq[x] = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * LM_THREADS + tid; i < n_items; i += (int64_t)gridDim.x * LM_THREADS) {
    unsigned long long run = 0ull;
#pragma unroll
    for (int x = 0; x < EVAL_MAX_KS; ++x)
      if (x < n_ks) {
        run += (unsigned long long)bucket[(int64_t)x * n_items + i];
        expo[(int64_t)x * n_items + i] = (long long)run;
        covered[x] += run ? 1ull : 0ull;
        total[x] += run;
        sq[x] += run * run;
      }
  }
#pragma unroll
  for (int x = 0; x < EVAL_MAX_KS; ++x) {  // every lane of the block takes part in every sum
    lm_block_add(s_acc, x * 4 + 0, covered[x], lane);
    lm_block_add(s_acc, x * 4 + 1, total[x], lane);
    lm_block_add(s_acc, x * 4 + 2, sq[x], lane);
  }
  __syncthreads();
  if (tid < n_ks * 4 && s_acc[tid]) atomicAdd(&stats[tid], s_acc[tid]);
}

__global__ __launch_bounds__(LM_THREADS) void lm_rank_sum_kernel(int32_t n_items, const long long* __restrict__ expo_x, const int32_t* __restrict__ order,
                                                                unsigned long long* __restrict__ out_r) {
  __shared__ unsigned long long s_acc[1];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  if (tid == 0) s_acc[0] = 0ull;
  __syncthreads();
  unsigned long long r = 0ull;
  for (int64_t p = (int64_t)blockIdx.x * LM_THREADS + tid; p < n_items; p += (int64_t)gridDim.x * LM_THREADS) {
    const int32_t i = order[p];
    if ((unsigned)i < (unsigned)n_items) r += (unsigned long long)(n_items - p) * (unsigned long long)expo_x[i];
  }
  lm_block_add(s_acc, 0, r, lane);
  __syncthreads();
  if (tid == 0 && s_acc[0]) atomicAdd(out_r, s_acc[0]);
}

__global__ __launch_bounds__(LM_THREADS) void lm_links_kernel(ListArgs a) {
  __shared__ int s_item[LM_NW][LM_SET_SLOTS];                   // the set: item, -1 = free
  __shared__ int s_first[LM_NW][LM_SET_SLOTS];                  // ... -> its first position
  __shared__ unsigned long long s_pre[LM_NW][REC_MAX_NUM + 1];  // exclusive prefix of the sources' row lengths
  __shared__ long long s_base[LM_NW][REC_MAX_NUM];              // where the source's similarity row starts
  __shared__ unsigned long long s_sum[2 * EVAL_MAX_KS];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  if (tid < 2 * EVAL_MAX_KS) s_sum[tid] = 0ull;
  __syncthreads();
  int* set_item = s_item[wave];
  int* set_first = s_first[wave];
  unsigned long long* pre = s_pre[wave];
  long long* base = s_base[wave];
  int my_k = 0;  // lane kappa < n_ks keeps cut-off ks[kappa]
#pragma unroll
  for (int x = 0; x < EVAL_MAX_KS; ++x)
    if (lane == x && x < a.n_ks) my_k = a.ks[x];
  unsigned long long sum_linked = 0ull, sum_pairs = 0ull;
  const int64_t n_waves = (int64_t)gridDim.x * LM_NW;
  for (int64_t q = (int64_t)blockIdx.x * LM_NW + wave; q < a.n_rows; q += n_waves) {  // wave-uniform
    const int c = lm_row_len(a, q);
    const int m_max = c < a.k_max ? c : a.k_max;  // no cut-off looks further: a position behind it is neither a source nor a target
    const int32_t* row = a.rec_idx + q * (int64_t)a.num;
    for (int h = lane; h < LM_SET_SLOTS; h += WAVE) {
      set_item[h] = -1;
      set_first[h] = 0x7fffffff;
    }
    expl_wave_sync();
    for (int j = lane; j < m_max; j += WAVE) {
      const int32_t item = row[j];
      if ((unsigned)item >= (unsigned)a.n_items) continue;
      unsigned h = lm_hash((unsigned)item) & (LM_SET_SLOTS - 1);
      for (int p = 0; p < LM_SET_SLOTS; ++p) {  // at most REC_MAX_NUM items: a slot is always found
        const int k = atomicCAS(&set_item[h], -1, item);
        if (k == -1 || k == item) {
          atomicMin(&set_first[h], j);
          break;
        }
        h = (h + 1u) & (LM_SET_SLOTS - 1);
      }
    }
    expl_wave_sync();
    unsigned long long carry = 0ull;
    for (int j0 = 0; j0 < m_max; j0 += WAVE) {  // wave-uniform
      const int j = j0 + lane;
      long long len = 0, start = 0;
      if (j < m_max) {
        const int32_t item = row[j];
        if ((unsigned)item < (unsigned)a.n_items) {
          unsigned h = lm_hash((unsigned)item) & (LM_SET_SLOTS - 1);
          while (set_item[h] != item) h = (h + 1u) & (LM_SET_SLOTS - 1);  // it was staged
          if (set_first[h] == j) {  // a later repeat is no source
            start = a.sim_row_ptr[item];
            len = a.sim_row_ptr[item + 1] - start;
            len = len > 0 ? len : 0;
          }
        }
      }
      unsigned long long incl = (unsigned long long)len;
      for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long y = (unsigned long long)shfl_i64((long long)incl, lane >= d ? lane - d : lane);
        if (lane >= d) incl += y;
      }
      if (j < m_max) {
        pre[j] = carry + incl - (unsigned long long)len;
        base[j] = start;
      }
      carry += (unsigned long long)shfl_i64((long long)incl, WAVE - 1);
    }
    if (lane == 0) pre[m_max] = carry;
    expl_wave_sync();
    const unsigned long long total = carry;
    unsigned cnt[EVAL_MAX_KS];
#pragma unroll
    for (int x = 0; x < EVAL_MAX_KS; ++x) cnt[x] = 0u;
    for (unsigned long long e0 = 0ull; e0 < total; e0 += WAVE) {  // wave-uniform
      const unsigned long long e = e0 + (unsigned long long)lane;
      if (e < total) {
        int lo = 0, hi = m_max;  // the last source with pre[.] <= e: the one whose row holds entry e (pre[0] = 0 <= e < pre[m_max])
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (pre[mid] <= e) lo = mid; else hi = mid;
        }
        const int32_t t = a.sim_col_idx[base[lo] + (long long)(e - pre[lo])];
        if ((unsigned)t < (unsigned)a.n_items && t != row[lo]) {
          unsigned h = lm_hash((unsigned)t) & (LM_SET_SLOTS - 1);
          int k = set_item[h];
          while (k != t && k != -1) {
            h = (h + 1u) & (LM_SET_SLOTS - 1);
            k = set_item[h];
          }
          if (k == t) {
            const int b = set_first[h];
            const int far = lo > b ? lo : b;
#pragma unroll
            for (int x = 0; x < EVAL_MAX_KS; ++x) cnt[x] += (x < a.n_ks && far < a.ks[x]) ? 1u : 0u;
          }
        }
      }
    }
    unsigned mine = 0u;
#pragma unroll
    for (int x = 0; x < EVAL_MAX_KS; ++x) {
      unsigned v = cnt[x];
      for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == x) mine = v;
    }
    if (lane < a.n_ks) {
      a.out_linked[q * a.n_ks + lane] = (int32_t)mine;
      const unsigned long long m = (unsigned long long)(my_k < c ? my_k : c);
      sum_linked += (unsigned long long)mine;
      sum_pairs += m > 0ull ? m * (m - 1ull) : 0ull;
    }
    expl_wave_sync();  // the next row clears the tables
  }
  if (!a.out_sums) return;  // uniform
  if (lane < a.n_ks) {
    if (sum_linked) atomicAdd(&s_sum[lane], sum_linked);
    if (sum_pairs) atomicAdd(&s_sum[a.n_ks + lane], sum_pairs);
  }
  __syncthreads();
  if (tid < 2 * a.n_ks && s_sum[tid]) atomicAdd(&a.out_sums[tid], s_sum[tid]);
}

// the rows of a tile of lm_exposure_kernel
inline int64_t list_tile_rows(int32_t num) { return LM_TILE_ENTRIES / num > 0 ? LM_TILE_ENTRIES / num : 1; }

hipError_t launch_list_exposure(hipStream_t st, int n_cu, ListArgs a) {
  if (a.n_rows <= 0 || a.n_items <= 0) return hipSuccess;
  a.tile_rows = list_tile_rows(a.num);
  int64_t blocks = (a.n_rows + a.tile_rows - 1) / a.tile_rows;
  if (blocks > (int64_t)n_cu * 4) blocks = (int64_t)n_cu * 4;  // 32 KiB of LDS a block
  hipLaunchKernelGGL(lm_exposure_kernel, dim3((unsigned)blocks), dim3(LM_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_exposure_stats(hipStream_t st, int n_cu, int32_t n_items, int32_t n_ks, const uint32_t* bucket, int64_t* out_expo, int64_t* out_stats,
                                 const FillOrderScratch& w, int32_t* order) {
  hipError_t e = hipMemsetAsync(out_stats, 0, sizeof(int64_t) * 4 * (size_t)n_ks, st);
  if (e != hipSuccess || n_items <= 0) return e;
  int64_t blocks = ((int64_t)n_items + LM_THREADS - 1) / LM_THREADS;
  if (blocks > (int64_t)n_cu * 8) blocks = (int64_t)n_cu * 8;
  unsigned long long* stats = reinterpret_cast<unsigned long long*>(out_stats);
  hipLaunchKernelGGL(lm_expo_kernel, dim3((unsigned)blocks), dim3(LM_THREADS), 0, st, n_items, n_ks, bucket, reinterpret_cast<long long*>(out_expo), stats);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int x = 0; x < n_ks; ++x) {
    const int64_t* field = out_expo + (size_t)x * (size_t)n_items;
    if ((e = launch_fill_order(st, n_items, &field, 1, w, order)) != hipSuccess) return e;
    hipLaunchKernelGGL(lm_rank_sum_kernel, dim3((unsigned)blocks), dim3(LM_THREADS), 0, st, n_items, reinterpret_cast<const long long*>(field), order, stats + x * 4 + 3);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_list_links(hipStream_t st, int n_cu, const ListArgs& a) {
  if (a.n_rows <= 0) return hipSuccess;
  int64_t blocks = (a.n_rows + LM_NW - 1) / LM_NW;
  if (blocks > (int64_t)n_cu * 8) blocks = (int64_t)n_cu * 8;  // 32 KiB of LDS a block
  hipLaunchKernelGGL(lm_links_kernel, dim3((unsigned)blocks), dim3(LM_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace urcco
