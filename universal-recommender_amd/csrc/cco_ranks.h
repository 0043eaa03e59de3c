// cco_ranks.h -- the backfill order of a model from up to RANK_MAX_FIELDS rank fields (urcco_dev_fill_order; DESIGN.md, decision D24): the permutation of
// the items sorted by (field 0 desc, field 1 desc, ..., item id asc), an item without a rank (RANK_NONE) last in its field -- the reference's
// `sort: [_score desc, <every ranking field> desc]` (buildQuerySort, URAlgorithm.scala:730-738) over documents that lack a field.
// Included once, from cco_misc.hip, behind cco_eval.h.
//
// A stable least-significant-digit radix sort of (key, item) pairs over 8-bit digits, the last field first, starting from the identity: what remains
// between equal tuples is the item id.  The contract's key is NONE ? 0 : value ^ 2^63, descending; the passes sort its distance from the field's smallest
// key, complemented, ascending (rk_key): the same order in fewer differing digits.
//   rk_base_kernel      base[f] = the smallest key of field f over the items that have a rank (a minimum: LDS, then one 64-bit atomic per block and field)
//   rk_differ_kernel    differ[f] = OR over the items of key ^ key of item 0: the digits of field f in which two keys differ.  Neither depends on the order
//                       of the items, so one launch each ahead of the passes serves all of them.  A digit whose byte of differ[f] is 0 takes no pass: its three
//                       kernels are still enqueued -- nothing is read back to the host -- and return at once.  Every kernel derives the side of the two
//                       (key, item) buffers it reads from the number of passes that ran before it (rk_side), which it counts from differ[] alone.
//   rk_gather_kernel    per field: key[j] = key of the item at position j of the order so far
//   rk_hist_kernel      per pass: hist[digit][tile] = the tile's pairs with that digit (LDS counters)
//   launch_scan_i32     the exclusive scan over (digit, tile): where the tile's pairs of a digit start
//   rk_scatter_kernel   a wave takes 64 consecutive pairs of the tile per round.  The lanes that hold one digit find each other by eight ballots (one per bit
//                       of the digit): a lane's place among them is the popcount of the lower lanes, the first of them writes their number into the wave's
//                       row of an LDS table.  A pair goes to run[digit] + the counts of the lower waves + its place in its wave; then thread t advances
//                       run[t] by the round's counts of digit t and clears them.  Tile order is element order, so equal digits keep their order.
// No atomic takes part in a placement: the counters of rk_hist_kernel, the minimum of rk_base_kernel and the OR of rk_differ_kernel hold values that do not
// depend on the order of the updates.  The order is reproducible bit for bit.  Wave primitives: __ballot and __popcll, under wave-uniform control flow, one per source line.
#pragma once

namespace urcco {

constexpr int RK_THREADS = 256;
constexpr int RK_NW = RK_THREADS / WAVE;
constexpr int RK_ROUNDS = RK_TILE / RK_THREADS;
static_assert(RK_TILE % RK_THREADS == 0 && RK_THREADS == 256, "a thread per digit; whole rounds");

struct RkFields {
  const int64_t* rank[RANK_MAX_FIELDS];
  int32_t n_fields;
};
struct RkBufs {
  unsigned long long* keys[2];
  int32_t* ids[2];
};

// The contract's key of a rank, larger = earlier: value ^ 2^63 (>= 1; NONE = 0).  The passes sort ascending on ~(NONE ? 0 : key - base + 1), base = the
// field's smallest key: the same order, and two keys differ only in the digits their DISTANCE from the smallest needs -- a trending or hot field, whose
// small signed values differ in every byte of the plain key (sign extension), takes one or two passes instead of eight.
__device__ __forceinline__ unsigned long long rk_raw(long long v) { return (unsigned long long)v ^ (1ull << 63); }
__device__ __forceinline__ unsigned long long rk_key(long long v, unsigned long long base) { return ~(v == RANK_NONE ? 0ull : rk_raw(v) - base + 1ull); }
// state[f] = the differing bits of field f, state[RANK_MAX_FIELDS + f] = its smallest key (all ones while no item has a rank)
__device__ __forceinline__ unsigned long long rk_base(const unsigned long long* __restrict__ state, int f) { return state[RANK_MAX_FIELDS + f]; }

// digits below `below` of a field in which two keys differ: the passes the field takes there
__device__ __forceinline__ int rk_live_digits(unsigned long long differ, int below) {
  int n = 0;
  for (int d = 0; d < below; ++d) n += ((differ >> (8 * d)) & 255ull) != 0ull;
  return n;
}
// the side that pass (f, d) reads: the parity of the passes before it -- the fields behind f in full, the digits below d of f
__device__ __forceinline__ int rk_side(const unsigned long long* __restrict__ differ, int n_fields, int f, int d) {
  int passes = rk_live_digits(differ[f], d);
  for (int g = n_fields - 1; g > f; --g) passes += rk_live_digits(differ[g], 8);
  return passes & 1;
}

__global__ __launch_bounds__(RK_THREADS) void rk_base_kernel(int32_t n, RkFields fields, unsigned long long* __restrict__ base /* [n_fields], all ones on entry */) {
  __shared__ unsigned long long s_min[RANK_MAX_FIELDS];
  if (threadIdx.x < RANK_MAX_FIELDS) s_min[threadIdx.x] = ~0ull;
  __syncthreads();
  for (int f = 0; f < fields.n_fields; ++f) {
    const int64_t* __restrict__ r = fields.rank[f];
    unsigned long long m = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RK_THREADS) {
      const long long v = r[i];
      if (v != RANK_NONE && rk_raw(v) < m) m = rk_raw(v);
    }
    if (m != ~0ull) atomicMin(&s_min[f], m);
  }
  __syncthreads();
  if ((int)threadIdx.x < fields.n_fields && s_min[threadIdx.x] != ~0ull) atomicMin(&base[threadIdx.x], s_min[threadIdx.x]);
}

__global__ __launch_bounds__(RK_THREADS) void rk_differ_kernel(int32_t n, RkFields fields, const unsigned long long* __restrict__ state,
                                                             unsigned* __restrict__ differ32 /* state[0 .. n_fields) as low, high words */) {
  __shared__ unsigned s_or[2 * RANK_MAX_FIELDS];
  if (threadIdx.x < 2 * RANK_MAX_FIELDS) s_or[threadIdx.x] = 0u;
  __syncthreads();
  for (int f = 0; f < fields.n_fields; ++f) {
    const int64_t* __restrict__ r = fields.rank[f];
    const unsigned long long base = rk_base(state, f), common = rk_key(r[0], base);
    unsigned long long d = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RK_THREADS) d |= rk_key(r[i], base) ^ common;
    if ((unsigned)d) atomicOr(&s_or[2 * f], (unsigned)d);
    if ((unsigned)(d >> 32)) atomicOr(&s_or[2 * f + 1], (unsigned)(d >> 32));
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * fields.n_fields && s_or[threadIdx.x]) atomicOr(&differ32[threadIdx.x], s_or[threadIdx.x]);
}

__global__ __launch_bounds__(RK_THREADS) void rk_iota_kernel(int32_t n, int32_t* __restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
  if (i < n) ids[i] = (int32_t)i;
}

__global__ __launch_bounds__(RK_THREADS) void rk_gather_kernel(int32_t n, const int64_t* __restrict__ rank, const unsigned long long* __restrict__ differ, int n_fields, int f,
                                                             RkBufs b) {
  if (differ[f] == 0ull) return;  // the field orders nothing: no pass reads its keys
  const int side = rk_side(differ, n_fields, f, 0);
  const int64_t j = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
  if (j >= n) return;
  const int id = b.ids[side][j];
  b.keys[side][j] = rk_key((unsigned)id < (unsigned)n ? rank[id] : RANK_NONE, rk_base(differ, f));
}

__global__ __launch_bounds__(RK_THREADS) void rk_hist_kernel(int32_t n, const unsigned long long* __restrict__ differ, int n_fields, int f, int d, RkBufs b,
                                                           int32_t* __restrict__ hist, int64_t n_tiles) {
  __shared__ int s_hist[256];
  if (((differ[f] >> (8 * d)) & 255ull) == 0ull) return;  // block-uniform
  const unsigned long long* __restrict__ keys = b.keys[rk_side(differ, n_fields, f, d)];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * RK_TILE;
#pragma unroll
  for (int r = 0; r < RK_ROUNDS; ++r) {
    const int64_t j = base + r * RK_THREADS + threadIdx.x;
    if (j < n) atomicAdd(&s_hist[(unsigned)(keys[j] >> (8 * d)) & 255u], 1);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = s_hist[threadIdx.x];
}

__global__ __launch_bounds__(RK_THREADS) void rk_scatter_kernel(int32_t n, const unsigned long long* __restrict__ differ, int n_fields, int f, int d, RkBufs b,
                                                              const int64_t* __restrict__ offsets, int64_t n_tiles) {
  __shared__ int s_cnt[RK_NW][256];  // per wave and digit: the pairs of the round
  __shared__ int s_run[256];         // per digit: where the tile's next pair goes
  if (((differ[f] >> (8 * d)) & 255ull) == 0ull) return;  // block-uniform
  const int side = rk_side(differ, n_fields, f, d);
  const unsigned long long* __restrict__ src_k = b.keys[side];
  const int32_t* __restrict__ src_i = b.ids[side];
  unsigned long long* __restrict__ dst_k = b.keys[side ^ 1];
  int32_t* __restrict__ dst_i = b.ids[side ^ 1];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  s_run[tid] = (int)offsets[(int64_t)tid * n_tiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < RK_NW; ++w) s_cnt[w][tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * RK_TILE;
  for (int r = 0; r < RK_ROUNDS; ++r) {  // block-uniform
    const int64_t j = base + r * RK_THREADS + tid;
    const bool valid = j < n;
    const unsigned long long key = valid ? src_k[j] : 0ull;
    const int id = valid ? src_i[j] : 0;
    const unsigned digit = (unsigned)(key >> (8 * d)) & 255u;
    unsigned long long same = __ballot(valid ? 1 : 0);
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned mine = (digit >> bit) & 1u;
      const unsigned long long m = __ballot((int)mine);
      same &= mine ? m : ~m;
    }
    const int below = __popcll(same & ((1ull << lane) - 1ull));
    if (valid && below == 0) s_cnt[wave][digit] = __popcll(same);
    __syncthreads();
    if (valid) {
      int pos = s_run[digit] + below;
      for (int w = 0; w < wave; ++w) pos += s_cnt[w][digit];
      if ((unsigned)pos < (unsigned)n) {
        dst_k[pos] = key;
        dst_i[pos] = id;
      }
    }
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < RK_NW; ++w) {
      tot += s_cnt[w][tid];
      s_cnt[w][tid] = 0;
    }
    s_run[tid] += tot;
    __syncthreads();
  }
}

__global__ __launch_bounds__(RK_THREADS) void rk_finish_kernel(int32_t n, const unsigned long long* __restrict__ differ, int n_fields, RkBufs b, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
  if (i < n) out[i] = b.ids[rk_side(differ, n_fields, 0, 8)][i];
}

hipError_t launch_fill_order(hipStream_t st, int32_t n_items, const int64_t* const* ranks, int n_fields, const FillOrderScratch& s, int32_t* out_order) {
  if (n_items <= 0) return hipSuccess;
  const unsigned flat = (unsigned)(((int64_t)n_items + RK_THREADS - 1) / RK_THREADS);
  if (n_fields == 0) {
    hipLaunchKernelGGL(rk_iota_kernel, dim3(flat), dim3(RK_THREADS), 0, st, n_items, out_order);
    return hipGetLastError();
  }
  const int64_t n_tiles = fill_order_tiles(n_items);
  RkFields fields{};
  fields.n_fields = n_fields;
  for (int f = 0; f < n_fields; ++f) fields.rank[f] = ranks[f];
  const RkBufs b{{s.keys[0], s.keys[1]}, {s.ids[0], s.ids[1]}};
  hipError_t e = hipMemsetAsync(s.differ, 0, sizeof(unsigned long long) * RANK_MAX_FIELDS, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(s.differ + RANK_MAX_FIELDS, 0xff, sizeof(unsigned long long) * RANK_MAX_FIELDS, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(s.hist, 0, sizeof(int32_t) * 256 * (size_t)n_tiles, st);  // the scan of a digit that takes no pass reads it all the same
  if (e != hipSuccess) return e;
  const unsigned reduce_blocks = (unsigned)(n_tiles < 1024 ? n_tiles : 1024);
  hipLaunchKernelGGL(rk_base_kernel, dim3(reduce_blocks), dim3(RK_THREADS), 0, st, n_items, fields, s.differ + RANK_MAX_FIELDS);
  hipLaunchKernelGGL(rk_differ_kernel, dim3(reduce_blocks), dim3(RK_THREADS), 0, st, n_items, fields, s.differ, reinterpret_cast<unsigned*>(s.differ));
  hipLaunchKernelGGL(rk_iota_kernel, dim3(flat), dim3(RK_THREADS), 0, st, n_items, s.ids[0]);
  for (int f = n_fields - 1; f >= 0; --f) {
    hipLaunchKernelGGL(rk_gather_kernel, dim3(flat), dim3(RK_THREADS), 0, st, n_items, ranks[f], s.differ, n_fields, f, b);
    for (int d = 0; d < 8; ++d) {
      hipLaunchKernelGGL(rk_hist_kernel, dim3((unsigned)n_tiles), dim3(RK_THREADS), 0, st, n_items, s.differ, n_fields, f, d, b, s.hist, n_tiles);
      e = launch_scan_i32(st, s.hist, 256 * n_tiles, s.offsets, s.tile_sums);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(rk_scatter_kernel, dim3((unsigned)n_tiles), dim3(RK_THREADS), 0, st, n_items, s.differ, n_fields, f, d, b, s.offsets, n_tiles);
    }
  }
  hipLaunchKernelGGL(rk_finish_kernel, dim3(flat), dim3(RK_THREADS), 0, st, n_items, s.differ, n_fields, b, out_order);
  return hipGetLastError();
}

}  // namespace urcco
