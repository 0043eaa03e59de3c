// Device-resident item properties (decision D25 of DESIGN.md 7a; include/urcco.h urcco_dev_props_*): the item half of the event store -- $set, $unset and
// $delete events aggregated where they arrive, and the rule matrices, date arrays and "deleted" mask a serving model reads.  Compiled into
// ingest_kernels.hip behind cco_sorted_rows.h: it uses that header's sort + unique tails in their sentinel-dropping forms, its host helpers, and
// ingest_kernels.hip's grid helper.
//
// State, per property and item: t_set = the largest time of a $set, pos_set = the largest stream position + 1 among the sets of that time, t_unset = the
// largest time of an $unset; per store and item: t_del = the largest time of a $delete.  Times are held as (uint64)t ^ 2^63, which orders as the signed
// time does and leaves 0 -- INT64_MIN, "no value" -- for "nothing seen".  Every word only grows, by a maximum: the state does not depend on the order or
// on the batching of the events, and is reproducible bit for bit.
//   pr_times_kernel    launch 1 of an apply: t_set / t_unset = max(., time)
//   pr_pos_kernel      launch 2: every $set whose time is the item's t_set: pos_set = max(., position + 1).  Positions only grow from batch to batch, so a
//                      set of an earlier batch that still holds t_set is beaten by position exactly as it would be inside one call
//   pr_delete_kernel   t_del = max(., time)
// Popular items are hit by thousands of events (an item that toggles between in stock and sold out): a maximum only grows, so each kernel reads the word
// first and issues the atomic only if its event would raise it.  A stale read (L1 is not coherent with other CUs' atomics) can only be too small: it
// costs one unnecessary atomic, never a wrong result.  One word read and at most one atomic per event and launch.
//   pr_bounds_kernel   the length of the winner's value slice of every item whose property is alive, else 0
//   pr_rows_wave_kernel / pr_rows_block_kernel   the winner's slice, value ids outside 0 .. n_cols dropped, sorted, distinct -> the raw row; the classes of
//                      cco_sorted_rows.h (<= 64: one wave; <= 4096: one block in LDS; larger: one block in the raw row)
//   pr_dates_kernel    the winner's date, else INT64_MIN
//   pr_exists_kernel   0 for an item with a $delete that no set of any property is later than
// The row kernels hold no atomic: the wave kernel walks every item and leaves those of more than 64 values to the block kernel, whose blocks find them
// again by a ballot over 256 items at a time.  Wave = 64 lanes; wave primitives under wave-uniform control flow only, one per source line.
namespace urcco {

namespace {
__device__ __forceinline__ unsigned long long pr_bias(long long t) { return (unsigned long long)t ^ (1ull << 63); }

// alive: a set exists and is later than the last unset and the last delete (a tie goes to the unset / the delete)
__device__ __forceinline__ bool pr_alive(const PropState& s, int i) {
  const unsigned long long ts = s.t_set[i];
  return ts != 0ull && ts > s.t_unset[i] && !(s.t_del && ts <= s.t_del[i]);
}

// the winner's stream position, or -1: the property is dead, or pos_set names no position of the stream
__device__ __forceinline__ int64_t pr_winner(const PropState& s, int i) {
  if (!pr_alive(s, i)) return -1;
  const int64_t p = (int64_t)s.pos_set[i] - 1;
  return p >= 0 && p < s.n_events ? p : -1;
}

// the winner's slice of `values`: its start and its length, both clamped into the array
__device__ __forceinline__ int pr_window(const PropRows& a, int i, int64_t& seg) {
  seg = 0;
  const int64_t p = pr_winner(a.st, i);
  if (p < 0) return 0;
  int64_t lo = a.val_ptr[p], hi = a.val_ptr[p + 1];
  if (lo < 0) lo = 0;
  if (hi > a.n_values) hi = a.n_values;
  if (hi <= lo) return 0;
  seg = lo;
  return hi - lo > 0x7fffffffll ? 0x7fffffff : (int)(hi - lo);
}

// the slice the row kernels gather for item i: nothing when the row's bound ends beyond the capacity, and never more than the raw row holds (it holds the
// whole slice when the state is the one the bounds were taken from)
__device__ __forceinline__ int pr_job(const PropRows& a, int64_t i, int64_t& seg) {
  const int64_t s = a.raw.raw_ptr[i], e = a.raw.raw_ptr[i + 1];
  seg = 0;
  if (s < 0 || e > a.raw.capacity || e <= s) return 0;
  const int w = pr_window(a, (int)i, seg);
  return w > e - s ? (int)(e - s) : w;
}
}  // namespace

__global__ __launch_bounds__(256) void pr_times_kernel(int32_t n_items, int64_t n, const int32_t* __restrict__ items, const int64_t* __restrict__ times,
                                                       const uint8_t* __restrict__ kinds, unsigned long long* t_set, unsigned long long* t_unset) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const int i = items[p];
    const unsigned long long bt = pr_bias(times[p]);
    const unsigned kind = kinds ? kinds[p] : PROP_SET;
    if ((unsigned)i >= (unsigned)n_items || bt == 0ull) continue;
    if (kind == PROP_SET) {
      if (t_set[i] < bt) atomicMax(&t_set[i], bt);
    } else if (kind == PROP_UNSET) {
      if (t_unset[i] < bt) atomicMax(&t_unset[i], bt);
    }
  }
}

__global__ __launch_bounds__(256) void pr_pos_kernel(int32_t n_items, int64_t n, const int32_t* __restrict__ items, const int64_t* __restrict__ times,
                                                     const uint8_t* __restrict__ kinds, unsigned pos_base, const unsigned long long* __restrict__ t_set,
                                                     unsigned* pos_set) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const int i = items[p];
    const unsigned long long bt = pr_bias(times[p]);
    if ((unsigned)i >= (unsigned)n_items || bt == 0ull || (kinds && kinds[p] != PROP_SET)) continue;
    const unsigned pos1 = pos_base + (unsigned)p + 1u;
    if (t_set[i] == bt && pos_set[i] < pos1) atomicMax(&pos_set[i], pos1);
  }
}

__global__ __launch_bounds__(256) void pr_delete_kernel(int32_t n_items, int64_t n, const int32_t* __restrict__ items, const int64_t* __restrict__ times,
                                                        unsigned long long* t_del) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const int i = items[p];
    const unsigned long long bt = pr_bias(times[p]);
    if ((unsigned)i >= (unsigned)n_items || bt == 0ull) continue;
    if (t_del[i] < bt) atomicMax(&t_del[i], bt);
  }
}

hipError_t launch_props_apply(hipStream_t st, int n_cu, int32_t n_items, int64_t n, const int32_t* items, const int64_t* times, const uint8_t* kinds, int64_t pos_base,
                              unsigned long long* t_set, unsigned* pos_set, unsigned long long* t_unset) {
  if (n == 0 || n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(pr_times_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n_items, n, items, times, kinds, t_set, t_unset);
  hipLaunchKernelGGL(pr_pos_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n_items, n, items, times, kinds, (unsigned)pos_base, t_set, pos_set);
  return hipGetLastError();
}

hipError_t launch_props_delete(hipStream_t st, int n_cu, int32_t n_items, int64_t n, const int32_t* items, const int64_t* times, unsigned long long* t_del) {
  if (n == 0 || n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(pr_delete_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n_items, n, items, times, t_del);
  return hipGetLastError();
}

// bnd[i] = the length of the winner's slice
__global__ __launch_bounds__(256) void pr_bounds_kernel(PropRows a, int32_t* __restrict__ bnd) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n_items; i += (int64_t)gridDim.x * 256) {
    int64_t seg;
    bnd[i] = pr_window(a, (int)i, seg);
  }
}

hipError_t launch_props_bounds(hipStream_t st, int n_cu, const PropRows& a, int32_t* bnd, int64_t* tile_sums, int64_t* row_ptr) {
  if (a.n_items == 0) return hipMemsetAsync(row_ptr, 0, sizeof(int64_t), st);
  hipLaunchKernelGGL(pr_bounds_kernel, dim3(ig_grid(a.n_items, n_cu)), dim3(256), 0, st, a, bnd);
  return launch_scan_i32(st, bnd, a.n_items, row_ptr, tile_sums);
}

// One wave per item.  A row whose bound ends beyond the capacity is left empty; one of more than 64 values is the block kernel's.
__global__ __launch_bounds__(256) void pr_rows_wave_kernel(PropRows a) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t i = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; i < a.n_items; i += n_waves) {  // wave-uniform
    int64_t seg;
    const int w = pr_job(a, i, seg);
    if (w > SR_WAVE) continue;
    if (w == 0) {
      if (lane == 0) a.raw.len[i] = 0;
      continue;
    }
    int v = SR_SENT;
    if (lane < w) {
      const int c = a.values[seg + lane];
      if (c >= 0 && c < a.n_cols) v = c;
    }
    const int len = sr_wave_tail<true>(v, lane, SR_WAVE, a.raw.tmp + a.raw.raw_ptr[i]);
    if (lane == 0) a.raw.len[i] = len;
  }
}

// 256 items per round and block: a ballot marks those of more than 64 values, then the whole block serves them one after the other.
__global__ __launch_bounds__(256) void pr_rows_block_kernel(PropRows a) {
  __shared__ int s_v[SR_LDS];
  __shared__ unsigned long long s_big[256 / SR_WAVE];
  const int lane = threadIdx.x & (SR_WAVE - 1), wave = threadIdx.x / SR_WAVE;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.n_items; base += (int64_t)gridDim.x * 256) {  // block-uniform
    const int64_t mine = base + threadIdx.x;
    bool big = false;
    if (mine < a.n_items) {
      int64_t seg;
      big = pr_job(a, mine, seg) > SR_WAVE;
    }
    const unsigned long long m = __ballot(big);
    if (lane == 0) s_big[wave] = m;
    __syncthreads();
    for (int wv = 0; wv < 256 / SR_WAVE; ++wv) {
      unsigned long long left = s_big[wv];  // block-uniform
      while (left) {
        const int64_t i = base + wv * SR_WAVE + __ffsll((long long)left) - 1;
        left &= left - 1ull;
        int64_t seg;
        const int w = pr_job(a, i, seg);
        const int32_t* __restrict__ src = a.values + seg;
        int32_t* row = a.raw.tmp + a.raw.raw_ptr[i];
        const int n_cols = a.n_cols;
        if (w <= SR_LDS) {
          int P = 2;
          while (P < w) P <<= 1;
          for (int t = threadIdx.x; t < P; t += 256) {
            int v = SR_SENT;
            if (t < w) {
              const int c = src[t];
              if (c >= 0 && c < n_cols) v = c;
            }
            s_v[t] = v;
          }
        } else {
          for (int t = threadIdx.x; t < w; t += 256) {
            const int c = src[t];
            row[t] = c >= 0 && c < n_cols ? c : SR_SENT;
          }
        }
        __syncthreads();  // the staged slice is complete
        const int len = sr_block_tail<true>(row, w, s_v);
        if (threadIdx.x == 0) a.raw.len[i] = len;
        __syncthreads();
      }
    }
    __syncthreads();  // s_big is read to the end before the next round writes it
  }
}

// a.raw: scratch.  row_ptr holds the bounds' scan on entry, the final row starts on return.
hipError_t launch_props_rows(hipStream_t st, int n_cu, const PropRows& a, int64_t* tile_sums, int64_t* row_ptr, int32_t* col_idx) {
  const RowsOut out{a.raw, row_ptr, col_idx};
  const hipError_t e = sr_seed_raw_ptr(st, &out, 1, a.n_items);
  if (e != hipSuccess || a.n_items == 0) return e;
  hipLaunchKernelGGL(pr_rows_wave_kernel, dim3(ig_grid((int64_t)a.n_items * SR_WAVE, n_cu)), dim3(256), 0, st, a);
  const int64_t rounds = ((int64_t)a.n_items + 255) / 256, bgrid = rounds < (int64_t)n_cu * 8 ? rounds : (int64_t)n_cu * 8;
  hipLaunchKernelGGL(pr_rows_block_kernel, dim3((unsigned)bgrid), dim3(256), 0, st, a);
  return sr_finish_rows(st, n_cu, &out, 1, a.n_items, tile_sums);
}

__global__ __launch_bounds__(256) void pr_dates_kernel(int32_t n_items, PropState s, const int64_t* __restrict__ date_values, int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * 256) {
    const int64_t p = pr_winner(s, (int)i);
    out[i] = p >= 0 ? date_values[p] : INT64_MIN;
  }
}

hipError_t launch_props_dates(hipStream_t st, int n_cu, int32_t n_items, const PropState& s, const int64_t* date_values, int64_t* out) {
  if (n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(pr_dates_kernel, dim3(ig_grid(n_items, n_cu)), dim3(256), 0, st, n_items, s, date_values, out);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void pr_exists_kernel(int32_t n_items, const unsigned long long* __restrict__ t_del, PropSets sets, uint8_t* __restrict__ mask) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * 256) {
    const unsigned long long td = t_del[i];
    bool later = td == 0ull;  // no $delete: the item exists
    for (int p = 0; p < sets.n_props; ++p) later |= sets.t_set[p][i] > td;
    mask[i] = later ? 1 : 0;
  }
}

hipError_t launch_props_exists(hipStream_t st, int n_cu, int32_t n_items, const unsigned long long* t_del, const PropSets& sets, uint8_t* mask) {
  if (n_items == 0) return hipSuccess;
  hipLaunchKernelGGL(pr_exists_kernel, dim3(ig_grid(n_items, n_cu)), dim3(256), 0, st, n_items, t_del, sets, mask);
  return hipGetLastError();
}

// ---- compaction (decision D28) -------------------------------------------------------------------------------------
// One property's stream without the values no item's state names any more: the winners -- the positions pos_set[i] - 1 inside the stream, one per item --
// numbered in ascending old position are the new stream.  Filter-then-compact, as the history's trim:
//   mark       W: one bit per stream position, zeroed; every item sets the bit of its winner (atomicOr: the only atomics, one per item with a set)
//   count      cnt[w] = popcount of word w; launch_scan_i32 -> base; rank(p) = ht_rank(base, W, p); K = base[number of words]
//   items      out_pos_set[i] = rank(winner) + 1, else 0; a list property: len[rank] = the winner's slice length, clamped as pr_window clamps it, when the
//              property is alive, else 0 (a maximum only grows: a dead winner never lives again), src[rank] = the slice's clamped start
//   positions  out_old_pos[rank(p)] = p for every set bit; a date property: out_date_values[rank(p)] = date_values[p]
//   scan       len over the bound min(n_items, n_events) of K (zero beyond K: the array is cleared first) -> the new slice starts, every one
//              clamped to n_values (only a malformed val_ptr, whose slices overlap, reaches the clamp): V = the last
//   copy       balanced by ENTRIES, the append's copy kernel over (new slice starts, src): a block takes PC_TILE consecutive entries of out_values,
//              finds the tile's first and last winner with one binary search each, and every entry then finds its winner among those -- staged in LDS when
//              the tile touches at most PC_LDS winners (empty slices in between included), in global memory otherwise.  One winner of 8193 values is four
//              tiles; a million of two values are a thousand winners a tile
// Two items that name one position set one bit and write the same rank; when one of them is alive and the other is not, which length wins is
// unspecified -- the result may be wrong, but every length is 0 or the clamped slice's, so no access leaves the arrays.
constexpr int PC_TILE = 2048;  // entries of out_values per block and round: 8 per thread
constexpr int PC_LDS = 2048;   // winners of a tile whose slice starts and sources are staged in LDS (8 + 16 KiB)
static_assert(PC_LDS >= PC_TILE, "a tile of one-value winners must fit the staging");

namespace {
// the winner of item i whatever the property's life: the position pos_set names, or -1
__device__ __forceinline__ int64_t pc_winner(const PropState& s, int64_t i) {
  const int64_t p = (int64_t)s.pos_set[i] - 1;
  return p >= 0 && p < s.n_events ? p : -1;
}
}  // namespace

__global__ __launch_bounds__(256) void pc_mark_kernel(CompactArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n_items; i += (int64_t)gridDim.x * 256) {
    const int64_t p = pc_winner(a.st, i);
    if (p >= 0) atomicOr(&a.bits[p >> 6], 1ull << (p & 63));
  }
}

__global__ __launch_bounds__(256) void pc_count_kernel(CompactArgs a) {
  const int64_t n_words = (a.st.n_events + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * 256) a.cnt[w] = __popcll(a.bits[w]);
}

__global__ __launch_bounds__(256) void pc_items_kernel(CompactArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n_items; i += (int64_t)gridDim.x * 256) {
    const int64_t p = pc_winner(a.st, i);
    if (p < 0) {
      a.out_pos_set[i] = 0u;
      continue;
    }
    const int64_t j = ht_rank(a.base, a.bits, p);
    a.out_pos_set[i] = (unsigned)j + 1u;
    if (!a.val_ptr) continue;
    int64_t lo = a.val_ptr[p], hi = a.val_ptr[p + 1];
    if (lo < 0) lo = 0;
    if (hi > a.n_values) hi = a.n_values;
    if (hi < lo) hi = lo;
    a.len[j] = pr_alive(a.st, (int)i) ? (hi - lo > 0x7fffffffll ? 0x7fffffff : (int32_t)(hi - lo)) : 0;
    a.src[j] = lo;
  }
}

__global__ __launch_bounds__(256) void pc_positions_kernel(CompactArgs a) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.st.n_events; p += (int64_t)gridDim.x * 256) {
    const unsigned long long word = a.bits[p >> 6];
    const int b = (int)(p & 63);
    if (!((word >> b) & 1ull)) continue;
    const int64_t j = a.base[p >> 6] + __popcll(word & ((1ull << b) - 1ull));
    a.out_old_pos[j] = (int32_t)p;
    if (a.date_values) a.out_date_values[j] = a.date_values[p];
  }
}

// out_val_ptr[0 .. K] = the scan of the lengths, clamped to n_values; the first thread writes the counts
__global__ __launch_bounds__(256) void pc_finish_kernel(CompactArgs a) {
  const int64_t k = a.base[(a.st.n_events + 63) >> 6];
  if (a.val_ptr)
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j <= k; j += (int64_t)gridDim.x * 256) {
      const int64_t v = a.val_base[j];
      a.out_val_ptr[j] = v < a.n_values ? v : a.n_values;
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.out_counts[0] = k;
    const int64_t v = a.val_ptr ? a.val_base[k] : 0;
    a.out_counts[1] = v < a.n_values ? v : a.n_values;
  }
}

// out_values[e] = values[src[j(e)] + e - out_val_ptr[j(e)]] for every entry e below V = out_val_ptr[K]: K and V are read here, the host knows only the bound n_values
__global__ __launch_bounds__(256) void pc_copy_kernel(CompactArgs a) {
  __shared__ int s_start[PC_LDS];      // slice starts relative to the tile's first entry; [0] = 0: the first winner's slice may begin before the tile
  __shared__ int64_t s_delta[PC_LDS];  // source index minus destination index of the winner's slice
  __shared__ int64_t s_j[2];
  const int64_t* __restrict__ vp = a.out_val_ptr;
  const int64_t k = a.base[(a.st.n_events + 63) >> 6];
  const int64_t n_v = vp[k];
  for (int64_t e0 = (int64_t)blockIdx.x * PC_TILE; e0 < n_v; e0 += (int64_t)gridDim.x * PC_TILE) {  // block-uniform
    const int n = (int)(n_v - e0 < PC_TILE ? n_v - e0 : PC_TILE);
    if (threadIdx.x < 2) s_j[threadIdx.x] = ha_user_of(vp, 0, k, threadIdx.x == 0 ? e0 : e0 + n - 1);
    __syncthreads();
    const int64_t j_lo = s_j[0], j_hi = s_j[1];
    const int64_t span = j_hi - j_lo + 1;
    if (span >= 1 && span <= PC_LDS) {  // block-uniform
      for (int i = threadIdx.x; i < (int)span; i += 256) {
        const int64_t r = vp[j_lo + i] - e0;
        s_start[i] = r < 0 ? 0 : (int)r;
        s_delta[i] = a.src[j_lo + i] - vp[j_lo + i];
      }
      __syncthreads();
      for (int t = threadIdx.x; t < n; t += 256) {
        int lo = 0, hi = (int)span;
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (s_start[mid] <= t) lo = mid;
          else hi = mid;
        }
        a.out_values[e0 + t] = a.values[e0 + t + s_delta[lo]];
      }
    } else {
      for (int t = threadIdx.x; t < n; t += 256) {
        const int64_t j = ha_user_of(vp, j_lo, j_hi + 1, e0 + t);
        a.out_values[e0 + t] = a.values[e0 + t + a.src[j] - vp[j]];
      }
    }
    __syncthreads();  // s_j and the staged slice are free for the next tile
  }
}

// a.bits, cnt, base, len, src, val_base, tile_sums: scratch.  Outputs must not overlap inputs.
hipError_t launch_props_compact(hipStream_t st, int n_cu, const CompactArgs& a) {
  const int64_t n = a.st.n_events, n_words = (n + 63) >> 6;
  const int64_t k_max = a.n_items < n ? a.n_items : n;
  hipError_t e;
  if (n_words > 0) {
    e = hipMemsetAsync(a.bits, 0, sizeof(unsigned long long) * (size_t)n_words, st);
    if (e != hipSuccess) return e;
    if (a.n_items > 0) hipLaunchKernelGGL(pc_mark_kernel, dim3(ig_grid(a.n_items, n_cu)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pc_count_kernel, dim3(ig_grid(n_words, n_cu)), dim3(256), 0, st, a);
  }
  e = launch_scan_i32(st, a.cnt, n_words, a.base, a.tile_sums);
  if (e != hipSuccess) return e;
  if (a.val_ptr && k_max > 0) {
    e = hipMemsetAsync(a.len, 0, sizeof(int32_t) * (size_t)k_max, st);
    if (e != hipSuccess) return e;
  }
  if (a.n_items > 0) hipLaunchKernelGGL(pc_items_kernel, dim3(ig_grid(a.n_items, n_cu)), dim3(256), 0, st, a);
  if (n > 0) hipLaunchKernelGGL(pc_positions_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, a);
  if (a.val_ptr) {
    e = launch_scan_i32(st, a.len, k_max, a.val_base, a.tile_sums);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pc_finish_kernel, dim3(ig_grid(k_max + 1, n_cu)), dim3(256), 0, st, a);
  if (a.val_ptr && a.n_values > 0 && k_max > 0) {
    const int64_t tiles = (a.n_values + PC_TILE - 1) / PC_TILE, cap = (int64_t)n_cu * 8;
    hipLaunchKernelGGL(pc_copy_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace urcco
