// Device-resident user history (decision D17 of DESIGN.md 7a; include/urcco.h urcco_dev_history_*): the event-store half of a
// batch of queries.  Compiled into ingest_kernels.hip behind cco_sorted_rows.h and cco_select.h (it uses their tails, host helpers and select, and the file's grid helper).
//
// What the reference reads from the event store per query (getBiasedRecentUserActions, URAlgorithm.scala:795-839: the most recent
// maxItemsPerUser events per event type, then distinct; getExcludedItems, :741-767: every item of the blacklist events) is here
//   index   stream positions by user: count per user -> scan -> scatter by cursor (order inside a user's segment unspecified)
//   append  the index of the stream grown by a batch: old segments copied at their shifts, the batch scattered behind them (D21)
//   trim    the stream and the index without the events before a cut-off and those of listed users: "kept" bitmaps, popcount scans, ranks (D22)
//   matrix  the Preparator's output from the index: the users that train, per event type the user x column CSR; heavy users through a column bitmap (D23)
//   bounds  per (query, type) min(n_u, max_items), per query the blacklist events + the extra exclusion row: scans = raw row starts
//   rows    per (query, type): the window = the min(n_u, max_items) largest keys (time, position) of the user's events -- found by an
//           8-bit radix SELECT over the 96-bit keys when n_u > max_items, never by sorting the events -- then sort + unique of the
//           window's columns; per query the same sort + unique tail over the mapped blacklist events and the extra row
//   compact raw rows -> final CSR
// Three classes by the number of events n_u of the (query, type), chosen on the device from the index:
//   <= 64     one wave: keys in registers, rank by cross-lane compares, bitonic network + ballot unique in registers
//   <= 4096   one block: keys in LDS, select with an LDS histogram per discriminating digit, window columns sorted in LDS
//   larger    the same block code with the keys re-read from global memory per discriminating digit; the window is staged in its
//             raw row (<= max_items entries) and sorted in LDS up to 4096 entries, in global memory beyond
// The select is the unit of cco_select.h.  A digit in which all keys of the user agree (the high bytes of millisecond times, every time byte
// without times) costs no pass: sel_differ ORs key ^ key[0] over the events first.  Keys are unique (the position is part of them), so the order is total and the
// rows do not depend on the order the index scatter left.  Wave = 64 lanes; wave primitives under wave-uniform control flow only.
namespace urcco {

namespace {
constexpr unsigned long long HS_SIGN = 0x8000000000000000ull;  // int64 time -> order-preserving unsigned

__device__ __forceinline__ int hs_user_events(const HistEvent& e, const int32_t* q_users, int64_t n_users, int64_t q, int64_t& seg) {
  const int u = q_users[q];
  if (u < 0 || u >= n_users) { seg = 0; return 0; }
  seg = e.idx_row_ptr[u];
  return (int)(e.idx_row_ptr[u + 1] - seg);
}

// an event's column as an exclusion: through the type's column map into the primary's items; SR_SENT = none
__device__ __forceinline__ int hs_excl_id(const HistEvent& e, int item, int n_items) {
  if (item < 0) return SR_SENT;
  if (e.col_map) item = item < e.n_cols ? e.col_map[item] : -1;
  return item >= 0 && item < n_items ? item : SR_SENT;
}
}  // namespace

// ---- index ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hs_count_users_kernel(int64_t n, const int32_t* __restrict__ users, int64_t n_users, int32_t* __restrict__ cnt) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const int u = users[p];
    if (u >= 0 && u < n_users) atomicAdd(&cnt[u], 1);
  }
}

__global__ __launch_bounds__(256) void hs_scatter_pos_kernel(int64_t n, const int32_t* __restrict__ users, int64_t n_users, const int64_t* __restrict__ row_ptr,
                                                             int32_t* __restrict__ cursor, int32_t* __restrict__ out_pos) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const int u = users[p];
    if (u >= 0 && u < n_users) out_pos[row_ptr[u] + atomicAdd(&cursor[u], 1)] = (int32_t)p;
  }
}

hipError_t launch_history_index(hipStream_t st, int n_cu, int64_t n, const int32_t* users, int64_t n_users, int32_t* cnt, int64_t* tile_sums,
                                int64_t* out_row_ptr, int32_t* out_pos) {
  if (n_users == 0) return hipMemsetAsync(out_row_ptr, 0, sizeof(int64_t), st);
  hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n_users, st);
  if (e != hipSuccess) return e;
  if (n > 0) hipLaunchKernelGGL(hs_count_users_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, users, n_users, cnt);
  e = launch_scan_i32(st, cnt, n_users, out_row_ptr, tile_sums);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n_users, st);  // now the scatter cursors
  if (e != hipSuccess) return e;
  if (n > 0) hipLaunchKernelGGL(hs_scatter_pos_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, users, n_users, out_row_ptr, cnt, out_pos);
  return hipGetLastError();
}

// ---- append (decision D21) -----------------------------------------------------------------------------------------
// The index of a stream that grew by a batch, from the old index and the batch's users alone.  add[u] = the batch's events of the users below u
// (count -> scan, as in the index build): user u's old segment moves from old_row_ptr[u] to old_row_ptr[u] + add[u] unchanged, the batch's positions
// n_old + p fill the gap behind it.  The copy is balanced by ENTRIES: a block takes HA_TILE consecutive entries of old_pos, whatever the users are,
// finds the tile's first and last user with one binary search each, and every entry then finds its user among those -- in LDS when the tile touches
// at most HA_LDS_USERS users (empty ones in between included), in global memory otherwise.  HA_LDS_USERS >= HA_TILE: a tile without empty users
// touches at most HA_TILE of them, so users with one event each are staged too and only a tile that crosses a run of empty users searches global
// memory.  A tile inside one user's segment is a coalesced copy at a constant shift; a run of empty users at a tile's edge costs the two searches that
// step over it.  No atomics here: the batch's positions are scattered by cursor.
constexpr int HA_TILE = 2048;       // old index entries per block and round: 8 per thread
constexpr int HA_LDS_USERS = 2048;  // users of a tile whose segment starts and shifts are staged in LDS (16 KiB)
static_assert(HA_LDS_USERS >= HA_TILE, "a tile of one-event users must fit the staging");

namespace {
// the largest u in [lo, hi) with rp[u] <= key; rp[lo] <= key < rp[hi] on entry: the user whose segment holds entry `key`, empty users stepped over
__device__ __forceinline__ int64_t ha_user_of(const int64_t* __restrict__ rp, int64_t lo, int64_t hi, int64_t key) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (rp[mid] <= key) lo = mid;
    else hi = mid;
  }
  return lo;
}
}  // namespace

// out_row_ptr[u] = old_row_ptr[min(u, n_users_old)] + add[u] for u = 0 .. n_users: users beyond the old id space start where the old index ends
__global__ __launch_bounds__(256) void hs_append_row_ptr_kernel(int64_t n_users, int64_t n_users_old, const int64_t* __restrict__ old_row_ptr,
                                                                const int64_t* __restrict__ add, int64_t* __restrict__ out_row_ptr) {
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u <= n_users; u += (int64_t)gridDim.x * 256)
    out_row_ptr[u] = (n_users_old > 0 ? old_row_ptr[u < n_users_old ? u : n_users_old] : 0) + add[u];
}

// out_pos[e + add[u(e)]] = old_pos[e] for every old entry e.  The entries are old_row_ptr[n_users_old] of them (read here: the host knows only the bound
// n_old, which sizes the grid and caps the count).  A row_ptr that does not ascend gives a wrong index, never a write outside out_pos: every e is below
// n_old and every shift is an add[u] of a user 0 .. n_users_old.
__global__ __launch_bounds__(256) void hs_append_copy_kernel(int64_t n_old, int64_t n_users_old, const int64_t* __restrict__ old_row_ptr,
                                                             const int32_t* __restrict__ old_pos, const int64_t* __restrict__ add, int32_t* __restrict__ out_pos) {
  __shared__ int s_start[HA_LDS_USERS];  // segment starts relative to the tile's first entry; [0] = 0: the first user's segment may begin before the tile
  __shared__ int s_add[HA_LDS_USERS];
  __shared__ int64_t s_u[2];
  int64_t n_e = old_row_ptr[n_users_old];
  if (n_e > n_old) n_e = n_old;
  for (int64_t e0 = (int64_t)blockIdx.x * HA_TILE; e0 < n_e; e0 += (int64_t)gridDim.x * HA_TILE) {  // block-uniform
    const int n = (int)(n_e - e0 < HA_TILE ? n_e - e0 : HA_TILE);
    if (threadIdx.x < 2) s_u[threadIdx.x] = ha_user_of(old_row_ptr, 0, n_users_old, threadIdx.x == 0 ? e0 : e0 + n - 1);
    __syncthreads();
    const int64_t u_lo = s_u[0], u_hi = s_u[1];
    const int64_t span = u_hi - u_lo + 1;
    if (span >= 1 && span <= HA_LDS_USERS) {  // block-uniform
      for (int i = threadIdx.x; i < (int)span; i += 256) {
        const int64_t r = old_row_ptr[u_lo + i] - e0;
        s_start[i] = r < 0 ? 0 : (int)r;
        s_add[i] = (int)add[u_lo + i];
      }
      __syncthreads();
      for (int k = threadIdx.x; k < n; k += 256) {
        int lo = 0, hi = (int)span;
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (s_start[mid] <= k) lo = mid;
          else hi = mid;
        }
        out_pos[e0 + k + s_add[lo]] = old_pos[e0 + k];
      }
    } else {
      for (int k = threadIdx.x; k < n; k += 256) {
        const int64_t u = ha_user_of(old_row_ptr, u_lo, u_hi + 1, e0 + k);
        out_pos[e0 + k + add[u]] = old_pos[e0 + k];
      }
    }
    __syncthreads();  // s_u and the staged slice are free for the next tile
  }
}

// the batch's positions behind the old segments: hs_scatter_pos_kernel with the base old end of u + add[u]
__global__ __launch_bounds__(256) void hs_append_scatter_kernel(int64_t n_old, int64_t n_new, const int32_t* __restrict__ new_users, int64_t n_users,
                                                                int64_t n_users_old, const int64_t* __restrict__ old_row_ptr, const int64_t* __restrict__ add,
                                                                int32_t* __restrict__ cursor, int32_t* __restrict__ out_pos) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_new; p += (int64_t)gridDim.x * 256) {
    const int u = new_users[p];
    if (u >= 0 && u < n_users) {
      const int64_t old_end = n_users_old > 0 ? old_row_ptr[u + 1 < n_users_old ? u + 1 : n_users_old] : 0;
      out_pos[old_end + add[u] + atomicAdd(&cursor[u], 1)] = (int32_t)(n_old + p);
    }
  }
}

// cnt [n_users], add [n_users + 1], tile_sums: scratch.  out_* must not overlap old_*.
hipError_t launch_history_append(hipStream_t st, int n_cu, int64_t n_old, int64_t n_users_old, const int64_t* old_row_ptr, const int32_t* old_pos, int64_t n_new,
                                 const int32_t* new_users, int64_t n_users, int32_t* cnt, int64_t* add, int64_t* tile_sums, int64_t* out_row_ptr, int32_t* out_pos) {
  if (n_users == 0) return hipMemsetAsync(out_row_ptr, 0, sizeof(int64_t), st);
  hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n_users, st);
  if (e != hipSuccess) return e;
  if (n_new > 0) hipLaunchKernelGGL(hs_count_users_kernel, dim3(ig_grid(n_new, n_cu)), dim3(256), 0, st, n_new, new_users, n_users, cnt);
  e = launch_scan_i32(st, cnt, n_users, add, tile_sums);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hs_append_row_ptr_kernel, dim3(ig_grid(n_users + 1, n_cu)), dim3(256), 0, st, n_users, n_users_old, old_row_ptr, add, out_row_ptr);
  if (n_users_old > 0 && n_old > 0) {
    const int64_t tiles = (n_old + HA_TILE - 1) / HA_TILE, cap = (int64_t)n_cu * 8;
    hipLaunchKernelGGL(hs_append_copy_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), 0, st, n_old, n_users_old, old_row_ptr, old_pos, add, out_pos);
  }
  if (n_new > 0) {
    e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n_users, st);  // now the scatter cursors
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hs_append_scatter_kernel, dim3(ig_grid(n_new, n_cu)), dim3(256), 0, st, n_old, n_new, new_users, n_users, n_users_old, old_row_ptr, add, cnt, out_pos);
  }
  return hipGetLastError();
}

// ---- trim (decision D22) -------------------------------------------------------------------------------------------
// A stream and its index without the events older than a cut-off and without the events of listed users, from the stream and the index alone.
// Stream rule: dropping events keeps the survivors' order, so new_of[p] = the kept positions below p renumbers them and the recency key orders them
// as before.  Index rule: a user's segment is contiguous, so the exclusive scan of "entry kept" over the index entries is the new place of every
// entry AND the new start of every user: out_row_ptr[u] = rank(idx_row_ptr[u]).  No `users` array, no per-user atomic, no per-user launch.
//   mark     D: one bit per stream position, zeroed; the segments of the listed users set the bits of their positions (atomicOr: the only atomics,
//            proportional to the dropped users' entries; duplicates in the list set the same bits again)
//   keep     S = time test passed and D clear, in place over D: one wave per word of 64 positions, the word is the wave's ballot, its popcount the count
//   entries  I[e] = S bit of idx_pos[e] for the n_e = min(idx_row_ptr[n_users], n_events) entries (read here, as the append's copy kernel reads it)
//   scans    launch_scan_i32 over the words' popcounts: word bases, the total behind the last word
//   rank(x)  base[x >> 6] + popcount(word[x >> 6] below bit x & 63); x & 63 == 0 reads no word: x may be the array's length on a word boundary
//   compact  kept position p -> out_items / out_times[rankS(p)]; kept entry e -> out_pos[rankI(e)] = rankS(idx_pos[e]); out_row_ptr[u] = rankI(start of u)
// The mark is balanced by ENTRIES as far as one list entry goes: a listed user's segment is cut into chunks of HT_CHUNK entries that HT_SPLIT blocks
// take in turn, so a user of 10^6 entries is 489 chunks over 32 blocks, about 128 atomics per thread; a user of up to HT_CHUNK entries costs one block
// one round and 31 blocks two loads of row starts each.  Entries of idx_pos outside 0 .. n_events count as dropped, row starts are clamped into
// 0 .. n_e: whatever the index holds, no access leaves the arrays.
constexpr int HT_CHUNK = 2048;  // index entries of a listed user per block and round: 8 per thread
constexpr int HT_SPLIT = 32;    // blocks that share one listed user's chunks

namespace {
// the entries of the index: what idx_row_ptr[n_users] says, at most n_events, never negative
__device__ __forceinline__ int64_t ht_entries(const int64_t* __restrict__ idx_row_ptr, int64_t n_users, int64_t n_events) {
  const int64_t n_e = n_users > 0 ? idx_row_ptr[n_users] : 0;
  return n_e < 0 ? 0 : n_e < n_events ? n_e : n_events;
}
__device__ __forceinline__ int64_t ht_clamp(int64_t x, int64_t hi) { return x < 0 ? 0 : x < hi ? x : hi; }
// set bits of `words` below x; x in 0 .. 64 * (number of words), base holds one more entry than there are words
__device__ __forceinline__ int64_t ht_rank(const int64_t* __restrict__ base, const unsigned long long* __restrict__ words, int64_t x) {
  const int b = (int)(x & 63);
  return base[x >> 6] + (b ? __popcll(words[x >> 6] & ((1ull << b) - 1ull)) : 0);
}
}  // namespace

__global__ __launch_bounds__(256) void ht_mark_kernel(int64_t n_events, int64_t n_users, const int64_t* __restrict__ idx_row_ptr, const int32_t* __restrict__ idx_pos,
                                                      int64_t n_drop, const int32_t* __restrict__ drop_users, unsigned long long* __restrict__ bits) {
  const int64_t n_e = ht_entries(idx_row_ptr, n_users, n_events);
  for (int64_t j = blockIdx.x; j < n_drop * HT_SPLIT; j += gridDim.x) {  // block-uniform
    const int u = drop_users[j / HT_SPLIT];
    if (u < 0 || u >= n_users) continue;
    const int64_t lo = ht_clamp(idx_row_ptr[u], n_e), hi = ht_clamp(idx_row_ptr[u + 1], n_e);
    for (int64_t c = lo + (j % HT_SPLIT) * HT_CHUNK; c < hi; c += (int64_t)HT_SPLIT * HT_CHUNK) {
      const int64_t end = c + HT_CHUNK < hi ? c + HT_CHUNK : hi;
      for (int64_t e = c + threadIdx.x; e < end; e += 256) {
        const int p = idx_pos[e];
        if (p >= 0 && p < n_events) atomicOr(&bits[p >> 6], 1ull << (p & 63));
      }
    }
  }
}

// bits: D on entry when has_drop (else not read), S on return; cnt[w] = popcount of word w.  Bits at and beyond n_events are 0.
__global__ __launch_bounds__(256) void ht_keep_kernel(int64_t n_events, const int64_t* __restrict__ times_ms, int64_t min_time_ms, bool has_drop,
                                                      unsigned long long* bits, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_words = (n_events + 63) >> 6, n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t w = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; w < n_words; w += n_waves) {  // wave-uniform
    const int64_t p = (w << 6) + lane;
    const unsigned long long d = has_drop ? bits[w] : 0ull;
    bool keep = p < n_events && !((d >> lane) & 1ull);
    if (keep && times_ms) keep = times_ms[p] >= min_time_ms;
    const unsigned long long word = __ballot(keep);
    if (lane == 0) {
      bits[w] = word;
      cnt[w] = __popcll(word);
    }
  }
}

// I[e] = S bit of idx_pos[e]; words and counts for all ceil(n_events / 64) words, zero at and beyond n_e
__global__ __launch_bounds__(256) void ht_entries_kernel(int64_t n_events, int64_t n_users, const int64_t* __restrict__ idx_row_ptr, const int32_t* __restrict__ idx_pos,
                                                         const unsigned long long* __restrict__ s_bits, unsigned long long* __restrict__ i_bits,
                                                         int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_e = ht_entries(idx_row_ptr, n_users, n_events);
  const int64_t n_words = (n_events + 63) >> 6, n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t w = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; w < n_words; w += n_waves) {  // wave-uniform
    const int64_t e = (w << 6) + lane;
    bool keep = false;
    if (e < n_e) {
      const int p = idx_pos[e];
      if (p >= 0 && p < n_events) keep = (s_bits[p >> 6] >> (p & 63)) & 1ull;
    }
    const unsigned long long word = __ballot(keep);
    if (lane == 0) {
      i_bits[w] = word;
      cnt[w] = __popcll(word);
    }
  }
}

// kept position p -> slot rankS(p): the kept positions of a wave's 64 fill one contiguous run
__global__ __launch_bounds__(256) void ht_compact_stream_kernel(int64_t n_events, const int32_t* __restrict__ items, const int64_t* __restrict__ times_ms,
                                                                const unsigned long long* __restrict__ s_bits, const int64_t* __restrict__ s_base,
                                                                int32_t* __restrict__ out_items, int64_t* __restrict__ out_times) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_events; p += (int64_t)gridDim.x * 256) {
    const unsigned long long word = s_bits[p >> 6];
    const int b = (int)(p & 63);
    if (!((word >> b) & 1ull)) continue;
    const int64_t dst = s_base[p >> 6] + __popcll(word & ((1ull << b) - 1ull));
    out_items[dst] = items[p];
    if (times_ms) out_times[dst] = times_ms[p];
  }
}

__global__ __launch_bounds__(256) void ht_compact_index_kernel(int64_t n_events, int64_t n_users, const int64_t* __restrict__ idx_row_ptr, const int32_t* __restrict__ idx_pos,
                                                               const unsigned long long* __restrict__ s_bits, const int64_t* __restrict__ s_base,
                                                               const unsigned long long* __restrict__ i_bits, const int64_t* __restrict__ i_base,
                                                               int32_t* __restrict__ out_pos) {
  const int64_t n_e = ht_entries(idx_row_ptr, n_users, n_events);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_e; e += (int64_t)gridDim.x * 256) {
    const unsigned long long word = i_bits[e >> 6];
    const int b = (int)(e & 63);
    if (!((word >> b) & 1ull)) continue;  // a kept entry names a position inside the stream: ht_entries_kernel tested it
    out_pos[i_base[e >> 6] + __popcll(word & ((1ull << b) - 1ull))] = (int32_t)ht_rank(s_base, s_bits, idx_pos[e]);
  }
}

// out_row_ptr[u] = rankI(start of u) for u = 0 .. n_users; the first thread writes the counts: the totals behind the last words
__global__ __launch_bounds__(256) void ht_row_ptr_kernel(int64_t n_events, int64_t n_users, const int64_t* __restrict__ idx_row_ptr,
                                                         const unsigned long long* __restrict__ i_bits, const int64_t* __restrict__ s_base,
                                                         const int64_t* __restrict__ i_base, int64_t* __restrict__ out_row_ptr, int64_t* __restrict__ out_counts) {
  const int64_t n_e = ht_entries(idx_row_ptr, n_users, n_events);
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u <= n_users; u += (int64_t)gridDim.x * 256)
    out_row_ptr[u] = ht_rank(i_base, i_bits, n_users > 0 ? ht_clamp(idx_row_ptr[u], n_e) : 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t n_words = (n_events + 63) >> 6;
    out_counts[0] = s_base[n_words];
    out_counts[1] = i_base[n_words];
  }
}

// a.s_bits, i_bits, s_cnt, i_cnt [ceil(n_events / 64)], s_base, i_base [that + 1], tile_sums: scratch.  out_* must not overlap the inputs.
hipError_t launch_history_trim(hipStream_t st, int n_cu, const TrimArgs& a) {
  const int64_t n = a.n_events, n_words = (n + 63) >> 6;
  hipError_t e;
  if (n > 0) {
    const bool has_drop = a.n_drop > 0 && a.n_users > 0;
    if (has_drop) {
      e = hipMemsetAsync(a.s_bits, 0, sizeof(unsigned long long) * (size_t)n_words, st);
      if (e != hipSuccess) return e;
      const int64_t jobs = a.n_drop * HT_SPLIT, cap = (int64_t)n_cu * 8;
      hipLaunchKernelGGL(ht_mark_kernel, dim3((unsigned)(jobs < cap ? jobs : cap)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.n_drop, a.drop_users,
                         a.s_bits);
    }
    hipLaunchKernelGGL(ht_keep_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.times_ms, a.min_time_ms, has_drop, a.s_bits, a.s_cnt);
    hipLaunchKernelGGL(ht_entries_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.s_bits, a.i_bits, a.i_cnt);
  }
  e = launch_scan_i32(st, a.s_cnt, n_words, a.s_base, a.tile_sums);
  if (e != hipSuccess) return e;
  e = launch_scan_i32(st, a.i_cnt, n_words, a.i_base, a.tile_sums);
  if (e != hipSuccess) return e;
  if (n > 0) {
    hipLaunchKernelGGL(ht_compact_stream_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.items, a.times_ms, a.s_bits, a.s_base, a.out_items, a.out_times);
    hipLaunchKernelGGL(ht_compact_index_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.s_bits, a.s_base, a.i_bits, a.i_base,
                       a.out_pos);
  }
  hipLaunchKernelGGL(ht_row_ptr_kernel, dim3(ig_grid(a.n_users + 1, n_cu)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.i_bits, a.s_base, a.i_base, a.out_row_ptr,
                     a.out_counts);
  return hipGetLastError();
}

// ---- cap (decision D27) --------------------------------------------------------------------------------------------
// The trim with one more rule: of every user only the max_per_user most recent events stay.  The cap marks what it drops into the bitmap D that
// ht_mark_kernel fills, before ht_keep_kernel turns D into S; everything behind the mark is the trim's sequence, unchanged.  The recency key is the
// rows' (time ^ sign, position): an entry is dropped when its key is not among the max_per_user largest of the user's valid entries (those naming a
// position inside the stream).  Three classes by the user's entries m = its clamped segment, chosen on the device:
//   m <= cap   nothing: a lane per user reads the two row starts and is done
//   <= 64      one wave, a user at a time by ballot rounds over the wave's 64 users: keys in registers, rank by cross-lane compares
//   larger     one block per user of `list` (cursor ctr[0], filled by the wave kernel): the threshold = the cap-th largest key by the select of
//              cco_select.h, keys in LDS up to SR_LDS entries, re-read from global memory per discriminating digit beyond; entries below it set their bit
// An entry that names no position has the key (0, 0) in the select and sets no bit: no valid key is smaller, so the threshold among all m keys is the
// threshold among the valid ones whenever more than cap of them exist, and (0, 0) -- nothing dropped -- otherwise.  No sort; atomicOr only for dropped
// entries, one atomicAdd on the cursor per user beyond a wave.  Row starts are clamped into 0 .. n_e as in the mark: no access leaves the arrays.
__global__ __launch_bounds__(256) void hc_mark_wave_kernel(int64_t n_events, int64_t n_users, const int64_t* __restrict__ idx_row_ptr, const int32_t* __restrict__ idx_pos,
                                                           const int64_t* __restrict__ times_ms, int32_t cap, unsigned long long* __restrict__ bits,
                                                           int32_t* __restrict__ list, unsigned long long* __restrict__ ctr) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_e = ht_entries(idx_row_ptr, n_users, n_events);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t u0 = ((int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE) * SR_WAVE; u0 < n_users; u0 += n_waves * SR_WAVE) {  // wave-uniform
    const int64_t u = u0 + lane;
    int64_t lo = 0, m = 0;
    if (u < n_users) {
      lo = ht_clamp(idx_row_ptr[u], n_e);
      m = ht_clamp(idx_row_ptr[u + 1], n_e) - lo;
    }
    if (m > SR_WAVE && m > cap) list[atomicAdd(ctr, 1ull)] = (int32_t)u;
    unsigned long long todo = __ballot(m > cap && m <= SR_WAVE);
    while (todo) {  // wave-uniform: one user of the wave class per round
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const int64_t seg = __shfl((long long)lo, src);
      const int n = (int)__shfl((long long)m, src);
      unsigned p = 0;
      unsigned long long tk = 0;
      bool valid = false;
      if (lane < n) {
        const int q = idx_pos[seg + lane];
        valid = q >= 0 && q < n_events;
        if (valid) {
          p = (unsigned)q;
          tk = times_ms ? (unsigned long long)times_ms[q] ^ HS_SIGN : 0ull;
        }
      }
      int rank = 0;  // valid entries of the user more recent than this lane's
      for (int o = 0; o < n; ++o) {
        const unsigned long long ot = __shfl(tk, o);
        const unsigned op = __shfl(p, o);
        const int ov = __shfl((int)valid, o);
        rank += (ov && (ot > tk || (ot == tk && op > p))) ? 1 : 0;
      }
      if (valid && rank >= cap) atomicOr(&bits[p >> 6], 1ull << (p & 63));
    }
  }
}

// The dropped entries of one user of m > max(cap, 64) entries, by the whole block behind the barrier that makes the LDS keys visible.  IN_LDS: the keys
// are s_time[i], s_pos[i] (the raw entry; s_time is 0 where it names no position); else they are read through ipos.  A template parameter for hs_window's reason.
template <bool IN_LDS>
__device__ __forceinline__ void hc_mark_user(int64_t n_events, unsigned n, unsigned cap, const int32_t* __restrict__ ipos, const int64_t* __restrict__ times,
                                             const unsigned long long* s_time, const unsigned* s_pos, SelScratch& s_select, unsigned long long* __restrict__ bits) {
  const unsigned n_ev = (unsigned)n_events;  // < 2^31: a negative entry is beyond it as an unsigned
  auto raw_p = [&](unsigned i) -> unsigned { return IN_LDS ? s_pos[i] : (unsigned)ipos[i]; };
  auto key_p = [&](unsigned i) -> unsigned {
    const unsigned p = raw_p(i);
    return p < n_ev ? p : 0u;
  };
  auto key_t = [&](unsigned i) -> unsigned long long {
    if (IN_LDS) return s_time[i];
    const unsigned p = (unsigned)ipos[i];
    return times && p < n_ev ? (unsigned long long)times[p] ^ HS_SIGN : 0ull;
  };
  SelKey common;
  const SelKey differ = sel_differ<256>(n, key_t, key_p, s_select, common);
  const SelKey thr = sel_kth_largest<256>(n, cap, key_t, key_p, differ, common, s_select);
  for (unsigned i = threadIdx.x; i < n; i += 256) {
    const unsigned p = raw_p(i);
    if (p >= n_ev) continue;
    const unsigned long long kt = key_t(i);
    if (kt < thr.hi || (kt == thr.hi && p < thr.lo)) atomicOr(&bits[p >> 6], 1ull << (p & 63));
  }
}

// One block per user of `list`.
__global__ __launch_bounds__(256) void hc_mark_block_kernel(int64_t n_events, int64_t n_users, const int64_t* __restrict__ idx_row_ptr, const int32_t* __restrict__ idx_pos,
                                                            const int64_t* __restrict__ times_ms, int32_t cap, unsigned long long* __restrict__ bits,
                                                            const int32_t* __restrict__ list, const unsigned long long* __restrict__ ctr) {
  __shared__ unsigned long long s_buf[SR_LDS + SR_LDS / 2];  // SR_LDS times (8 bytes), then SR_LDS raw entries
  __shared__ SelScratch s_select;
  unsigned long long* s_time = s_buf;
  unsigned* s_pos = reinterpret_cast<unsigned*>(s_buf + SR_LDS);
  const int64_t n_e = ht_entries(idx_row_ptr, n_users, n_events);
  int64_t n_big = (int64_t)ctr[0];
  if (n_big > n_users) n_big = n_users;
  for (int64_t li = blockIdx.x; li < n_big; li += gridDim.x) {  // block-uniform
    const int u = list[li];
    if (u < 0 || u >= n_users) continue;
    const int64_t lo = ht_clamp(idx_row_ptr[u], n_e);
    const int64_t m = ht_clamp(idx_row_ptr[u + 1], n_e) - lo;
    if (m <= cap) continue;
    const bool in_lds = m <= SR_LDS;
    const int32_t* __restrict__ ipos = idx_pos + lo;
    if (in_lds)
      for (int i = threadIdx.x; i < (int)m; i += 256) {
        const int q = ipos[i];
        s_pos[i] = (unsigned)q;
        s_time[i] = times_ms && q >= 0 && q < n_events ? (unsigned long long)times_ms[q] ^ HS_SIGN : 0ull;
      }
    __syncthreads();
    if (in_lds) hc_mark_user<true>(n_events, (unsigned)m, (unsigned)cap, ipos, times_ms, s_time, s_pos, s_select, bits);
    else hc_mark_user<false>(n_events, (unsigned)m, (unsigned)cap, ipos, times_ms, s_time, s_pos, s_select, bits);
    __syncthreads();  // the keys and the select's scratch are free for the next user
  }
}

// launch_history_trim with the cap's mark in front of the keep: c.list [n_users], c.ctr [1] and the trim's scratch.  max_per_user == INT32_MAX launches what the trim launches.
hipError_t launch_history_cap(hipStream_t st, int n_cu, const CapArgs& c) {
  const TrimArgs& a = c.trim;
  const int64_t n = a.n_events, n_words = (n + 63) >> 6;
  hipError_t e;
  if (n > 0) {
    const bool has_drop = a.n_drop > 0 && a.n_users > 0;
    const bool has_cap = c.max_per_user != 0x7fffffff && a.n_users > 0;
    if (has_drop || has_cap) {
      e = hipMemsetAsync(a.s_bits, 0, sizeof(unsigned long long) * (size_t)n_words, st);
      if (e != hipSuccess) return e;
    }
    if (has_drop) {
      const int64_t jobs = a.n_drop * HT_SPLIT, cap = (int64_t)n_cu * 8;
      hipLaunchKernelGGL(ht_mark_kernel, dim3((unsigned)(jobs < cap ? jobs : cap)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.n_drop, a.drop_users,
                         a.s_bits);
    }
    if (has_cap) {
      e = hipMemsetAsync(c.ctr, 0, sizeof(unsigned long long), st);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(hc_mark_wave_kernel, dim3(ig_grid(a.n_users, n_cu)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.times_ms, c.max_per_user,
                         a.s_bits, c.list, c.ctr);
      const int64_t heavy = n / SR_WAVE + 1;  // users of more than a wave's entries, at most
      const int64_t most = heavy < a.n_users ? heavy : a.n_users, grid = most < (int64_t)n_cu * 8 ? most : (int64_t)n_cu * 8;
      hipLaunchKernelGGL(hc_mark_block_kernel, dim3((unsigned)grid), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.times_ms, c.max_per_user, a.s_bits,
                         c.list, c.ctr);
    }
    hipLaunchKernelGGL(ht_keep_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.times_ms, a.min_time_ms, has_drop || has_cap, a.s_bits, a.s_cnt);
    hipLaunchKernelGGL(ht_entries_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.s_bits, a.i_bits, a.i_cnt);
  }
  e = launch_scan_i32(st, a.s_cnt, n_words, a.s_base, a.tile_sums);
  if (e != hipSuccess) return e;
  e = launch_scan_i32(st, a.i_cnt, n_words, a.i_base, a.tile_sums);
  if (e != hipSuccess) return e;
  if (n > 0) {
    hipLaunchKernelGGL(ht_compact_stream_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.items, a.times_ms, a.s_bits, a.s_base, a.out_items, a.out_times);
    hipLaunchKernelGGL(ht_compact_index_kernel, dim3(ig_grid(n, n_cu)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.idx_pos, a.s_bits, a.s_base, a.i_bits, a.i_base,
                       a.out_pos);
  }
  hipLaunchKernelGGL(ht_row_ptr_kernel, dim3(ig_grid(a.n_users + 1, n_cu)), dim3(256), 0, st, n, a.n_users, a.idx_row_ptr, a.i_bits, a.s_base, a.i_base, a.out_row_ptr,
                     a.out_counts);
  return hipGetLastError();
}

// ---- matrices (decision D23) ---------------------------------------------------------------------------------------
// The Preparator's output from the index and the item stream alone: which users train (users), and per event type the user x column matrix whose rows are
// the users' distinct in-window columns, ascending (matrix) -- the arrays launch_csr_from_pairs gives for the pairs (row_of[user], item), without a `users` array.
//   users   I[e] = "the position of index entry e is in the window" as in the trim (one wave per word of 64 entries: balanced by ENTRIES), popcount scan,
//           c[u] = rankI(end of u) - rankI(start of u), keep[u] = c[u] >= min_events, scan of keep = the row numbers
//   matrix  the raw row of user u is tmp[lo .. hi), lo / hi = u's clamped row starts: idx_row_ptr is the prefix of the raw lengths, no bounds pass.
//           Three classes by the raw entries m = hi - lo, chosen on the device:
//             <= 64     sr_wave_tail<true>: a lane per entry, entries outside the window or the columns are SR_SENT
//             <= 4096   sr_block_tail<true>: the gathered columns staged in LDS
//             larger    column bitmap: a block owns ceil(n_cols / 32) words of scratch, all zero between rows; one atomicOr per kept entry, then one walk
//                       over the words that takes each word with atomicExch(.., 0) -- reading it and leaving the bitmap zero for the block's next row in
//                       one access -- and writes its set bits as columns at the offsets a block scan of the popcounts gives, 256 words at a time.  No
//                       sort: the row is ascending and distinct by construction.  Every access to a bitmap is an atomic (performed at L2), so no line of
//                       it is ever held in a CU's L1.  HM_BITMAP_BUDGET bytes bound the bitmaps of a launch: min(HM_BITMAP_BLOCKS, budget / bitmap) blocks
//           then the scan of the lengths and the compaction of the raw rows' fronts into the caller's CSR
// A row is written iff hi <= capacity; row r's place in the result ends at or before its raw end, so nothing is written at or past out_col_idx[capacity].
// Whatever idx_row_ptr, idx_pos and row_of hold, no access leaves the arrays: entries outside the stream are dropped, row starts clamped into 0 .. n_e,
// row numbers outside 0 .. n_rows skipped, and the compaction checks both ends (segments that overlap, or two users of one row, can sum to more than n_e).
namespace {
constexpr long long HM_OPEN = 0x7fffffffffffffffll;  // t_hi == INT64_MAX: no upper end

__device__ __forceinline__ bool hm_in_window(const int64_t* __restrict__ times, int p, int64_t t_lo, int64_t t_hi) {
  if (!times) return true;
  const int64_t t = times[p];
  return t >= t_lo && (t_hi == HM_OPEN || t < t_hi);
}

// the column index entry `p` gives its user's row, SR_SENT when it gives none
__device__ __forceinline__ int hm_column(const MatrixArgs& a, int p) {
  if (p < 0 || p >= a.n_events) return SR_SENT;
  if (!hm_in_window(a.times_ms, p, a.t_lo, a.t_hi)) return SR_SENT;
  const int item = a.items[p];
  return item >= 0 && item < a.n_cols ? item : SR_SENT;
}

// user u's row number, -1: none; its raw row [lo, hi)
__device__ __forceinline__ int64_t hm_row(const MatrixArgs& a, int64_t u, int64_t n_e, int64_t& lo, int64_t& hi) {
  lo = ht_clamp(a.idx_row_ptr[u], n_e);
  hi = ht_clamp(a.idx_row_ptr[u + 1], n_e);
  const int64_t r = a.row_of ? a.row_of[u] : u;
  return r >= 0 && r < a.n_rows ? r : -1;
}
}  // namespace

__global__ __launch_bounds__(256) void hu_flags_kernel(UsersArgs a) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_e = ht_entries(a.idx_row_ptr, a.n_users, a.n_events);
  const int64_t n_words = (a.n_events + 63) >> 6, n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t w = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; w < n_words; w += n_waves) {  // wave-uniform
    const int64_t e = (w << 6) + lane;
    bool in = false;
    if (e < n_e) {
      const int p = a.idx_pos[e];
      if (p >= 0 && p < a.n_events) in = hm_in_window(a.times_ms, p, a.t_lo, a.t_hi);
    }
    const unsigned long long word = __ballot(in);
    if (lane == 0) {
      a.i_bits[w] = word;
      a.i_cnt[w] = __popcll(word);
    }
  }
}

__global__ __launch_bounds__(256) void hu_keep_kernel(UsersArgs a) {
  const int64_t n_e = ht_entries(a.idx_row_ptr, a.n_users, a.n_events);
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < a.n_users; u += (int64_t)gridDim.x * 256) {
    const int64_t c = ht_rank(a.i_base, a.i_bits, ht_clamp(a.idx_row_ptr[u + 1], n_e)) - ht_rank(a.i_base, a.i_bits, ht_clamp(a.idx_row_ptr[u], n_e));
    a.keep[u] = c >= a.min_events ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void hu_row_of_kernel(UsersArgs a) {
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < a.n_users; u += (int64_t)gridDim.x * 256)
    a.out_row_of[u] = a.keep[u] ? (int32_t)a.prefix[u] : -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.out_n_rows[0] = a.prefix[a.n_users];
}

hipError_t launch_history_users(hipStream_t st, int n_cu, const UsersArgs& a) {
  if (a.n_users == 0) return hipMemsetAsync(a.out_n_rows, 0, sizeof(int64_t), st);
  const int64_t n_words = (a.n_events + 63) >> 6;
  if (a.n_events > 0) hipLaunchKernelGGL(hu_flags_kernel, dim3(ig_grid(a.n_events, n_cu)), dim3(256), 0, st, a);
  hipError_t e = launch_scan_i32(st, a.i_cnt, n_words, a.i_base, a.tile_sums);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hu_keep_kernel, dim3(ig_grid(a.n_users, n_cu)), dim3(256), 0, st, a);
  e = launch_scan_i32(st, a.keep, a.n_users, a.prefix, a.tile_sums);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hu_row_of_kernel, dim3(ig_grid(a.n_users, n_cu)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// One wave per user of <= 64 raw entries; the others go on the list: up to SR_LDS entries from the front (ctr[0]), heavier ones from the back (ctr[1]).
__global__ __launch_bounds__(256) void hm_rows_wave_kernel(MatrixArgs a) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  const int64_t n_e = ht_entries(a.idx_row_ptr, a.n_users, a.n_events);
  for (int64_t u = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; u < a.n_users; u += n_waves) {  // wave-uniform
    int64_t lo, hi;
    const int64_t r = hm_row(a, u, n_e, lo, hi);
    const int64_t m = hi - lo;
    if (r < 0 || m <= 0 || hi > a.capacity) continue;  // no row, or one that stays empty: len[r] is 0
    if (m > SR_WAVE) {
      if (lane == 0) {
        if (m <= SR_LDS) a.list[atomicAdd(&a.ctr[0], 1ull)] = (int32_t)u;
        else a.list[a.n_users - 1 - (int64_t)atomicAdd(&a.ctr[1], 1ull)] = (int32_t)u;
      }
      continue;
    }
    const int v = lane < m ? hm_column(a, a.idx_pos[lo + lane]) : SR_SENT;
    const int len = sr_wave_tail<true>(v, lane, SR_WAVE, a.tmp + lo);
    if (lane == 0) {
      a.len[r] = len;
      a.raw_start[r] = (int32_t)lo;
    }
  }
}

// One block per listed user of 65 .. SR_LDS raw entries.
__global__ __launch_bounds__(256) void hm_rows_block_kernel(MatrixArgs a) {
  __shared__ int s_v[SR_LDS];
  const int64_t n_e = ht_entries(a.idx_row_ptr, a.n_users, a.n_events);
  const int64_t n_big = (int64_t)a.ctr[0];
  for (int64_t li = blockIdx.x; li < n_big; li += gridDim.x) {  // block-uniform
    const int64_t u = a.list[li];
    int64_t lo, hi;
    const int64_t r = hm_row(a, u, n_e, lo, hi);
    const int m = (int)(hi - lo);  // 65 .. SR_LDS: the wave kernel listed the user
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = threadIdx.x; i < P; i += 256) s_v[i] = i < m ? hm_column(a, a.idx_pos[lo + i]) : SR_SENT;
    __syncthreads();  // the staged row is complete
    const int len = sr_block_tail<true>(a.tmp + lo, m, s_v);
    if (threadIdx.x == 0) {
      a.len[r] = len;
      a.raw_start[r] = (int32_t)lo;
    }
    __syncthreads();
  }
}

// The listed users of more than SR_LDS raw entries, dealt to the grid's blocks; block b owns bitmap b, zero on entry and between its rows.
__global__ __launch_bounds__(256) void hm_rows_bitmap_kernel(MatrixArgs a) {
  __shared__ int s_wsum[256 / SR_WAVE];
  const int lane = threadIdx.x & (SR_WAVE - 1), wave = threadIdx.x / SR_WAVE;
  const int n_words = (int)(((int64_t)a.n_cols + 31) >> 5);
  unsigned* bm = a.bitmaps + (int64_t)blockIdx.x * n_words;
  const int64_t n_e = ht_entries(a.idx_row_ptr, a.n_users, a.n_events);
  const int64_t n_heavy = (int64_t)a.ctr[1];
  for (int64_t li = blockIdx.x; li < n_heavy; li += gridDim.x) {  // block-uniform
    const int64_t u = a.list[a.n_users - 1 - li];
    int64_t lo, hi;
    const int64_t r = hm_row(a, u, n_e, lo, hi);
    for (int64_t e = lo + threadIdx.x; e < hi; e += 256 * 4) {  // four independent gather chains per thread in flight
      int c[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = e + k * 256 < hi ? hm_column(a, a.idx_pos[e + k * 256]) : SR_SENT;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c[k] != SR_SENT) atomicOr(&bm[c[k] >> 5], 1u << (c[k] & 31));
    }
    __threadfence();  // this thread's bit sets are performed ...
    __syncthreads();  // ... and so are everybody's: the walk may take the words
    int32_t* __restrict__ row = a.tmp + lo;  // distinct columns <= kept entries <= hi - lo: the walk stays inside the raw row
    int carry = 0;
    for (int w0 = 0; w0 < n_words; w0 += 256) {  // block-uniform
      const int w = w0 + (int)threadIdx.x;
      unsigned word = w < n_words ? atomicExch(&bm[w], 0u) : 0u;
      const int c = __popc(word);
      int incl = c;
      for (int o = 1; o < SR_WAVE; o <<= 1) {  // inclusive wave scan of the popcounts
        const int below = __shfl_up(incl, o);
        if (lane >= o) incl += below;
      }
      if (lane == SR_WAVE - 1) s_wsum[wave] = incl;
      __syncthreads();
      int before = 0, tot = 0;
#pragma unroll
      for (int k = 0; k < 256 / SR_WAVE; ++k) {
        const int s = s_wsum[k];
        if (k < wave) before += s;
        tot += s;
      }
      int pos = carry + before + incl - c;
      while (word) {
        row[pos++] = (w << 5) + __ffsll((unsigned long long)word) - 1;
        word &= word - 1u;
      }
      carry += tot;
      __syncthreads();  // s_wsum is free; behind the last round: every word is zero again before the next row sets bits
    }
    if (threadIdx.x == 0) {
      a.len[r] = carry;
      a.raw_start[r] = (int32_t)lo;
    }
  }
}

// row r of the result = the front of its raw row; one wave per row.  Both ends are checked: see the section's head.
__global__ __launch_bounds__(256) void hm_compact_kernel(MatrixArgs a) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t r = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; r < a.n_rows; r += n_waves) {
    const int64_t s = a.raw_start[r], d = a.out_row_ptr[r];
    const int64_t L = a.out_row_ptr[r + 1] - d;
    for (int64_t t = lane; t < L; t += SR_WAVE)
      if (s + t < a.n_events && d + t < a.capacity) a.out_col_idx[d + t] = a.tmp[s + t];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.out_nnz[0] = a.out_row_ptr[a.n_rows];
}

int32_t history_bitmap_blocks(int32_t n_cols, int64_t budget_bytes) {
  const int64_t bytes = (((int64_t)n_cols + 31) >> 5) * (int64_t)sizeof(unsigned);
  const int64_t b = budget_bytes / (bytes > 0 ? bytes : 1);
  return (int32_t)(b < 1 ? 1 : b < HM_BITMAP_BLOCKS ? b : HM_BITMAP_BLOCKS);
}

hipError_t launch_history_matrix(hipStream_t st, int n_cu, const MatrixArgs& a) {
  hipError_t e;
  if (a.n_rows == 0) {
    e = hipMemsetAsync(a.out_row_ptr, 0, sizeof(int64_t), st);
    return e != hipSuccess ? e : hipMemsetAsync(a.out_nnz, 0, sizeof(int64_t), st);
  }
  e = hipMemsetAsync(a.len, 0, sizeof(int32_t) * (size_t)a.n_rows, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.raw_start, 0, sizeof(int32_t) * (size_t)a.n_rows, st);
  if (e != hipSuccess) return e;
  if (a.n_users > 0 && a.n_events > 0) {
    e = hipMemsetAsync(a.ctr, 0, sizeof(unsigned long long) * 2, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hm_rows_wave_kernel, dim3(ig_grid(a.n_users * SR_WAVE, n_cu)), dim3(256), 0, st, a);
    if (a.n_events > SR_WAVE) {
      const int64_t bgrid = a.n_users < (int64_t)n_cu * 8 ? a.n_users : (int64_t)n_cu * 8;
      hipLaunchKernelGGL(hm_rows_block_kernel, dim3((unsigned)bgrid), dim3(256), 0, st, a);
    }
    if (a.bm_blocks > 0) {
      e = hipMemsetAsync(a.bitmaps, 0, sizeof(unsigned) * (size_t)a.bm_blocks * (size_t)(((int64_t)a.n_cols + 31) >> 5), st);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(hm_rows_bitmap_kernel, dim3((unsigned)a.bm_blocks), dim3(256), 0, st, a);
    }
  }
  e = launch_scan_i32(st, a.len, a.n_rows, a.out_row_ptr, a.tile_sums);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hm_compact_kernel, dim3(ig_grid(a.n_rows * SR_WAVE, n_cu)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---- bounds --------------------------------------------------------------------------------------------------------
// bnd[t * n_queries + q] = min(n_u, max_items) of type t; bnd[n_types * n_queries + q] = blacklist events + the extra row's length
__global__ __launch_bounds__(256) void hs_bounds_kernel(HistArgs a, int32_t* __restrict__ bnd) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < a.n_queries; q += (int64_t)gridDim.x * 256) {
    int64_t excl = a.extra_row_ptr ? a.extra_row_ptr[q + 1] - a.extra_row_ptr[q] : 0;
    for (int t = 0; t < a.n_types; ++t) {
      int64_t seg;
      const int n = hs_user_events(a.ev[t], a.q_users, a.n_users, q, seg);
      bnd[(int64_t)t * a.n_queries + q] = n < a.ev[t].max_items ? n : a.ev[t].max_items;
      if (a.ev[t].blacklist) excl += n;
    }
    bnd[(int64_t)a.n_types * a.n_queries + q] = excl > 0x7fffffffll ? 0x7fffffff : (int32_t)excl;  // saturated: the rows kernels never write past a raw row
  }
}

hipError_t launch_history_bounds(hipStream_t st, int n_cu, const HistArgs& a, int32_t* bnd, int64_t* tile_sums, int64_t* const* term_row_ptr, int64_t* excl_row_ptr) {
  if (a.n_queries == 0) {
    for (int t = 0; t < a.n_types; ++t) {
      const hipError_t e = hipMemsetAsync(term_row_ptr[t], 0, sizeof(int64_t), st);
      if (e != hipSuccess) return e;
    }
    return hipMemsetAsync(excl_row_ptr, 0, sizeof(int64_t), st);
  }
  hipLaunchKernelGGL(hs_bounds_kernel, dim3(ig_grid(a.n_queries, n_cu)), dim3(256), 0, st, a, bnd);
  for (int t = 0; t <= a.n_types; ++t) {
    const hipError_t e = launch_scan_i32(st, bnd + (int64_t)t * a.n_queries, a.n_queries, t < a.n_types ? term_row_ptr[t] : excl_row_ptr, tile_sums);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

// ---- rows ----------------------------------------------------------------------------------------------------------
// job j = t * n_queries + q; t == n_types is the exclusion row of query q.  ctr[0] = jobs left to the block kernel (big_list),
// ctr[1 + HIST_STAT_*] = the statistics of include/urcco.h.
// One wave per job of <= 64 events (exclusion rows: <= 64 raw entries); the others go on big_list.
__global__ __launch_bounds__(256) void hs_rows_wave_kernel(HistArgs a) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  const int64_t n_jobs = a.n_queries * (a.n_types + 1);
  unsigned n_term = 0, n_excl = 0, n_sel = 0, n_over = 0;
  for (int64_t j = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; j < n_jobs; j += n_waves) {  // wave-uniform
    const int t = (int)(j / a.n_queries);
    const int64_t q = j - (int64_t)t * a.n_queries;
    if (t < a.n_types) {
      const HistEvent& e = a.ev[t];
      int64_t seg;
      const int n = hs_user_events(e, a.q_users, a.n_users, q, seg);
      if (e.raw.raw_ptr[q + 1] > e.raw.capacity) {  // the caller's buffers are smaller than the bounds: an empty row, counted
        if (lane == 0) e.raw.len[q] = 0;
        ++n_over;
        continue;
      }
      if (n > SR_WAVE) {
        if (lane == 0) a.big_list[atomicAdd(&a.ctr[0], 1ull)] = (int32_t)j;
        continue;
      }
      ++n_term;
      unsigned p = 0;
      unsigned long long tk = 0;
      int item = -1;
      if (lane < n) {
        p = (unsigned)e.idx_pos[seg + lane];
        tk = e.times_ms ? (unsigned long long)e.times_ms[p] ^ HS_SIGN : 0ull;
        item = e.items[p];
      }
      bool in = lane < n;
      if (n > e.max_items) {  // wave-uniform: rank = events of the user more recent than this lane's
        ++n_sel;
        int rank = 0;
        for (int o = 0; o < n; ++o) {
          const unsigned long long ot = __shfl(tk, o);
          const unsigned op = __shfl(p, o);
          rank += (ot > tk || (ot == tk && op > p)) ? 1 : 0;
        }
        in = in && rank < e.max_items;
      }
      const int len = sr_wave_tail<true>(in && item >= 0 && item < e.n_cols ? item : SR_SENT, lane, SR_WAVE, e.raw.tmp + e.raw.raw_ptr[q]);
      if (lane == 0) e.raw.len[q] = len;
    } else {
      const int64_t s = a.excl.raw_ptr[q];
      const int64_t L = a.excl.raw_ptr[q + 1] - s;
      if (a.excl.raw_ptr[q + 1] > a.excl.capacity) {
        if (lane == 0) a.excl.len[q] = 0;
        ++n_over;
        continue;
      }
      if (L > SR_WAVE) {
        if (lane == 0) a.big_list[atomicAdd(&a.ctr[0], 1ull)] = (int32_t)j;
        continue;
      }
      ++n_excl;
      int v = SR_SENT;
      int64_t base = 0;
      for (int t2 = 0; t2 < a.n_types; ++t2) {
        const HistEvent& e = a.ev[t2];
        if (!e.blacklist) continue;
        int64_t seg;
        const int n = hs_user_events(e, a.q_users, a.n_users, q, seg);
        if (lane >= base && lane < base + n) v = hs_excl_id(e, e.items[e.idx_pos[seg + lane - base]], a.n_items);
        base += n;
      }
      if (a.extra_row_ptr) {
        const int64_t xs = a.extra_row_ptr[q], xn = a.extra_row_ptr[q + 1] - xs;
        if (lane >= base && lane < base + xn) {
          const int x = a.extra_col_idx[xs + lane - base];
          v = x >= 0 && x < a.n_items ? x : SR_SENT;
        }
      }
      const int len = sr_wave_tail<true>(v, lane, SR_WAVE, a.excl.tmp + s);
      if (lane == 0) a.excl.len[q] = len;
    }
  }
  if (lane == 0) {
    if (n_term) atomicAdd(&a.ctr[1 + HIST_STAT_WAVE], (unsigned long long)n_term);
    if (n_sel) atomicAdd(&a.ctr[1 + HIST_STAT_SELECT], (unsigned long long)n_sel);
    if (n_excl) atomicAdd(&a.ctr[1 + HIST_STAT_EXCL_WAVE], (unsigned long long)n_excl);
    if (n_over) atomicAdd(&a.ctr[1 + HIST_STAT_OVERFLOW], (unsigned long long)n_over);
  }
}

// The window of one (query, type) of n events -> its raw row, slots by the LDS counter *s_cnt (the sort that follows makes the order irrelevant).  Called by
// the whole block behind the barrier that makes the LDS keys visible.  IN_LDS: the keys are s_time[i], s_pos[i]; else they are read through ipos from
// global memory.  A template parameter and not a branch inside the accessors: the compiler merges the two loads of such a branch into one load through
// a pointer chosen at run time, a flat load (cco_sorted_rows.h, sr_unique).
template <bool IN_LDS>
__device__ __forceinline__ void hs_window(const HistEvent& e, int n, const int32_t* __restrict__ ipos, const unsigned long long* s_time, const unsigned* s_pos,
                                          SelScratch& s_select, int* s_cnt, int32_t* __restrict__ row, int room) {
  const int64_t* __restrict__ times = e.times_ms;
  auto key_p = [&](unsigned i) -> unsigned { return IN_LDS ? s_pos[i] : (unsigned)ipos[i]; };
  auto key_t = [&](unsigned i) -> unsigned long long {
    if (IN_LDS) return s_time[i];
    return times ? (unsigned long long)times[(unsigned)ipos[i]] ^ HS_SIGN : 0ull;
  };
  const int K = e.max_items;
  const bool all = n <= K;  // block-uniform: no select
  SelKey thr{0ull, 0u};
  if (!all) {  // the K-th largest key; digits in which all keys of the user agree take no pass
    SelKey common;
    const SelKey differ = sel_differ<256>((unsigned)n, key_t, key_p, s_select, common);
    thr = sel_kth_largest<256>((unsigned)n, (unsigned)K, key_t, key_p, differ, common, s_select);
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    const unsigned long long kt = key_t((unsigned)i);
    const unsigned kp = key_p((unsigned)i);
    if (all || kt > thr.hi || (kt == thr.hi && kp >= thr.lo)) {
      const int item = e.items[kp];
      if (item >= 0 && item < e.n_cols) {
        const int slot = atomicAdd(s_cnt, 1);
        if (slot < room) row[slot] = item;
      }
    }
  }
}

// One block per job of big_list.
__global__ __launch_bounds__(256) void hs_rows_block_kernel(HistArgs a) {
  // keys of the LDS class: SR_LDS times (8 bytes), then SR_LDS positions; once the window is staged in its raw row the front is the sort buffer
  __shared__ unsigned long long s_buf[SR_LDS + SR_LDS / 2];
  __shared__ SelScratch s_select;
  __shared__ int s_cnt;
  unsigned long long* s_time = s_buf;
  unsigned* s_pos = reinterpret_cast<unsigned*>(s_buf + SR_LDS);
  int* s_v = reinterpret_cast<int*>(s_buf);
  const int64_t n_big = (int64_t)a.ctr[0];
  for (int64_t li = blockIdx.x; li < n_big; li += gridDim.x) {  // block-uniform
    const int64_t j = a.big_list[li];
    const int t = (int)(j / a.n_queries);
    const int64_t q = j - (int64_t)t * a.n_queries;
    if (threadIdx.x == 0) s_cnt = 0;
    int32_t* row;
    int room;
    if (t < a.n_types) {
      const HistEvent& e = a.ev[t];
      int64_t seg;
      const int n = hs_user_events(e, a.q_users, a.n_users, q, seg);
      row = e.raw.tmp + e.raw.raw_ptr[q];
      room = (int)(e.raw.raw_ptr[q + 1] - e.raw.raw_ptr[q]);
      const bool in_lds = n <= SR_LDS;
      const int32_t* __restrict__ ipos = e.idx_pos + seg;
      const int64_t* __restrict__ times = e.times_ms;
      if (in_lds)
        for (int i = threadIdx.x; i < n; i += 256) {
          const unsigned p = (unsigned)ipos[i];
          s_pos[i] = p;
          s_time[i] = times ? (unsigned long long)times[p] ^ HS_SIGN : 0ull;
        }
      __syncthreads();
      if (threadIdx.x == 0) {
        atomicAdd(&a.ctr[1 + (in_lds ? HIST_STAT_BLOCK : HIST_STAT_GLOBAL)], 1ull);
        if (n > e.max_items) atomicAdd(&a.ctr[1 + HIST_STAT_SELECT], 1ull);
      }
      if (in_lds) hs_window<true>(e, n, ipos, s_time, s_pos, s_select, &s_cnt, row, room);
      else hs_window<false>(e, n, ipos, s_time, s_pos, s_select, &s_cnt, row, room);
    } else {
      row = a.excl.tmp + a.excl.raw_ptr[q];
      const int64_t room64 = a.excl.raw_ptr[q + 1] - a.excl.raw_ptr[q];
      room = room64 > 0x7fffffffll ? 0x7fffffff : (int)room64;
      if (threadIdx.x == 0) atomicAdd(&a.ctr[1 + HIST_STAT_EXCL_BLOCK], 1ull);
      __syncthreads();
      for (int t2 = 0; t2 < a.n_types; ++t2) {
        const HistEvent& e = a.ev[t2];
        if (!e.blacklist) continue;
        int64_t seg;
        const int n = hs_user_events(e, a.q_users, a.n_users, q, seg);
        for (int i = threadIdx.x; i < n; i += 256) {
          const int v = hs_excl_id(e, e.items[e.idx_pos[seg + i]], a.n_items);
          if (v != SR_SENT) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < room) row[slot] = v;
          }
        }
      }
      if (a.extra_row_ptr) {
        const int64_t xs = a.extra_row_ptr[q], xn = a.extra_row_ptr[q + 1] - xs;
        for (int64_t i = threadIdx.x; i < xn; i += 256) {
          const int x = a.extra_col_idx[xs + i];
          if (x >= 0 && x < a.n_items) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < room) row[slot] = x;
          }
        }
      }
    }
    __syncthreads();  // the raw row is complete (its writers are this block's threads), the keys in LDS are dead
    const int m = s_cnt < room ? s_cnt : room;
    const int len = sr_block_tail(row, m, s_v);
    if (threadIdx.x == 0) {
      if (t < a.n_types) a.ev[t].raw.len[q] = len;
      else a.excl.len[q] = len;
    }
    __syncthreads();
  }
}

// a.ev[t].raw, a.excl, a.big_list, a.ctr: scratch.  term_row_ptr[t] / excl_row_ptr hold the bounds' scans on entry, the final row starts on return.
hipError_t launch_history_rows(hipStream_t st, int n_cu, const HistArgs& a, int64_t* tile_sums, int64_t* const* term_row_ptr, int32_t* const* term_col_idx,
                               int64_t* excl_row_ptr, int32_t* excl_col_idx, int64_t* stats_dev) {
  hipError_t e = hipMemsetAsync(a.ctr, 0, sizeof(unsigned long long) * (1 + HIST_STATS_LEN), st);
  if (e != hipSuccess) return e;
  const int64_t nq = a.n_queries;
  const int n_out = a.n_types + 1;
  RowsOut out[REC_MAX_CLAUSES + 1];
  for (int t = 0; t < a.n_types; ++t) out[t] = RowsOut{a.ev[t].raw, term_row_ptr[t], term_col_idx[t]};
  out[a.n_types] = RowsOut{a.excl, excl_row_ptr, excl_col_idx};
  e = sr_seed_raw_ptr(st, out, n_out, nq);
  if (e != hipSuccess) return e;
  if (nq > 0) {
    const int64_t n_jobs = nq * n_out;
    hipLaunchKernelGGL(hs_rows_wave_kernel, dim3(ig_grid(n_jobs * SR_WAVE, n_cu)), dim3(256), 0, st, a);
    const int64_t bgrid = n_jobs < (int64_t)n_cu * 8 ? n_jobs : (int64_t)n_cu * 8;
    hipLaunchKernelGGL(hs_rows_block_kernel, dim3((unsigned)bgrid), dim3(256), 0, st, a);
    e = sr_finish_rows(st, n_cu, out, n_out, nq, tile_sums);
    if (e != hipSuccess) return e;
  }
  if (stats_dev) {
    e = hipMemcpyAsync(stats_dev, a.ctr + 1, sizeof(int64_t) * HIST_STATS_LEN, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

}  // namespace urcco
