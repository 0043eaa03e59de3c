// cco_audience.h -- the audience of an item (urcco_dev_audience): for every query item i the best num users in the order (score desc, user id asc),
//   score(u, i) = sum over the clauses c, in call order, of boost_c * |T_c(u) ^ I_c(i)|   (weighted: the sum of the clamped weights of the shared terms, 2^-15)
// over the users with a positive score whose exclusion row does not hold i (decision D33).  Included once, from cco_misc.hip, behind
// cco_explain.h.  The recommend kernels answer the transposed question -- a query per user, the catalogue as candidates -- and keep num items per user;
// here the users stream past once and a tile of query items stays resident.
//
//   aud_plan_kernel   one block: the pair count of every query item (the summed lengths of its rows of I_c), their exclusive scan, then wave 0 cuts the
//                     items greedily into tiles of at most AUD_TILE items and `limit` pairs -- a tile a step: lane l asks whether l + 1 more items fit, one
//                     ballot.  An item index outside the catalogue and an item whose own rows exceed the limit are reported in the header, which the host reads.
//   aud_scan_kernel   a block of 256 threads per (tile, slab of users), grid-stride over the flattened list.
//     table           the tile's rows, all clauses, are hashed into an open-addressing LDS table keyed (clause, term): 64-bit key, 64-bit value = the set of
//                     tile items holding the term (atomicCAS on the key, atomicOr on the set).  4096 slots x 16 B = 64 KiB: two blocks share a CU's 160 KiB.
//     a user          one wave, one user at a time.  Per clause the lanes take the user's terms 64 a round; each lane probes the table and gets an item
//                     set.  An OR over the wave gives the items that matched at all; for each of those bits alone, a ballot of the bit over the lanes
//                     gives the match count by popcount (weighted: the weights of the balloted lanes are summed, one shuffle a match).  Lane j owns
//                     item j: it keeps the clause's integer counter and folds it into its f64 score with the expression of rec_rows_kernel.  The cost
//                     is by matches, not by 64 x terms.  After the last clause lane j with a positive score searches the user's exclusion row
//                     (ascending, distinct: cco_history.h, hist_excl_*) for its item and appends (score, user) to the block's list of item j.
//     lists           AUD_TILE lists of `cap` = num + 2 * AUD_ROUND entries per block in arena scratch, their lengths in LDS.  A round of at most AUD_ROUND
//                     users appends at most one entry per user and item, so a list that holds at most cap - AUD_ROUND entries at a round's start cannot
//                     overflow in it.  At the round's end (a block barrier) a longer list is cut to its best num by sel_kth_largest over the 96-bit key
//                     (score bits, ~user id) -- through the spare list, then back -- and the threshold stays in LDS: later entries below it are
//                     dropped before they are appended.  At the slab's end every list is cut to num and written to the slab's partial area.
//                     No block waits for another one: no spin, no lock, no flag.
//   aud_merge_kernel  a block per query item: the partials of all slabs and the running result of the earlier chunks, as one more partial, form one strided
//                     list (a slot behind a part's count is keyed (0, 0), below every live key); one select, the winners go to LDS, are ranked by
//                     counting and replace the running result.  The keys are distinct (distinct user ids: the caller's duty), and the top num of a union
//                     is the top num of its parts' top num: the result does not depend on slabs, grid or chunking, bit for bit.
//   Integer match counts, no float atomics, every fold in clause order: reproducible bit for bit.
#pragma once

namespace urcco {

constexpr int AUD_THREADS = 256;
constexpr int AUD_NW = AUD_THREADS / WAVE;
constexpr unsigned long long AUD_EMPTY = ~0ull;  // no (clause, term) pair: clause < 16
static_assert(AUD_TILE == WAVE, "a lane per tile item, the item sets are 64-bit words");
static_assert(AUD_ROUND == AUD_THREADS && AUD_ROUND == AUD_NW * WAVE, "a wave scans 64 users of a round");
static_assert((AUD_SLOTS & (AUD_SLOTS - 1)) == 0 && AUD_TERMS * 4 <= AUD_SLOTS * 3, "power-of-two table, load factor <= 3/4");
static_assert(sizeof(AudArgs) <= 4096, "kernel arguments: the clause table travels by value");

__device__ __forceinline__ unsigned aud_hash(unsigned long long key) {
  unsigned x = (unsigned)key * 2654435761u + (unsigned)(key >> 32) * 0x85ebca6bu;
  return (x ^ (x >> 15)) & (unsigned)(AUD_SLOTS - 1);
}

// tile item j holds `key`; false: no free slot (cannot happen under the plan's limit; counted)
__device__ __forceinline__ bool aud_insert(unsigned long long* s_key, unsigned long long* s_val, unsigned long long key, int j) {
  unsigned h = aud_hash(key);
  for (int probe = 0; probe < AUD_SLOTS; ++probe) {
    const unsigned long long k = atomicCAS(&s_key[h], AUD_EMPTY, key);
    if (k == AUD_EMPTY || k == key) {
      atomicOr(&s_val[h], 1ull << j);
      return true;
    }
    h = (h + 1u) & (unsigned)(AUD_SLOTS - 1);
  }
  return false;
}

// the tile items that hold `key`; the table is never full, so an absent key ends at an empty slot
__device__ __forceinline__ unsigned long long aud_probe(const unsigned long long* s_key, const unsigned long long* s_val, unsigned long long key) {
  unsigned h = aud_hash(key);
  for (int probe = 0; probe < AUD_SLOTS; ++probe) {
    const unsigned long long k = s_key[h];
    if (k == key) return s_val[h];
    if (k == AUD_EMPTY) return 0ull;
    h = (h + 1u) & (unsigned)(AUD_SLOTS - 1);
  }
  return 0ull;
}

// ---- the plan: pair counts, their scan, the greedy cut ----
__global__ __launch_bounds__(AUD_THREADS) void aud_plan_kernel(AudArgs a) {
  __shared__ long long s_wave[AUD_NW];
  __shared__ int s_bad_index, s_bad_rows;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  if (tid == 0) { s_bad_index = 0x7fffffff; s_bad_rows = 0x7fffffff; }
  if (tid < AUD_STATS_LEN) a.stats[tid] = 0ull;
  __syncthreads();
  long long carry = 0;
  for (int base = 0; base < a.n_query; base += AUD_THREADS) {  // block-uniform
    const int i = base + tid;
    long long len = 0;
    if (i < a.n_query) {
      const int32_t item = a.items[i];
      if ((unsigned)item >= (unsigned)a.n_items) {
        atomicMin(&s_bad_index, i);
      } else {
        for (int c = 0; c < a.n_clauses; ++c) {
          const long long d = a.c[c].m_row_ptr[item + 1] - a.c[c].m_row_ptr[item];
          len += d > 0 ? d : 0;
        }
        if (len > (long long)a.limit) atomicMin(&s_bad_rows, i);
      }
    }
    long long tot;
    const long long ex = block_exclusive_scan<AUD_THREADS>(len, s_wave, &tot);
    if (i < a.n_query) a.prefix[i] = carry + ex;
    carry += tot;
  }
  if (tid == 0) a.prefix[a.n_query] = carry;
  __syncthreads();
  if (tid < WAVE) {  // wave 0: a tile a step (an item beyond the limit gets a tile of its own; the call fails on the header)
    int s = 0, t = 0;
    while (s < a.n_query) {  // wave-uniform
      if (lane == 0) a.tile_start[t] = s;
      const int e = s + lane + 1;
      const bool fits = e <= a.n_query && a.prefix[e] - a.prefix[s] <= (long long)a.limit;
      const unsigned long long b = __ballot(fits ? 1 : 0);
      int run = b == ~0ull ? WAVE : __ffsll(~b) - 1;  // the lengths are >= 0: the lanes that fit are a prefix
      s += run < 1 ? 1 : run;
      ++t;
    }
    if (lane == 0) {
      a.tile_start[t] = a.n_query;
      a.hdr[AUD_HDR_TILES] = t;
      a.hdr[AUD_HDR_BAD_INDEX] = s_bad_index;
      a.hdr[AUD_HDR_BAD_ROWS] = s_bad_rows;
      a.stats[AUD_STAT_TILES] = (unsigned long long)t;
      a.stats[AUD_STAT_SLABS] = (unsigned long long)a.n_slabs;
    }
  }
}

// Cut list j of the block to its best `keep` entries (n > keep of them, block-uniform): select the keep-th largest key, move the entries at or above it
// to the spare list and back.  All threads; on return the list, s_len[j] and the threshold of item j are visible to the block.
__device__ __forceinline__ void aud_cut(double* l_score, int32_t* l_user, int cap, int j, unsigned n, unsigned keep, unsigned* s_len, unsigned long long* s_thi,
                                        unsigned* s_tlo, unsigned* s_cnt, SelScratch& s_select) {
  const int tid = threadIdx.x;
  const double* sc = l_score + (size_t)j * cap;
  const int32_t* us = l_user + (size_t)j * cap;
  double* sp_sc = l_score + (size_t)AUD_TILE * cap;
  int32_t* sp_us = l_user + (size_t)AUD_TILE * cap;
  if (tid == 0) *s_cnt = 0u;  // (the select's first pass has barriers: differ is all ones)
  const SelKey thr = sel_kth_largest<AUD_THREADS>(
      n, keep, [&](unsigned e) { return (unsigned long long)__double_as_longlong(sc[e]); }, [&](unsigned e) { return ~(unsigned)us[e]; }, SelKey{~0ull, ~0u},
      SelKey{0ull, 0u}, s_select);
  for (unsigned e = tid; e < n; e += AUD_THREADS) {
    const unsigned long long hi = (unsigned long long)__double_as_longlong(sc[e]);
    const unsigned lo = ~(unsigned)us[e];
    if (hi < thr.hi || (hi == thr.hi && lo < thr.lo)) continue;
    const unsigned at = atomicAdd(s_cnt, 1u);
    if (at < keep) {  // (always, when the keys are distinct)
      sp_sc[at] = sc[e];
      sp_us[at] = us[e];
    }
  }
  __syncthreads();
  const unsigned m = *s_cnt < keep ? *s_cnt : keep;
  for (unsigned e = tid; e < m; e += AUD_THREADS) {
    l_score[(size_t)j * cap + e] = sp_sc[e];
    l_user[(size_t)j * cap + e] = sp_us[e];
  }
  __syncthreads();
  if (tid == 0) {
    s_len[j] = m;
    s_thi[j] = thr.hi;
    s_tlo[j] = thr.lo;
  }
  __syncthreads();
}

// One user, one wave: the scores of the tile's items, lane j item j; the eligible ones are appended to the block's lists.
template <bool WEIGHTED>
__device__ __forceinline__ void aud_user(const AudArgs& a, int64_t q, int nt, const unsigned long long* s_key, const unsigned long long* s_val, const double* s_boost,
                                         const int32_t* s_item, const unsigned long long* s_thi, const unsigned* s_tlo, unsigned* s_len, double* l_score,
                                         int32_t* l_user, int lane, unsigned* n_kept, unsigned* n_over) {
  const int32_t uid = a.user_ids ? a.user_ids[q] : (int32_t)q;
  if (uid < 0) return;  // wave-uniform: nobody
  double score = 0.0;
  for (int c = 0; c < a.n_clauses; ++c) {
    const ExplClause& cl = a.c[c];
    const int64_t te = cl.q_row_ptr[q + 1];
    unsigned long long m = 0ull;  // lane j: the clause's counter of item j (unweighted: a match count)
    for (int64_t p0 = cl.q_row_ptr[q]; p0 < te; p0 += WAVE) {  // wave-uniform
      const int64_t p = p0 + lane;
      unsigned long long mask = 0ull;
      int32_t term = -1;
      if (p < te) {
        term = cl.q_col_idx[p];
        if ((unsigned)term < (unsigned)cl.n_cols) mask = aud_probe(s_key, s_val, ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(unsigned)term);
      }
      const unsigned long long hit = __ballot(mask != 0ull ? 1 : 0);
      if (!hit) continue;
      unsigned wt = (unsigned)REC_WEIGHT_ONE;
      if (WEIGHTED && mask != 0ull && cl.weight) {  // one load per matching term; clamped exactly as rec_rows_kernel clamps it
        wt = cl.weight[term];
        wt = wt < 1u ? 1u : wt > (unsigned)REC_WEIGHT_MAX ? (unsigned)REC_WEIGHT_MAX : wt;
      }
      unsigned long long items = mask;  // the items that matched at all
      for (int o = WAVE / 2; o > 0; o >>= 1) items |= shfl_xor_u64(items, o);
      while (items) {  // wave-uniform: the set bits only
        const int j = __ffsll(items) - 1;
        items &= items - 1ull;
        unsigned long long b = __ballot((int)((mask >> j) & 1ull));
        if (WEIGHTED) {
          unsigned long long sum = 0ull;
          while (b) {  // wave-uniform
            const int src = __ffsll(b) - 1;
            b &= b - 1ull;
            sum += (unsigned long long)(unsigned)__shfl((int)wt, src);
          }
          if (lane == j) m += sum;
        } else {
          if (lane == j) m += (unsigned long long)__popcll(b);
        }
      }
    }
    if (m) score = score + s_boost[c] * (WEIGHTED ? (double)m * REC_WEIGHT_UNIT : (double)m);  // (the translation unit is compiled with -ffp-contract=off)
  }
  if (lane < nt && score > 0.0) {
    const int32_t item = s_item[lane];
    bool excluded = false;
    if (a.excl_row_ptr) {  // first entry >= item of the ascending row
      int64_t lo = a.excl_row_ptr[q], hi = a.excl_row_ptr[q + 1];
      const int64_t end = hi;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.excl_col_idx[mid] < item) lo = mid + 1; else hi = mid;
      }
      excluded = lo < end && a.excl_col_idx[lo] == item;
    }
    const unsigned long long kh = (unsigned long long)__double_as_longlong(score);  // positive doubles order as their bits do
    const unsigned kl = ~(unsigned)uid;
    if (!excluded && (kh > s_thi[lane] || (kh == s_thi[lane] && kl >= s_tlo[lane]))) {
      const unsigned at = atomicAdd(&s_len[lane], 1u);
      if (at < (unsigned)a.cap) {
        l_score[(size_t)lane * a.cap + at] = score;
        l_user[(size_t)lane * a.cap + at] = uid;
        ++*n_kept;
      } else {
        ++*n_over;
      }
    }
  }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(AUD_THREADS) void aud_scan_kernel(AudArgs a) {
  __shared__ unsigned long long s_key[AUD_SLOTS];
  __shared__ unsigned long long s_val[AUD_SLOTS];
  __shared__ unsigned long long s_thi[AUD_TILE];
  __shared__ unsigned s_tlo[AUD_TILE];
  __shared__ unsigned s_len[AUD_TILE];
  __shared__ int32_t s_item[AUD_TILE];
  __shared__ double s_boost[REC_MAX_CLAUSES];
  __shared__ SelScratch s_select;
  __shared__ unsigned s_cnt;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int cap = a.cap, num = a.num;
  double* l_score = a.list_score + (size_t)blockIdx.x * (size_t)(AUD_TILE + 1) * (size_t)cap;
  int32_t* l_user = a.list_user + (size_t)blockIdx.x * (size_t)(AUD_TILE + 1) * (size_t)cap;
  unsigned n_kept = 0u, n_over = 0u, n_compact = 0u;
  if (tid < a.n_clauses) s_boost[tid] = a.c[tid].boost;
  const int64_t n_work = (int64_t)a.n_tiles * a.n_slabs;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {  // block-uniform
    const int tile = (int)(w / a.n_slabs), slab = (int)(w - (int64_t)tile * a.n_slabs);
    const int t0 = a.tile_start[tile], nt = a.tile_start[tile + 1] - t0;  // 1 .. AUD_TILE
    __syncthreads();  // the block has left the previous table and lists
    for (int h = tid; h < AUD_SLOTS; h += AUD_THREADS) { s_key[h] = AUD_EMPTY; s_val[h] = 0ull; }
    if (tid < AUD_TILE) {
      s_len[tid] = 0u; s_thi[tid] = 0ull; s_tlo[tid] = 0u;
      s_item[tid] = tid < nt ? a.items[t0 + tid] : -1;
    }
    __syncthreads();
    for (int pair = wave; pair < nt * a.n_clauses; pair += AUD_NW) {  // a wave per (tile item, clause) row
      const int j = pair / a.n_clauses, c = pair - j * a.n_clauses;
      const ExplClause& cl = a.c[c];
      const int64_t re = cl.m_row_ptr[s_item[j] + 1];
      for (int64_t p = cl.m_row_ptr[s_item[j]] + lane; p < re; p += WAVE) {
        const int32_t col = cl.m_col_idx[p];
        if ((unsigned)col >= (unsigned)cl.n_cols) continue;  // never matches
        if (!aud_insert(s_key, s_val, ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(unsigned)col, j)) ++n_over;
      }
    }
    __syncthreads();
    const int64_t u_lo = (int64_t)slab * a.slab_users;
    const int64_t u_hi = u_lo + a.slab_users < a.n_users ? u_lo + a.slab_users : a.n_users;
    for (int64_t r0 = u_lo; r0 < u_hi; r0 += AUD_ROUND) {  // block-uniform
      const int64_t q0 = r0 + (int64_t)wave * WAVE;
      const int64_t q1 = q0 + WAVE < u_hi ? q0 + WAVE : u_hi;
      for (int64_t q = q0; q < q1; ++q)  // wave-uniform
        aud_user<WEIGHTED>(a, q, nt, s_key, s_val, s_boost, s_item, s_thi, s_tlo, s_len, l_score, l_user, lane, &n_kept, &n_over);
      __syncthreads();
      for (int j = 0; j < nt; ++j) {
        const unsigned n = s_len[j] < (unsigned)cap ? s_len[j] : (unsigned)cap;  // block-uniform
        if (n <= (unsigned)(cap - AUD_ROUND)) continue;                          // the next round fits (cap - AUD_ROUND >= num)
        aud_cut(l_score, l_user, cap, j, n, (unsigned)num, s_len, s_thi, s_tlo, &s_cnt, s_select);
        if (tid == 0) ++n_compact;
      }
      __syncthreads();
    }
    for (int j = 0; j < nt; ++j) {  // the slab's partial result: the best num of every list
      unsigned n = s_len[j] < (unsigned)cap ? s_len[j] : (unsigned)cap;
      if (n > (unsigned)num) {
        aud_cut(l_score, l_user, cap, j, n, (unsigned)num, s_len, s_thi, s_tlo, &s_cnt, s_select);
        n = s_len[j];
      }
      const size_t part = (size_t)slab * (size_t)a.n_query + (size_t)(t0 + j);
      for (unsigned e = tid; e < n; e += AUD_THREADS) {
        a.part_score[part * (size_t)num + e] = l_score[(size_t)j * cap + e];
        a.part_user[part * (size_t)num + e] = l_user[(size_t)j * cap + e];
      }
      if (tid == 0) a.part_count[part] = (int32_t)n;
    }
  }
  if (n_kept) atomicAdd(&a.stats[AUD_STAT_KEPT], (unsigned long long)n_kept);
  if (n_over) atomicAdd(&a.stats[AUD_STAT_OVERFLOW], (unsigned long long)n_over);
  if (n_compact) atomicAdd(&a.stats[AUD_STAT_COMPACTIONS], (unsigned long long)n_compact);
}

// ---- the merge: a block per query item over the slabs' partials and the running result ----
__global__ __launch_bounds__(AUD_THREADS) void aud_merge_kernel(AudArgs a) {
  __shared__ SelScratch s_select;
  __shared__ double s_wscore[AUDIENCE_MAX_NUM];
  __shared__ int32_t s_wuser[AUDIENCE_MAX_NUM];
  __shared__ int s_pc[AUD_MAX_SLABS + 1];  // entries of every part; the last part is the running result
  __shared__ unsigned s_live, s_nwin;
  const int tid = threadIdx.x;
  const int i = blockIdx.x, num = a.num, n_parts = a.n_slabs + 1;
  const unsigned n_all = (unsigned)n_parts * (unsigned)num;  // <= 1025 * 1024
  if (tid == 0) { s_live = 0u; s_nwin = 0u; }
  __syncthreads();
  for (int s = tid; s < n_parts; s += AUD_THREADS) {
    int n = s < a.n_slabs ? a.part_count[(size_t)s * a.n_query + i] : a.io_count[i];
    n = n < 0 ? 0 : n > num ? num : n;
    s_pc[s] = n;
    if (n) atomicAdd(&s_live, (unsigned)n);
  }
  __syncthreads();
  // slot e of the strided list: part e / num, entry e % num
  auto live = [&](unsigned e) -> bool { const unsigned s = e / (unsigned)num; return (int)(e - s * (unsigned)num) < s_pc[s]; };
  auto score_at = [&](unsigned e) -> double {
    const unsigned s = e / (unsigned)num, r = e - s * (unsigned)num;
    return (int)s < a.n_slabs ? a.part_score[((size_t)s * a.n_query + i) * (size_t)num + r] : a.io_score[(size_t)i * num + r];
  };
  auto user_at = [&](unsigned e) -> int32_t {
    const unsigned s = e / (unsigned)num, r = e - s * (unsigned)num;
    return (int)s < a.n_slabs ? a.part_user[((size_t)s * a.n_query + i) * (size_t)num + r] : a.io_user[(size_t)i * num + r];
  };
  SelKey thr{0ull, 0u};
  if (s_live > (unsigned)num)  // a slot behind its part's count is keyed (0, 0): below every live key (score > 0)
    thr = sel_kth_largest<AUD_THREADS>(
        n_all, (unsigned)num, [&](unsigned e) { return live(e) ? (unsigned long long)__double_as_longlong(score_at(e)) : 0ull; },
        [&](unsigned e) { return live(e) ? ~(unsigned)user_at(e) : 0u; }, SelKey{~0ull, ~0u}, SelKey{0ull, 0u}, s_select);
  for (unsigned e = tid; e < n_all; e += AUD_THREADS) {
    if (!live(e)) continue;
    const double sc = score_at(e);
    const int32_t u = user_at(e);
    const unsigned long long hi = (unsigned long long)__double_as_longlong(sc);
    if (hi < thr.hi || (hi == thr.hi && ~(unsigned)u < thr.lo)) continue;
    const unsigned at = atomicAdd(&s_nwin, 1u);
    if (at < (unsigned)num) {  // (always, when the keys are distinct)
      s_wscore[at] = sc;
      s_wuser[at] = u;
    }
  }
  __syncthreads();  // every read of the running result lies before its first write
  const unsigned n_win = s_nwin < (unsigned)num ? s_nwin : (unsigned)num;
  for (unsigned e = tid; e < n_win; e += AUD_THREADS) {  // ranked by counting: (score desc, user id asc)
    const unsigned long long hi = (unsigned long long)__double_as_longlong(s_wscore[e]);
    const unsigned u = (unsigned)s_wuser[e];
    unsigned r = 0u;
    for (unsigned f = 0; f < n_win; ++f) {
      const unsigned long long fh = (unsigned long long)__double_as_longlong(s_wscore[f]);
      r += (fh > hi || (fh == hi && (unsigned)s_wuser[f] < u)) ? 1u : 0u;
    }
    a.io_score[(size_t)i * num + r] = s_wscore[e];
    a.io_user[(size_t)i * num + r] = s_wuser[e];
  }
  if (tid == 0) a.io_count[i] = (int32_t)n_win;
}

// The slabs: enough (tile, slab) pairs for two blocks a CU when every tile is full; never shorter than AUD_SLAB_MIN users, nor more than the merge kernel's
// LDS list holds or than 512 MiB of partials.  The lists are sized for `blocks`, the most the scan will launch.
void audience_geometry(int64_t n_users, int32_t n_query, int32_t num, int n_cu, AudArgs* a) {
  const int64_t target = 2 * (int64_t)(n_cu > 0 ? n_cu : 1);
  const int64_t min_tiles = ((int64_t)n_query + AUD_TILE - 1) / AUD_TILE;
  int64_t slabs = target / (min_tiles > 0 ? min_tiles : 1);
  const int64_t by_users = n_users / AUD_SLAB_MIN;  // a slab pays for a table build and a partial of num entries per item: eight rounds at least
  const int64_t by_bytes = ((int64_t)512 << 20) / ((int64_t)(n_query > 0 ? n_query : 1) * num * 12);
  if (slabs > by_users) slabs = by_users;
  if (slabs > AUD_MAX_SLABS) slabs = AUD_MAX_SLABS;
  if (slabs > by_bytes) slabs = by_bytes;
  if (slabs < 1) slabs = 1;
  int64_t slab_users = ((n_users + slabs - 1) / slabs + AUD_ROUND - 1) / AUD_ROUND * AUD_ROUND;
  if (slab_users < AUD_ROUND) slab_users = AUD_ROUND;
  slabs = (n_users + slab_users - 1) / slab_users;
  if (slabs < 1) slabs = 1;
  a->cap = num + 2 * AUD_ROUND;
  a->n_slabs = (int32_t)slabs;
  a->slab_users = (int32_t)slab_users;
  const int64_t most = (int64_t)n_query * slabs;  // a tile holds an item at least
  a->blocks = (int32_t)(most < target ? (most > 0 ? most : 1) : target);
}

hipError_t launch_audience_plan(hipStream_t st, const AudArgs& a) {
  hipLaunchKernelGGL(aud_plan_kernel, dim3(1), dim3(AUD_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_audience(hipStream_t st, const AudArgs& a, bool weighted) {
  if (a.n_query <= 0 || a.n_users <= 0 || a.n_tiles <= 0) return hipSuccess;
  if (weighted) hipLaunchKernelGGL(aud_scan_kernel<true>, dim3((unsigned)a.blocks), dim3(AUD_THREADS), 0, st, a);
  else hipLaunchKernelGGL(aud_scan_kernel<false>, dim3((unsigned)a.blocks), dim3(AUD_THREADS), 0, st, a);
  hipLaunchKernelGGL(aud_merge_kernel, dim3((unsigned)a.n_query), dim3(AUD_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace urcco
