// cco_recommend.h -- batch recommendations from a built CCO model (urcco_dev_recommend): per query row the top `num` of
//   score(q, i) = sum over should-clauses c, in call order, of boost_c * | T_c(q) ^ I_c(i) |
// over the eligible items, in the total order (score desc, backfill position asc), zero-score items as backfill (decision D15).
// Included once, from cco_misc.hip behind cco_select.h (the CPU suite compiles a fixed list of translation units).
//
//   rec_inverse_kernel   pos[fill_order[p]] = p: the backfill position of every item
//   rec_work_kernel      w(q) = sum_c sum_{h in T_c(q)} len(column h of I_c) + exclusions of q: the upper bound of the distinct items the query
//                        touches; w <= REC_LIMIT goes to the LDS class (list filled from the front), everything else to the global class (from the back)
//   rec_rows_kernel<0, R>  LDS class: a block per query, an open-addressing table keyed by the item in LDS
//   rec_rows_kernel<1, R>  global class: the same walk on a dense per-block accumulator of n_items slots in arena scratch, cleared through its touched lists
//   rec_rules_ok           R = true (urcco_dev_recommend_rules, decision D16): the per-(query, item) eligibility rules, evaluated wherever item_mask is consulted --
//                          when an absent item is claimed (a rejected item becomes a tombstone) and per walked backfill position; R = false is the rule-free call
// Both classes: exclusions enter first as tombstones, masked-out items become tombstones when they are first hit; clause by clause the hits raise a 32-bit
// match counter per slot (the claiming lane appends the slot to the candidate list), then `score += boost * m; m = 0` is folded over the list -- the f64 sum
// has the order of the clauses whatever the order of the hits.  Selection: the radix select of cco_select.h over the 96-bit key (score bits, ~position) finds
// the num-th best candidate, the (at most num) winners are ranked by counting; then the backfill walks fill_order from the front.
//   rec_rows_kernel<., ., true>  W = true (urcco_dev_recommend_weighted, decision D20): a hit of term h raises the counter by the clause's integer weight w_c[h]
//                          (units of 2^-15, 1 .. REC_WEIGHT_MAX; a clause without an array: REC_WEIGHT_ONE) and the fold adds boost * ((double)M * 2^-15); the LDS
//                          class keeps its 32-bit counters, the global class counts in a 64-bit array of its own (g_m64) in place of g_m; W = false is the code above
//   rec_idf_kernel         urcco_dev_idf_weights: w[h] = clamp(llrint(log(1 + (n_docs - df + 0.5) / (df + 0.5)) * 2^15), 1, REC_WEIGHT_MAX), a thread per column
#pragma once

namespace urcco {

constexpr int REC_THREADS = 256;
constexpr int REC_NW = REC_THREADS / WAVE;
constexpr int REC_CAP_LOG2 = 12;
constexpr int REC_CAP = 1 << REC_CAP_LOG2;  // slots of the LDS table
constexpr int REC_LIMIT = REC_LDS_LIMIT;    // most distinct items (candidates + tombstones) a query of the LDS class can hold: load factor 0.75
static_assert(REC_LIMIT * 4 <= REC_CAP * 3 && REC_LIMIT <= 65536, "load factor of the LDS table; 16-bit slot numbers");
// Weighted counters (D20) cannot overflow.  LDS class: w(q) <= REC_LIMIT bounds the hits of a query, so M <= REC_LIMIT * REC_WEIGHT_MAX = 3072 * 2^20 < 2^32 and
// the 32-bit s_m stays (the kernel clamps every loaded weight to 1 .. REC_WEIGHT_MAX, so a bad array cannot break the bound).  Global class: no cap on the
// terms, so its weighted form counts in 64 bits: fewer than 2^43 hits of at most 2^20 each.
static_assert((unsigned long long)REC_LIMIT * (unsigned long long)REC_WEIGHT_MAX < (1ull << 32), "weighted 32-bit LDS match counters: REC_LIMIT hits of REC_WEIGHT_MAX each");
constexpr double REC_WEIGHT_UNIT = 1.0 / (double)REC_WEIGHT_ONE;  // 2^-15, exact
constexpr unsigned REC_EMPTY = 0xffffffffu; // (item ids are < 2^31 - 1)
constexpr unsigned REC_TOMB = 0x80000000u;  // slot of an item that may not be returned
static_assert(REC_MAX_NUM <= REC_THREADS, "one thread ranks one winner");

struct RecArgs {
  RecClause c[REC_MAX_CLAUSES];
  int64_t n_queries;
  int32_t n_items, n_clauses, num, flags;
  int32_t lds_limit;          // w(q) up to here: LDS class (<= REC_LIMIT)
  const int64_t* excl_row_ptr;
  const int32_t* excl_col_idx;
  const uint8_t* item_mask;
  const int32_t* fill_order;
  const int32_t* pos;         // nullable: backfill position per item (NULL: the item index)
  int32_t* list;              // [n_queries]: LDS-class queries from the front, global-class queries from the back
  unsigned long long* ctr;    // [5]: queries of the LDS class, of the global class, table overflows, candidates, backfill steps (only counted under rules)
  int32_t* out_count;
  int32_t* out_idx;
  double* out_score;
  // global class: g_blocks slices of n_items words each; g_state and g_m are zero between queries
  unsigned* g_state;          // 0 untouched, 1 candidate, 2 tombstone
  unsigned* g_m;
  int32_t* g_list;            // candidates from the front, tombstones from the back
  double* g_score;            // by candidate ordinal
  int32_t g_blocks;
  int32_t n_rules;
  RecRule r[REC_MAX_RULES];   // read by the <., true, .> instantiations only
  // read by the <., ., true> instantiations only (urcco_dev_recommend_weighted)
  const uint32_t* w[REC_MAX_CLAUSES];  // per clause: [n_cols] term weights in units of 2^-15, or NULL = REC_WEIGHT_ONE throughout
  unsigned long long* g_m64;           // global class: the 64-bit match counters, g_blocks slices of n_items, zero between queries (takes the place of g_m)
};
static_assert(sizeof(RecArgs) <= 4096, "kernel arguments: the clause and rule tables travel by value");

__global__ __launch_bounds__(256) void rec_inverse_kernel(int32_t n_items, const int32_t* __restrict__ fill_order, int32_t* __restrict__ pos) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_items; p += (int64_t)gridDim.x * 256) {
    const int32_t i = fill_order[p];
    if ((unsigned)i < (unsigned)n_items) pos[i] = (int32_t)p;
  }
}

// a wave per query
__global__ __launch_bounds__(REC_THREADS) void rec_work_kernel(RecArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * REC_NW;
  for (int64_t q = (int64_t)blockIdx.x * REC_NW + threadIdx.x / WAVE; q < a.n_queries; q += n_waves) {
    long long w = 0;
    for (int c = 0; c < a.n_clauses; ++c) {
      const RecClause& cl = a.c[c];
      const int64_t e = cl.q_row_ptr[q + 1];
      for (int64_t t = cl.q_row_ptr[q] + lane; t < e; t += WAVE) {
        const int32_t h = cl.q_col_idx[t];
        if ((unsigned)h < (unsigned)cl.n_cols) w += cl.ind_col_ptr[h + 1] - cl.ind_col_ptr[h];
      }
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) w += shfl_xor_u64((unsigned long long)w, o);
    if (a.excl_row_ptr) w += a.excl_row_ptr[q + 1] - a.excl_row_ptr[q];
    if (lane == 0) {
      if (w <= a.lds_limit) a.list[atomicAdd(&a.ctr[0], 1ull)] = (int32_t)q;
      else a.list[a.n_queries - 1 - (int64_t)atomicAdd(&a.ctr[1], 1ull)] = (int32_t)q;
    }
  }
}

__device__ __forceinline__ unsigned rec_hash(unsigned item) { return (item * 2654435761u) >> (32 - REC_CAP_LOG2); }

// Do all rules of the call hold for (q, item)?  item < n_items.  ANY / NONE: the entries of row `item` of the rule's matrix (any order, duplicates allowed, a
// column outside 0..n_cols never matches) are looked up one by one in the query's sorted row; RANGE: lo <= value < hi, an item without a value fails.  Pure: a
// plain per-lane loop over short rows (a handful of property values, at most k indicator entries), no atomics; the first failing rule ends it.
template <bool RULES>
__device__ __forceinline__ bool rec_rules_ok(const RecArgs& a, int64_t q, int32_t item) {
  if (!RULES) return true;
  for (int j = 0; j < a.n_rules; ++j) {
    const RecRule& r = a.r[j];
    if (r.kind == REC_RULE_RANGE) {
      const int64_t v = r.item_value[item];
      if (v == INT64_MIN || v < r.q_lo[q] || v >= r.q_hi[q]) return false;
      continue;
    }
    const int64_t qb = r.q_row_ptr[q], qe = r.q_row_ptr[q + 1];
    bool any = false;
    if (qe > qb) {
      const int64_t e = r.m_row_ptr[item + 1];
      for (int64_t t = r.m_row_ptr[item]; t < e && !any; ++t) {
        const int32_t col = r.m_col_idx[t];
        if ((unsigned)col >= (unsigned)r.n_cols) continue;
        int64_t lo = qb, hi = qe;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (r.q_col_idx[mid] < col) lo = mid + 1;
          else hi = mid;
        }
        any = lo < qe && r.q_col_idx[lo] == col;
      }
    }
    if (any != (r.kind == REC_RULE_ANY)) return false;
  }
  return true;
}

// Slot of `item` in the LDS table, or -1 when the item may not be returned (tombstone) or the table is full (err).  An absent item is
// claimed -- as a candidate (*fresh = true) when `live`, the mask and the rules admit it, else as a tombstone.
template <bool RULES>
__device__ __forceinline__ int rec_lds_touch(unsigned* keys, unsigned item, bool live, const uint8_t* __restrict__ mask, bool* fresh, unsigned long long* err,
                                             const RecArgs& a, int64_t q) {
  unsigned h = rec_hash(item);
  for (int probe = 0; probe < REC_CAP; ++probe) {
    unsigned k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == REC_EMPTY) {
      const bool ok = live && (!mask || mask[item] != 0) && rec_rules_ok<RULES>(a, q, (int32_t)item);
      k = atomicCAS(&keys[h], REC_EMPTY, ok ? item : (item | REC_TOMB));
      if (k == REC_EMPTY) {
        *fresh = ok;
        return ok ? (int)h : -1;
      }
    }
    if ((k & ~REC_TOMB) == item) return (k & REC_TOMB) ? -1 : (int)h;
    h = (h + 1) & (REC_CAP - 1);
  }
  atomicAdd(err, 1ull);
  return -1;
}
// is the item in the table (candidate or tombstone)?
__device__ __forceinline__ bool rec_lds_has(const unsigned* keys, unsigned item) {
  unsigned h = rec_hash(item);
  for (int probe = 0; probe < REC_CAP; ++probe) {
    const unsigned k = keys[h];
    if (k == REC_EMPTY) return false;
    if ((k & ~REC_TOMB) == item) return true;
    h = (h + 1) & (REC_CAP - 1);
  }
  return false;
}

template <bool DENSE, bool RULES, bool WEIGHTED>
__global__ __launch_bounds__(REC_THREADS) void rec_rows_kernel(RecArgs a) {
  __shared__ unsigned s_keys[DENSE ? 1 : REC_CAP];
  __shared__ unsigned s_m[DENSE ? 1 : REC_CAP];
  __shared__ unsigned short s_cand[DENSE ? 1 : REC_LIMIT];  // slot of every candidate
  __shared__ double s_score[DENSE ? 1 : REC_LIMIT];         // by candidate ordinal
  __shared__ SelScratch s_select;
  __shared__ unsigned s_ncand, s_ntomb, s_nwin;
  __shared__ unsigned s_wcnt[REC_NW];
  __shared__ double s_wscore[REC_MAX_NUM];
  __shared__ int32_t s_wpos[REC_MAX_NUM];
  __shared__ int32_t s_witem[REC_MAX_NUM];

  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int32_t n_items = a.n_items;
  const int num = a.num;
  const uint8_t* __restrict__ mask = a.item_mask;
  const int32_t* __restrict__ pos_of = a.pos;
  unsigned* g_state = DENSE ? a.g_state + (size_t)blockIdx.x * (size_t)n_items : nullptr;
  unsigned* g_m = DENSE && !WEIGHTED ? a.g_m + (size_t)blockIdx.x * (size_t)n_items : nullptr;
  unsigned long long* g_m64 = DENSE && WEIGHTED ? a.g_m64 + (size_t)blockIdx.x * (size_t)n_items : nullptr;
  int32_t* g_list = DENSE ? a.g_list + (size_t)blockIdx.x * (size_t)n_items : nullptr;
  double* g_score = DENSE ? a.g_score + (size_t)blockIdx.x * (size_t)n_items : nullptr;
  const long long n_mine = (long long)a.ctr[DENSE ? 1 : 0];

  if (!DENSE)
    for (int s = tid; s < REC_CAP; s += REC_THREADS) s_m[s] = 0;  // every fold returns the counters to zero

  for (long long at = blockIdx.x; at < n_mine; at += gridDim.x) {
    const int64_t q = DENSE ? a.list[a.n_queries - 1 - at] : a.list[at];
    if (!DENSE)
      for (int s = tid; s < REC_CAP; s += REC_THREADS) s_keys[s] = REC_EMPTY;
    if (tid == 0) { s_ncand = 0; s_ntomb = 0; s_nwin = 0; }
    __syncthreads();

    // one hit of a clause term of weight `wt` (WEIGHTED only) on `item`
    auto hit = [&](int32_t item, unsigned wt) {
      if ((unsigned)item >= (unsigned)n_items) return;
      if (DENSE) {
        unsigned st = __hip_atomic_load(&g_state[item], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (st == 0) {
          const bool ok = (!mask || mask[item] != 0) && rec_rules_ok<RULES>(a, q, item);
          st = atomicCAS(&g_state[item], 0u, ok ? 1u : 2u);
          if (st == 0) {
            if (ok) {
              const unsigned j = atomicAdd(&s_ncand, 1u);
              g_list[j] = item;
              g_score[j] = 0.0;
            } else {
              g_list[n_items - 1 - (int32_t)atomicAdd(&s_ntomb, 1u)] = item;
            }
            st = ok ? 1u : 2u;
          }
        }
        if (st == 1) {
          if (WEIGHTED) atomicAdd(&g_m64[item], (unsigned long long)wt);
          else atomicAdd(&g_m[item], 1u);
        }
      } else {
        bool fresh = false;
        const int slot = rec_lds_touch<RULES>(s_keys, (unsigned)item, true, mask, &fresh, &a.ctr[2], a, q);
        if (slot < 0) return;
        if (fresh) {
          const unsigned j = atomicAdd(&s_ncand, 1u);
          if (j < (unsigned)REC_LIMIT) {
            s_cand[j] = (unsigned short)slot;
            s_score[j] = 0.0;
          } else {
            atomicAdd(&a.ctr[2], 1ull);
          }
        }
        atomicAdd(&s_m[slot], WEIGHTED ? wt : 1u);
      }
    };

    // ---- exclusions: tombstones ----
    if (a.excl_row_ptr) {
      const int64_t e = a.excl_row_ptr[q + 1];
      for (int64_t t = a.excl_row_ptr[q] + tid; t < e; t += REC_THREADS) {
        const int32_t item = a.excl_col_idx[t];
        if ((unsigned)item >= (unsigned)n_items) continue;
        if (DENSE) {
          if (atomicCAS(&g_state[item], 0u, 2u) == 0) g_list[n_items - 1 - (int32_t)atomicAdd(&s_ntomb, 1u)] = item;
        } else {
          bool fresh = false;
          (void)rec_lds_touch<RULES>(s_keys, (unsigned)item, false, mask, &fresh, &a.ctr[2], a, q);
        }
      }
      __syncthreads();
    }

    // ---- the clauses, in call order ----
    for (int c = 0; c < a.n_clauses; ++c) {
      const RecClause& cl = a.c[c];
      const int64_t tb = cl.q_row_ptr[q], nt = cl.q_row_ptr[q + 1] - tb;
      for (int64_t t = 0; t < nt; ++t) {  // short columns: a wave per term; long ones: the whole block
        const int32_t h = cl.q_col_idx[tb + t];
        if ((unsigned)h >= (unsigned)cl.n_cols) continue;
        const int64_t s = cl.ind_col_ptr[h], e = cl.ind_col_ptr[h + 1];
        unsigned wt = 1u;
        if (WEIGHTED) {  // one load per term, uniform for whoever walks the column; clamped, so the 32-bit LDS counter holds whatever the array says
          wt = a.w[c] ? a.w[c][h] : (unsigned)REC_WEIGHT_ONE;
          wt = wt < 1u ? 1u : wt > (unsigned)REC_WEIGHT_MAX ? (unsigned)REC_WEIGHT_MAX : wt;
        }
        if (e - s >= 2 * REC_THREADS) {
          for (int64_t p = s + tid; p < e; p += REC_THREADS) hit(cl.ind_row_idx[p], wt);
        } else if ((int)(t & (REC_NW - 1)) == wave) {
          for (int64_t p = s + lane; p < e; p += WAVE) hit(cl.ind_row_idx[p], wt);
        }
      }
      __syncthreads();
      const unsigned nc = s_ncand < (unsigned)(DENSE ? n_items : REC_LIMIT) ? s_ncand : (unsigned)(DENSE ? n_items : REC_LIMIT);
      const double boost = cl.boost;
      for (unsigned j = tid; j < nc; j += REC_THREADS) {
        if (DENSE && WEIGHTED) {  // (the translation unit is compiled with -ffp-contract=off: product, then sum, one rounding each)
          const int32_t item = g_list[j];
          const unsigned long long m = g_m64[item];
          if (m) { g_score[j] = g_score[j] + boost * ((double)m * REC_WEIGHT_UNIT); g_m64[item] = 0; }
        } else if (DENSE) {
          const int32_t item = g_list[j];
          const unsigned m = g_m[item];
          if (m) { g_score[j] = g_score[j] + boost * (double)m; g_m[item] = 0; }
        } else {
          const unsigned slot = s_cand[j];
          const unsigned m = s_m[slot];
          if (m) { s_score[j] = s_score[j] + boost * (WEIGHTED ? (double)m * REC_WEIGHT_UNIT : (double)m); s_m[slot] = 0; }
        }
      }
      __syncthreads();
    }

    const unsigned nc = s_ncand < (unsigned)(DENSE ? n_items : REC_LIMIT) ? s_ncand : (unsigned)(DENSE ? n_items : REC_LIMIT);
    auto cand_item = [&](unsigned j) -> int32_t { return DENSE ? g_list[j] : (int32_t)s_keys[s_cand[j]]; };
    auto cand_score = [&](unsigned j) -> double { return DENSE ? g_score[j] : s_score[j]; };
    auto item_pos = [&](int32_t item) -> int32_t { return pos_of ? pos_of[item] : item; };

    // ---- selection: threshold key (thi, tlo) = the num-th largest of (score bits, ~position); every candidate when there are no more than num ----
    SelKey thr{0ull, 0u};
    if (nc > (unsigned)num)  // (differ = all ones: whether sel_differ's pass would pay here has not been measured)
      thr = sel_kth_largest<REC_THREADS>(
          nc, (unsigned)num, [&](unsigned j) { return (unsigned long long)__double_as_longlong(cand_score(j)); },
          [&](unsigned j) { return ~(unsigned)item_pos(cand_item(j)); }, SelKey{~0ull, ~0u}, SelKey{0ull, 0u}, s_select);
    const unsigned long long thi = thr.hi;
    const unsigned tlo = thr.lo;
    // ---- winners (at most num: the keys are distinct), ranked by counting ----
    for (unsigned j = tid; j < nc; j += REC_THREADS) {
      const double sc = cand_score(j);
      const unsigned long long hi = (unsigned long long)__double_as_longlong(sc);
      if (hi < thi) continue;
      const int32_t item = cand_item(j);
      const int32_t p = item_pos(item);
      if (hi == thi && ~(unsigned)p < tlo) continue;
      const unsigned w = atomicAdd(&s_nwin, 1u);
      if (w < (unsigned)REC_MAX_NUM) { s_wscore[w] = sc; s_wpos[w] = p; s_witem[w] = item; }
    }
    __syncthreads();
    unsigned nw = s_nwin < (unsigned)num ? s_nwin : (unsigned)num;  // (more only if fill_order is no permutation)
    if ((unsigned)tid < nw) {
      const double sc = s_wscore[tid];
      const unsigned p = (unsigned)s_wpos[tid];
      unsigned r = 0;
      for (unsigned u = 0; u < nw; ++u) {
        const double su = s_wscore[u];
        r += (su > sc || (su == sc && ((unsigned)s_wpos[u] < p || ((unsigned)s_wpos[u] == p && u < (unsigned)tid)))) ? 1u : 0u;
      }
      a.out_idx[q * num + r] = s_witem[tid];
      a.out_score[q * num + r] = sc;
    }

    // ---- backfill: eligible items nothing hit, in fill order ----
    unsigned n_out = nw;
    unsigned steps = 0;  // of 256 positions each (reported under rules: a rare filter makes the walk cross the catalogue)
    if (!(a.flags & REC_NO_BACKFILL)) {
      for (int64_t p0 = 0; p0 < n_items && n_out < (unsigned)num; p0 += REC_THREADS) {
        const int64_t p = p0 + tid;
        int32_t item = -1;
        bool ok = false;
        if (p < n_items) {
          item = a.fill_order ? a.fill_order[p] : (int32_t)p;
          ok = (unsigned)item < (unsigned)n_items && (!mask || mask[item] != 0);
          if (ok) ok = DENSE ? g_state[item] == 0 : !rec_lds_has(s_keys, (unsigned)item);
          if (RULES && ok) ok = rec_rules_ok<RULES>(a, q, item);
        }
        ++steps;
        const unsigned long long b = __ballot(ok ? 1 : 0);
        if (lane == 0) s_wcnt[wave] = (unsigned)__popcll(b);
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int x = 0; x < REC_NW; ++x) {
          before += x < wave ? s_wcnt[x] : 0u;
          total += s_wcnt[x];
        }
        const unsigned slot = n_out + before + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
        if (ok && slot < (unsigned)num) {
          a.out_idx[q * num + slot] = item;
          a.out_score[q * num + slot] = 0.0;
        }
        n_out = n_out + total < (unsigned)num ? n_out + total : (unsigned)num;
        __syncthreads();
      }
    }
    if (tid == 0) {
      a.out_count[q] = (int32_t)n_out;
      atomicAdd(&a.ctr[3], (unsigned long long)nc);
      if (RULES) atomicAdd(&a.ctr[4], (unsigned long long)steps);
    }
    if (DENSE) {  // leave the accumulator as it was found
      for (unsigned j = tid; j < nc; j += REC_THREADS) g_state[g_list[j]] = 0;
      const unsigned ntomb = s_ntomb;
      for (unsigned j = tid; j < ntomb; j += REC_THREADS) g_state[g_list[n_items - 1 - (int32_t)j]] = 0;
    }
    __syncthreads();
  }
}

__global__ void rec_stats_kernel(const unsigned long long* __restrict__ ctr, int64_t* __restrict__ stats) {
  const int t = threadIdx.x;
  if (t < REC_STATS_LEN) stats[t] = t < 5 ? (int64_t)ctr[t] : 0;
}

// urcco_dev_idf_weights: a thread per column.  df = the column's length (clamped to 0 .. n_docs); Lucene's BM25 idf in f64, rounded to units of 2^-15.
__global__ __launch_bounds__(256) void rec_idf_kernel(int32_t n_cols, const int64_t* __restrict__ col_ptr, int64_t n_docs, uint32_t* __restrict__ out) {
  for (int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x; h < n_cols; h += (int64_t)gridDim.x * 256) {
    int64_t df = col_ptr[h + 1] - col_ptr[h];
    if (df > n_docs) df = n_docs;
    long long w = 1;
    if (df > 0) {
      const double idf = log(1.0 + ((double)(n_docs - df) + 0.5) / ((double)df + 0.5));
      w = llrint(idf * (double)REC_WEIGHT_ONE);
      w = w < 1 ? 1 : w > (long long)REC_WEIGHT_MAX ? (long long)REC_WEIGHT_MAX : w;
    }
    out[h] = (uint32_t)w;
  }
}

hipError_t launch_idf_weights(hipStream_t st, int n_cu, int32_t n_cols, const int64_t* col_ptr, int64_t n_docs, uint32_t* out) {
  if (n_cols <= 0) return hipSuccess;
  int64_t blocks = ((int64_t)n_cols + 255) / 256;
  if (blocks > (int64_t)n_cu * 8) blocks = (int64_t)n_cu * 8;
  hipLaunchKernelGGL(rec_idf_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n_cols, col_ptr, n_docs, out);
  return hipGetLastError();
}

// resident blocks of the global class: 20 bytes of scratch per item and block (g_state, g_m, g_list: 4 each; g_score: 8), at most 512 MiB; the weighted
// call counts in g_m64 (8) in place of g_m: 24 bytes
int32_t recommend_global_blocks(int64_t n_queries, int32_t n_items, int n_cu, bool weighted) {
  int64_t blocks = ((int64_t)512 << 20) / ((int64_t)(n_items > 0 ? n_items : 1) * (weighted ? 24 : 20));
  if (blocks > 2 * (int64_t)n_cu) blocks = 2 * (int64_t)n_cu;
  if (blocks > n_queries) blocks = n_queries;
  return (int32_t)(blocks < 1 ? 1 : blocks);
}

hipError_t launch_recommend(hipStream_t st, int n_cu, int64_t n_queries, int32_t n_items, const RecClause* clauses, int32_t n_clauses, const int64_t* excl_row_ptr,
                            const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order, int32_t num, int32_t flags, int32_t* out_count,
                            int32_t* out_idx, double* out_score, int64_t* stats_dev, unsigned long long* ctr, int32_t* list, int32_t* pos, int32_t g_blocks,
                            unsigned* g_state, unsigned* g_m, int32_t* g_list, double* g_score, int32_t lds_limit, const RecRule* rules, int32_t n_rules,
                            const uint32_t* const* weights, unsigned long long* g_m64) {
  const bool weighted = weights != nullptr;  // then g_m64 is the counter array of the global class and g_m is not read
  RecArgs a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < n_clauses; ++c) a.c[c] = clauses[c];
  for (int j = 0; j < n_rules; ++j) a.r[j] = rules[j];
  a.n_rules = n_rules;
  if (weighted)
    for (int c = 0; c < n_clauses; ++c) a.w[c] = weights[c];
  a.g_m64 = g_m64;
  a.n_queries = n_queries; a.n_items = n_items; a.n_clauses = n_clauses; a.num = num; a.flags = flags;
  a.lds_limit = lds_limit < REC_LIMIT ? lds_limit : REC_LIMIT;
  a.excl_row_ptr = excl_row_ptr; a.excl_col_idx = excl_col_idx; a.item_mask = item_mask; a.fill_order = fill_order;
  a.pos = fill_order ? pos : nullptr;
  a.list = list; a.ctr = ctr; a.out_count = out_count; a.out_idx = out_idx; a.out_score = out_score;
  a.g_state = g_state; a.g_m = g_m; a.g_list = g_list; a.g_score = g_score; a.g_blocks = g_blocks;
  hipError_t e = hipMemsetAsync(ctr, 0, 5 * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  if (n_queries > 0) {
    if (fill_order && n_items > 0) {
      int64_t blocks = ((int64_t)n_items + 255) / 256;
      if (blocks > (int64_t)n_cu * 8) blocks = (int64_t)n_cu * 8;
      hipLaunchKernelGGL(rec_inverse_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n_items, fill_order, pos);
    }
    const size_t slice = (size_t)g_blocks * (size_t)(n_items > 0 ? n_items : 1);
    if ((e = hipMemsetAsync(g_state, 0, slice * sizeof(unsigned), st)) != hipSuccess) return e;
    if ((e = weighted ? hipMemsetAsync(g_m64, 0, slice * sizeof(unsigned long long), st) : hipMemsetAsync(g_m, 0, slice * sizeof(unsigned), st)) != hipSuccess) return e;
    int64_t wb = (n_queries + REC_NW - 1) / REC_NW;
    if (wb > (int64_t)n_cu * 8) wb = (int64_t)n_cu * 8;
    hipLaunchKernelGGL(rec_work_kernel, dim3((unsigned)wb), dim3(REC_THREADS), 0, st, a);
    const int64_t lb = n_queries < (int64_t)n_cu * 2 ? n_queries : (int64_t)n_cu * 2;  // the LDS table lets two blocks share a CU
    if (weighted && n_rules > 0) {
      hipLaunchKernelGGL((rec_rows_kernel<false, true, true>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<true, true, true>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    } else if (weighted) {
      hipLaunchKernelGGL((rec_rows_kernel<false, false, true>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<true, false, true>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    } else if (n_rules > 0) {
      hipLaunchKernelGGL((rec_rows_kernel<false, true, false>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<true, true, false>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    } else {
      hipLaunchKernelGGL((rec_rows_kernel<false, false, false>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<true, false, false>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    }
  }
  if (stats_dev) hipLaunchKernelGGL(rec_stats_kernel, dim3(1), dim3(64), 0, st, ctr, stats_dev);
  return hipGetLastError();
}

}  // namespace urcco
