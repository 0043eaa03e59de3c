// cco_recommend.h -- batch recommendations from a built CCO model (urcco_dev_recommend): per query row the top `num` of
//   score(q, i) = sum over should-clauses c, in call order, of boost_c * | T_c(q) ^ I_c(i) |
// over the eligible items, in the total order (score desc, backfill position asc), zero-score items as backfill (decision D15).
// Included once, from cco_misc.hip behind cco_select.h (the CPU suite compiles a fixed list of translation units).
//
//   rec_inverse_kernel   pos[fill_order[p]] = p: the backfill position of every item
//   rec_work_kernel      w(q) = sum_c sum_{h in T_c(q)} len(column h of I_c) + exclusions of q: the upper bound of the distinct items the query
//                        touches; w <= REC_LIMIT goes to the LDS class (list filled from the front), everything else to the global class (from the back);
//                        with the hashed class on (REC_HASHED, decision D31) a query beyond the LDS limit with w <= REC_HASH_LIMIT goes to a list of its own
//   rec_rows_kernel<0, R>  LDS class: a block per query, an open-addressing table keyed by the item in LDS
//   rec_rows_kernel<1, R>  global (dense) class: the same walk on a dense per-block accumulator of n_items slots in arena scratch, cleared through its touched lists
//   rec_rows_kernel<2, R>  hashed class: the same walk on an open-addressing table of REC_HASH_CAP = 2^17 slots per resident block in arena scratch -- keys
//                          (REC_EMPTY, REC_TOMB and item ids as in the LDS table), match counters by slot, a list of SLOTS (candidates from the front, tombstones
//                          from the back) and the scores by candidate ordinal: 2.125 MiB per block (2.625 MiB weighted) whatever n_items is.  Home slot of an item:
//                            (item * 2654435761u) >> (32 - REC_HASH_CAP_LOG2),  linear probing that wraps at the end of the table.
//                          w(q) <= REC_HASH_LIMIT = 3/4 of the slots bounds the distinct items of a query, so the table cannot fill (the LDS table's argument);
//                          at the end of a query the keys are reset through the two ends of the list, never by a sweep.  Results are the dense class's bit for bit.
//   rec_rules_ok           R = true (urcco_dev_recommend_rules, decision D16): the per-(query, item) eligibility rules, evaluated wherever item_mask is consulted --
//                          when an absent item is claimed (a rejected item becomes a tombstone) and per walked backfill position; R = false is the rule-free call
// Both classes: exclusions enter first as tombstones, masked-out items become tombstones when they are first hit; clause by clause the hits raise a 32-bit
// match counter per slot (the claiming lane appends the slot to the candidate list), then `score += boost * m; m = 0` is folded over the list -- the f64 sum
// has the order of the clauses whatever the order of the hits.  Selection: the radix select of cco_select.h over the 96-bit key (score bits, ~position) finds
// the num-th best candidate, the (at most num) winners are ranked by counting; then the backfill walks fill_order from the front.
//   rec_rows_kernel<., ., true>  W = true (urcco_dev_recommend_weighted, decision D20): a hit of term h raises the counter by the clause's integer weight w_c[h]
//                          (units of 2^-15, 1 .. REC_WEIGHT_MAX; a clause without an array: REC_WEIGHT_ONE) and the fold adds boost * ((double)M * 2^-15); the LDS
//                          class keeps its 32-bit counters, the global and the hashed class count in a 64-bit array of their own (g_m64 / h.m64) in place of
//                          g_m / h.m; W = false is the code above
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
// Hashed class: w(q) <= REC_HASH_LIMIT bounds the hits.  Unweighted, a counter holds at most REC_HASH_LIMIT < 2^32: 32-bit counters (h.m).  Weighted,
// REC_HASH_LIMIT * REC_WEIGHT_MAX = 98 304 * 2^20 exceeds 2^32: that instantiation counts in 64 bits (h.m64), as the dense class does.
static_assert(REC_HASH_LIMIT * 4ll <= REC_HASH_CAP * 3ll && REC_HASH_CAP_LOG2 < 31, "load factor of the hashed table; 31-bit slot numbers in an int32 list");
static_assert((unsigned long long)REC_HASH_LIMIT < (1ull << 32), "unweighted hashed class: 32-bit match counters hold REC_HASH_LIMIT hits of 1");
static_assert((unsigned long long)REC_HASH_LIMIT * (unsigned long long)REC_WEIGHT_MAX >= (1ull << 32) &&
                  (unsigned long long)REC_HASH_LIMIT * (unsigned long long)REC_WEIGHT_MAX < (1ull << 63),
              "weighted hashed class: REC_HASH_LIMIT hits of REC_WEIGHT_MAX overflow 32 bits, so it relies on the 64-bit counters");
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
  unsigned long long* ctr;    // [8]: queries of the LDS class, of the global class, table overflows, candidates, backfill steps (only counted under rules),
                              //      queries of the hashed class
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
  // hashed class (h.queries == NULL: the class is off): h.blocks slices; between queries every key is REC_EMPTY and every counter zero
  RecHashed h;
};
static_assert(sizeof(RecArgs) <= 4096, "kernel arguments: the clause and rule tables travel by value");

__global__ __launch_bounds__(256) void rec_inverse_kernel(int32_t n_items, const int32_t* __restrict__ fill_order, int32_t* __restrict__ pos) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_items; p += (int64_t)gridDim.x * 256) {
    const int32_t i = fill_order[p];
    if ((unsigned)i < (unsigned)n_items) pos[i] = (int32_t)p;
  }
}

// the w-based split of one query, by the wave that owns it
__device__ __forceinline__ void rec_work_bin(const RecArgs& a, int64_t q, int lane) {
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
    else if (a.h.queries && w <= a.h.limit) a.h.queries[atomicAdd(&a.ctr[5], 1ull)] = (int32_t)q;
    else a.list[a.n_queries - 1 - (int64_t)atomicAdd(&a.ctr[1], 1ull)] = (int32_t)q;
  }
}

// a wave per query
__global__ __launch_bounds__(REC_THREADS) void rec_work_kernel(RecArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * REC_NW;
  for (int64_t q = (int64_t)blockIdx.x * REC_NW + threadIdx.x / WAVE; q < a.n_queries; q += n_waves) rec_work_bin(a, q, lane);
}

// The binning of a call with drivers: d(q) first -- per driver the summed lengths of the columns of its matrix that the query's rule row names, the smallest
// over the drivers (they ascend by rule, so the lowest rule index wins a tie) -- and a query with d <= limit goes to the driven list; the rest as above.
__global__ __launch_bounds__(REC_THREADS) void rec_work_driven_kernel(RecArgs a, RecDriven dv) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * REC_NW;
  for (int64_t q = (int64_t)blockIdx.x * REC_NW + threadIdx.x / WAVE; q < a.n_queries; q += n_waves) {
    long long best = 0;
    int best_j = -1;
    for (int j = 0; j < dv.n_drivers; ++j) {
      const RecRule& r = a.r[dv.d[j].rule];
      const int64_t* __restrict__ cp = dv.d[j].m_col_ptr;
      long long d = 0;
      const int64_t e = r.q_row_ptr[q + 1];
      for (int64_t t = r.q_row_ptr[q] + lane; t < e; t += WAVE) {
        const int32_t v = r.q_col_idx[t];
        if ((unsigned)v < (unsigned)r.n_cols) d += cp[v + 1] - cp[v];
      }
      for (int o = WAVE / 2; o > 0; o >>= 1) d += shfl_xor_u64((unsigned long long)d, o);
      if (best_j < 0 || d < best) { best = d; best_j = j; }
    }
    if (best_j >= 0 && best <= dv.limit) {
      if (lane == 0) {
        dv.queries[atomicAdd(&a.ctr[6], 1ull)] = (int32_t)q;
        dv.driver_of[q] = best_j;
      }
    } else {
      rec_work_bin(a, q, lane);
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

// ---- the hashed class's table: the LDS table's protocol on a slice of global memory that one block owns ----
__device__ __forceinline__ unsigned rec_hash_home(unsigned item) { return (item * 2654435761u) >> (32 - REC_HASH_CAP_LOG2); }

// Slot of `item` in the block's table, or -1 when the table is full (err).  An absent item is claimed -- as a candidate when `live`, the mask and the rules
// admit it, else as a tombstone; *claimed: this lane won the slot and owes the list its entry; *tomb: the slot holds an item that may not be returned.
template <bool RULES>
__device__ __forceinline__ int rec_hash_touch(unsigned* keys, unsigned item, bool live, const uint8_t* __restrict__ mask, bool* claimed, bool* tomb,
                                              unsigned long long* err, const RecArgs& a, int64_t q) {
  unsigned h = rec_hash_home(item);
  for (int probe = 0; probe < REC_HASH_CAP; ++probe) {
    unsigned k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == REC_EMPTY) {
      const bool ok = live && (!mask || mask[item] != 0) && rec_rules_ok<RULES>(a, q, (int32_t)item);
      k = atomicCAS(&keys[h], REC_EMPTY, ok ? item : (item | REC_TOMB));
      if (k == REC_EMPTY) {
        *claimed = true;
        *tomb = !ok;
        return (int)h;
      }
    }
    if ((k & ~REC_TOMB) == item) {
      *tomb = (k & REC_TOMB) != 0;
      return (int)h;
    }
    h = (h + 1) & (REC_HASH_CAP - 1);
  }
  atomicAdd(err, 1ull);
  return -1;
}
// is the item in the block's table (candidate or tombstone)?  The global twin of rec_lds_has.
__device__ __forceinline__ bool rec_hash_has(const unsigned* keys, unsigned item) {
  unsigned h = rec_hash_home(item);
  for (int probe = 0; probe < REC_HASH_CAP; ++probe) {
    const unsigned k = keys[h];
    if (k == REC_EMPTY) return false;
    if ((k & ~REC_TOMB) == item) return true;
    h = (h + 1) & (REC_HASH_CAP - 1);
  }
  return false;
}

// CLASS: 0 = LDS, 1 = dense (global), 2 = hashed
template <int CLASS, bool RULES, bool WEIGHTED>
__global__ __launch_bounds__(REC_THREADS) void rec_rows_kernel(RecArgs a) {
  static_assert(CLASS >= 0 && CLASS <= 2, "0 = LDS, 1 = dense, 2 = hashed");
  constexpr bool LDS = CLASS == 0, DENSE = CLASS == 1, HASHED = CLASS == 2;
  __shared__ unsigned s_keys[LDS ? REC_CAP : 1];
  __shared__ unsigned s_m[LDS ? REC_CAP : 1];
  __shared__ unsigned short s_cand[LDS ? REC_LIMIT : 1];  // slot of every candidate
  __shared__ double s_score[LDS ? REC_LIMIT : 1];         // by candidate ordinal
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
  unsigned* h_keys = HASHED ? a.h.keys + (size_t)blockIdx.x * (size_t)REC_HASH_CAP : nullptr;
  unsigned* h_m = HASHED && !WEIGHTED ? a.h.m + (size_t)blockIdx.x * (size_t)REC_HASH_CAP : nullptr;
  unsigned long long* h_m64 = HASHED && WEIGHTED ? a.h.m64 + (size_t)blockIdx.x * (size_t)REC_HASH_CAP : nullptr;
  int32_t* h_list = HASHED ? a.h.list + (size_t)blockIdx.x * (size_t)REC_HASH_LIMIT : nullptr;
  double* h_score = HASHED ? a.h.score + (size_t)blockIdx.x * (size_t)REC_HASH_LIMIT : nullptr;
  const long long n_mine = (long long)a.ctr[DENSE ? 1 : HASHED ? 5 : 0];
  constexpr unsigned CAND_MAX_FIXED = HASHED ? (unsigned)REC_HASH_LIMIT : (unsigned)REC_LIMIT;  // most candidates of the two table classes

  if (LDS)
    for (int s = tid; s < REC_CAP; s += REC_THREADS) s_m[s] = 0;  // every fold returns the counters to zero

  for (long long at = blockIdx.x; at < n_mine; at += gridDim.x) {
    const int64_t q = DENSE ? a.list[a.n_queries - 1 - at] : HASHED ? a.h.queries[at] : a.list[at];
    if (LDS)
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
      } else if (HASHED) {
        bool claimed = false, tomb = false;
        const int slot = rec_hash_touch<RULES>(h_keys, (unsigned)item, true, mask, &claimed, &tomb, &a.ctr[2], a, q);
        if (slot < 0) return;
        if (claimed) {  // the two ends of the list cannot meet: candidates + tombstones <= w(q) <= REC_HASH_LIMIT
          const unsigned j = atomicAdd(tomb ? &s_ntomb : &s_ncand, 1u);
          if (j >= (unsigned)REC_HASH_LIMIT) {
            atomicAdd(&a.ctr[2], 1ull);
          } else if (tomb) {
            h_list[REC_HASH_LIMIT - 1 - (int32_t)j] = slot;
          } else {
            h_list[j] = slot;
            h_score[j] = 0.0;
          }
        }
        if (!tomb) {
          if (WEIGHTED) atomicAdd(&h_m64[slot], (unsigned long long)wt);
          else atomicAdd(&h_m[slot], 1u);
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
        } else if (HASHED) {
          bool claimed = false, tomb = false;
          const int slot = rec_hash_touch<RULES>(h_keys, (unsigned)item, false, mask, &claimed, &tomb, &a.ctr[2], a, q);
          if (claimed) {
            const unsigned j = atomicAdd(&s_ntomb, 1u);
            if (j < (unsigned)REC_HASH_LIMIT) h_list[REC_HASH_LIMIT - 1 - (int32_t)j] = slot;
            else atomicAdd(&a.ctr[2], 1ull);
          }
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
      const unsigned nc = s_ncand < (DENSE ? (unsigned)n_items : CAND_MAX_FIXED) ? s_ncand : (DENSE ? (unsigned)n_items : CAND_MAX_FIXED);
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
        } else if (HASHED && WEIGHTED) {
          const int32_t slot = h_list[j];
          const unsigned long long m = h_m64[slot];
          if (m) { h_score[j] = h_score[j] + boost * ((double)m * REC_WEIGHT_UNIT); h_m64[slot] = 0; }
        } else if (HASHED) {
          const int32_t slot = h_list[j];
          const unsigned m = h_m[slot];
          if (m) { h_score[j] = h_score[j] + boost * (double)m; h_m[slot] = 0; }
        } else {
          const unsigned slot = s_cand[j];
          const unsigned m = s_m[slot];
          if (m) { s_score[j] = s_score[j] + boost * (WEIGHTED ? (double)m * REC_WEIGHT_UNIT : (double)m); s_m[slot] = 0; }
        }
      }
      __syncthreads();
    }

    const unsigned nc = s_ncand < (DENSE ? (unsigned)n_items : CAND_MAX_FIXED) ? s_ncand : (DENSE ? (unsigned)n_items : CAND_MAX_FIXED);
    auto cand_item = [&](unsigned j) -> int32_t { return DENSE ? g_list[j] : HASHED ? (int32_t)h_keys[h_list[j]] : (int32_t)s_keys[s_cand[j]]; };
    auto cand_score = [&](unsigned j) -> double { return DENSE ? g_score[j] : HASHED ? h_score[j] : s_score[j]; };
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
          if (ok) ok = DENSE ? g_state[item] == 0 : HASHED ? !rec_hash_has(h_keys, (unsigned)item) : !rec_lds_has(s_keys, (unsigned)item);
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
    if (HASHED) {  // leave the table as it was found: through the two ends of the list, never a sweep (the fold left every counter zero)
      for (unsigned j = tid; j < nc; j += REC_THREADS) h_keys[h_list[j]] = REC_EMPTY;
      const unsigned ntomb = s_ntomb < (unsigned)REC_HASH_LIMIT ? s_ntomb : (unsigned)REC_HASH_LIMIT;
      for (unsigned j = tid; j < ntomb; j += REC_THREADS) h_keys[h_list[REC_HASH_LIMIT - 1 - (int32_t)j]] = REC_EMPTY;
    }
    __syncthreads();
  }
}

// ---- the driven class (REC_DRIVEN, decision D32): a block per query answers it from the item list of its driving rule ----
//   gather   the block walks the columns of the driver's CSC that the query's rule row names (a wave per column below 512 entries, the block beyond) and claims
//            every item in the LDS table: the union removes its own duplicates, and d(q) <= REC_DRIVE_LIMIT claims cannot fill the 4096 slots.  The claiming lane
//            alone tests the mask and the rules (all of them: the driving rule costs one short search more, and the predicate stays the one of the other
//            classes) -- a rejected item turns into a tombstone in place, an admitted one is appended to the candidate list.  Meanwhile the query's term rows
//            T_c(q) are staged side by side in LDS when they hold no more than REC_DRV_TERMS entries together.
//   strike   the exclusion row is looked up entry by entry; what is found becomes a tombstone: a blacklist costs probes and no table space.
//   score    a group of 16 lanes per candidate (an indicator row has at most k entries, a property row a handful: a whole wave would idle three quarters of
//            its lanes), lanes over the entries of row i of the CSR of I_c, each entry searched in the sorted T_c(q) -- in LDS or, beyond the staging
//            capacity, in global memory: two instantiations of the body behind one block-uniform branch, so that every load is a ds_read or a global_load.
//            The matches' weights are summed in 64-bit registers and across the group by integer shuffles; lane 0 folds the clauses in call order with the
//            expression of the other classes.  No atomic on a score, no accumulator.  A struck candidate scores -1: dead.
//   select   one sel_kth_largest over the whole list, a dead candidate (struck, or zero under NO_BACKFILL) keyed (0, 0) below every live key ((score bits,
//            ~position), ~position >= 2^31); the live keys at or above the num-th are the winners, ranked by counting.  The zero-score winners ARE the backfill.
constexpr int REC_DRV_TERMS = 4096;                        // staged entries of the query's term rows, all clauses together (16 KiB: the LDS class's s_m)
constexpr int REC_DRV_GROUP = 16;                          // lanes per candidate in the score phase
constexpr int REC_DRV_NG = REC_THREADS / REC_DRV_GROUP;    // candidates per pass
static_assert(REC_DRIVE_LIMIT <= REC_LIMIT, "the driven list lives in the LDS class's table");
static_assert(sizeof(RecArgs) + sizeof(RecDriven) <= 4096, "kernel arguments: both tables travel by value");

// Claim `item` in the table: its slot when this lane inserted it, -1 when it was there (or the table is full: err).
__device__ __forceinline__ int rec_drv_claim(unsigned* keys, unsigned item, unsigned long long* err) {
  unsigned h = rec_hash(item);
  for (int probe = 0; probe < REC_CAP; ++probe) {
    unsigned k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == REC_EMPTY) {
      k = atomicCAS(&keys[h], REC_EMPTY, item);
      if (k == REC_EMPTY) return (int)h;
    }
    if ((k & ~REC_TOMB) == item) return -1;
    h = (h + 1) & (REC_CAP - 1);
  }
  atomicAdd(err, 1ull);
  return -1;
}
// slot of the item in the table, -1 when absent
__device__ __forceinline__ int rec_drv_slot(const unsigned* keys, unsigned item) {
  unsigned h = rec_hash(item);
  for (int probe = 0; probe < REC_CAP; ++probe) {
    const unsigned k = keys[h];
    if (k == REC_EMPTY) return -1;
    if ((k & ~REC_TOMB) == item) return (int)h;
    h = (h + 1) & (REC_CAP - 1);
  }
  return -1;
}
// is `col` in the sorted row of n entries?  IN_LDS picks the one pointer that is read (see sr_unique: never one pointer chosen at run time)
template <bool IN_LDS>
__device__ __forceinline__ bool rec_drv_find(const int32_t* __restrict__ g_row, const int32_t* s_row, int n, int32_t col) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int32_t v = IN_LDS ? s_row[mid] : g_row[mid];
    if (v < col) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && (IN_LDS ? s_row[lo] : g_row[lo]) == col;
}

// The score phase over the nc listed candidates; returns this thread's count of live candidates with a positive score.
template <bool WEIGHTED, bool IN_LDS>
__device__ __forceinline__ unsigned rec_drv_score(const RecArgs& a, const RecDriven& dv, int64_t q, unsigned nc, const unsigned* s_keys, const unsigned short* s_cand,
                                                  double* s_score, const int32_t* s_terms, const int* s_toff) {
  const int grp = threadIdx.x / REC_DRV_GROUP, gl = threadIdx.x & (REC_DRV_GROUP - 1);
  unsigned n_pos = 0;
  for (unsigned j0 = 0; j0 < nc; j0 += REC_DRV_NG) {  // block-uniform: every lane takes part in every shuffle
    const unsigned j = j0 + (unsigned)grp;
    const unsigned key = j < nc ? s_keys[s_cand[j]] : REC_TOMB;
    const bool live = (key & REC_TOMB) == 0;
    const int32_t item = (int32_t)(key & ~REC_TOMB);
    double score = 0.0;
    for (int c = 0; c < a.n_clauses; ++c) {
      const RecClause& cl = a.c[c];
      unsigned long long m = 0;
      if (live) {
        const int64_t tb = cl.q_row_ptr[q];
        const int nt = IN_LDS ? s_toff[c + 1] - s_toff[c] : (int)(cl.q_row_ptr[q + 1] - tb);
        const int32_t* __restrict__ g_row = cl.q_col_idx + tb;
        const int32_t* s_row = s_terms + (IN_LDS ? s_toff[c] : 0);
        const int64_t e = nt > 0 ? dv.rows[c].m_row_ptr[item + 1] : 0;
        for (int64_t t = nt > 0 ? dv.rows[c].m_row_ptr[item] + gl : 0; t < e; t += REC_DRV_GROUP) {
          const int32_t col = dv.rows[c].m_col_idx[t];
          if ((unsigned)col >= (unsigned)cl.n_cols || !rec_drv_find<IN_LDS>(g_row, s_row, nt, col)) continue;
          unsigned wt = 1u;
          if (WEIGHTED) {  // clamped as the other classes clamp it
            wt = a.w[c] ? a.w[c][col] : (unsigned)REC_WEIGHT_ONE;
            wt = wt < 1u ? 1u : wt > (unsigned)REC_WEIGHT_MAX ? (unsigned)REC_WEIGHT_MAX : wt;
          }
          m += wt;
        }
      }
      for (int o = REC_DRV_GROUP / 2; o > 0; o >>= 1) m += shfl_xor_u64(m, o);  // exact, inside the group of 16
      // (the translation unit is compiled with -ffp-contract=off: product, then sum, one rounding each -- the other classes' expression)
      if (m) score = score + cl.boost * (WEIGHTED ? (double)m * REC_WEIGHT_UNIT : (double)m);
    }
    if (gl == 0 && j < nc) {
      s_score[j] = live ? score : -1.0;
      n_pos += live && score > 0.0 ? 1u : 0u;
    }
  }
  return n_pos;
}

template <bool WEIGHTED>
__global__ __launch_bounds__(REC_THREADS) void rec_driven_kernel(RecArgs a, RecDriven dv) {
  __shared__ unsigned s_keys[REC_CAP];
  __shared__ int32_t s_terms[REC_DRV_TERMS];
  __shared__ unsigned short s_cand[REC_LIMIT];  // slot of every candidate
  __shared__ double s_score[REC_LIMIT];         // by candidate ordinal; -1: struck by the exclusion row
  __shared__ SelScratch s_select;
  __shared__ unsigned s_ncand, s_ngath, s_npos, s_nwin;
  __shared__ int s_toff[REC_MAX_CLAUSES + 1];   // start of every clause's staged row; s_staged: they all fit
  __shared__ int s_staged;
  __shared__ double s_wscore[REC_MAX_NUM];
  __shared__ int32_t s_wpos[REC_MAX_NUM];
  __shared__ int32_t s_witem[REC_MAX_NUM];

  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int32_t n_items = a.n_items;
  const int num = a.num;
  const uint8_t* __restrict__ mask = a.item_mask;
  const int32_t* __restrict__ pos_of = a.pos;
  const bool no_backfill = (a.flags & REC_NO_BACKFILL) != 0;
  const long long n_mine = (long long)a.ctr[6];

  for (long long at = blockIdx.x; at < n_mine; at += gridDim.x) {
    const int64_t q = dv.queries[at];
    for (int s = tid; s < REC_CAP; s += REC_THREADS) s_keys[s] = REC_EMPTY;
    if (tid == 0) {
      s_ncand = 0; s_ngath = 0; s_npos = 0; s_nwin = 0;
      long long total = 0;
      s_toff[0] = 0;
      for (int c = 0; c < a.n_clauses; ++c) {
        total += a.c[c].q_row_ptr[q + 1] - a.c[c].q_row_ptr[q];
        s_toff[c + 1] = total <= REC_DRV_TERMS ? (int)total : REC_DRV_TERMS;
      }
      s_staged = total <= REC_DRV_TERMS ? 1 : 0;
    }
    __syncthreads();

    // ---- gather: the union of the driver's columns, eligibility by the claiming lane ----
    const RecDriver& drv = dv.d[dv.driver_of[q]];
    const RecRule& dr = a.r[drv.rule];
    const int64_t vb = dr.q_row_ptr[q], nv = dr.q_row_ptr[q + 1] - vb;
    unsigned gathered = 0;
    auto claim = [&](int32_t item) {
      if ((unsigned)item >= (unsigned)n_items) return;
      const int slot = rec_drv_claim(s_keys, (unsigned)item, &a.ctr[2]);
      if (slot < 0) return;
      ++gathered;
      if ((!mask || mask[item] != 0) && rec_rules_ok<true>(a, q, item)) {
        const unsigned j = atomicAdd(&s_ncand, 1u);
        if (j < (unsigned)REC_LIMIT) s_cand[j] = (unsigned short)slot;
        else atomicAdd(&a.ctr[2], 1ull);
      } else {
        __hip_atomic_store(&s_keys[slot], (unsigned)item | REC_TOMB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    };
    for (int64_t t = 0; t < nv; ++t) {  // short columns: a wave per column; long ones: the whole block
      const int32_t v = dr.q_col_idx[vb + t];
      if ((unsigned)v >= (unsigned)dr.n_cols) continue;
      const int64_t s = drv.m_col_ptr[v], e = drv.m_col_ptr[v + 1];
      if (e - s >= 2 * REC_THREADS) {
        for (int64_t p = s + tid; p < e; p += REC_THREADS) claim(drv.m_row_idx[p]);
      } else if ((int)(t & (REC_NW - 1)) == wave) {
        for (int64_t p = s + lane; p < e; p += WAVE) claim(drv.m_row_idx[p]);
      }
    }
    if (gathered) atomicAdd(&s_ngath, gathered);
    const bool staged = s_staged != 0;
    if (staged)
      for (int c = 0; c < a.n_clauses; ++c) {
        const int32_t* __restrict__ row = a.c[c].q_col_idx + a.c[c].q_row_ptr[q];
        const int off = s_toff[c], n = s_toff[c + 1] - off;
        for (int x = tid; x < n; x += REC_THREADS) s_terms[off + x] = row[x];
      }
    __syncthreads();

    // ---- strike: the exclusion row against the table ----
    if (a.excl_row_ptr) {
      const int64_t e = a.excl_row_ptr[q + 1];
      for (int64_t t = a.excl_row_ptr[q] + tid; t < e; t += REC_THREADS) {
        const int32_t item = a.excl_col_idx[t];
        if ((unsigned)item >= (unsigned)n_items) continue;
        const int slot = rec_drv_slot(s_keys, (unsigned)item);
        if (slot >= 0) s_keys[slot] = (unsigned)item | REC_TOMB;  // (twice in the row: the same word twice)
      }
      __syncthreads();
    }

    // ---- score: every candidate from its own rows ----
    const unsigned nc = s_ncand < (unsigned)REC_LIMIT ? s_ncand : (unsigned)REC_LIMIT;
    const unsigned n_pos = staged ? rec_drv_score<WEIGHTED, true>(a, dv, q, nc, s_keys, s_cand, s_score, s_terms, s_toff)
                                  : rec_drv_score<WEIGHTED, false>(a, dv, q, nc, s_keys, s_cand, s_score, s_terms, s_toff);
    if (n_pos) atomicAdd(&s_npos, n_pos);
    __syncthreads();

    auto dead = [&](unsigned j) -> bool { const double sc = s_score[j]; return sc < 0.0 || (no_backfill && !(sc > 0.0)); };
    auto cand_pos = [&](unsigned j) -> int32_t {
      const int32_t item = (int32_t)(s_keys[s_cand[j]] & ~REC_TOMB);
      return pos_of ? pos_of[item] : item;
    };
    // ---- selection: the num-th largest key of the list, dead candidates at (0, 0) ----
    SelKey thr{0ull, 0u};
    if (nc > (unsigned)num)
      thr = sel_kth_largest<REC_THREADS>(
          nc, (unsigned)num, [&](unsigned j) { return dead(j) ? 0ull : (unsigned long long)__double_as_longlong(s_score[j]); },
          [&](unsigned j) { return dead(j) ? 0u : ~(unsigned)cand_pos(j); }, SelKey{~0ull, ~0u}, SelKey{0ull, 0u}, s_select);
    const unsigned long long thi = thr.hi;
    const unsigned tlo = thr.lo;
    // ---- winners (at most num: the live keys are distinct), ranked by counting ----
    for (unsigned j = tid; j < nc; j += REC_THREADS) {
      if (dead(j)) continue;
      const double sc = s_score[j];
      const unsigned long long hi = (unsigned long long)__double_as_longlong(sc);
      if (hi < thi) continue;
      const int32_t p = cand_pos(j);
      if (hi == thi && ~(unsigned)p < tlo) continue;
      const unsigned w = atomicAdd(&s_nwin, 1u);
      if (w < (unsigned)REC_MAX_NUM) { s_wscore[w] = sc; s_wpos[w] = p; s_witem[w] = (int32_t)(s_keys[s_cand[j]] & ~REC_TOMB); }
    }
    __syncthreads();
    const unsigned nw = s_nwin < (unsigned)num ? s_nwin : (unsigned)num;  // (more only if fill_order is no permutation)
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
    if (tid == 0) {
      a.out_count[q] = (int32_t)nw;
      atomicAdd(&a.ctr[3], (unsigned long long)s_npos);
      atomicAdd(&a.ctr[7], (unsigned long long)s_ngath);
    }
    __syncthreads();
  }
}

__global__ void rec_stats_kernel(const unsigned long long* __restrict__ ctr, int64_t* __restrict__ stats) {
  const int t = threadIdx.x;
  // ctr[5]: queries of the hashed class (0 with the class off); ctr[6], ctr[7]: queries of the driven class and the items they gathered (0 without drivers)
  if (t < REC_STATS_LEN) stats[t] = (int64_t)ctr[t];
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

// resident blocks of the hashed class: a slice is keys + m (4 bytes a slot; weighted: m64, 8) + list (4) + score (8) per REC_HASH_LIMIT entries -- 2.125 MiB, or
// 2.625 MiB weighted -- at most 512 MiB in all: 240 blocks, 195 weighted.  The catalogue's size is not in the formula.
size_t recommend_hashed_block_bytes(bool weighted) { return (size_t)REC_HASH_CAP * (weighted ? 12 : 8) + (size_t)REC_HASH_LIMIT * 12; }
int32_t recommend_hashed_blocks(int64_t n_queries, int n_cu, bool weighted) {
  int64_t blocks = ((int64_t)512 << 20) / (int64_t)recommend_hashed_block_bytes(weighted);
  if (blocks > 2 * (int64_t)n_cu) blocks = 2 * (int64_t)n_cu;
  if (blocks > n_queries) blocks = n_queries;
  return (int32_t)(blocks < 1 ? 1 : blocks);
}

hipError_t launch_recommend(hipStream_t st, int n_cu, int64_t n_queries, int32_t n_items, const RecClause* clauses, int32_t n_clauses, const int64_t* excl_row_ptr,
                            const int32_t* excl_col_idx, const uint8_t* item_mask, const int32_t* fill_order, int32_t num, int32_t flags, int32_t* out_count,
                            int32_t* out_idx, double* out_score, int64_t* stats_dev, unsigned long long* ctr, int32_t* list, int32_t* pos, int32_t g_blocks,
                            unsigned* g_state, unsigned* g_m, int32_t* g_list, double* g_score, int32_t lds_limit, const RecRule* rules, int32_t n_rules,
                            const uint32_t* const* weights, unsigned long long* g_m64, const RecHashed* hashed, const RecDriven* driven) {
  const bool weighted = weights != nullptr;  // then g_m64 is the counter array of the global class and g_m is not read
  RecArgs a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < n_clauses; ++c) a.c[c] = clauses[c];
  for (int j = 0; j < n_rules; ++j) a.r[j] = rules[j];
  a.n_rules = n_rules;
  if (weighted)
    for (int c = 0; c < n_clauses; ++c) a.w[c] = weights[c];
  a.g_m64 = g_m64;
  if (hashed) {
    a.h = *hashed;
    if (a.h.limit > REC_HASH_LIMIT) a.h.limit = REC_HASH_LIMIT;
  }
  a.n_queries = n_queries; a.n_items = n_items; a.n_clauses = n_clauses; a.num = num; a.flags = flags;
  a.lds_limit = lds_limit < REC_LIMIT ? lds_limit : REC_LIMIT;
  a.excl_row_ptr = excl_row_ptr; a.excl_col_idx = excl_col_idx; a.item_mask = item_mask; a.fill_order = fill_order;
  a.pos = fill_order ? pos : nullptr;
  a.list = list; a.ctr = ctr; a.out_count = out_count; a.out_idx = out_idx; a.out_score = out_score;
  a.g_state = g_state; a.g_m = g_m; a.g_list = g_list; a.g_score = g_score; a.g_blocks = g_blocks;
  hipError_t e = hipMemsetAsync(ctr, 0, 8 * sizeof(unsigned long long), st);
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
    if (hashed) {  // once per call: every query leaves its slice as it found it
      const size_t slots = (size_t)a.h.blocks * (size_t)REC_HASH_CAP;
      if ((e = hipMemsetAsync(a.h.keys, 0xff, slots * sizeof(unsigned), st)) != hipSuccess) return e;
      if ((e = weighted ? hipMemsetAsync(a.h.m64, 0, slots * sizeof(unsigned long long), st) : hipMemsetAsync(a.h.m, 0, slots * sizeof(unsigned), st)) != hipSuccess) return e;
    }
    int64_t wb = (n_queries + REC_NW - 1) / REC_NW;
    if (wb > (int64_t)n_cu * 8) wb = (int64_t)n_cu * 8;
    const int64_t lb = n_queries < (int64_t)n_cu * 2 ? n_queries : (int64_t)n_cu * 2;  // the LDS table lets two blocks share a CU
    if (driven && n_rules > 0 && driven->n_drivers > 0) {  // the driven queries leave the binning first and are answered by a kernel of their own
      RecDriven dv = *driven;
      if (dv.limit > REC_DRIVE_LIMIT) dv.limit = REC_DRIVE_LIMIT;
      hipLaunchKernelGGL(rec_work_driven_kernel, dim3((unsigned)wb), dim3(REC_THREADS), 0, st, a, dv);
      if (weighted) hipLaunchKernelGGL((rec_driven_kernel<true>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a, dv);
      else hipLaunchKernelGGL((rec_driven_kernel<false>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a, dv);
    } else {
      hipLaunchKernelGGL(rec_work_kernel, dim3((unsigned)wb), dim3(REC_THREADS), 0, st, a);
    }
    if (weighted && n_rules > 0) {
      hipLaunchKernelGGL((rec_rows_kernel<0, true, true>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      if (hashed) hipLaunchKernelGGL((rec_rows_kernel<2, true, true>), dim3((unsigned)a.h.blocks), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<1, true, true>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    } else if (weighted) {
      hipLaunchKernelGGL((rec_rows_kernel<0, false, true>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      if (hashed) hipLaunchKernelGGL((rec_rows_kernel<2, false, true>), dim3((unsigned)a.h.blocks), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<1, false, true>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    } else if (n_rules > 0) {
      hipLaunchKernelGGL((rec_rows_kernel<0, true, false>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      if (hashed) hipLaunchKernelGGL((rec_rows_kernel<2, true, false>), dim3((unsigned)a.h.blocks), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<1, true, false>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    } else {
      hipLaunchKernelGGL((rec_rows_kernel<0, false, false>), dim3((unsigned)lb), dim3(REC_THREADS), 0, st, a);
      if (hashed) hipLaunchKernelGGL((rec_rows_kernel<2, false, false>), dim3((unsigned)a.h.blocks), dim3(REC_THREADS), 0, st, a);
      hipLaunchKernelGGL((rec_rows_kernel<1, false, false>), dim3((unsigned)g_blocks), dim3(REC_THREADS), 0, st, a);
    }
  }
  if (stats_dev) hipLaunchKernelGGL(rec_stats_kernel, dim3(1), dim3(64), 0, st, ctr, stats_dev);
  return hipGetLastError();
}

}  // namespace urcco
