// cco_quota.h -- the quota rule (urcco_dev_quota_cut): a post-pass over a result table that keeps, row by row and in result order, the first num
// candidates such that no value of a rule's property is held by more than that rule's max_per_value kept items (decision D34).  Included once,
// from cco_misc.hip, behind cco_audience.h.  The selection is greedy in result order, so sequential by definition; here a wave decides 64 candidates at a
// time and gives the sequential answer exactly.  When out_short[r] == 0 the row equals the answer over an unbounded pool; nothing beyond that is claimed.
//
//   quota_init_kernel   one wave: the header and the statistics (no memset is recorded).
//   quota_plan_kernel   a wave per row: the total value count of every candidate over the call's rules; the first candidate above QUOTA_MAX_VALUES is
//                       reported in the header, which the host reads -- the call's one synchronisation.
//   quota_cut_lds_kernel, quota_cut_global_kernel   quota_row<false> and quota_row<true>: four waves a block, a wave per row, grid-striding.
//     table             per wave an open-addressing table keyed (rule << 32 | value): one 64-bit word holds the key above a 16-bit count of the kept items
//                       with the value, a second word the 64-bit set of the round's lanes that hold it (`pend`).  false: 1024 slots a wave in LDS -- 16 KiB
//                       a wave, 64 KiB a block, two blocks a CU; true: up to 2^16 slots per resident wave in arena scratch, sized by the row.  Two
//                       compile-time instantiations of one body: every table access is a ds_* or a global_* instruction, none a flat one.
//     a round           the next 64 candidates, lane l candidate l.  Every lane claims its keys and sets its bit in their lane sets; then the lanes iterate:
//                         rejected   one of its keys stands at its rule's maximum,
//                         admitted   for each of its keys, count + |lane set & undecided lanes & lanes below| < maximum,
//                         undecided  otherwise;
//                       the admitted lanes raise their keys' counts after every lane has read.  The lowest undecided lane has nobody undecided below it:
//                       its bound is exact, an iteration decides it at least -- at most 64 iterations, one or two on real data.  A later lane is only
//                       admitted with every earlier undecided holder of its keys counted in, so no admission takes room from an earlier lane, and a
//                       count reaches a maximum while an earlier lane is undecided only through lanes before that one: both verdicts are the sequential
//                       walk's.  After the round the kept lanes are ranked by ballot and popcount: the rank is the output position and cuts the row at
//                       num; no atomic touches the output.  The lane sets are cleared through the lanes' own keys.
//     overflow (LDS)    the values of the rounds walked so far, repeats included, exceed 3/4 of the slots: the row is appended to the overflow list -- the
//                       one atomic between waves -- and the GLOBAL instantiation, launched behind, redoes it from its start and writes all of its outputs again.
//   No spin, lock or flag between blocks; no float arithmetic: the scores travel as 64-bit words.
#pragma once

namespace urcco {

constexpr int QUOTA_THREADS = 256;
constexpr int QUOTA_NW = QUOTA_THREADS / WAVE;
constexpr int QUOTA_COUNT_BITS = 16;
constexpr unsigned long long QUOTA_EMPTY = ~0ull;  // no key: a key lies below 2^34
static_assert((QUOTA_LDS_SLOTS & (QUOTA_LDS_SLOTS - 1)) == 0 && (QUOTA_GLOBAL_SLOTS & (QUOTA_GLOBAL_SLOTS - 1)) == 0, "power-of-two tables");
static_assert((long long)REC_MAX_NUM * QUOTA_MAX_VALUES * 4 <= (long long)QUOTA_GLOBAL_SLOTS * 3, "a full row of the widest items fits the global table at load 3/4");
static_assert(REC_MAX_NUM < (1 << QUOTA_COUNT_BITS) && QUOTA_MAX_RULES <= 4, "the count of a slot, two bits of rule above the value");

struct QuotaTally { unsigned long long rows, examined, rejected, iters, shorts; };

__device__ __forceinline__ unsigned quota_hash(unsigned long long key, unsigned mask) {
  const unsigned x = (unsigned)key * 2654435761u + (unsigned)(key >> 32) * 0x85ebca6bu;
  return (x ^ (x >> 15)) & mask;
}
// table words are read and written as relaxed atomics: in arena scratch the lanes of a wave meet in the L2, where the read-modify-writes execute
__device__ __forceinline__ unsigned long long quota_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void quota_st(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot of `key`, claimed when absent; -1: no free slot (excluded by the load bound)
__device__ __forceinline__ int quota_claim(unsigned long long* slot, unsigned slots, unsigned long long key) {
  unsigned h = quota_hash(key, slots - 1u);
  for (unsigned probe = 0; probe < slots; ++probe) {
    const unsigned long long k = atomicCAS(&slot[h], QUOTA_EMPTY, key << QUOTA_COUNT_BITS);
    if (k == QUOTA_EMPTY || (k >> QUOTA_COUNT_BITS) == key) return (int)h;
    h = (h + 1u) & (slots - 1u);
  }
  return -1;
}
// the slot of a key that was claimed; -1: absent
__device__ __forceinline__ int quota_find(const unsigned long long* slot, unsigned slots, unsigned long long key) {
  unsigned h = quota_hash(key, slots - 1u);
  for (unsigned probe = 0; probe < slots; ++probe) {
    const unsigned long long k = quota_ld(&slot[h]);
    if ((k >> QUOTA_COUNT_BITS) == key) return (int)h;
    if (k == QUOTA_EMPTY) return -1;
    h = (h + 1u) & (slots - 1u);
  }
  return -1;
}

// f(rule, key) over the values item holds under every rule, until it returns false
template <typename F>
__device__ __forceinline__ void quota_keys(const QuotaArgs& a, int32_t item, F&& f) {
  for (int q = 0; q < a.n_rules; ++q) {
    const int64_t e = a.rule[q].row_ptr[item + 1];
    for (int64_t p = a.rule[q].row_ptr[item]; p < e; ++p)
      if (!f(q, ((unsigned long long)(unsigned)q << 32) | (unsigned long long)(unsigned)a.rule[q].col_idx[p])) return;
  }
}
// the values item holds under all rules together
__device__ __forceinline__ unsigned quota_values(const QuotaArgs& a, int32_t item) {
  long long n = 0;
  for (int q = 0; q < a.n_rules; ++q) {
    const long long d = a.rule[q].row_ptr[item + 1] - a.rule[q].row_ptr[item];
    n += d > 0 ? d : 0;
  }
  return n > 0x7fffffffll ? 0x7fffffffu : (unsigned)n;
}
__device__ __forceinline__ unsigned long long quota_wave_sum(unsigned long long v) {
  for (int o = WAVE / 2; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
  return v;
}
__device__ __forceinline__ int quota_row_len(const QuotaArgs& a, int64_t r) {
  const int n = a.in_count[r];
  return n < 0 ? 0 : n > a.width ? a.width : n;
}

// One row, one wave.  false (LDS tier only): the row does not fit the table; nothing is tallied, and what was written is written again by the other tier.
template <bool GLOBAL>
__device__ __forceinline__ bool quota_row(const QuotaArgs& a, int64_t r, unsigned long long* slot, unsigned long long* pend, unsigned slots, int lane,
                                          QuotaTally& t) {
  const int width = a.width, num = a.num, n = quota_row_len(a, r);
  const int32_t* idx = a.in_idx + (size_t)r * (size_t)width;
  const unsigned long long* score = a.in_score + (size_t)r * (size_t)width;
  int32_t* o_idx = a.out_idx + (size_t)r * (size_t)num;
  unsigned long long* o_score = a.out_score + (size_t)r * (size_t)num;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned limit = slots / 4u * 3u;
  for (unsigned h = (unsigned)lane; h < slots; h += WAVE) {
    quota_st(&slot[h], QUOTA_EMPTY);
    quota_st(&pend[h], 0ull);
  }
  expl_wave_sync();
  int total = 0;
  unsigned long long used = 0ull, examined = 0ull, rejected = 0ull, iters = 0ull;
  for (int base = 0; base < n && total < num; base += WAVE) {  // wave-uniform
    const int j = base + lane;
    const bool valid = j < n;
    const int32_t item = valid ? idx[j] : -1;
    const bool live = valid && (unsigned)item < (unsigned)a.n_items;  // an index outside the catalogue is never kept
    used += quota_wave_sum(live ? (unsigned long long)quota_values(a, item) : 0ull);
    if (!GLOBAL && used > (unsigned long long)limit) return false;
    int state = live ? 0 : 2;  // 0 undecided, 1 kept, 2 rejected
    if (live)
      quota_keys(a, item, [&](int, unsigned long long key) {
        const int h = quota_claim(slot, slots, key);
        if (h < 0) { state = 2; return false; }
        atomicOr(&pend[h], 1ull << lane);
        return true;
      });
    expl_wave_sync();
    unsigned long long undecided = __ballot(state == 0 ? 1 : 0);
    while (undecided) {  // wave-uniform
      ++iters;
      int next = state;
      if (state == 0) {
        next = 1;
        quota_keys(a, item, [&](int q, unsigned long long key) {
          const int h = quota_find(slot, slots, key);
          const unsigned long long most = (unsigned long long)a.rule[q].max_per_value;
          const unsigned long long c = h < 0 ? most : quota_ld(&slot[h]) & ((1ull << QUOTA_COUNT_BITS) - 1ull);
          if (c >= most) { next = 2; return false; }
          if (c + (unsigned long long)__popcll(quota_ld(&pend[h]) & undecided & below) >= most) next = 0;
          return true;
        });
      }
      expl_wave_sync();  // every count is read before one is raised
      if (state == 0 && next == 1)
        quota_keys(a, item, [&](int, unsigned long long key) {
          const int h = quota_find(slot, slots, key);
          if (h >= 0) atomicAdd(&slot[h], 1ull);
          return true;
        });
      state = next;
      expl_wave_sync();
      undecided = __ballot(state == 0 ? 1 : 0);
    }
    const unsigned long long kept = __ballot(state == 1 ? 1 : 0), cand = __ballot(valid ? 1 : 0);
    const int rank = __popcll(kept & below), n_kept = __popcll(kept);
    int seen = __popcll(cand);  // candidates the sequential walk examines in this round: up to the one that fills the row
    const unsigned long long filler = __ballot(state == 1 && total + rank == num - 1 ? 1 : 0);
    if (filler) seen = __ffsll(filler);
    if (state == 1 && total + rank < num) {
      o_idx[total + rank] = item;
      o_score[total + rank] = score[j];
    }
    const unsigned long long walked = seen >= WAVE ? ~0ull : (1ull << seen) - 1ull;
    examined += (unsigned long long)seen;
    rejected += (unsigned long long)__popcll(cand & ~kept & walked);
    total = total + n_kept < num ? total + n_kept : num;
    if (total < num && base + WAVE < n) {  // another round follows: its lane sets start empty
      if (live)
        quota_keys(a, item, [&](int, unsigned long long key) {
          const int h = quota_find(slot, slots, key);
          if (h >= 0) quota_st(&pend[h], 0ull);
          return true;
        });
      expl_wave_sync();
    }
  }
  for (int p = total + lane; p < num; p += WAVE) {
    o_idx[p] = -1;
    o_score[p] = 0ull;
  }
  const bool is_short = total < num && n == width;  // a full pool that did not fill the row: a wider one might
  if (lane == 0) {
    a.out_count[r] = total;
    if (a.out_short) a.out_short[r] = is_short ? 1 : 0;
  }
  t.rows += 1ull;
  t.examined += examined;
  t.rejected += rejected;
  t.iters += iters;
  t.shorts += is_short ? 1ull : 0ull;
  return true;
}

__device__ __forceinline__ void quota_tally(const QuotaArgs& a, const QuotaTally& t, int tier, int lane) {
  if (lane != 0 || !t.rows) return;
  atomicAdd(&a.stats[tier], t.rows);
  atomicAdd(&a.stats[QUOTA_STAT_EXAMINED], t.examined);
  atomicAdd(&a.stats[QUOTA_STAT_REJECTED], t.rejected);
  atomicAdd(&a.stats[QUOTA_STAT_ITERATIONS], t.iters);
  atomicAdd(&a.stats[QUOTA_STAT_SHORT], t.shorts);
}

__global__ __launch_bounds__(WAVE) void quota_init_kernel(QuotaArgs a) {
  const int tid = threadIdx.x;
  if (tid < QUOTA_STATS_LEN) a.stats[tid] = 0ull;
  if (tid < QUOTA_HDR_LEN) a.hdr[tid] = tid == QUOTA_HDR_BAD ? ~0ull : 0ull;
}

__global__ __launch_bounds__(QUOTA_THREADS) void quota_plan_kernel(QuotaArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * QUOTA_NW;
  unsigned long long bad = ~0ull;
  for (int64_t r = (int64_t)blockIdx.x * QUOTA_NW + threadIdx.x / WAVE; r < a.n_rows; r += n_waves) {
    const int n = quota_row_len(a, r);
    for (int j = lane; j < n; j += WAVE) {
      const int32_t item = a.in_idx[(size_t)r * (size_t)a.width + (size_t)j];
      if ((unsigned)item >= (unsigned)a.n_items || quota_values(a, item) <= (unsigned)QUOTA_MAX_VALUES) continue;
      const unsigned long long at = ((unsigned long long)r << 8) | (unsigned long long)j;  // width <= 256
      bad = at < bad ? at : bad;
    }
  }
  if (bad != ~0ull) atomicMin(&a.hdr[QUOTA_HDR_BAD], bad);
}

__global__ __launch_bounds__(QUOTA_THREADS) void quota_cut_lds_kernel(QuotaArgs a) {
  __shared__ unsigned long long s_slot[QUOTA_NW][QUOTA_LDS_SLOTS];
  __shared__ unsigned long long s_pend[QUOTA_NW][QUOTA_LDS_SLOTS];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
  const int64_t n_waves = (int64_t)gridDim.x * QUOTA_NW;
  QuotaTally t{0ull, 0ull, 0ull, 0ull, 0ull};
  for (int64_t r = (int64_t)blockIdx.x * QUOTA_NW + wave; r < a.n_rows; r += n_waves) {  // wave-uniform
    if (quota_row<false>(a, r, s_slot[wave], s_pend[wave], (unsigned)a.lds_slots, lane, t)) continue;
    if (lane == 0) a.ovf_rows[atomicAdd(&a.hdr[QUOTA_HDR_OVERFLOWS], 1ull)] = (int32_t)r;
  }
  quota_tally(a, t, QUOTA_STAT_LDS_ROWS, lane);
}

__global__ __launch_bounds__(QUOTA_THREADS) void quota_cut_global_kernel(QuotaArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t gw = (int64_t)blockIdx.x * QUOTA_NW + __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
  const int64_t n_waves = (int64_t)gridDim.x * QUOTA_NW;  // == a.g_waves, rounded up to whole blocks
  const int64_t n_ovf = (int64_t)a.hdr[QUOTA_HDR_OVERFLOWS];
  if (gw >= a.g_waves) return;
  unsigned long long* slot = a.g_slot + (size_t)gw * QUOTA_GLOBAL_SLOTS;
  unsigned long long* pend = a.g_pend + (size_t)gw * QUOTA_GLOBAL_SLOTS;
  QuotaTally t{0ull, 0ull, 0ull, 0ull, 0ull};
  for (int64_t w = gw; w < n_ovf; w += n_waves) {  // wave-uniform
    const int64_t r = a.ovf_rows[w];
    const int n = quota_row_len(a, r);
    unsigned long long values = 0ull;  // the table is sized by the row: what is cleared is what can be used
    for (int j = lane; j < n; j += WAVE) {
      const int32_t item = a.in_idx[(size_t)r * (size_t)a.width + (size_t)j];
      if ((unsigned)item < (unsigned)a.n_items) values += (unsigned long long)quota_values(a, item);
    }
    values = quota_wave_sum(values);
    unsigned slots = WAVE;
    while (slots < (unsigned)QUOTA_GLOBAL_SLOTS && (unsigned long long)(slots / 4u * 3u) < values) slots <<= 1;
    quota_row<true>(a, r, slot, pend, slots, lane, t);
  }
  quota_tally(a, t, QUOTA_STAT_GLOBAL_ROWS, lane);
}

hipError_t launch_quota_plan(hipStream_t st, int n_cu, const QuotaArgs& a) {
  hipLaunchKernelGGL(quota_init_kernel, dim3(1), dim3(WAVE), 0, st, a);
  int64_t blocks = (a.n_rows + QUOTA_NW - 1) / QUOTA_NW;
  if (blocks > (int64_t)n_cu * 8) blocks = (int64_t)n_cu * 8;
  hipLaunchKernelGGL(quota_plan_kernel, dim3((unsigned)blocks), dim3(QUOTA_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_quota_cut(hipStream_t st, int n_cu, const QuotaArgs& a) {
  int64_t blocks = (a.n_rows + QUOTA_NW - 1) / QUOTA_NW;
  if (blocks > (int64_t)n_cu * 2) blocks = (int64_t)n_cu * 2;  // the LDS tables leave two blocks a CU
  hipLaunchKernelGGL(quota_cut_lds_kernel, dim3((unsigned)blocks), dim3(QUOTA_THREADS), 0, st, a);
  hipLaunchKernelGGL(quota_cut_global_kernel, dim3((unsigned)((a.g_waves + QUOTA_NW - 1) / QUOTA_NW)), dim3(QUOTA_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace urcco
