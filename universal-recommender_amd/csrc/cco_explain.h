// cco_explain.h -- the terms behind a score (urcco_dev_explain): for every slot (q, j) of a strided top-num table, as urcco_dev_recommend leaves it, the exact
// per-clause sums M_c(q, i) = sum of w_c[h] over the entries h of row i of I_c that lie in T_c(q), and the best max_terms matches in the total order
// (contribution desc, clause asc, term asc), contribution = boost_c * ((double)w_c[h] * 2^-15) (decision D30).  Included once, from cco_misc.hip,
// behind cco_eval.h.  rec_rows_kernel cannot deliver this: it folds every hit of an item into one counter and forgets the term.
//
//   explain_kernel   a block of 256 threads per query (grid-stride), a wave per result slot (j = wave, wave + 4, ...).
//     query terms    the block reads the clause row bounds, thread 0 sums L(q) = sum_c |T_c(q)|; L(q) <= EXPL_LDS_TERMS: the term rows of all clauses are
//                    staged once, concatenated, in LDS (s_terms, per-clause offsets s_off) and every search of the block's num slots reads LDS; otherwise
//                    the same body (expl_slot<false>) searches the rows where they lie.  A block-uniform branch: no pre-pass, no second list.
//     row walk       per clause the item's row of I_c goes through the wave 64 entries a round: one coalesced load of the columns, one binary search per
//                    lane, a ballot of the hits; a lane adds its own weights into a 64-bit integer, one xor-reduction per clause that had a hit gives M_c.
//     top max_terms  the hits are appended by ballot prefix to the wave's LDS buffer of EXPL_BUF = 128 keys (contribution bits; clause << 32 | term).  Only
//                    when a round would overflow it is the buffer pruned to its best max_terms -- by counting ranks, the slot number breaking ties of
//                    equal keys so that the ranks are a permutation; at that point it holds more than 64 >= max_terms keys, so exactly max_terms stay and
//                    the round's at most 64 hits fit.  One last ranking writes the outputs in order: a result with at most 128 matches is ranked once.
//   LDS: 32 KiB of terms + 4 x 2 KiB of keys + the clause table.  Integer sums, no atomics at all: every output is reproducible bit for bit.
//   Cost per query: num x sum_c len(row i of I_c) searches of log2 |T_c(q)| steps, plus n^2 / 64 compares per ranking of n keys.
#pragma once

namespace urcco {

constexpr int EXPL_THREADS = 256;
constexpr int EXPL_NW = EXPL_THREADS / WAVE;
constexpr int EXPL_LDS_TERMS = 8192;  // L(q) up to here: the query's term rows are staged in LDS
constexpr int EXPL_BUF = 2 * WAVE;    // keys a wave collects before it prunes
static_assert(EXPLAIN_MAX_TERMS <= WAVE, "a pruned buffer and one round of hits fit EXPL_BUF");
static_assert(sizeof(ExplArgs) <= 4096, "kernel arguments: the clause table travels by value");

// LDS hand-off inside one wave: its DS operations execute in program order, a compiler-level fence is all a write needs before another lane's read
__device__ __forceinline__ void expl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// keys of the buffer that come before key e = (kh, kl) in the order (contribution desc, clause asc, term asc, slot asc)
__device__ __forceinline__ int expl_rank(const unsigned long long* hi, const unsigned long long* lo, int n, int e, unsigned long long kh, unsigned long long kl) {
  int r = 0;
  for (int f = 0; f < n; ++f) {  // every lane reads the same word: LDS broadcasts
    const unsigned long long fh = hi[f], fl = lo[f];
    r += (fh > kh || (fh == kh && (fl < kl || (fl == kl && f < e)))) ? 1 : 0;
  }
  return r;
}

// the best `keep` of the n buffered keys move to the slots 0 .. keep - 1 (n > keep); all reads lie before the first write
__device__ __forceinline__ void expl_prune(unsigned long long* hi, unsigned long long* lo, int n, int keep, int lane) {
  expl_wave_sync();
  unsigned long long kh[2] = {0ull, 0ull}, kl[2] = {0ull, 0ull};
  int r[2];
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int e = lane + x * WAVE;
    r[x] = keep;
    if (e < n) {
      kh[x] = hi[e];
      kl[x] = lo[e];
      r[x] = expl_rank(hi, lo, n, e, kh[x], kl[x]);
    }
  }
  expl_wave_sync();
#pragma unroll
  for (int x = 0; x < 2; ++x)
    if (r[x] < keep) {
      hi[r[x]] = kh[x];
      lo[r[x]] = kl[x];
    }
  expl_wave_sync();
}

// One result slot, one wave.  STAGED: the term rows lie in s_terms at s_off[c]; else in global memory at q_col_idx + s_qb[c].  s_ql[c] = |T_c(q)|.
template <bool STAGED>
__device__ __forceinline__ void expl_slot(const ExplArgs& a, int64_t slot, int32_t item, const int32_t* s_terms, const int* s_off, const long long* s_qb,
                                          const long long* s_ql, unsigned long long* b_hi, unsigned long long* b_lo, int lane) {
  int n_buf = 0;        // keys in the buffer; wave-uniform, like everything that steers a loop here
  long long total = 0;  // matches over all clauses
  for (int c = 0; c < a.n_clauses; ++c) {
    const ExplClause& cl = a.c[c];
    const long long ql = s_ql[c];
    unsigned long long m = 0ull;
    bool any = false;
    if (ql > 0 && cl.n_cols > 0) {
      const int64_t re = cl.m_row_ptr[item + 1];
      const double boost = cl.boost;
      for (int64_t p0 = cl.m_row_ptr[item]; p0 < re; p0 += WAVE) {
        const int64_t p = p0 + lane;
        bool hit = false;
        int32_t col = -1;
        if (p < re) {
          col = cl.m_col_idx[p];
          if ((unsigned)col < (unsigned)cl.n_cols) {  // first term >= col
            if (STAGED) {
              const int32_t* t = s_terms + s_off[c];
              int lo = 0, hi = (int)ql;
              while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (t[mid] < col) lo = mid + 1; else hi = mid;
              }
              hit = lo < (int)ql && t[lo] == col;
            } else {
              const int32_t* __restrict__ t = cl.q_col_idx + s_qb[c];
              long long lo = 0, hi = ql;
              while (lo < hi) {
                const long long mid = lo + ((hi - lo) >> 1);
                if (t[mid] < col) lo = mid + 1; else hi = mid;
              }
              hit = lo < ql && t[lo] == col;
            }
          }
        }
        const unsigned long long b = __ballot(hit ? 1 : 0);
        if (!b) continue;
        const int nh = __popcll(b);
        any = true;
        total += nh;
        if (n_buf + nh > EXPL_BUF) {  // n_buf > 64 >= max_terms
          expl_prune(b_hi, b_lo, n_buf, a.max_terms, lane);
          n_buf = a.max_terms;
        }
        if (hit) {
          unsigned wt = cl.weight ? cl.weight[col] : (unsigned)REC_WEIGHT_ONE;  // clamped exactly as rec_rows_kernel clamps it
          wt = wt < 1u ? 1u : wt > (unsigned)REC_WEIGHT_MAX ? (unsigned)REC_WEIGHT_MAX : wt;
          const int at = n_buf + __popcll(b & ((1ull << lane) - 1ull));
          // (the translation unit is compiled with -ffp-contract=off.)  Positive doubles order as their bits do.
          b_hi[at] = (unsigned long long)__double_as_longlong(boost * ((double)wt * REC_WEIGHT_UNIT));
          b_lo[at] = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(unsigned)col;
          m += (unsigned long long)wt;
        }
        n_buf += nh;
      }
    }
    if (any)
      for (int o = WAVE / 2; o > 0; o >>= 1) m += shfl_xor_u64(m, o);
    if (lane == 0) a.out_m[slot * a.n_clauses + c] = (int64_t)m;
  }
  const int n_out = total < (long long)a.max_terms ? (int)total : a.max_terms;  // <= n_buf
  expl_wave_sync();
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int e = lane + x * WAVE;
    if (e < n_buf) {
      const unsigned long long kh = b_hi[e], kl = b_lo[e];
      const int r = expl_rank(b_hi, b_lo, n_buf, e, kh, kl);
      if (r < n_out) {
        const int64_t o = slot * a.max_terms + r;
        a.out_clause[o] = (int32_t)(kl >> 32);
        a.out_term[o] = (int32_t)(unsigned)kl;
        a.out_contrib[o] = __longlong_as_double((long long)kh);
      }
    }
  }
  if (lane == 0) a.out_n[slot] = n_out;
  expl_wave_sync();  // the next slot of this wave writes the buffer
}

__global__ __launch_bounds__(EXPL_THREADS) void explain_kernel(ExplArgs a) {
  __shared__ int32_t s_terms[EXPL_LDS_TERMS];
  __shared__ unsigned long long s_hi[EXPL_NW][EXPL_BUF];
  __shared__ unsigned long long s_lo[EXPL_NW][EXPL_BUF];
  __shared__ long long s_qb[REC_MAX_CLAUSES];
  __shared__ long long s_ql[REC_MAX_CLAUSES];
  __shared__ int s_off[REC_MAX_CLAUSES];
  __shared__ int s_staged;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int num = a.num, n_clauses = a.n_clauses;
  for (int64_t q = blockIdx.x; q < a.n_queries; q += gridDim.x) {
    if (tid < n_clauses) {
      const long long b = a.c[tid].q_row_ptr[q], e = a.c[tid].q_row_ptr[q + 1];
      s_qb[tid] = b;
      s_ql[tid] = e > b ? e - b : 0;
    }
    __syncthreads();
    if (tid == 0) {
      long long L = 0;
      for (int c = 0; c < n_clauses; ++c) {
        s_off[c] = L <= EXPL_LDS_TERMS ? (int)L : 0;
        L = L <= EXPL_LDS_TERMS ? L + s_ql[c] : L;  // (saturates: L only says which side of the limit the query lies on)
      }
      s_staged = L <= EXPL_LDS_TERMS ? 1 : 0;
    }
    __syncthreads();
    const bool staged = s_staged != 0;  // block-uniform
    if (staged)
      for (int c = 0; c < n_clauses; ++c) {
        const int32_t* __restrict__ src = a.c[c].q_col_idx + s_qb[c];
        const int n = (int)s_ql[c], off = s_off[c];
        for (int t = tid; t < n; t += EXPL_THREADS) s_terms[off + t] = src[t];
      }
    __syncthreads();
    int cnt = a.rec_count[q];
    cnt = cnt < 0 ? 0 : cnt > num ? num : cnt;
    for (int j = wave; j < num; j += EXPL_NW) {  // wave-uniform
      const int64_t slot = q * num + j;
      const int32_t item = j < cnt ? a.rec_idx[slot] : -1;  // nothing at or behind the count is read
      if ((unsigned)item >= (unsigned)a.n_items) {
        if (lane < n_clauses) a.out_m[slot * n_clauses + lane] = 0;
        if (lane == 0) a.out_n[slot] = 0;
        continue;
      }
      if (staged) expl_slot<true>(a, slot, item, s_terms, s_off, s_qb, s_ql, s_hi[wave], s_lo[wave], lane);
      else expl_slot<false>(a, slot, item, s_terms, s_off, s_qb, s_ql, s_hi[wave], s_lo[wave], lane);
    }
    __syncthreads();  // the next query restages the terms
  }
}

hipError_t launch_explain(hipStream_t st, int n_cu, const ExplArgs& a) {
  if (a.n_queries <= 0) return hipSuccess;
  int64_t blocks = a.n_queries;
  if (blocks > (int64_t)n_cu * 16) blocks = (int64_t)n_cu * 16;  // 40 KiB of LDS: three blocks share a CU
  hipLaunchKernelGGL(explain_kernel, dim3((unsigned)blocks), dim3(EXPL_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace urcco
