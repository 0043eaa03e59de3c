// cco_eval.h -- hold-out evaluation of recommendations (urcco_dev_rank_metrics, urcco_dev_tree_sum): per query the hits, the average precision and the
// NDCG at up to EVAL_MAX_KS cut-offs of a strided top-num table (as urcco_dev_recommend leaves it) against a sorted truth row, and their sums over the
// queries (decision D19).  Included once, from cco_misc.hip, behind cco_recommend.h.
//
//   eval_ideal_kernel   ideal[n] = discount[0] + ... + discount[n - 1], summed from 0.0 in ascending order: once per call, one thread
//   eval_rank_kernel    a wave per query, a lane per position of a round of 64: the lane searches its item in the truth row, the 64-bit ballot of the round
//                       gives H(j) = carry + popcount of the lower lanes, the lane forms its own term H(j) / (j + 1) and loads its own discount; the ordered
//                       f64 sums then walk the set bits of the ballot in ascending order -- lane kappa keeps the sums of cut-off ks[kappa] and takes the
//                       broadcast term of position j iff j < ks[kappa].  Every sum is the serial one of the decision: from 0.0, ascending j, one rounding
//                       per division and per add.  The integer sums collect per lane, then per block in LDS, then by one integer atomic per block.
//   eval_tree_kernel    tree(x) of the decision, 256 positions per block: xor-shuffles 1..32 inside a wave, the same pairing over the four waves in LDS;
//                       a pass over the partials per further factor of 256.  An add is made iff the partner's subtree starts inside the power of two the
//                       decision pads to (padding inside it holds +0.0 and IS added, nothing beyond it is): bit for bit the numpy loop, for every n.
// No float atomics.
#pragma once

namespace urcco {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_NW = EVAL_THREADS / WAVE;

struct EvalArgs {
  int64_t n_queries;
  int32_t num, n_ks, k_max;
  int32_t ks[EVAL_MAX_KS];
  const int32_t* rec_count;
  const int32_t* rec_idx;
  const int64_t* truth_row_ptr;
  const int32_t* truth_col_idx;
  const double* discount;       // nullable
  const double* ideal;          // [num + 1], with discount
  int32_t* out_hits;
  double* out_ap;
  double* out_ndcg;             // nullable, with discount
  unsigned long long* sums_i;   // nullable: [2 + 2 * n_ks], zero before the launch
};

__global__ void eval_ideal_kernel(int32_t num, const double* __restrict__ discount, double* __restrict__ ideal) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = 0.0;
  ideal[0] = s;
  for (int j = 0; j < num; ++j) {
    s = s + discount[j];
    ideal[j + 1] = s;
  }
}

template <bool NDCG>
__global__ __launch_bounds__(EVAL_THREADS) void eval_rank_kernel(EvalArgs a) {
  __shared__ unsigned long long s_i[2 + 2 * EVAL_MAX_KS];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  if (tid < 2 + 2 * EVAL_MAX_KS) s_i[tid] = 0ull;
  __syncthreads();
  const int num = a.num, n_ks = a.n_ks;
  int my_k = 0;  // lane kappa < n_ks keeps cut-off ks[kappa]; the other lanes take no term
#pragma unroll
  for (int x = 0; x < EVAL_MAX_KS; ++x)
    if (lane == x && x < n_ks) my_k = a.ks[x];
  unsigned long long sum_hits = 0ull, sum_pos = 0ull, n_eval = 0ull, n_skip = 0ull;
  const int64_t n_waves = (int64_t)gridDim.x * EVAL_NW;
  for (int64_t q = (int64_t)blockIdx.x * EVAL_NW + tid / WAVE; q < a.n_queries; q += n_waves) {  // wave-uniform
    int c = a.rec_count[q];
    c = c < 0 ? 0 : c > num ? num : c;
    const int64_t tb = a.truth_row_ptr[q], t = a.truth_row_ptr[q + 1] - tb;
    int hits = 0;
    double ap = 0.0, dcg = 0.0;
    if (t > 0) {
      const int m_max = c < a.k_max ? c : a.k_max;  // no cut-off looks further
      int carry = 0;                                 // H of the rounds before this one
      for (int j0 = 0; j0 < m_max; j0 += WAVE) {
        const int j = j0 + lane;
        bool rel = false;
        if (j < m_max) {
          const int32_t r = a.rec_idx[q * num + j];
          int64_t lo = 0, hi = t;  // first entry >= r
          while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.truth_col_idx[tb + mid] < r) lo = mid + 1; else hi = mid;
          }
          rel = lo < t && a.truth_col_idx[tb + lo] == r;
        }
        unsigned long long b = __ballot(rel ? 1 : 0);
        const int h = carry + __popcll(b & ((2ull << lane) - 1ull));  // H(j): the hits at or before this lane
        const double term = rel ? (double)h / (double)(j + 1) : 0.0;
        const double disc = (NDCG && rel) ? a.discount[j] : 0.0;
        carry += __popcll(b);
        while (b) {  // the set bits, ascending: wave-uniform
          const int p = __ffsll(b) - 1;
          b &= b - 1ull;
          const double tp = __shfl(term, p);
          const double dp = NDCG ? __shfl(disc, p) : 0.0;
          if (j0 + p < my_k) {
            ap = ap + tp;
            if (NDCG) dcg = dcg + dp;
            ++hits;
          }
        }
      }
    }
    if (lane < n_ks) {
      const int64_t o = q * n_ks + lane;
      const int mt = t < (int64_t)my_k ? (int)t : my_k;  // min(k, |T|)
      a.out_hits[o] = hits;
      a.out_ap[o] = t > 0 ? ap / (double)mt : 0.0;
      if (NDCG) a.out_ndcg[o] = t > 0 ? dcg / a.ideal[mt] : 0.0;
      sum_hits += (unsigned long long)hits;
      sum_pos += hits > 0 ? 1ull : 0ull;
    }
    if (t > 0) ++n_eval; else ++n_skip;
  }
  if (!a.sums_i) return;  // uniform
  if (lane == 0) {
    if (n_eval) atomicAdd(&s_i[0], n_eval);
    if (n_skip) atomicAdd(&s_i[1], n_skip);
  }
  if (lane < n_ks) {
    if (sum_hits) atomicAdd(&s_i[2 + lane], sum_hits);
    if (sum_pos) atomicAdd(&s_i[2 + n_ks + lane], sum_pos);
  }
  __syncthreads();
  if (tid < 2 + 2 * n_ks && s_i[tid]) atomicAdd(&a.sums_i[tid], s_i[tid]);
}

// out[c * out_col_stride + block] = the tree sum of the block's 256 positions of column c; position i of the column lies at in[i * row_stride + c * col_stride]
// and stands for a subtree of the queries.  p_level = positions of this level inside the padded power of two (>= 1).
__global__ __launch_bounds__(EVAL_THREADS) void eval_tree_kernel(const double* __restrict__ in, int64_t n_in, int64_t row_stride, int64_t col_stride, int64_t p_level,
                                                                 double* __restrict__ out, int64_t out_col_stride) {
  __shared__ double s_w[EVAL_NW];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int64_t i0 = (int64_t)blockIdx.x * EVAL_THREADS, i = i0 + tid;
  const int64_t c = blockIdx.y;
  double x = i < n_in ? in[i * row_stride + c * col_stride] : 0.0;
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) {
    const double y = __shfl_xor(x, m);
    if (((i ^ (int64_t)m) & ~(int64_t)(m - 1)) < p_level) x = x + y;  // (the lanes whose value reaches lane 0 see the partners lane 0's tree names)
  }
  if (lane == 0) s_w[wave] = x;
  __syncthreads();
  if (tid == 0) {
    static_assert(EVAL_NW == 4, "two levels over the waves");
    double u = s_w[0], v = s_w[2];
    if (i0 + WAVE < p_level) u = u + s_w[1];
    if (i0 + 3 * WAVE < p_level) v = v + s_w[3];
    if (i0 + 2 * WAVE < p_level) u = u + v;
    out[c * out_col_stride + blockIdx.x] = u;
  }
}

// partial sums a tree sum over n positions of n_cols columns needs: pa[0], pb[1] doubles
void tree_sum_scratch(int64_t n, int32_t n_cols, size_t* pa, size_t* pb) {
  const int64_t l1 = (n + EVAL_THREADS - 1) / EVAL_THREADS, l2 = (l1 + EVAL_THREADS - 1) / EVAL_THREADS;
  *pa = (size_t)(l1 > 0 ? l1 : 1) * (size_t)n_cols;
  *pb = (size_t)(l2 > 0 ? l2 : 1) * (size_t)n_cols;
}

// out[c] = tree(x[:, c]) for x [n, n_cols] row-major
hipError_t launch_tree_sum(hipStream_t st, const double* x, int64_t n, int32_t n_cols, double* out, double* pa, double* pb) {
  if (n <= 0) return hipMemsetAsync(out, 0, sizeof(double) * (size_t)n_cols, st);
  int64_t padded = 1;
  while (padded < n) padded <<= 1;
  const double* in = x;
  int64_t n_in = n, row_stride = n_cols, col_stride = 1;
  int span_log2 = 0;
  for (int pass = 0;; ++pass) {
    const int64_t n_out = (n_in + EVAL_THREADS - 1) / EVAL_THREADS;
    double* dst = n_out == 1 ? out : (pass & 1) ? pb : pa;
    const int64_t p_level = (padded >> span_log2) > 0 ? (padded >> span_log2) : 1;
    hipLaunchKernelGGL(eval_tree_kernel, dim3((unsigned)n_out, (unsigned)n_cols), dim3(EVAL_THREADS), 0, st, in, n_in, row_stride, col_stride, p_level, dst,
                       n_out == 1 ? (int64_t)1 : n_out);
    if (n_out == 1) break;
    in = dst; n_in = n_out; row_stride = 1; col_stride = n_out; span_log2 += 8;
  }
  return hipGetLastError();
}

hipError_t launch_rank_metrics(hipStream_t st, int n_cu, int64_t n_queries, int32_t num, const int32_t* rec_count, const int32_t* rec_idx, const int64_t* truth_row_ptr,
                               const int32_t* truth_col_idx, const int32_t* ks, int32_t n_ks, const double* discount, double* ideal, int32_t* out_hits, double* out_ap,
                               double* out_ndcg, int64_t* out_sums_i, double* out_sums_f, double* pa, double* pb) {
  hipError_t e;
  if (out_sums_i) {
    if ((e = hipMemsetAsync(out_sums_i, 0, sizeof(int64_t) * (size_t)(2 + 2 * n_ks), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(out_sums_f, 0, sizeof(double) * (size_t)(2 * n_ks), st)) != hipSuccess) return e;
  }
  if (n_queries <= 0) return hipSuccess;
  EvalArgs a;
  memset(&a, 0, sizeof(a));
  a.n_queries = n_queries; a.num = num; a.n_ks = n_ks; a.k_max = ks[n_ks - 1];
  for (int x = 0; x < n_ks; ++x) a.ks[x] = ks[x];
  a.rec_count = rec_count; a.rec_idx = rec_idx; a.truth_row_ptr = truth_row_ptr; a.truth_col_idx = truth_col_idx;
  a.discount = discount; a.ideal = ideal; a.out_hits = out_hits; a.out_ap = out_ap; a.out_ndcg = out_ndcg;
  a.sums_i = reinterpret_cast<unsigned long long*>(out_sums_i);
  int64_t blocks = (n_queries + EVAL_NW - 1) / EVAL_NW;
  if (blocks > (int64_t)n_cu * 32) blocks = (int64_t)n_cu * 32;
  if (discount) {
    hipLaunchKernelGGL(eval_ideal_kernel, dim3(1), dim3(WAVE), 0, st, num, discount, ideal);
    hipLaunchKernelGGL((eval_rank_kernel<true>), dim3((unsigned)blocks), dim3(EVAL_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL((eval_rank_kernel<false>), dim3((unsigned)blocks), dim3(EVAL_THREADS), 0, st, a);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (out_sums_f) {
    if ((e = launch_tree_sum(st, out_ap, n_queries, n_ks, out_sums_f, pa, pb)) != hipSuccess) return e;
    if (discount && (e = launch_tree_sum(st, out_ndcg, n_queries, n_ks, out_sums_f + n_ks, pa, pb)) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace urcco
