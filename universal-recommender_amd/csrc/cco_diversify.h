// cco_diversify.h -- greedy maximal-marginal-relevance re-rank of a result table over indicator links (urcco_dev_diversify; DESIGN.md, decision D36): per row
// the best entry, then the best given what was already picked -- every link to a chosen item costs w = penalty * the row's best score.  Included once, from
// cco_misc.hip, behind cco_listmetrics.h (whose set constants and hash it shares).  The selection is sequential by definition; the work is the adjacency.
//
//   diversify_kernel        a wave per table row, four rows a block, grid-striding.  Three phases, all inside the wave:
//     stage      the row's valid items go into a 512-slot LDS set, item -> first position (atomicCAS, atomicMin): position j is ELIGIBLE iff first == j.
//     adjacency  a bit matrix in LDS, c rows of W = ceil(c / 64) 64-bit words packed at stride W (8 KiB a wave at c = 256); only those c * W words are
//                cleared, one contiguous sweep.  The sources are taken 64 positions a chunk: the lengths and starts of their matrix rows go to LDS (65 + 64
//                words -- a quarter of a whole-row prefix, which is what lets three blocks share a CU), the exclusive prefix comes from a wave scan, and
//                the chunk's FLATTENED entries are walked 64 at a time, a lane finding its source by a six-step binary search.  An entry found in the set at
//                first position b != a (b == a is the self entry) sets bit b of row a and bit a of row b by an LDS atomicOr, unless the first is there already.
//     select     lane l holds candidates l, l + 64, l + 128, l + 192 in registers (item, score, links to the chosen, alive).  A step forms the lane's best
//                of four keys fl(score - fl(w * n)), reduces (key, position) over the wave by six xor-shuffles (larger key, then smaller position), reads
//                the winner's W adjacency words -- every lane the same address: LDS broadcasts -- and each lane raises n where its bit is set.  The
//                winner's lane writes output slot t.  Register arrays are only ever indexed by unrolled constants: nothing spills.
//   diversify_stats_kernel  one wave adds the blocks' partial statistics: no atomic touches memory outside LDS, every number is reproducible.
// Wave primitives under wave-uniform control flow only, one per source line.  The translation unit is compiled with -ffp-contract=off: the product and the
// difference of a key round separately.
#pragma once

namespace urcco {

constexpr int DIV_THREADS = 256;
constexpr int DIV_NW = DIV_THREADS / WAVE;
constexpr int DIV_SLOTS = REC_MAX_NUM / WAVE;  // candidates a lane holds; words of a full adjacency row
constexpr int DIV_BLOCKS_PER_CU = 3;           // what the LDS of a block (profiles/diversify_kernel_resources.txt) leaves resident
static_assert(DIV_SLOTS == 4 && DIV_NW == 4 && LM_SET_SLOTS >= 2 * REC_MAX_NUM, "four candidates a lane, four waves a block, the set at load 1/2");

// (key, position) a beats b: the larger key, on equal keys the smaller position.  Keys are never NaN here, so the order is total and every lane of a
// butterfly ends on the same winner.
__device__ __forceinline__ bool div_better(double ka, int pa, double kb, int pb) { return ka > kb || (ka == kb && pa < pb); }

__global__ __launch_bounds__(DIV_THREADS) void diversify_kernel(DivArgs a) {
  __shared__ int s_item[DIV_NW][LM_SET_SLOTS];                             // the set: item, -1 = free
  __shared__ int s_first[DIV_NW][LM_SET_SLOTS];                            // ... -> its first position
  __shared__ unsigned long long s_adj[DIV_NW][REC_MAX_NUM * DIV_SLOTS];    // the links: row j = words j * W .. j * W + W - 1
  __shared__ unsigned long long s_pre[DIV_NW][WAVE + 1];                   // a chunk of sources: exclusive prefix of their row lengths
  __shared__ long long s_base[DIV_NW][WAVE];                               // ... and where their matrix rows start
  __shared__ unsigned long long s_part[DIV_NW][3];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  int* set_item = s_item[wave];
  int* set_first = s_first[wave];
  unsigned long long* adj = s_adj[wave];
  unsigned long long* pre = s_pre[wave];
  long long* base = s_base[wave];
  unsigned long long sum_walked = 0ull, sum_bits = 0ull, sum_prefix = 0ull;  // sum_walked, sum_prefix: wave-uniform, counted by lane 0
  const int64_t n_waves = (int64_t)gridDim.x * DIV_NW;
  for (int64_t q = (int64_t)blockIdx.x * DIV_NW + wave; q < a.n_rows; q += n_waves) {  // wave-uniform
    int c = a.in_count[q];
    c = c < 0 ? 0 : c > a.width ? a.width : c;
    const int W = (c + WAVE - 1) / WAVE;
    const int32_t* row = a.in_idx + q * (int64_t)a.width;
    const unsigned long long* row_score = a.in_score + q * (int64_t)a.width;
    // ---- stage: item -> first position
    for (int h = lane; h < LM_SET_SLOTS; h += WAVE) {
      set_item[h] = -1;
      set_first[h] = 0x7fffffff;
    }
    for (int i = lane; i < c * W; i += WAVE) adj[i] = 0ull;
    expl_wave_sync();
    int32_t item[DIV_SLOTS];
#pragma unroll
    for (int s = 0; s < DIV_SLOTS; ++s) {
      const int j = s * WAVE + lane;
      item[s] = j < c ? row[j] : -1;
      if ((unsigned)item[s] >= (unsigned)a.n_items) {
        item[s] = -1;
        continue;
      }
      unsigned h = lm_hash((unsigned)item[s]) & (LM_SET_SLOTS - 1);
      for (int p = 0; p < LM_SET_SLOTS; ++p) {  // at most REC_MAX_NUM items: a slot is always found
        const int k = atomicCAS(&set_item[h], -1, item[s]);
        if (k == -1 || k == item[s]) {
          atomicMin(&set_first[h], j);
          break;
        }
        h = (h + 1u) & (LM_SET_SLOTS - 1);
      }
    }
    expl_wave_sync();
    bool alive[DIV_SLOTS];  // eligible and not yet chosen
#pragma unroll
    for (int s = 0; s < DIV_SLOTS; ++s) {
      alive[s] = false;
      if (item[s] < 0) continue;
      unsigned h = lm_hash((unsigned)item[s]) & (LM_SET_SLOTS - 1);
      while (set_item[h] != item[s]) h = (h + 1u) & (LM_SET_SLOTS - 1);  // it was staged
      alive[s] = set_first[h] == s * WAVE + lane;                       // a later repeat is never output, is no source and no target
    }
    // ---- adjacency: the flattened entries of the eligible sources' matrix rows, 64 sources a chunk
#pragma unroll
    for (int s = 0; s < DIV_SLOTS; ++s) {
      if (s >= W) break;  // wave-uniform
      long long len = 0, start = 0;
      if (alive[s]) {
        start = a.sim_row_ptr[item[s]];
        len = a.sim_row_ptr[item[s] + 1] - start;
        len = len > 0 ? len : 0;
      }
      unsigned long long incl = (unsigned long long)len;
      for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long y = (unsigned long long)shfl_i64((long long)incl, lane >= d ? lane - d : lane);
        if (lane >= d) incl += y;
      }
      pre[lane] = incl - (unsigned long long)len;
      base[lane] = start;
      if (lane == WAVE - 1) pre[WAVE] = incl;
      const unsigned long long total = (unsigned long long)shfl_i64((long long)incl, WAVE - 1);
      expl_wave_sync();
      sum_walked += total;
      for (unsigned long long e0 = 0ull; e0 < total; e0 += WAVE) {  // wave-uniform
        const unsigned long long e = e0 + (unsigned long long)lane;
        if (e < total) {
          int lo = 0;  // the last source with pre[.] <= e: the one whose row holds entry e (pre[0] = 0 <= e < pre[WAVE])
#pragma unroll
          for (int half = WAVE / 2; half > 0; half >>= 1)
            if (pre[lo + half] <= e) lo += half;
          const int32_t t = a.sim_col_idx[base[lo] + (long long)(e - pre[lo])];
          if ((unsigned)t < (unsigned)a.n_items) {
            unsigned h = lm_hash((unsigned)t) & (LM_SET_SLOTS - 1);
            int k = set_item[h];
            while (k != t && k != -1) {
              h = (h + 1u) & (LM_SET_SLOTS - 1);
              k = set_item[h];
            }
            const int src = s * WAVE + lo;
            const int b = k == t ? set_first[h] : src;  // a first position is eligible and lies below c; b == src: the row names itself
            if (b != src && !((adj[src * W + (b >> 6)] >> (b & 63)) & 1ull)) {  // whoever set that bit sets its mirror before the wave moves on
              atomicOr(&adj[src * W + (b >> 6)], 1ull << (b & 63));
              atomicOr(&adj[b * W + (src >> 6)], 1ull << (src & 63));
            }
          }
        }
      }
      expl_wave_sync();  // the next chunk overwrites pre and base; the selection reads adj
    }
    // ---- the weight: top = the best eligible score
    double score[DIV_SLOTS];
    int links[DIV_SLOTS];
    double top = -__builtin_inf();
    int eligible = 0;
#pragma unroll
    for (int s = 0; s < DIV_SLOTS; ++s) {
      const int j = s * WAVE + lane;
      score[s] = __longlong_as_double((long long)(j < c ? row_score[j] : 0ull));
      links[s] = 0;
      if (alive[s]) top = score[s] > top ? score[s] : top;
      if (alive[s])
        for (int w = 0; w < W; ++w) sum_bits += (unsigned long long)__popcll(adj[j * W + w]);
      const unsigned long long m = __ballot(alive[s]);
      eligible += __popcll(m);
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const double y = __shfl_xor(top, o);
      top = y > top ? y : top;
    }
    const double w = top > 0.0 ? a.penalty * top : 0.0;
    // ---- select
    const int steps = a.num < eligible ? a.num : eligible;
    const int64_t out0 = q * (int64_t)a.num;
    int prev = -1;
    bool ascending = true;
    for (int t = 0; t < steps; ++t) {  // wave-uniform
      double bk = -__builtin_inf();
      int bp = REC_MAX_NUM;  // no candidate
#pragma unroll
      for (int s = 0; s < DIV_SLOTS; ++s) {
        double k = score[s] - w * (double)links[s];
        k = k == k ? k : -__builtin_inf();  // scores and penalty * top are finite by contract; a NaN would leave no winner
        if (alive[s] && div_better(k, s * WAVE + lane, bk, bp)) {
          bk = k;
          bp = s * WAVE + lane;
        }
      }
      for (int o = WAVE / 2; o > 0; o >>= 1) {
        const double ok = __shfl_xor(bk, o);
        const int op = __shfl_xor(bp, o);
        if (div_better(ok, op, bk, bp)) {
          bk = ok;
          bp = op;
        }
      }
      // an alive candidate exists (t < eligible) and beats "no candidate" at least on its position: bp < c
      const int ws = bp >> 6;
#pragma unroll
      for (int s = 0; s < DIV_SLOTS; ++s) {
        if (s == ws && lane == (bp & (WAVE - 1))) {
          alive[s] = false;
          a.out_idx[out0 + t] = item[s];
          a.out_score[out0 + t] = (unsigned long long)__double_as_longlong(score[s]);
          if (a.out_pos) a.out_pos[out0 + t] = bp;
          if (a.out_links) a.out_links[out0 + t] = links[s];
        }
        if (s < W) links[s] += (int)((adj[bp * W + s] >> lane) & 1ull);
      }
      ascending = ascending && bp > prev;
      prev = bp;
    }
    for (int k = steps + lane; k < a.num; k += WAVE) {
      a.out_idx[out0 + k] = -1;
      a.out_score[out0 + k] = 0ull;
      if (a.out_pos) a.out_pos[out0 + k] = -1;
      if (a.out_links) a.out_links[out0 + k] = 0;
    }
    if (lane == 0) a.out_count[q] = steps;
    // the output is the eligible prefix in input order iff the chosen positions ascend and no eligible position below the last one was passed over
    int below = 0;
#pragma unroll
    for (int s = 0; s < DIV_SLOTS; ++s) {
      const unsigned long long m = __ballot(alive[s] && s * WAVE + lane < prev);  // alive by now: eligible and not chosen
      below += __popcll(m);
    }
    sum_prefix += ascending && below == 0 ? 1ull : 0ull;
    expl_wave_sync();  // the next row clears the tables
  }
  if (!a.partial) return;  // uniform
  sum_bits = lm_wave_sum(sum_bits);
  if (lane == 0) {
    s_part[wave][0] = sum_walked;
    s_part[wave][1] = sum_bits;
    s_part[wave][2] = sum_prefix;
  }
  __syncthreads();
  if (tid < 3) a.partial[(int64_t)blockIdx.x * 3 + tid] = s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
}

// stats = [rows, matrix entries walked, linked unordered pairs, rows left as their eligible prefix, 0, 0, 0, 0] from the blocks' partial sums
__global__ __launch_bounds__(WAVE) void diversify_stats_kernel(const unsigned long long* __restrict__ partial, int blocks, int64_t n_rows,
                                                               unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x;
  unsigned long long v[3] = {0ull, 0ull, 0ull};
  for (int b = lane; b < blocks; b += WAVE) {
#pragma unroll
    for (int x = 0; x < 3; ++x) v[x] += partial[(int64_t)b * 3 + x];
  }
#pragma unroll
  for (int x = 0; x < 3; ++x) v[x] = lm_wave_sum(v[x]);
  if (lane == 0) {
    stats[0] = (unsigned long long)n_rows;
    stats[1] = v[0];
    stats[2] = v[1] / 2ull;  // every linked pair set two bits
    stats[3] = v[2];
  }
  if (lane >= 4 && lane < DIV_STATS_LEN) stats[lane] = 0ull;
}

int64_t diversify_blocks(int64_t n_rows, int n_cu) {
  const int64_t blocks = (n_rows + DIV_NW - 1) / DIV_NW, most = (int64_t)n_cu * DIV_BLOCKS_PER_CU;
  return blocks < most ? blocks : most;
}

hipError_t launch_diversify(hipStream_t st, int n_cu, const DivArgs& a) {
  const int64_t blocks = diversify_blocks(a.n_rows, n_cu);
  if (blocks > 0) hipLaunchKernelGGL(diversify_kernel, dim3((unsigned)blocks), dim3(DIV_THREADS), 0, st, a);
  if (a.stats) hipLaunchKernelGGL(diversify_stats_kernel, dim3(1), dim3(WAVE), 0, st, a.partial, (int)blocks, a.n_rows, a.stats);
  return hipGetLastError();
}

}  // namespace urcco
