// Raw rows -> sorted, duplicate-free rows: the one unit behind the Preparator's CSR build (ingest_kernels.hip), the history rows (cco_history.h,
// D17) and the item rows (cco_items.h, D18).  Compiled into ingest_kernels.hip, ahead of all three; it uses that file's grid helper.
//
// A caller owns a RawRows (cco_kernels.h): raw row r is tmp[raw_ptr[r] .. raw_ptr[r + 1]), an upper bound of the final row.  Its kernels bring the
// row's columns to one of the two tails below, which leave the sorted, distinct columns at the row's start, and store the length in len[r];
// sr_finish_rows turns (raw_ptr, tmp, len) into the caller's CSR.  Two classes by the number of raw entries:
//   <= 64     sr_wave_tail: one wave, a lane per entry, bitonic network + ballot unique in registers
//   larger    sr_block_tail: one block, bitonic network in LDS up to 4096 entries, in global memory (the raw row itself) beyond; unique by a
//             block scan, 256 entries at a time, in place
// Wave = 64 lanes; wave primitives under wave-uniform control flow only, one per source line (tests/hostsim tells them apart by line).
namespace urcco {

namespace {
constexpr int SR_WAVE = 64;
constexpr int SR_SENT = 0x7fffffff;  // "no column": sorts behind every id.  Padding, and to the callers that say so an entry to drop
constexpr int SR_LDS = 4096;         // entries of a row one block sorts in LDS

// one wave: sort the lanes' values and write the distinct ones to dst; returns their number (all lanes).
// DROP_SENT false: the lanes hold n real entries and SR_SENT in the others; the n smallest are the row, so a real entry equal to SR_SENT is kept.
// DROP_SENT true: SR_SENT marks an entry to drop, anywhere among the lanes; n is not looked at.
template <bool DROP_SENT>
__device__ __forceinline__ int sr_wave_tail(int v, int lane, int n, int32_t* __restrict__ dst) {
  for (int k2 = 2; k2 <= SR_WAVE; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      const int o = __shfl_xor(v, j);
      const bool keep_small = ((lane & j) == 0) == ((lane & k2) == 0);  // lower lane of an ascending block
      if (keep_small ? o < v : o > v) v = o;
    }
  }
  const int prev = __shfl_up(v, 1);
  const bool fresh = (DROP_SENT ? v != SR_SENT : lane < n) && (lane == 0 || v != prev);
  const unsigned long long m = __ballot(fresh);
  if (fresh) dst[__popcll(m & ((1ull << lane) - 1ull))] = v;
  return __popcll(m);
}

// the unique step of sr_block_tail: the sorted entries sorted[0..m) -- s_v (IN_LDS) or row itself -- keep those that differ from their predecessor
// (DROP_SENT: and from SR_SENT), compacted into row[0..); positions by block scan, 256 entries at a time.  s_wsum: one int of LDS per wave.
// IN_LDS is a template parameter so that every load is a ds_read or a global_load: through one pointer chosen at run time it is a flat load, and
// with the predecessor's - 1 folded into its base the address of entry 0 of a buffer at LDS offset 0 lies below the LDS aperture.
template <bool DROP_SENT, bool IN_LDS>
__device__ __forceinline__ int sr_unique(int32_t* __restrict__ row, int64_t m, const int* s_v, int* s_wsum) {
  const int lane = threadIdx.x & (SR_WAVE - 1), wave = threadIdx.x / SR_WAVE;
  int carry = 0;
  for (int64_t base = 0; base < m; base += 256) {  // block-uniform
    const int64_t t = base + threadIdx.x;
    int v = 0;
    bool fresh = false;
    if (t < m) {
      v = IN_LDS ? s_v[t] : row[t];
      const int pv = t == 0 ? 0 : (IN_LDS ? s_v[t - 1] : row[t - 1]);
      fresh = (t == 0 || v != pv) && (!DROP_SENT || v != SR_SENT);
    }
    const unsigned long long mk = __ballot(fresh);
    if (lane == 0) s_wsum[wave] = __popcll(mk);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 256 / SR_WAVE; ++w) {
      const int c = s_wsum[w];
      if (w < wave) before += c;
      tot += c;
    }
    const int pos = carry + before + __popcll(mk & ((1ull << lane) - 1ull));
    __syncthreads();  // every read of row[base .. base + 256) and of s_wsum precedes the writes below
    if (fresh) row[pos] = v;  // pos <= t: in-place compaction towards the front, chunk by chunk
    carry += tot;
    __syncthreads();
  }
  return carry;
}

// one block of 256 threads: row[0..m) (global) -> sorted, duplicate-free, in place; returns the length (all threads).  s_v: SR_LDS ints of LDS.
// Nothing but duplicates is dropped: SR_SENT among the m entries is a column like any other.
// STAGED (cco_items.h): the caller has put the m entries where the sort reads them -- s_v[0 .. 2^ceil(log2 m)), SR_SENT behind the m-th, when
// m <= SR_LDS, else row[0..m) -- and SR_SENT among them marks an entry to drop; the result still goes to row.
template <bool STAGED = false>
__device__ __forceinline__ int sr_block_tail(int32_t* __restrict__ row, int64_t m, int* s_v) {
  __shared__ int s_wsum[256 / SR_WAVE];
  if (m <= 0) return 0;  // block-uniform
  int64_t P = 1;
  while (P < m) P <<= 1;
  const bool in_lds = m <= SR_LDS;
  if (in_lds) {
    const int p = (int)P;
    if (!STAGED)
      for (int t = threadIdx.x; t < p; t += 256) s_v[t] = t < m ? row[t] : SR_SENT;
    __syncthreads();
    for (int k2 = 2; k2 <= p; k2 <<= 1) {
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < p; t += 256) {
          const int u = t ^ j;
          if (u > t) {
            const int a = s_v[t], b = s_v[u];
            const bool asc = (t & k2) == 0;
            if (asc ? a > b : a < b) { s_v[t] = b; s_v[u] = a; }
          }
        }
        __syncthreads();
      }
    }
  } else {
    // In global memory, as P = 2^ceil(log2 m) entries whose tail [m, P) is +inf.  The ascending-only formulation of the
    // bitonic network (partner = t ^ (k2 - 1) on the first step of a level, t ^ j afterwards; the smaller value always
    // goes to the lower index) never moves a real value into the padding, so exchanges that touch it are skipped.
    for (int64_t k2 = 2; k2 <= P; k2 <<= 1) {
      for (int64_t j = k2 >> 1; j > 0; j >>= 1) {
        for (int64_t t = threadIdx.x; t < P; t += 256) {
          const int64_t u = (j == (k2 >> 1)) ? (t ^ (k2 - 1)) : (t ^ j);
          if (u > t && u < m) {
            const int a = row[t], b = row[u];
            if (a > b) { row[t] = b; row[u] = a; }
          }
        }
        __syncthreads();
      }
    }
  }
  return in_lds ? sr_unique<STAGED, true>(row, m, s_v, s_wsum) : sr_unique<STAGED, false>(row, m, s_v, s_wsum);
}
}  // namespace

// the fronts of the raw rows -> the final CSR; one wave per row
__global__ __launch_bounds__(256) void ig_compact_rows_kernel(int64_t n_rows, const int64_t* __restrict__ raw_ptr, const int32_t* __restrict__ tmp,
                                                              const int64_t* __restrict__ out_rp, int32_t* __restrict__ out_ci) {
  const int lane = threadIdx.x & (SR_WAVE - 1);
  const int64_t n_waves = (int64_t)gridDim.x * (256 / SR_WAVE);
  for (int64_t r = (int64_t)blockIdx.x * (256 / SR_WAVE) + threadIdx.x / SR_WAVE; r < n_rows; r += n_waves) {
    const int64_t s = raw_ptr[r], d = out_rp[r];
    const int64_t L = out_rp[r + 1] - d;
    for (int64_t t = lane; t < L; t += SR_WAVE) out_ci[d + t] = tmp[s + t];
  }
}

// what a caller of the two-call protocol (bounds, then rows) hands over per output CSR: row_ptr holds the bounds' scan on entry, the final row
// starts on return
struct RowsOut {
  RawRows raw;
  int64_t* row_ptr;
  int32_t* col_idx;
};

// ahead of the caller's row kernels: raw_ptr = the bounds' scan, per output.  No rows: the empty CSRs, and nothing is left to do.
static hipError_t sr_seed_raw_ptr(hipStream_t st, const RowsOut* out, int n_out, int64_t n_rows) {
  for (int i = 0; i < n_out; ++i) {
    const hipError_t e = n_rows > 0 ? hipMemcpyAsync(out[i].raw.raw_ptr, out[i].row_ptr, sizeof(int64_t) * (size_t)(n_rows + 1), hipMemcpyDeviceToDevice, st)
                                    : hipMemsetAsync(out[i].row_ptr, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// behind them: the rows' lengths are in raw.len, their columns at the fronts of the raw rows.  Per output, row_ptr = scan of the lengths, col_idx = the
// compacted rows.
static hipError_t sr_finish_rows(hipStream_t st, int n_cu, const RowsOut* out, int n_out, int64_t n_rows, int64_t* tile_sums) {
  for (int i = 0; i < n_out; ++i) {
    const hipError_t e = launch_scan_i32(st, out[i].raw.len, n_rows, out[i].row_ptr, tile_sums);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ig_compact_rows_kernel, dim3(ig_grid(n_rows * SR_WAVE, n_cu)), dim3(256), 0, st, n_rows, out[i].raw.raw_ptr, out[i].raw.tmp, out[i].row_ptr,
                       out[i].col_idx);
  }
  return hipGetLastError();
}

}  // namespace urcco
