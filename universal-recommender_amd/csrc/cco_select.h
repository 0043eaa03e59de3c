// The k-th largest of n composite keys (64 high bits, 32 low bits) by one thread block: an MSB-first radix select, 8-bit digits, one 256-bin LDS
// histogram.  The one unit behind the selection of the recommend kernels (cco_recommend.h: score bits, ~position), of the history rows' block class
// (cco_history.h: time, stream position) and of the global class of the row kernels (cco_rows.hip: LLR bits, ~column).  DESIGN.md 7a.
// It needs the HIP runtime and a wave of 64, nothing else of the library; wave primitives under wave-uniform control flow only, one per source line.
//
// sel_kth_largest<NT>(n, k, hi_at, lo_at, differ, common, s): called by all NT threads of the block with block-uniform arguments, n > k >= 1.
//   hi_at(i) -> u64, lo_at(i) -> u32   the key of element i < n.  lo_at is called only in a pass over a low digit and only for an element whose high
//                                      half equals the threshold's: what a caller gathers behind it is gathered for those elements alone.
//   differ                             the bits in which two keys of the list may differ (all ones is always legal; sel_differ computes the exact set)
//   common                             any one key's value in the other bits
//   returns T such that {i : key_i >= T} has at least k members -- exactly k when the keys are distinct; with duplicates, every copy of the k-th
//   largest key besides.  The function assumes nothing about distinctness.
// A digit whose byte of `differ` is 0 takes no pass: T carries `common` there.  Every other digit, most significant first, takes one pass over the
// elements that agree with T in all higher digits, then wave 0 finds the bucket that holds the cut: lane l owns digits 4 l .. 4 l + 3, a suffix sum
// over the lanes gives the elements of the larger digits.  When that bucket holds exactly the members still needed the select stops: T is 0 in every
// bit of `differ` below the digit.
//
// Barriers.  A pass is: clear the counters | barrier | count | barrier | wave 0 searches, writes s.sel | barrier | all threads read s.sel.  So
//   on entry   no barrier before the first write of the scratch: the keys must be visible to the block (a barrier after their last write is the
//              caller's) and no thread may still be reading LDS that overlays the scratch.  A preceding sel_differ or sel_kth_largest on the same scratch
//              needs no barrier in between: the reads that follow its last barrier are of s.sel, which is next written two barriers later.
//   on exit    the last barrier is followed only by reads of s.sel: the keys may be overwritten at once; LDS that overlays the scratch may be
//              written after one more barrier.  With no digit to pass (differ = 0) the function executes no barrier at all.
// sel_differ executes two barriers, the first after clearing s.sel, and reads s.sel behind the second: the same rules.
#pragma once

#include <hip/hip_runtime.h>

namespace urcco {

constexpr int SEL_WAVE = 64;

struct SelKey {
  unsigned long long hi;
  unsigned lo;
};

// the LDS scratch of one block, declared __shared__ by the caller
struct SelScratch {
  unsigned hist[256];
  unsigned sel[3];  // digit chosen, members still to take from its bucket, size of the bucket; sel_differ: the OR, low to high word
};

// differ = OR over the list of key_i ^ key_0, common = key_0.  n >= 1.
template <int NT, class HiAt, class LoAt>
__device__ __forceinline__ SelKey sel_differ(unsigned n, HiAt hi_at, LoAt lo_at, SelScratch& s, SelKey& common) {
  const unsigned tid = threadIdx.x;
  if (tid < 3) s.sel[tid] = 0u;
  __syncthreads();
  common.hi = hi_at(0u);
  common.lo = lo_at(0u);
  unsigned long long dh = 0ull;
  unsigned dl = 0u;
  for (unsigned i = tid; i < n; i += NT) {
    dh |= hi_at(i) ^ common.hi;
    dl |= lo_at(i) ^ common.lo;
  }
  if (dl) atomicOr(&s.sel[0], dl);
  if ((unsigned)dh) atomicOr(&s.sel[1], (unsigned)dh);
  if ((unsigned)(dh >> 32)) atomicOr(&s.sel[2], (unsigned)(dh >> 32));
  __syncthreads();
  return SelKey{(unsigned long long)s.sel[1] | ((unsigned long long)s.sel[2] << 32), s.sel[0]};
}

template <int NT, class HiAt, class LoAt>
__device__ __forceinline__ SelKey sel_kth_largest(unsigned n, unsigned k, HiAt hi_at, LoAt lo_at, SelKey differ, SelKey common, SelScratch& s) {
  static_assert(NT >= 256 && NT % SEL_WAVE == 0, "a thread per counter; wave 0 is whole");
  const unsigned tid = threadIdx.x, lane = tid & (SEL_WAVE - 1);
  SelKey T{common.hi & ~differ.hi, common.lo & ~differ.lo};
  unsigned need = k;
  for (int d = 0; d < 12; ++d) {  // block-uniform: the skip and the break are on values every thread agrees on
    const bool high = d < 8;
    const int sh = high ? 56 - 8 * d : 24 - 8 * (d - 8);
    if (((high ? (unsigned)(differ.hi >> sh) : differ.lo >> sh) & 255u) == 0u) continue;
    if (tid < 256) s.hist[tid] = 0u;
    __syncthreads();
    const unsigned long long above_hi = (T.hi >> sh) >> 8;  // the digits above this one (two shifts: sh + 8 may be the width)
    const unsigned above_lo = (T.lo >> sh) >> 8;
    for (unsigned i = tid; i < n; i += NT) {
      const unsigned long long hi = hi_at(i);
      unsigned digit;
      if (high) {
        const unsigned long long x = hi >> sh;
        if ((x >> 8) != above_hi) continue;
        digit = (unsigned)x & 255u;
      } else {
        if (hi != T.hi) continue;
        const unsigned x = lo_at(i) >> sh;
        if ((x >> 8) != above_lo) continue;
        digit = x & 255u;
      }
      atomicAdd(&s.hist[digit], 1u);
    }
    __syncthreads();
    if (tid < SEL_WAVE) {
      unsigned h4[4], sum = 0u;
#pragma unroll
      for (int x = 0; x < 4; ++x) { h4[x] = s.hist[4 * lane + x]; sum += h4[x]; }
      unsigned v = sum;
      for (int o = 1; o < SEL_WAVE; o <<= 1) {
        const unsigned t = __shfl_down(v, (unsigned)o);
        if (lane + o < SEL_WAVE) v += t;
      }
      unsigned above = v - sum;
#pragma unroll
      for (int x = 3; x >= 0; --x) {
        if (above < need && need <= above + h4[x]) { s.sel[0] = 4u * lane + (unsigned)x; s.sel[1] = need - above; s.sel[2] = h4[x]; }
        above += h4[x];
      }
    }
    __syncthreads();
    const unsigned digit = s.sel[0];
    need = s.sel[1];
    if (high) T.hi |= (unsigned long long)digit << sh;
    else T.lo |= digit << sh;
    if (need == s.sel[2]) break;  // the whole bucket is wanted
  }
  return T;
}

}  // namespace urcco
