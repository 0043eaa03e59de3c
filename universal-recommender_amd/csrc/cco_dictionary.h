// Growable device dictionary (decision D26 of DESIGN.md 7a; include/urcco.h urcco_dev_dictionary_extend): a batch of keys against a LIVE key table -- the
// keys it knows keep their ids, the keys it does not know get the next ids in order of first appearance in the batch, and the table grows by rehashing
// when the batch could push its load beyond one half.  Compiled into ingest_kernels.hip behind cco_props.h: it uses that file's ig_mix, ig_find, ig_grid
// and IG_EMPTY, and the tiled scan.
//
// The state after build(S0), extend(B1), ..., extend(Bk) answers every lookup as the table of one build over S0 ++ B1 ++ ... ++ Bk with min_count = 1.
//
// THE INVARIANT.  In a table that extend accepts (built with min_count = 1) every claimed slot has id >= 0 between two calls: the build's and every extend's
// assign pass gives each slot claimed in that call its id before the call returns.  Inside a call, id < 0 on a claimed slot therefore means "claimed in THIS
// call", and such a slot was empty before: its minpos still holds the ~0 it was initialised with, so the position minimum of the batch starts from a clean
// word.  A slot claimed in an earlier call has id >= 0; its minpos (a position of an earlier batch) and its count are stale and are NEVER read again --
// dx_insert_kernel and dx_firsts_kernel test the id first.  The rehash moves (key, id) alone and gives the new table no count array at all.
//
//   dx_reserved_kernel   gate[0] = the selected positions that hold the reserved key ~0.  It runs before the first CAS: the build can throw its table away,
//                        this call cannot, so dx_insert_kernel touches nothing when gate[0] != 0 and the host refuses the call
//   dx_insert_kernel     a key found with id >= 0 is an OLD key: it is read and left alone -- no CAS, no atomicMin -- and its id goes straight into ids[p].
//                        The hot keys of a live stream are old keys, so the common event costs one probe and no atomic.  A key not found is claimed by CAS;
//                        the minimum of its batch positions is kept with the read-first atomicMin of ig_insert_kernel (a stale read costs one unnecessary
//                        atomic, never a wrong result).  flag[p] = 1 for such a candidate, else 0; ids[p] = DX_PENDING for it
//   dx_firsts_kernel     candidates only: flag[p] = (id[slot] < 0 && minpos[slot] == p) -- the first appearance of a key that is new in this call
//   launch_scan_i32      the rank of each first among the firsts; prefix[n] = the number of new ids
//   dx_assign_kernel     id[slot] = n_before + rank, new_pos[rank] = p
//   dx_ids_kernel        the positions left DX_PENDING get their key's fresh id: one more probe for the new keys' events only
//   dx_rehash_kernel     every (key, id) pair with id >= 0 into a fresh table, one CAS per pair (keys are distinct: a CAS never meets its own key)
// No wave primitive is used: the kernels run unchanged on the host simulator.  Slot placement depends on the order in which the CASs land and on the
// batching (a rehash re-homes every key); no result does: ids follow batch positions, which the minimum makes independent of the winners.
namespace urcco {

namespace {
constexpr int32_t DX_PENDING = -2;  // ids[p] between dx_insert_kernel and dx_ids_kernel: the key is new in this call
}

__global__ __launch_bounds__(256) void dx_reserved_kernel(int64_t n, const unsigned long long* __restrict__ keys, const int32_t* __restrict__ select,
                                                          unsigned* __restrict__ gate) {
  unsigned n_reserved = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256)
    if (!(select && select[p] < 0) && keys[p] == IG_EMPTY) ++n_reserved;
  if (n_reserved) atomicAdd(gate, n_reserved);
}

__global__ __launch_bounds__(256) void dx_insert_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys,
                                                        const int32_t* __restrict__ select, const unsigned* __restrict__ gate,
                                                        int32_t* __restrict__ flag, int32_t* __restrict__ ids) {
  if (gate[0]) return;  // the batch holds the reserved key: the table stays as it is (uniform over the grid)
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    int32_t id = -1;
    int f = 0;
    if (!(select && select[p] < 0)) {
      const unsigned long long key = keys[p];
      unsigned long long slot = ig_mix(key) & t.mask;
      for (;;) {
        unsigned long long cur = t.keys[slot];
        if (cur == IG_EMPTY) cur = atomicCAS(&t.keys[slot], IG_EMPTY, key);
        if (cur == key) {
          id = t.id[slot];  // >= 0: an old key, done.  (No pass before dx_assign_kernel writes an id: the read cannot be stale)
          if (id >= 0) break;
        }
        if (cur == IG_EMPTY || cur == key) {  // new in this call: claimed here, or by another position of the batch
          if ((unsigned)p < t.minpos[slot]) atomicMin(&t.minpos[slot], (unsigned)p);
          id = DX_PENDING;
          f = 1;
          break;
        }
        slot = (slot + 1) & t.mask;
      }
    }
    flag[p] = f;
    if (ids) ids[p] = id;
  }
}

__global__ __launch_bounds__(256) void dx_firsts_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ gate,
                                                        int32_t* __restrict__ flag) {
  if (gate[0]) return;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    if (!flag[p]) continue;
    const unsigned long long slot = ig_find(t, keys[p]);
    flag[p] = t.id[slot] < 0 && t.minpos[slot] == (unsigned)p;
  }
}

__global__ __launch_bounds__(256) void dx_assign_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ gate,
                                                        const int32_t* __restrict__ flag, const int64_t* __restrict__ prefix, int64_t n_before,
                                                        int64_t* __restrict__ new_pos) {
  if (gate[0]) return;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    if (!flag[p]) continue;
    const int64_t rank = prefix[p];  // < the number of firsts <= n: inside new_pos
    t.id[ig_find(t, keys[p])] = (int32_t)(n_before + rank);
    new_pos[rank] = p;
  }
}

__global__ __launch_bounds__(256) void dx_ids_kernel(KeyTable t, int64_t n, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ gate,
                                                     int32_t* __restrict__ ids) {
  if (gate[0]) return;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256)
    if (ids[p] == DX_PENDING) ids[p] = t.id[ig_find(t, keys[p])];
}

// `to`: keys ~0, minpos ~0, id -1 throughout, at least twice as many slots as `from` holds pairs
__global__ __launch_bounds__(256) void dx_rehash_kernel(KeyTable from, KeyTable to) {
  const int64_t cap = (int64_t)from.mask + 1;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < cap; s += (int64_t)gridDim.x * 256) {
    const unsigned long long key = from.keys[s];
    if (key == IG_EMPTY) continue;
    const int32_t id = from.id[s];
    if (id < 0) continue;  // (the invariant: no such slot between two calls)
    unsigned long long slot = ig_mix(key) & to.mask;
    for (;;) {
      if (to.keys[slot] == IG_EMPTY && atomicCAS(&to.keys[slot], IG_EMPTY, key) == IG_EMPTY) break;
      slot = (slot + 1) & to.mask;
    }
    to.id[slot] = id;
  }
}

hipError_t launch_dictionary_rehash(hipStream_t st, int n_cu, KeyTable from, KeyTable to) {
  hipLaunchKernelGGL(dx_rehash_kernel, dim3(ig_grid((int64_t)from.mask + 1, n_cu)), dim3(256), 0, st, from, to);
  return hipGetLastError();
}

hipError_t launch_dictionary_extend(hipStream_t st, int n_cu, const DictExtend& a) {
  hipError_t e = hipMemsetAsync(a.gate, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  if (a.n == 0) return hipMemsetAsync(a.prefix, 0, sizeof(int64_t), st);
  const dim3 grid(ig_grid(a.n, n_cu)), block(256);
  hipLaunchKernelGGL(dx_reserved_kernel, grid, block, 0, st, a.n, a.keys, a.select, a.gate);
  hipLaunchKernelGGL(dx_insert_kernel, grid, block, 0, st, a.t, a.n, a.keys, a.select, a.gate, a.flag, a.ids);
  hipLaunchKernelGGL(dx_firsts_kernel, grid, block, 0, st, a.t, a.n, a.keys, a.gate, a.flag);
  e = launch_scan_i32(st, a.flag, a.n, a.prefix, a.tile_sums);  // (over words nobody wrote when the gate is shut: the host drops the sum)
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dx_assign_kernel, grid, block, 0, st, a.t, a.n, a.keys, a.gate, a.flag, a.prefix, a.n_before, a.new_pos);
  if (a.ids) hipLaunchKernelGGL(dx_ids_kernel, grid, block, 0, st, a.t, a.n, a.keys, a.gate, a.ids);
  return hipGetLastError();
}

}  // namespace urcco
