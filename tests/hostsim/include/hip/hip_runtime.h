// TEST-ONLY host simulator of the HIP subset used by universal-recommender_amd/csrc.
//
// This header is NOT part of the product and is never on the include path of the shipped library
// (liburcco.so is built by hipcc for gfx950 only and fails loudly without a GPU).  It exists because
// the build container has no GPU: compiling the *unchanged* kernel sources against this header with g++
// lets the CPU test-suite exercise kernel LOGIC (indexing, hashing, compaction, selection, the C-ABI
// orchestration) before a scarce MI355X slot is spent.  Parity claims are made only by the `-m gpu`
// tests on real hardware.
//
// Model: a block's threads are fibers on one OS thread; blocks are spread over OS threads (OpenMP).
//  * __syncthreads() parks a fiber until every live fiber of the block is parked at the barrier.
//  * wave ops (__ballot/__shfl*) park a fiber until every live lane of its 64-wide wave is parked;
//    lanes parked at the same wave op then exchange values (lanes that exited or sit at a block
//    barrier are inactive, as on hardware).  All lanes must sit at the SAME call site, else abort:
//    kernels are required to call wave ops under wave-uniform control flow.
//  * `__shared__` is `static thread_local` (one copy per OS thread == per running block).
//  * atomics are real (__atomic builtins), global memory is the host heap.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <type_traits>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __shared__ static thread_local
#define __constant__ static const

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
struct alignas(8) int2 { int x, y; };
struct alignas(8) uint2 { unsigned x, y; };
static inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
static inline int2 make_int2(int x, int y) { return int2{x, y}; }
static inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }

typedef int hipError_t;
enum { hipErrorNotReady = 600, hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1, hipErrorNoDevice = 100, hipErrorInvalidDevice = 101, hipErrorInvalidHandle = 400,
       hipErrorUnknown = 999 };
// Devices are modelled as far as the host code can get them wrong: every thread has a current device, streams and events
// belong to the device that was current when they were created, an event may only be recorded on a stream of its own device
// and a kernel may only be launched on a stream of the current device (both are errors on real HIP).
struct hipsimStream { int device; };
typedef void* hipStream_t;
struct hipsimEvent { std::chrono::steady_clock::time_point t; int device; };
typedef hipsimEvent* hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
struct hipDeviceProp_t { int multiProcessorCount; char name[64]; char gcnArchName[64]; size_t totalGlobalMem; };

namespace hipsim {
struct Idx { unsigned x, y, z; };
extern thread_local Idx tIdx, bIdx, bDim, gDim;
void launch(dim3 grid, dim3 block, const std::function<void()>& body);
extern thread_local int cur_device;
extern thread_local int last_error;  // sticky until read by hipGetLastError
static inline int stream_device(void* st) { return st ? static_cast<hipsimStream*>(st)->device : cur_device; }
void sync_threads();
enum WaveOp { OP_BALLOT = 1, OP_SHFL = 2 };
uint64_t wave_op(int op, uint64_t payload, int arg, const void* site);
int lane_id();
// HIPSIM_GUARD=1 (tests/test_sim_guard.py): every hipMalloc ends (to 16 bytes) at a PROT_NONE page, and the session arena places every
// sub-buffer the same way, so that a kernel reading or writing past the end of a buffer faults here the way it can on the GPU.
bool guard_on();
void* guard_alloc(size_t n);
bool guard_free(void* p);                       // false: not a guarded allocation
void arena_unguard(void* base, size_t cap);     // make the whole arena read/write again (its layout is about to change)
char* arena_place(char* base, size_t off, size_t bytes, size_t* new_off);  // address of a sub-buffer ending at a guard page
constexpr size_t GUARD_PAGE = 4096;
// Live-object counters (tests/test_sim_resources.py): what the library has created and not yet given back, read through hipsim_live(kind).
enum LiveKind { LIVE_DEVICE = 0, LIVE_HOST = 1, LIVE_EVENT = 2, LIVE_STREAM = 3, LIVE_KINDS = 4 };
void live_add(int kind, long long delta);
static inline void* raw_alloc(size_t n, int kind) {
  void* p = guard_on() ? guard_alloc(n ? n : 1) : malloc(n ? n : 1);
  if (p) live_add(kind, 1);
  return p;
}
static inline void raw_free(void* p, int kind) {
  if (!p) return;
  live_add(kind, -1);
  if (!guard_free(p)) free(p);
}
}  // namespace hipsim
#define HIPSIM_HOST_BUILD 1

#define threadIdx (hipsim::tIdx)
#define blockIdx (hipsim::bIdx)
#define blockDim (hipsim::bDim)
#define gridDim (hipsim::gDim)
#define warpSize 64

#define hipLaunchKernelGGL(kern, grid, block, shmem, stream, ...) \
  do {                                                                                                              \
    if (hipsim::stream_device(stream) != hipsim::cur_device) hipsim::last_error = hipErrorInvalidHandle;             \
    else hipsim::launch(dim3(grid), dim3(block), [=]() { kern(__VA_ARGS__); });                                      \
  } while (0)

static inline void __syncthreads() { hipsim::sync_threads(); }

// Wave ops are identified by their SOURCE LINE (g++ may duplicate a call site by jump threading / loop unswitching,
// so a return address would not identify the source-level operation).
#define HIPSIM_SITE(line) (reinterpret_cast<const void*>(static_cast<uintptr_t>(line)))
static inline unsigned long long hipsim_ballot(int line, int pred) {
  return hipsim::wave_op(hipsim::OP_BALLOT, pred ? 1 : 0, 0, HIPSIM_SITE(line));
}
#define __ballot(...) hipsim_ballot(__LINE__, __VA_ARGS__)
template <typename T>
static inline T hipsim_shfl(int line, T v, int src, int width = 64) {
  static_assert(sizeof(T) <= 8, "shfl payload");
  uint64_t p = 0;
  memcpy(&p, &v, sizeof(T));
  int lane = hipsim::lane_id();
  int s = (lane & ~(width - 1)) | (src & (width - 1));
  uint64_t r = hipsim::wave_op(hipsim::OP_SHFL, p, s, HIPSIM_SITE(line));
  T out;
  memcpy(&out, &r, sizeof(T));
  return out;
}
template <typename T>
static inline T hipsim_shfl_xor(int line, T v, int mask, int width = 64) {
  uint64_t p = 0;
  memcpy(&p, &v, sizeof(T));
  int lane = hipsim::lane_id();
  int s = lane ^ mask;
  if ((s & ~(width - 1)) != (lane & ~(width - 1))) s = lane;
  uint64_t r = hipsim::wave_op(hipsim::OP_SHFL, p, s, HIPSIM_SITE(line));
  T out;
  memcpy(&out, &r, sizeof(T));
  return out;
}
template <typename T>
static inline T hipsim_shfl_down(int line, T v, unsigned delta, int width = 64) {
  uint64_t p = 0;
  memcpy(&p, &v, sizeof(T));
  int lane = hipsim::lane_id();
  int s = lane + (int)delta;
  if ((s & ~(width - 1)) != (lane & ~(width - 1))) s = lane;
  uint64_t r = hipsim::wave_op(hipsim::OP_SHFL, p, s, HIPSIM_SITE(line));
  T out;
  memcpy(&out, &r, sizeof(T));
  return out;
}
template <typename T>
static inline T hipsim_shfl_up(int line, T v, unsigned delta, int width = 64) {
  uint64_t p = 0;
  memcpy(&p, &v, sizeof(T));
  int lane = hipsim::lane_id();
  int s = lane - (int)delta;
  if (s < 0 || (s & ~(width - 1)) != (lane & ~(width - 1))) s = lane;
  uint64_t r = hipsim::wave_op(hipsim::OP_SHFL, p, s, HIPSIM_SITE(line));
  T out;
  memcpy(&out, &r, sizeof(T));
  return out;
}

#define __shfl(...) hipsim_shfl(__LINE__, __VA_ARGS__)
#define __shfl_xor(...) hipsim_shfl_xor(__LINE__, __VA_ARGS__)
#define __shfl_down(...) hipsim_shfl_down(__LINE__, __VA_ARGS__)
#define __shfl_up(...) hipsim_shfl_up(__LINE__, __VA_ARGS__)

static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline int __ffsll(unsigned long long x) { return __builtin_ffsll((long long)x); }
static inline int __clz(int x) { return x == 0 ? 32 : __builtin_clz((unsigned)x); }
static inline int __clzll(long long x) { return x == 0 ? 64 : __builtin_clzll((unsigned long long)x); }
static inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, 8); return r; }
static inline double __longlong_as_double(long long l) { double r; memcpy(&r, &l, 8); return r; }
static inline int __double2hiint(double d) { return (int)(__double_as_longlong(d) >> 32); }
static inline int __double2loint(double d) { return (int)(__double_as_longlong(d) & 0xffffffffll); }
static inline double __hiloint2double(int hi, int lo) {
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

// ---- atomics (relaxed, device scope) -------------------------------------------------------
template <typename T> static inline T atomicAdd(T* p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <typename T> static inline T atomicSub(T* p, T v) { return __atomic_fetch_sub(p, v, __ATOMIC_RELAXED); }
template <typename T> static inline T atomicOr(T* p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
template <typename T> static inline T atomicAnd(T* p, T v) { return __atomic_fetch_and(p, v, __ATOMIC_RELAXED); }
template <typename T> static inline T atomicExch(T* p, T v) { return __atomic_exchange_n(p, v, __ATOMIC_RELAXED); }
template <typename T> static inline T atomicCAS(T* p, T cmp, T v) {
  __atomic_compare_exchange_n(p, &cmp, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
  return cmp;
}
template <typename T> static inline T atomicMax(T* p, T v) {
  T old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
template <typename T> static inline T atomicMin(T* p, T v) {
  T old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
#define __HIP_MEMORY_SCOPE_SINGLETHREAD 1
#define __HIP_MEMORY_SCOPE_WAVEFRONT 2
#define __HIP_MEMORY_SCOPE_WORKGROUP 3
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __HIP_MEMORY_SCOPE_SYSTEM 5
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n(p, v, order)
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add(p, v, order)
static inline void __threadfence() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }
static inline void __threadfence_block() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }
static inline void __builtin_amdgcn_s_sleep(int) {}
#define __builtin_amdgcn_fence(order, scope) ((void)0)
static inline void hipsim_wave_barrier(int line) { hipsim::wave_op(hipsim::OP_BALLOT, 0, 0, HIPSIM_SITE(line)); }
#define __builtin_amdgcn_wave_barrier() hipsim_wave_barrier(__LINE__)

// DPP (data-parallel primitives) of GFX9: row_shr:n (0x110 + n), row_shl:n (0x100 + n) inside rows of 16 lanes, row_bcast15
// (0x142: lane 15 of a row -> the next row) and row_bcast31 (0x143: lane 31 -> rows 2 and 3).  A lane that is masked off
// by row_mask / bank_mask keeps `old`; a lane whose source falls outside its row gets 0 (bound_ctrl) or `old`.
static inline int hipsim_update_dpp(int line, int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
  const int lane = hipsim::lane_id();
  const int row = lane >> 4, bank = (lane >> 2) & 3;
  int s = -1;
  if (ctrl > 0x110 && ctrl <= 0x11f) { const int n = ctrl - 0x110; s = (lane & 15) >= n ? lane - n : -1; }
  else if (ctrl > 0x100 && ctrl <= 0x10f) { const int n = ctrl - 0x100; s = (lane & 15) + n < 16 ? lane + n : -1; }
  else if (ctrl == 0x142) s = row >= 1 ? row * 16 - 1 : -1;
  else if (ctrl == 0x143) s = lane >= 32 ? 31 : -1;
  else abort();
  uint64_t p = (uint32_t)src;
  const uint64_t r = hipsim::wave_op(hipsim::OP_SHFL, p, s < 0 ? lane : s, HIPSIM_SITE(line));
  if (!((row_mask >> row) & 1) || !((bank_mask >> bank) & 1)) return old;
  if (s < 0) return bound_ctrl ? 0 : old;
  return (int)(uint32_t)r;
}
#define __builtin_amdgcn_update_dpp(...) hipsim_update_dpp(__LINE__, __VA_ARGS__)
#define __builtin_amdgcn_readlane(v, l) hipsim_shfl(__LINE__, (int)(v), (int)(l))
#define __builtin_amdgcn_ds_bpermute(addr, v) hipsim_shfl(__LINE__, (int)(v), ((int)(addr) >> 2) & 63)  /* byte address of the source lane */
#define __builtin_amdgcn_readfirstlane(v) (v)  /* only ever applied to wave-uniform values */
static inline unsigned __builtin_amdgcn_mbcnt_lo(unsigned mask, unsigned base) {
  const int lane = hipsim::lane_id();
  return base + (unsigned)__builtin_popcount(mask & (lane >= 32 ? 0xffffffffu : ((1u << lane) - 1u)));
}
static inline unsigned __builtin_amdgcn_mbcnt_hi(unsigned mask, unsigned base) {
  const int lane = hipsim::lane_id();
  return base + (unsigned)__builtin_popcount(mask & (lane <= 32 ? 0u : ((1u << (lane - 32)) - 1u)));
}

// ---- runtime API ---------------------------------------------------------------------------
static inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "hipSuccess(sim)" : "hipError(sim)"; }
static inline hipError_t hipGetLastError() { const int e = hipsim::last_error; hipsim::last_error = hipSuccess; return e; }
static inline hipError_t hipPeekAtLastError() { return hipSuccess; }
static inline hipError_t hipMalloc(void** p, size_t n) { *p = hipsim::raw_alloc(n, hipsim::LIVE_DEVICE); return *p ? hipSuccess : hipErrorOutOfMemory; }
template <typename T> static inline hipError_t hipMalloc(T** p, size_t n) { return hipMalloc((void**)p, n); }
static inline hipError_t hipFree(void* p) { hipsim::raw_free(p, hipsim::LIVE_DEVICE); return hipSuccess; }
enum { hipHostMallocDefault = 0, hipHostMallocPortable = 1, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000 };
static inline hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) { *dev = host; return hipSuccess; }
static inline hipError_t hipHostMalloc(void** p, size_t n, unsigned = 0) { *p = hipsim::raw_alloc(n, hipsim::LIVE_HOST); return *p ? hipSuccess : hipErrorOutOfMemory; }
static inline hipError_t hipHostFree(void* p) { hipsim::raw_free(p, hipsim::LIVE_HOST); return hipSuccess; }
static inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { if (n) memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t = nullptr) { if (n) memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipMemset(void* d, int v, size_t n) { if (n) memset(d, v, n); return hipSuccess; }
static inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t = nullptr) { if (n) memset(d, v, n); return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
static inline hipError_t hipStreamCreate(hipStream_t* s) { *s = new hipsimStream{hipsim::cur_device}; hipsim::live_add(hipsim::LIVE_STREAM, 1); return hipSuccess; }
static inline hipError_t hipStreamDestroy(hipStream_t s) { if (s) hipsim::live_add(hipsim::LIVE_STREAM, -1); delete static_cast<hipsimStream*>(s); return hipSuccess; }
enum { hipStreamDefault = 0, hipStreamNonBlocking = 1 };
static inline hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) { *least = 0; *greatest = 0; return hipSuccess; }
static inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return hipStreamCreate(s); }
static inline hipError_t hipGetDeviceCount(int* n);
static inline hipError_t hipSetDevice(int d) {
  int n = 1;
  hipGetDeviceCount(&n);
  if (d < 0 || d >= n) return hipErrorInvalidDevice;
  hipsim::cur_device = d;
  return hipSuccess;
}
static inline hipError_t hipGetDevice(int* d) { *d = hipsim::cur_device; return hipSuccess; }
static inline hipError_t hipGetDeviceCount(int* n) {  // HIPSIM_DEVICE_COUNT: pretend to hold several GPUs (multi-GPU orchestration tests)
  const char* e = getenv("HIPSIM_DEVICE_COUNT");
  *n = e ? atoi(e) : 1;
  if (*n < 1) *n = 1;
  return hipSuccess;
}
static inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {
  memset(p, 0, sizeof(*p));
  p->multiProcessorCount = 8;
  strcpy(p->name, "hostsim");
  strcpy(p->gcnArchName, "hostsim");
  p->totalGlobalMem = (size_t)8 << 30;
  return hipSuccess;
}
template <typename F> static inline hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, F, int, size_t) { *n = 2; return hipSuccess; }
static inline hipError_t hipEventCreate(hipEvent_t* e) { *e = new hipsimEvent(); (*e)->device = hipsim::cur_device; hipsim::live_add(hipsim::LIVE_EVENT, 1); return hipSuccess; }
enum { hipEventDefault = 0, hipEventDisableTiming = 2 };
static inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
static inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t e) { if (e) hipsim::live_add(hipsim::LIVE_EVENT, -1); delete e; return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t st = nullptr) {
  if (e->device != hipsim::stream_device(st)) return hipErrorInvalidHandle;  // an event belongs to the device it was created on
  e->t = std::chrono::steady_clock::now();
  return hipSuccess;
}
static inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }  // the simulator executes synchronously: every recorded event has completed
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  *ms = std::chrono::duration<float, std::milli>(b->t - a->t).count();
  return hipSuccess;
}
