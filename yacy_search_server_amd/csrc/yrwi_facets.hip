// yrwi_facets.hip -- the kernels of yrwi_host_facets_batch (yrwi_facets.cpp): the hosts of the
// joined container of every query of a call and how many postings each has.
//
// A group-by over (query, host) of all the containers at once:
//   k_facet_keys    one thread per container row, tiles of LR_TILE as k_local_count has them:
//                   key = (query << 36) | host36(dictionary key of the row's url id), value = the
//                   url id; a row an exclusion removed gets the sentinel nq << 36, which sorts
//                   behind every kept row -- no compaction, no wait before the sort
//   sort            one stable radix sort of the pairs over bits [0, 36 + bits(nq))
//   k_facet_flag    the first element of every (query, host) run, and the first element that
//                   is no kept row (the terminal: it closes the last run), by a look at the
//                   left neighbour -- a run that crosses a workgroup edge is no special case
//   scan            exclusive sum of the flags: the run of every head
//   k_facet_runs    per run its key, where it starts and its first value: a container ascends
//                   in url id and the sort is stable, so that is the host's smallest url hash
//   k_facet_query   per query a binary search of the run keys: its first run, its hosts, and
//                   how many of them the call writes
//   scan            those into host_off
// and, once the host knows the number of runs and the total,
//   k_facet_order   YRWI_FACETS_BY_COUNT: (query << 26) | (2^26 - 1 - count) per run, sorted
//                   stably -- equal counts stay in host order
//   k_facet_pack    per written host its six characters, its count and its url hash
// No atomics anywhere: every word has one writer.
#include <hipcub/hipcub.hpp>

#include "yrwi_device.h"
#include "yrwi_internal.h"

namespace yrwi {

namespace {

constexpr uint64_t HOST_MASK = (1ull << 36) - 1;

unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

// the keep test of k_local_count (local_keep, yrwi_kernels.hip)
__device__ __forceinline__ bool facet_keep(const LocalJob& J, int64_t i) {
  const gmem_u8* removed = (const gmem_u8*)(uintptr_t)J.removed;
  return i < J.n && !(removed && removed[i]);
}

__global__ __launch_bounds__(LR_TILE) void k_facet_keys(const LocalJob* __restrict__ jobs,
                                                        const int64_t* __restrict__ tile_base,
                                                        const int64_t* __restrict__ row_base, int32_t njobs,
                                                        const uint64_t* __restrict__ dkhi,
                                                        const uint8_t* __restrict__ dklo, uint64_t sentinel,
                                                        uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const int64_t t = blockIdx.x;
  const int32_t j = seg_of<int32_t>(tile_base, 0, njobs - 1, t);
  const LocalJob& J = jobs[j];
  const int64_t i = (t - J.tile0) * LR_TILE + threadIdx.x;
  if (i >= J.n) return;
  uint64_t k = sentinel;
  uint32_t u = 0;
  if (facet_keep(J, i)) {
    u = ((const gmem_u32*)(uintptr_t)J.uid)[i];
    k = ((uint64_t)(uint32_t)J.evjob << 36) | host36(dkhi[u], dklo[u]);
  }
  key[row_base[j] + i] = k;
  val[row_base[j] + i] = u;
}

// flag[i], i <= n, over the sorted keys: 1 on the first element of a run of kept rows and on the
// terminal, the first position that holds no kept row (n when every row is kept)
__global__ __launch_bounds__(256) void k_facet_flag(const uint64_t* __restrict__ key, int64_t n, uint64_t sentinel,
                                                    int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  const bool real = i < n && key[i] < sentinel;
  const bool left_real = i > 0 && key[i - 1] < sentinel;
  flag[i] = real ? (i == 0 || key[i] != key[i - 1]) : (i == 0 || left_real);
}

// run r = hx[i] of head i: its key, its first position and its first value; the terminal's run
// holds the sentinel and the number of kept rows, so run r has rpos[r + 1] - rpos[r] rows
__global__ __launch_bounds__(256) void k_facet_runs(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                    int64_t n, uint64_t sentinel, const int32_t* __restrict__ flag,
                                                    const int64_t* __restrict__ hx, uint64_t* __restrict__ rkey,
                                                    uint32_t* __restrict__ rpos, uint32_t* __restrict__ ruid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n || !flag[i]) return;
  const int64_t r = hx[i];
  const bool real = i < n && key[i] < sentinel;
  rkey[r] = real ? key[i] : sentinel;
  rpos[r] = (uint32_t)i;
  ruid[r] = real ? val[i] : 0u;
}

// first run of [0, nruns) whose key is not below k
__device__ __forceinline__ int64_t facet_lb(const uint64_t* __restrict__ rkey, int64_t nruns, uint64_t k) {
  int64_t lo = 0, hi = nruns;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rkey[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// query q <= nq: qstart[q] = its first run (the runs are in query order; hx[n] = their number);
// q < nq: nhosts[q] = its runs, nwrite[q] = min(nhosts[q], max_hosts), all of them for
// max_hosts == 0; nwrite[nq] = 0, the last element of the scan that gives host_off
__global__ __launch_bounds__(256) void k_facet_query(const uint64_t* __restrict__ rkey, const int64_t* __restrict__ hx,
                                                     int64_t n, int32_t nq, int32_t max_hosts,
                                                     int64_t* __restrict__ qstart, int64_t* __restrict__ nhosts,
                                                     int64_t* __restrict__ nwrite) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q > nq) return;
  const int64_t nruns = hx[n];
  const int64_t a = facet_lb(rkey, nruns, (uint64_t)q << 36);
  qstart[q] = a;
  if (q == nq) {
    nwrite[q] = 0;
    return;
  }
  const int64_t h = facet_lb(rkey, nruns, (uint64_t)(q + 1) << 36) - a;
  nhosts[q] = h;
  nwrite[q] = max_hosts > 0 && h > max_hosts ? max_hosts : h;
}

__global__ __launch_bounds__(256) void k_facet_order(const uint64_t* __restrict__ rkey,
                                                     const uint32_t* __restrict__ rpos, int64_t nruns,
                                                     uint64_t* __restrict__ okey, uint32_t* __restrict__ oval) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nruns) return;
  const uint64_t cnt = rpos[r + 1] - rpos[r];  // at most MAX_LIST = 53,687,091 < 2^26
  okey[r] = ((rkey[r] >> 36) << 26) | (((1ull << 26) - 1) - cnt);
  oval[r] = (uint32_t)r;
}

// written host j < total: the host at rank j - host_off[q] of its query q, in host order (perm ==
// nullptr) or in the order of k_facet_order's sort.  hosts6 in three 16-bit words, urls12 in three
// 32-bit words (urls12 == nullptr: not asked for).
__global__ __launch_bounds__(256) void k_facet_pack(const int64_t* __restrict__ host_off, int32_t nq, int64_t total,
                                                    const int64_t* __restrict__ qstart,
                                                    const uint32_t* __restrict__ perm,
                                                    const uint64_t* __restrict__ rkey,
                                                    const uint32_t* __restrict__ rpos,
                                                    const uint32_t* __restrict__ ruid,
                                                    const uint64_t* __restrict__ dkhi, const uint8_t* __restrict__ dklo,
                                                    uint16_t* __restrict__ hosts6, int64_t* __restrict__ counts,
                                                    uint32_t* __restrict__ urls12) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= total) return;
  const int32_t q = seg_of<int32_t>(host_off, 0, nq - 1, j);  // the last query that starts at or before j
  const int64_t s = qstart[q] + (j - host_off[q]);
  const int64_t r = perm ? (int64_t)perm[s] : s;
  const uint64_t h = rkey[r] & HOST_MASK;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t c0 = b64_char((uint32_t)(h >> (6 * (5 - 2 * k))) & 63u);
    const uint32_t c1 = b64_char((uint32_t)(h >> (6 * (4 - 2 * k))) & 63u);
    hosts6[j * 3 + k] = (uint16_t)(c0 | (c1 << 8));
  }
  counts[j] = (int64_t)(rpos[r + 1] - rpos[r]);
  if (!urls12) return;
  const uint32_t u = ruid[r];
  const uint64_t hi = dkhi[u];
  const uint32_t lo = dklo[u];
  const uint64_t x = hi >> 4;
  uint32_t w[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 12; c++) {  // key_chars' rule (yrwi_host.h)
    const uint32_t v = c < 10 ? (uint32_t)(x >> (6 * (9 - c))) & 63u
                              : c == 10 ? (((uint32_t)hi & 15u) << 2) | (lo >> 6) : lo & 63u;
    w[c >> 2] |= b64_char(v) << (8 * (c & 3));
  }
#pragma unroll
  for (int k = 0; k < 3; k++) urls12[j * 3 + k] = w[k];
}

int rc(hipError_t e) { return e == hipSuccess ? 0 : -1; }

}  // namespace

int facet_key_bits(int32_t nq) {
  int b = 1;
  while (b < 28 && ((int64_t)1 << b) <= (int64_t)nq) b++;  // the sentinel nq is the largest query value
  return b;
}

size_t facet_tmp_bytes(int64_t n, int32_t nq) {
  uint64_t* k = nullptr;
  uint32_t* v = nullptr;
  int32_t* f = nullptr;
  int64_t* x = nullptr;
  size_t a = 0, c = 0, d = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, k, v, v, (int)n, 0, 36 + facet_key_bits(nq), nullptr) !=
          hipSuccess ||
      hipcub::DeviceScan::ExclusiveSum(nullptr, c, f, x, (int)(n + 1), nullptr) != hipSuccess ||
      hipcub::DeviceScan::ExclusiveSum(nullptr, d, x, x, (int)nq + 1, nullptr) != hipSuccess)
    return 0;
  return std::max(std::max(a, c), std::max(d, (size_t)256));
}

size_t facet_order_tmp_bytes(int64_t nruns, int32_t nq) {
  uint64_t* k = nullptr;
  uint32_t* v = nullptr;
  size_t b = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, b, k, k, v, v, (int)nruns, 0, 26 + facet_key_bits(nq), nullptr) !=
      hipSuccess)
    return 0;
  return std::max(b, (size_t)256);
}

int launch_facet_group(const FacetDev& F, void* st) {
  hipStream_t s = static_cast<hipStream_t>(st);
  if (F.njobs <= 0 || F.tiles <= 0 || F.n <= 0 || F.nq <= 0) return 0;
  if (F.tiles > 0x7FFFFFFFLL || F.n >= 0x7FFFFFFFLL) return -1;
  const uint64_t sentinel = (uint64_t)(uint32_t)F.nq << 36;
  hipLaunchKernelGGL(k_facet_keys, dim3((unsigned)F.tiles), dim3(LR_TILE), 0, s, F.jobs, F.tile_base, F.row_base,
                     F.njobs, F.dkhi, F.dklo, sentinel, F.key, F.val);
  size_t tb = F.tmp_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(F.tmp, tb, F.key, F.skey, F.val, F.sval, (int)F.n, 0,
                                         36 + facet_key_bits(F.nq), s) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(k_facet_flag, dim3(nblk(F.n + 1)), dim3(256), 0, s, F.skey, F.n, sentinel, F.flag);
  tb = F.tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(F.tmp, tb, F.flag, F.hx, (int)(F.n + 1), s) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_facet_runs, dim3(nblk(F.n + 1)), dim3(256), 0, s, F.skey, F.sval, F.n, sentinel, F.flag, F.hx,
                     F.rkey, F.rpos, F.ruid);
  hipLaunchKernelGGL(k_facet_query, dim3(nblk((int64_t)F.nq + 1)), dim3(256), 0, s, F.rkey, F.hx, F.n, F.nq,
                     F.max_hosts, F.qstart, F.nhosts, F.nwrite);
  tb = F.tmp_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(F.tmp, tb, F.nwrite, F.host_off, (int)F.nq + 1, s) != hipSuccess) return -1;
  return rc(hipGetLastError());
}

int launch_facet_order(const FacetDev& F, int64_t nruns, void* tmp, size_t tmp_bytes, void* st) {
  hipStream_t s = static_cast<hipStream_t>(st);
  if (nruns <= 0 || nruns > F.n || !tmp) return -1;
  // the element arrays are free again: the runs have their own copies
  hipLaunchKernelGGL(k_facet_order, dim3(nblk(nruns)), dim3(256), 0, s, F.rkey, F.rpos, nruns, F.key, F.val);
  size_t tb = tmp_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(tmp, tb, F.key, F.skey, F.val, F.sval, (int)nruns, 0,
                                         26 + facet_key_bits(F.nq), s) != hipSuccess)
    return -1;
  return rc(hipGetLastError());
}

int launch_facet_pack(const FacetDev& F, int64_t total, bool by_count, uint8_t* d_hosts6, int64_t* d_counts,
                      uint8_t* d_urls12, void* st) {
  hipStream_t s = static_cast<hipStream_t>(st);
  if (total <= 0) return 0;
  hipLaunchKernelGGL(k_facet_pack, dim3(nblk(total)), dim3(256), 0, s, F.host_off, F.nq, total, F.qstart,
                     by_count ? F.sval : nullptr, F.rkey, F.rpos, F.ruid, F.dkhi, F.dklo,
                     reinterpret_cast<uint16_t*>(d_hosts6), d_counts, reinterpret_cast<uint32_t*>(d_urls12));
  return rc(hipGetLastError());
}

}  // namespace yrwi
