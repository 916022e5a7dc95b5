// yrwi_device.h -- device helpers of the index-maintenance sources (yrwi_update.hip,
// yrwi_load.hip, yrwi_dict.hip, yrwi_dump.hip, yrwi_dht.hip) and of the host facets
// (yrwi_facets.hip): the searches and copies of the code that reads or rewrites the index in
// place, each defined once.  The query path (yrwi_kernels.hip) has its own and does not
// include this.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace yrwi {

// the pointers of a job table come out of memory, so the compiler cannot know their address
// space: typed as global memory they load with global instead of flat loads
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#ifdef __HIP_DEVICE_COMPILE__
typedef u32x4 __attribute__((address_space(1))) gmem_u4;
typedef u32x2 __attribute__((address_space(1))) gmem_u2;
typedef uint64_t __attribute__((address_space(1))) gmem_u64;
typedef uint32_t __attribute__((address_space(1))) gmem_u32;
typedef uint8_t __attribute__((address_space(1))) gmem_u8;
#else
typedef u32x4 gmem_u4;
typedef u32x2 gmem_u2;
typedef uint64_t gmem_u64;
typedef uint32_t gmem_u32;
typedef uint8_t gmem_u8;
#endif

// last j in [lo, hi] with off[j] <= x (off[lo] <= x): the segment, record or cell that holds
// element x of a flattened table.  I: the caller's index type (int or int64_t).
template <class I>
__device__ __forceinline__ I seg_of(const int64_t* __restrict__ off, I lo, I hi, int64_t x) {
  while (lo < hi) {
    const I mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// 72-bit key order: (hi, lo) lexicographic
__device__ __forceinline__ bool key_lt(uint64_t ah, uint32_t al, uint64_t bh, uint32_t bl) {
  return ah < bh || (ah == bh && al < bl);
}

// first i in [lo, hi) whose key is not below (h, l), hi if there is none
__device__ __forceinline__ int64_t lb_key(const uint64_t* __restrict__ kh, const uint8_t* __restrict__ kl, int64_t lo,
                                          int64_t hi, uint64_t h, uint32_t l) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key_lt(kh[mid], kl[mid], h, l)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void copy_row(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src) {
  const uint64_t* s = reinterpret_cast<const uint64_t*>(src);  // rows are 8-byte aligned (40 B, 256 B bases)
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
#pragma unroll
  for (int i = 0; i < 5; i++) d[i] = s[i];
}

// url-hash chars 6..11 (the host hash) = the key's low 36 bits (key_host36, yrwi_kernels.hip)
__device__ __forceinline__ uint64_t host36(uint64_t hi, uint32_t lo) { return ((hi & 0xFFFFFFFull) << 8) | (lo & 0xFFu); }

// character v of Base64Order.enhancedCoder's alphabet (ALPHA, yrwi_host.h)
__device__ __forceinline__ uint32_t b64_char(uint32_t v) {
  return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '-' : '_';
}

}  // namespace yrwi
