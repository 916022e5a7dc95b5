// yrwi_update.hip -- index updates on the device: postings added and urls removed in bulk
// (IndexCell.add(termHash, entry) / add(container) / remove(termHash, urlHashes),
// Segment.removeAllUrlReferences).
//
// yrwi_add_postings: the batch is uploaded through the lane's pinned staging and keyed by
// k_validate; the host maps every row's term to a job (one per touched list); the device
// sorts the batch by (job, 72-bit url key, arrival index) with two stable radix sorts (low
// 64 key bits, then job | top 8 key bits); k_upd_pick lets the head of every run of equal
// (job, url) pick the run's winner under the policy, take its lower bound in the job's list
// and settle it against an existing row; one scan over the batch rows numbers the new keys;
// one read-back brings the per-job counts and the validation bits; the new lists come from
// index memory in one round; k_upd_old places the old rows of the changed lists (flattened
// over a prefix table) and k_upd_new the surviving batch rows.  Nothing is launched or
// waited for per term.
//
// yrwi_remove_postings: k_rm_count looks every key of the named lists up in the sorted,
// deduplicated url set and counts the hits per list (read back once); only the lists that
// lose rows are compacted (compact_commit below, flagged by k_rm_flag).
//
// yrwi_remove_hosts / yrwi_count_hosts: the predicate is the host hash, url-hash characters
// 6..11 = the low 36 bits of the 72-bit key every list stores next to its rows (host36), so
// one streaming pass (k_host_mark) over the flattened khi / klo of the selected lists, 9 B per
// posting, marks every posting of the sorted, deduplicated host set and reads no row.  The
// set is staged in LDS and searched there when it holds at most YRWI_HOST_LDS_MAX = 2048
// keys (16 KiB per workgroup); a larger set is searched in global memory; the two searches
// are the same function over another pointer.  At most 2048 workgroups each take a contiguous
// span of the flattened postings, so a workgroup stages the set once for all its postings and a
// lane looks its list up again only where it passes a list's end.  Hits are counted
// per list with one atomic per list per wave (the lanes of a list are neighbours and a wave's
// lists ascend: it sums a list's hits over its steps and adds them on leaving the list); per host
// (count_hosts only) in LDS per workgroup and then one global atomic per hit slot per
// workgroup when the set is in LDS, else one global atomic per slot per wave.  The per-list
// counts are read back once; the lists that lose rows are compacted (compact_commit, flagged by
// k_host_flag).
//
// compact_commit, the second half of both removals: from the per-list removed counts it plans the
// lists that lose rows (an emptied list needs no compaction), takes their new lists from index
// memory and compacts them in chunks: runs of whole lists of at most YRWI_RM_CHUNK rows in all
// (environment, read per call, at least 256, default 2^26; a longer list is a chunk of its own),
// each flag -> scan -> place (the caller's flag kernel, one scan, k_rm_place) in the scratch of
// the chunk before it, 12 B per row of the largest chunk, with no host wait between chunks:
// launches and syncs depend on the number of chunks alone, and nothing stops at 2^31 postings.
// Then the bookkeeping of every list that lost rows.
//
// yrwi_host_census: which hosts the selected lists hold and how many postings each, the index-wide
// form of the per-container host counts of ReferenceOrder.doms (UNVERIFIED against a reference
// line: the reference has no single method that groups the whole RWI by host).  The same streaming
// pass over the 9 key bytes of every selected posting, grid and spans as k_host_mark, but a group-by
// with an unknown key set instead of a lookup in a given one (k_census): every workgroup sums in an
// LDS table of YRWI_CENSUS_LDS_SLOTS slots (12 B each: key host36 + 1, 0 = empty, and a 32-bit
// count; a wave whose live lanes carry one host makes one LDS add, else every lane inserts with at
// most 64 probes) and adds its slots into the device table at the end of its span, one global
// atomic per host per workgroup; a posting whose lane finds no place in LDS goes straight to the
// device table, equal keys of the wave as one add (lds_bypass).  The device table is open
// addressing with linear probing, 16 B per slot, 64-bit atomicCAS / atomicAdd; an insert that finds
// no place within 128 probes sets an overflow word and drops the posting (the waves then leave
// the pass at their next step), and the host runs the
// pass again with four times the slots.  The table's hosts with at least min_postings are flagged,
// scanned, compacted and radix-sorted on the device (by the 36-bit key; BY_COUNT: then stably by
// count descending), and only the first min(hosts_passing, cap) cross PCIe.  All scratch is the
// lane's arena; 5 launches and one sync per counting pass, 5 or 6 launches and one sync after them.
//
// yrwi_url_census / yrwi_host_url_census: which urls the selected lists hold, in how many of them each, and
// the distinct urls and postings of every host; a group-by over the 4-byte url ids, described with its kernels
// behind the census of the hosts.  It shares the selection, the spans, the cursor and the frame of a pass.
//
// yrwi_retain / yrwi_retention_count: removal by the age of a posting and a cap on the length of a list;
// described with their kernels at the end of this file.  They share the selection, the spans and
// compact_commit with the host calls.
//
// yrwi_url_references: the read-only form of yrwi_remove_postings, counts and rows of the postings of a url
// set; described with its kernels at the end of this file.  It shares the selection, the spans and the
// cursor with the host calls.
//
// What the streaming passes share stands once, in front of the first kernel: the span of a workgroup (span_of,
// span_blocks, SPAN_TILE, SPAN_BLOCKS), the cursor (SegCursor), the four key loads of a step (key_tile; day_tile
// is its counterpart over the rows), the per-list sum of a wave (ListTally), equal keys of a wave as one atomic
// (wave_add_by), the search of a sorted set (set_slot, host_slot) and its staging in LDS (stage_set).  On the
// host the first pass of every call but yrwi_add_postings runs in one frame (pass_begin: a new pass, the tables
// allocated and uploaded at once, the result block zeroed; pass_end: one read-back, one wait), and the two calls
// that take urls prepare them in url_set.
//
// A changed list is a new list in index memory (the old copy is dead until repack_index,
// reached through ensure_url_ids) and goes through index_changed like a replaced list.

#include <hipcub/hipcub.hpp>

#include "yrwi_device.h"
#include "yrwi_host.h"

using namespace yrwi;

namespace {

constexpr int HOST_LDS_MAX = YRWI_HOST_LDS_MAX;         // host keys searched in LDS (8 B each)
constexpr int SPAN_TILE = 1024;    // postings a workgroup of a streaming pass takes per step: 4 per thread, their loads in flight together
constexpr int SPAN_BLOCKS = 2048;  // the grid cap of the streaming passes
constexpr int64_t RM_CHUNK_DEFAULT = (int64_t)1 << 26;  // rows compacted at a time (YRWI_RM_CHUNK)

unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// the grid of a streaming pass over n flattened postings
unsigned span_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + SPAN_TILE - 1) / SPAN_TILE, SPAN_BLOCKS); }

struct UpdJob {  // one touched list and the job's rows in the sorted batch
  const uint64_t* akhi;
  const uint8_t* aklo;
  const uint8_t* arows;
  int64_t an;
  uint64_t* okhi;
  uint8_t* oklo;
  uint8_t* orows;
  int64_t boff, bn;
};

struct RmJob {
  const uint64_t* khi;
  const uint8_t* klo;
  const uint8_t* rows;
  int64_t n;
  uint64_t* okhi;
  uint8_t* oklo;
  uint8_t* orows;
};

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Every lane of the wave holds one row to move (dstp null: none).  The wave's 64 rows are
// 320 8-byte words: in each of 5 rounds lane l moves word 64 k + l, so neighbouring lanes
// read neighbouring words of neighbouring rows (full 128-B lines where the rows are
// consecutive, as the old rows of a list are).  Called by every thread of the block.
__device__ __forceinline__ void wave_move_rows(const uint8_t* srcp, uint8_t* dstp) {
  const int lane = threadIdx.x & 63;
  const uint64_t s = (uint64_t)srcp, d = (uint64_t)dstp;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const int w = k * 64 + lane;
    const int r = w / 5, word = w - r * 5;
    const uint64_t sp = shfl64(s, r), dp = shfl64(d, r);
    if (dp) *reinterpret_cast<uint64_t*>(dp + word * 8) = *reinterpret_cast<const uint64_t*>(sp + word * 8);
  }
}

// lastModified: the row's `a` cell (bytes 12-13, big endian)
__device__ __forceinline__ uint32_t row_lm(const uint8_t* __restrict__ r) { return ((uint32_t)r[12] << 8) | r[13]; }

// ---------------------------------------------------------------- what the kernels below share

// slot of (h, l) in the ascending 72-bit set kh / kl[0, n), -1: not in it.  I: int for a set of at most 2^31
// keys, as the streaming passes take, int64_t for k_rm_*'s.
template <class I>
__device__ __forceinline__ I set_slot(const uint64_t* kh, const uint8_t* kl, I n, uint64_t h, uint32_t l) {
  I lo = 0, hi = n;
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (key_lt(kh[mid], kl[mid], h, l)) lo = mid + 1; else hi = mid;
  }
  return lo < n && kh[lo] == h && (uint32_t)kl[lo] == l ? lo : (I)-1;
}

// slot of h in the ascending set hs[0, nh), -1: not in it
__device__ __forceinline__ int host_slot(const uint64_t* __restrict__ hs, int nh, uint64_t h) {
  int lo = 0, hi = nh;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (hs[mid] < h) lo = mid + 1; else hi = mid;
  }
  return lo < nh && hs[lo] == h ? lo : -1;
}

// The sorted set of a streaming pass into LDS (LDS = true: it fits; the pass then searches it there), or left
// where it is.  A set of 8-byte keys kh, or (LOW) of 8 + 1-byte keys kh / kl.
template <bool LDS, bool LOW = false>
__device__ __forceinline__ void stage_set(uint64_t* s_kh, const uint64_t* __restrict__ kh, int n,
                                          uint8_t* s_kl = nullptr, const uint8_t* __restrict__ kl = nullptr) {
  if (!LDS) return;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    s_kh[i] = kh[i];
    if (LOW) s_kl[i] = kl[i];
  }
  __syncthreads();
}

// A lane's place in the flattened lists.  A workgroup walks a contiguous span of postings upwards, so a
// lane's postings ascend: its list is looked up again (a binary search over the lists above) only when
// it passes the end of the one it is in, and the list's pointers stay in registers meanwhile.
struct SegCursor {
  int c = -1;
  int64_t lo = 0, hi = 0;  // list c holds postings [lo, hi)
  const uint64_t* kh = nullptr;
  const uint8_t* kl = nullptr;
};

__device__ __forceinline__ void seg_seek(SegCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                         int nj, int64_t total, int64_t i) {
  if (i < s.hi) return;
  const int above = nj - s.c - 1;  // lists above c (i < total: one of them holds it)
  s.c += 1 + seg_of(off + s.c + 1, 0, above - 1, i);
  s.lo = off[s.c];
  s.hi = s.c + 1 < nj ? off[s.c + 1] : total;
  s.kh = jobs[s.c].khi;
  s.kl = jobs[s.c].klo;
}

// the workgroup's span [begin, end) of the flattened postings: whole tiles, the same for every thread
__device__ __forceinline__ void span_of(int64_t total, int64_t* begin, int64_t* end) {
  const int64_t per = ((total + gridDim.x - 1) / gridDim.x + SPAN_TILE - 1) / SPAN_TILE * SPAN_TILE;
  *begin = std::min<int64_t>((int64_t)blockIdx.x * per, total);
  *end = std::min<int64_t>(*begin + per, total);
}

// One step of a thread over the keys: postings base + 256 u + thread (u < 4) below end -> their lists (-1: past
// end), rows in the list and keys.  The four key loads are issued here, before the caller's first use of one.
__device__ __forceinline__ void key_tile(SegCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                         int nj, int64_t total, int64_t base, int64_t end, int c[4], int64_t k[4],
                                         uint64_t h[4], uint32_t l[4]) {
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int64_t i = base + u * 256 + threadIdx.x;
    c[u] = -1;
    k[u] = 0;
    h[u] = 0;
    l[u] = 0;
    if (i < end) {
      seg_seek(s, jobs, off, nj, total, i);
      c[u] = s.c;
      k[u] = i - s.lo;
      h[u] = s.kh[k[u]];
      l[u] = s.kl[k[u]];
    }
  }
}

// cnt[key] += the wave's hits of that key: one atomic per distinct key.  Called by the whole wave; -> the hits.
__device__ __forceinline__ uint32_t wave_add_by(bool hit, int key, unsigned long long* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const uint64_t all = __ballot(hit);
  uint64_t act = all;
  while (act) {
    const int lead = __ffsll((unsigned long long)act) - 1;
    const int lk = __shfl(key, lead, 64);
    const uint64_t same = __ballot(hit && key == lk);
    if (lane == lead) atomicAdd(&cnt[lk], (unsigned long long)__popcll(same));
    act &= ~same;
  }
  return (uint32_t)__popcll(all);
}

// The hits of a wave per list, where the lists of a wave's postings ascend (a streaming pass): the lanes of one
// list are neighbours, so the wave sums a list's hits over its steps (c, n: the same in every lane) and adds
// them once, on leaving the list: one atomic per list per wave.  add() is called by the whole wave.
struct ListTally {
  int c = -1;
  uint32_t n = 0;
  // this step's hits: the lane has one (hit) of list lc
  __device__ __forceinline__ void add(bool hit, int lc, unsigned long long* cnt) {
    uint64_t act = __ballot(hit);
    while (act) {
      const int lead = __ffsll((unsigned long long)act) - 1;
      const int c1 = __shfl(lc, lead, 64);
      const uint64_t same = __ballot(hit && lc == c1);
      if (c1 != c) {
        flush(cnt);
        c = c1;
        n = 0;
      }
      n += (uint32_t)__popcll(same);
      act &= ~same;
    }
  }
  __device__ __forceinline__ void flush(unsigned long long* cnt) const {
    if (n && (threadIdx.x & 63) == 0) atomicAdd(&cnt[c], (unsigned long long)n);
  }
};

// ---------------------------------------------------------------- add: sort keys
__global__ void k_upd_key_a(const uint64_t* __restrict__ khi, const uint8_t* __restrict__ klo, int64_t n,
                            uint64_t* __restrict__ ka, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ka[i] = (khi[i] << 8) | (uint64_t)klo[i];
  idx[i] = (uint32_t)i;
}

__global__ void k_upd_key_b(const uint64_t* __restrict__ khi, const int32_t* __restrict__ job,
                            const uint32_t* __restrict__ idx, int64_t n, uint64_t* __restrict__ kb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = idx[i];
  kb[i] = ((uint64_t)(uint32_t)job[p] << 8) | (khi[p] >> 56);
}

__global__ void k_upd_gather(const uint64_t* __restrict__ khi, const uint8_t* __restrict__ klo,
                             const int32_t* __restrict__ job, const uint32_t* __restrict__ perm, int64_t n,
                             uint64_t* __restrict__ skh, uint8_t* __restrict__ skl, int32_t* __restrict__ sjob) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t p = perm[s];
  skh[s] = khi[p];
  skl[s] = klo[p];
  sjob[s] = job[p];
}

// The head of every run of equal (job, url key) -- the run is in arrival order -- picks the
// run's winner: REPLACE the last, KEEP the first, RECENT the last of the largest
// lastModified; then settles it against the list's row of that key, if there is one.
// ins = the winner brings a new key, rep = it takes an existing row's place.  The head walks its
// run alone: a run is as long as one (term, url) pair repeats in the batch, 1 in a crawl's batch.
__global__ void k_upd_pick(const UpdJob* __restrict__ jobs, const uint8_t* __restrict__ rows,
                           const uint32_t* __restrict__ perm, const uint64_t* __restrict__ skh,
                           const uint8_t* __restrict__ skl, const int32_t* __restrict__ sjob, int64_t n, int policy,
                           int32_t* __restrict__ ins, uint8_t* __restrict__ rep, int64_t* __restrict__ lbA,
                           uint32_t* __restrict__ src, unsigned long long* __restrict__ jcnt) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int32_t j = sjob[s];
  const uint64_t h = skh[s];
  const uint32_t l = skl[s];
  if (s > 0 && sjob[s - 1] == j && skh[s - 1] == h && (uint32_t)skl[s - 1] == l) {
    ins[s] = 0;
    rep[s] = 0;
    return;
  }
  int64_t w = s;
  uint32_t lmw = 0;
  if (policy == YRWI_ADD_RECENT) lmw = row_lm(rows + (int64_t)perm[s] * YRWI_ROW_BYTES);
  if (policy != YRWI_ADD_KEEP) {
    for (int64_t e = s + 1; e < n && sjob[e] == j && skh[e] == h && (uint32_t)skl[e] == l; e++) {
      if (policy == YRWI_ADD_REPLACE) {
        w = e;
      } else {
        const uint32_t lme = row_lm(rows + (int64_t)perm[e] * YRWI_ROW_BYTES);
        if (lme >= lmw) {
          w = e;
          lmw = lme;
        }
      }
    }
  }
  const UpdJob J = jobs[j];
  const int64_t p = lb_key(J.akhi, J.aklo, 0, J.an, h, l);
  const bool exists = p < J.an && J.akhi[p] == h && (uint32_t)J.aklo[p] == l;
  int i = 0, r = 0;
  if (!exists) i = 1;
  else if (policy == YRWI_ADD_REPLACE) r = 1;
  else if (policy == YRWI_ADD_RECENT) r = lmw >= row_lm(J.arows + p * YRWI_ROW_BYTES);
  ins[s] = i;
  rep[s] = (uint8_t)r;
  lbA[s] = p;
  src[s] = perm[w];
  if (i) atomicAdd(&jcnt[2 * (int64_t)j], 1ull);
  if (r) atomicAdd(&jcnt[2 * (int64_t)j + 1], 1ull);
}

// Old rows of the changed lists, flattened over aoff: row k of its list goes to k + (new
// keys of the job below its key), unless a batch row takes its place.
__global__ __launch_bounds__(256) void k_upd_old(const UpdJob* __restrict__ jobs, const int32_t* __restrict__ cj,
                                                 const int64_t* __restrict__ aoff, int ncj, int64_t total,
                                                 const uint64_t* __restrict__ skh, const uint8_t* __restrict__ skl,
                                                 const int64_t* __restrict__ insx, const uint8_t* __restrict__ rep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint8_t* srcp = nullptr;
  uint8_t* dstp = nullptr;
  if (i < total) {
    const int c = seg_of(aoff, 0, ncj - 1, i);
    const UpdJob J = jobs[cj[c]];
    const int64_t k = i - aoff[c];
    const uint64_t h = J.akhi[k];
    const uint32_t l = J.aklo[k];
    const int64_t bend = J.boff + J.bn;
    const int64_t lb = lb_key(skh, skl, J.boff, bend, h, l);  // the head of the key's run, if the batch has it
    const bool taken = lb < bend && skh[lb] == h && (uint32_t)skl[lb] == l && rep[lb];
    if (!taken) {
      const int64_t pos = k + (insx[lb] - insx[J.boff]);
      J.okhi[pos] = h;
      J.oklo[pos] = (uint8_t)l;
      srcp = J.arows + k * YRWI_ROW_BYTES;
      dstp = J.orows + pos * YRWI_ROW_BYTES;
    }
  }
  wave_move_rows(srcp, dstp);
}

// Surviving batch rows: lower bound in the old list + new keys of the job before it.
__global__ void k_upd_new(const UpdJob* __restrict__ jobs, const uint8_t* __restrict__ rows, int64_t n,
                          const uint64_t* __restrict__ skh, const uint8_t* __restrict__ skl,
                          const int32_t* __restrict__ sjob, const int32_t* __restrict__ ins,
                          const uint8_t* __restrict__ rep, const int64_t* __restrict__ insx,
                          const int64_t* __restrict__ lbA, const uint32_t* __restrict__ src) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n || !(ins[s] || rep[s])) return;
  const UpdJob J = jobs[sjob[s]];
  const int64_t pos = lbA[s] + (insx[s] - insx[J.boff]);
  J.okhi[pos] = skh[s];
  J.oklo[pos] = skl[s];
  copy_row(J.orows + pos * YRWI_ROW_BYTES, rows + (int64_t)src[s] * YRWI_ROW_BYTES);
}

// ---------------------------------------------------------------- remove
__global__ void k_rm_count(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off, int nj, int64_t total,
                           const uint64_t* __restrict__ ukh, const uint8_t* __restrict__ ukl, int64_t nu,
                           unsigned long long* __restrict__ jrem) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = seg_of(off, 0, nj - 1, i);
  const int64_t k = i - off[c];
  if (set_slot(ukh, ukl, nu, jobs[c].khi[k], jobs[c].klo[k]) >= 0) atomicAdd(&jrem[c], 1ull);
}

// keep[i] = posting i of the chunk's flattened lists stays; keep[total] = 0 (the scan's last element)
__global__ void k_rm_flag(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off, int nj, int64_t total,
                          const uint64_t* __restrict__ ukh, const uint8_t* __restrict__ ukl, int64_t nu,
                          int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) keep[total] = 0;
  if (i >= total) return;
  const int c = seg_of(off, 0, nj - 1, i);
  const int64_t k = i - off[c];
  keep[i] = set_slot(ukh, ukl, nu, jobs[c].khi[k], jobs[c].klo[k]) >= 0 ? 0 : 1;
}

__global__ __launch_bounds__(256) void k_rm_place(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                  int nj, int64_t total, const int32_t* __restrict__ keep,
                                                  const int64_t* __restrict__ kx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint8_t* srcp = nullptr;
  uint8_t* dstp = nullptr;
  if (i < total && keep[i]) {
    const int c = seg_of(off, 0, nj - 1, i);
    const RmJob J = jobs[c];
    const int64_t k = i - off[c];
    const int64_t pos = kx[i] - kx[off[c]];
    J.okhi[pos] = J.khi[k];
    J.oklo[pos] = J.klo[k];
    srcp = J.rows + k * YRWI_ROW_BYTES;
    dstp = J.orows + pos * YRWI_ROW_BYTES;
  }
  wave_move_rows(srcp, dstp);
}

// ---------------------------------------------------------------- hosts

// a key tile -> its postings' host slots (-1: not of the set, or past end) and lists
__device__ __forceinline__ void mark_tile(SegCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                          int nj, int64_t total, const uint64_t* hs, int nh, int64_t base, int64_t end,
                                          int slot[4], int c[4]) {
  int64_t k[4];
  uint64_t h[4];
  uint32_t l[4];
  key_tile(s, jobs, off, nj, total, base, end, c, k, h, l);
#pragma unroll
  for (int u = 0; u < 4; u++) slot[u] = c[u] >= 0 ? host_slot(hs, nh, host36(h[u], l[u])) : -1;
}

// Marking pass: jrem[c] += postings of list c whose host is in the set; COUNT: hcnt[slot] += postings of
// host slot.  Every wave of a workgroup runs every step whole (the ballots).
template <bool LDS, bool COUNT>
__global__ __launch_bounds__(256) void k_host_mark(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                   int nj, int64_t total, const uint64_t* __restrict__ hset, int nh,
                                                   unsigned long long* __restrict__ jrem,
                                                   unsigned long long* __restrict__ hcnt) {
  __shared__ uint64_t s_set[LDS ? HOST_LDS_MAX : 1];
  __shared__ uint32_t s_cnt[LDS && COUNT ? HOST_LDS_MAX : 1];
  if (LDS && COUNT)
    for (int i = threadIdx.x; i < nh; i += blockDim.x) s_cnt[i] = 0;
  stage_set<LDS>(s_set, hset, nh);
  const uint64_t* hs = LDS ? s_set : hset;
  const int lane = threadIdx.x & 63;
  int64_t begin, end;
  span_of(total, &begin, &end);
  SegCursor cur;
  ListTally per_list;
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    int slots[4], cs[4];
    mark_tile(cur, jobs, off, nj, total, hs, nh, base, end, slots, cs);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int slot = slots[u];
      const bool hit = slot >= 0;
      per_list.add(hit, cs[u], jrem);
      if (COUNT) {
        const uint64_t act = __ballot(hit);
        if (LDS) {
          // one host owns the wave's hits (a hot spot): one LDS add; else one per lane, spread over the slots
          const int lead = act ? __ffsll((unsigned long long)act) - 1 : 0;
          const int ls = __shfl(slot, lead, 64);
          if (__ballot(hit && slot != ls) == 0) {
            if (act && lane == lead) atomicAdd(&s_cnt[ls], (uint32_t)__popcll(act));
          } else if (hit) {
            atomicAdd(&s_cnt[slot], 1u);
          }
        } else {
          wave_add_by(hit, slot, hcnt);
        }
      }
    }
  }
  per_list.flush(jrem);
  if (LDS && COUNT) {  // one global atomic per hit slot per workgroup
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += blockDim.x)
      if (s_cnt[i]) atomicAdd(&hcnt[i], (unsigned long long)s_cnt[i]);
  }
}

// keep[i] = posting i of the chunk's flattened lists stays; keep[total] = 0 (the scan's last element)
template <bool LDS>
__global__ __launch_bounds__(256) void k_host_flag(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                   int nj, int64_t total, const uint64_t* __restrict__ hset, int nh,
                                                   int32_t* __restrict__ keep) {
  __shared__ uint64_t s_set[LDS ? HOST_LDS_MAX : 1];
  stage_set<LDS>(s_set, hset, nh);
  const uint64_t* hs = LDS ? s_set : hset;
  if (blockIdx.x == 0 && threadIdx.x == 0) keep[total] = 0;
  int64_t begin, end;
  span_of(total, &begin, &end);
  SegCursor cur;
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    int slots[4], cs[4];
    mark_tile(cur, jobs, off, nj, total, hs, nh, base, end, slots, cs);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (cs[u] >= 0) keep[base + u * 256 + threadIdx.x] = slots[u] < 0;
  }
}

// what the call enqueued (kernels, device-library calls, copies, memsets) and waited for
struct Tally {
  int32_t launches = 0, syncs = 0;
};

// n host rows -> d_rows through the lane's pinned staging, two pieces in turn; the stage
// keeps `extra` bytes after the pieces for the call's table uploads (upload())
int stage_rows(yrwi_ctx* ctx, Lane* L, const uint8_t* rows, size_t total, uint8_t* d_rows, size_t extra, Tally* T) {
  const size_t piece = std::min((size_t)16 << 20, al256(total));
  uint8_t* stg = stage_reserve(L, &L->stage, 2 * piece + extra, true);
  if (!stg) return ctx->take(L, YRWI_E_HIP);
  hipEvent_t done[2] = {L->event(), L->event()};
  bool used[2] = {false, false};
  for (size_t off = 0, k = 0; off < total; off += piece, k ^= 1) {
    const size_t m = std::min(piece, total - off);
    if (used[k]) {
      HIPCHK(ctx, hipEventSynchronize(done[k]));
      T->syncs++;
    }
    std::memcpy(stg + k * piece, rows + off, m);
    HIPCHK(ctx, hipMemcpyAsync(d_rows + off, stg + k * piece, m, hipMemcpyHostToDevice, L->stream));
    HIPCHK(ctx, hipEventRecord(done[k], L->stream));
    used[k] = true;
    T->launches++;
  }
  L->stage.used = 2 * piece;
  return 0;
}

void put_stats(yrwi_update_stats* st, const yrwi_update_stats& S, const Tally& T) {
  if (!st) return;
  *st = S;
  st->launches = T.launches;
  st->syncs = T.syncs;
}

// ---- what the removals, the host counts and the census start from: the selected lists, flattened
struct RmTable {
  std::vector<KeyT> jkey;
  std::vector<RmJob> jobs;
  std::vector<int64_t> off;  // list j's first posting among the flattened ones
  int64_t total = 0;
};

void rm_table(const ListSel& sel, RmTable* t) {
  for (const auto& s : sel) {
    const ListRec& R = *s.second;
    t->jkey.push_back(s.first);
    t->jobs.push_back(RmJob{R.khi, R.klo, R.rows, R.n, nullptr, nullptr, nullptr});
    t->off.push_back(t->total);
    t->total += R.n;
  }
}

// ---- the frame of a marking pass: what the maintenance calls do around the launches of their first pass
struct PassDev {  // the device view of an RmTable, and the pass's result words
  RmJob* jobs = nullptr;
  int64_t* off = nullptr;
  unsigned long long* res = nullptr;
};

inline bool pass_tables(Lane*, UpEnt*, int&) { return true; }
template <class T, class... R>
bool pass_tables(Lane* L, UpEnt* e, int& n, T** dst, const std::vector<T>& v, R&&... rest) {
  *dst = arena_alloc<T>(L, (int64_t)v.size());
  e[n++] = UpEnt{*dst, v.data(), v.size() * sizeof(T)};
  return *dst && pass_tables(L, e, n, std::forward<R>(rest)...);
}

// The begin of a pass on lane L (a new pass): the list table, the caller's tables (extra: pairs of where the
// device pointer goes and the host vector) and a result block of zero_bytes (0: none) take their place in the
// arena; one upload brings every table, one memset zeroes the block.  One sync; one or two launches.
template <class... Extra>
int pass_begin(yrwi_ctx* ctx, Lane* L, const RmTable& t, size_t zero_bytes, const char* nomem, PassDev* D, Tally* T,
               Extra&&... extra) {
  if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
  T->syncs++;
  UpEnt e[2 + sizeof...(Extra) / 2];
  int n = 0;
  bool ok = pass_tables(L, e, n, std::forward<Extra>(extra)..., &D->jobs, t.jobs, &D->off, t.off);
  if (zero_bytes) D->res = reinterpret_cast<unsigned long long*>(L->arena.alloc(zero_bytes));
  if (!ok || (zero_bytes && !D->res)) return ctx->fail(YRWI_E_NOMEM, nomem);
  if (int rc = upload_list(L, e, n)) return ctx->take(L, rc);  // (one copy kernel)
  T->launches++;
  if (zero_bytes) {
    HIPCHK(ctx, hipMemsetAsync(D->res, 0, zero_bytes, L->stream));
    T->launches++;
  }
  return 0;
}

// The end of a pass: the first nres result words read back once and waited for.  *h: the words in the pinned
// landing buffer, good until the lane's next read-back; a caller that needs them longer copies them.  One
// launch, one sync.
int pass_end(yrwi_ctx* ctx, Lane* L, const PassDev& D, int64_t nres, const int64_t** h, Tally* T) {
  *h = reinterpret_cast<const int64_t*>(readback(L, &L->down_stage, D.res, nres, 8, 8));
  if (!*h) return ctx->take(L, YRWI_E_HIP);
  T->launches++;
  HIPCHK(ctx, lane_sync(L));
  T->syncs++;
  return 0;
}

// The url hashes of a call as keys: as given, and as the set the kernels search, sorted and each once, in the
// device's two arrays.  YRWI_E_HASH for one that is not well formed.
struct UrlSet {
  std::vector<KeyT> in, uk;
  std::vector<uint64_t> kh;
  std::vector<uint8_t> kl;
};

int url_set(yrwi_ctx* ctx, const uint8_t* urls12, int64_t nurls, UrlSet* U) {
  U->in.resize((size_t)nurls);
  for (int64_t i = 0; i < nurls; i++)
    if (!key_of(urls12 + i * 12, &U->in[(size_t)i])) return ctx->fail(YRWI_E_HASH, "url hash is not well-formed Base64");
  U->uk = U->in;
  std::sort(U->uk.begin(), U->uk.end());
  U->uk.erase(std::unique(U->uk.begin(), U->uk.end()), U->uk.end());
  U->kh.resize(U->uk.size());
  U->kl.resize(U->uk.size());
  for (size_t i = 0; i < U->uk.size(); i++) {
    U->kh[i] = U->uk[i].hi;
    U->kl[i] = (uint8_t)U->uk[i].lo;
  }
  return 0;
}

// rows compacted at a time: YRWI_RM_CHUNK, read per call (tests force chunk boundaries with it)
int64_t rm_chunk() {
  const char* e = getenv("YRWI_RM_CHUNK");
  const int64_t v = e ? atoll(e) : RM_CHUNK_DEFAULT;
  return std::min<int64_t>(std::max<int64_t>(v, 256), (int64_t)INT32_MAX - 1);
}

// what compact_commit hands a flag functor besides the chunk: the scan's output and scratch (free until
// the chunk's own scan), and, when asked for, every chunk list's index in the selection
struct ChunkAux {
  int64_t* kx;
  void* tmp;
  size_t tb;
  const int32_t* sel;  // sel[c] = list c of the chunk is list sel[c] of the RmTable (want_sel only)
};

// List j of t loses rem[j] postings (counted by the caller's marking pass): the lists that lose
// some but not all are compacted into new lists from index memory, in chunks of whole lists, and
// every list that lost rows is committed to the context.  flag(jobs, off, nj, n, keep, aux) enqueues
// the caller's flag kernel for one chunk (keep[i] = posting i stays, keep[n] = 0).  One upload,
// three launches per chunk and one wait; none of them if no list needs compaction.
template <class Flag>
int compact_commit(yrwi_ctx* ctx, Lane* L, RmTable& t, const std::vector<int64_t>& rem, const char* nomem, Flag flag,
                   yrwi_update_stats* S, Tally* T, bool want_sel = false) {
  const int nj = (int)t.jobs.size();
  std::vector<int> lose;
  std::vector<RmJob> cjobs;
  std::vector<int64_t> coff;            // offsets within the list's chunk
  std::vector<int32_t> csel;            // want_sel: the list's index in t
  std::vector<std::pair<int, int>> ch;  // chunks: [first, last) of cjobs
  const int64_t cap = rm_chunk();
  int64_t ctotal = 0, maxc = 0;
  for (int j = 0; j < nj; j++) {
    if (rem[(size_t)j] == 0) continue;
    lose.push_back(j);
    if (rem[(size_t)j] == t.jobs[(size_t)j].n) continue;
    RmJob& J = t.jobs[(size_t)j];
    const size_t nn = (size_t)(J.n - rem[(size_t)j]);
    J.orows = ctx->index_mem.alloc(nn * 40);
    J.okhi = reinterpret_cast<uint64_t*>(ctx->index_mem.alloc(nn * 8));
    J.oklo = ctx->index_mem.alloc(nn);
    if (!J.orows || !J.okhi || !J.oklo) return ctx->fail(YRWI_E_NOMEM, "device index allocation failed");
    if (ch.empty() || ctotal + J.n > cap) {  // (a list longer than the cap: a chunk of its own)
      ch.push_back({(int)cjobs.size(), (int)cjobs.size()});
      ctotal = 0;
    }
    cjobs.push_back(J);
    coff.push_back(ctotal);
    if (want_sel) csel.push_back(j);
    ctotal += J.n;
    ch.back().second = (int)cjobs.size();
    maxc = std::max(maxc, ctotal);
  }
  if (!ch.empty()) {
    RmJob* d_cjobs = arena_alloc<RmJob>(L, (int64_t)cjobs.size());
    int64_t* d_coff = arena_alloc<int64_t>(L, (int64_t)cjobs.size());
    int32_t* d_csel = arena_alloc<int32_t>(L, (int64_t)csel.size());
    int32_t* keep = arena_alloc<int32_t>(L, maxc + 1);
    int64_t* kx = arena_alloc<int64_t>(L, maxc + 1);
    size_t tb = 0;
    HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, keep, kx, (int)(maxc + 1), L->stream));
    void* tmp = L->arena.alloc(tb);
    if (!d_cjobs || !d_coff || !d_csel || !keep || !kx || !tmp) return ctx->fail(YRWI_E_NOMEM, nomem);
    if (int rc = upload(L, d_cjobs, cjobs, d_coff, coff, d_csel, csel)) return ctx->take(L, rc);  // (one copy kernel)
    T->launches++;
    for (const auto& c : ch) {  // flag -> scan -> place, each chunk in the scratch of the one before
      const int ncj = c.second - c.first;
      const int64_t n = coff[(size_t)c.second - 1] + cjobs[(size_t)c.second - 1].n;
      const RmJob* dj = d_cjobs + c.first;
      const int64_t* doff = d_coff + c.first;
      flag(dj, doff, ncj, n, keep, ChunkAux{kx, tmp, tb, d_csel + c.first});
      size_t tbc = tb;
      HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tbc, keep, kx, (int)(n + 1), L->stream));
      hipLaunchKernelGGL(k_rm_place, dim3(blocks(n)), dim3(256), 0, L->stream, dj, doff, ncj, n, keep, kx);
      HIPCHK(ctx, hipGetLastError());
      T->launches += 3;
    }
    HIPCHK(ctx, lane_sync(L));
    T->syncs++;
  }
  // ---- bookkeeping: the removed postings are the dictionary churn
  for (int j : lose) {
    const RmJob& J = t.jobs[(size_t)j];
    auto it = ctx->lists.find(t.jkey[(size_t)j]);
    S->removed += rem[(size_t)j];
    S->terms++;
    ctx->npostings -= rem[(size_t)j];
    if (rem[(size_t)j] == J.n) {  // as yrwi_put_list(n = 0) leaves things
      index_changed(ctx, t.jkey[(size_t)j], J.n, false);
      ctx->lists.erase(it);
      S->emptied_terms++;
    } else {
      ListRec R;
      R.khi = J.okhi;
      R.klo = J.oklo;
      R.rows = J.orows;
      R.n = J.n - rem[(size_t)j];
      it->second = R;
      index_changed(ctx, t.jkey[(size_t)j], rem[(size_t)j], true);
    }
  }
  return 0;
}

}  // namespace

extern "C" int yrwi_add_postings(yrwi_ctx* ctx, const uint8_t* terms12, const uint8_t* rows40, int64_t n, int policy,
                                 yrwi_update_stats* st) {
  if (!ctx || n < 0 || (n > 0 && (!terms12 || !rows40))) return YRWI_E_ARG;
  if (policy != YRWI_ADD_REPLACE && policy != YRWI_ADD_KEEP && policy != YRWI_ADD_RECENT)
    return ctx->fail(YRWI_E_ARG, "unknown add policy");
  if (n >= (int64_t)INT32_MAX) return ctx->fail(YRWI_E_ARG, "2^31 - 1 or more postings in one batch");
  yrwi_update_stats S;
  std::memset(&S, 0, sizeof(S));
  Tally T;
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- grouping: every row's term -> its job (host, O(n))
  std::unordered_map<KeyT, int32_t, KeyHash> jobof;
  std::vector<KeyT> jkey;
  std::vector<int32_t> job((size_t)n);
  std::vector<int64_t> bcnt;
  for (int64_t i = 0; i < n; i++) {
    KeyT tk;
    if (!key_of(terms12 + i * 12, &tk)) return ctx->fail(YRWI_E_HASH, "term hash is not well-formed Base64");
    auto ins = jobof.emplace(tk, (int32_t)jkey.size());
    if (ins.second) {
      jkey.push_back(tk);
      bcnt.push_back(0);
    }
    job[(size_t)i] = ins.first->second;
    bcnt[(size_t)ins.first->second]++;
  }
  hipSetDevice(ctx->device);
  drain(ctx);  // in-flight batches read the list table
  if (n == 0) return 0;
  Lane* L = ctx->lanes[0];
  if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
  T.syncs++;
  const int nj = (int)jkey.size();
  std::vector<UpdJob> jobs((size_t)nj);
  std::vector<const ListRec*> old((size_t)nj, nullptr);
  for (int j = 0; j < nj; j++) {
    UpdJob& J = jobs[(size_t)j];
    std::memset(&J, 0, sizeof(J));
    auto it = ctx->lists.find(jkey[(size_t)j]);
    if (it != ctx->lists.end() && it->second.n > 0) {
      old[(size_t)j] = &it->second;
      J.akhi = it->second.khi;
      J.aklo = it->second.klo;
      J.arows = it->second.rows;
      J.an = it->second.n;
    }
    J.boff = j ? jobs[(size_t)j - 1].boff + jobs[(size_t)j - 1].bn : 0;
    J.bn = bcnt[(size_t)j];
  }
  // ---- scratch (lane arena)
  uint8_t* d_rows = L->arena.alloc((size_t)n * 40);
  uint64_t* khi = arena_alloc<uint64_t>(L, n);
  uint8_t* klo = arena_alloc<uint8_t>(L, n);
  int32_t* d_job = arena_alloc<int32_t>(L, n);
  uint64_t* ka = arena_alloc<uint64_t>(L, n);
  uint64_t* kb = arena_alloc<uint64_t>(L, n);
  uint32_t* ia = arena_alloc<uint32_t>(L, n);
  uint32_t* ib = arena_alloc<uint32_t>(L, n);
  uint64_t* skh = arena_alloc<uint64_t>(L, n);
  uint8_t* skl = arena_alloc<uint8_t>(L, n);
  int32_t* sjob = arena_alloc<int32_t>(L, n);
  int32_t* ins = arena_alloc<int32_t>(L, n + 1);
  int64_t* insx = arena_alloc<int64_t>(L, n + 1);
  uint8_t* rep = arena_alloc<uint8_t>(L, n);
  int64_t* lbA = arena_alloc<int64_t>(L, n);
  uint32_t* src = arena_alloc<uint32_t>(L, n);
  UpdJob* d_jobs = arena_alloc<UpdJob>(L, nj);
  int32_t* d_cj = arena_alloc<int32_t>(L, nj);
  int64_t* d_aoff = arena_alloc<int64_t>(L, nj);
  int64_t* res = arena_alloc<int64_t>(L, 1 + 2 * (int64_t)nj);  // validation bits, then (new, replacing) per job
  if (!d_rows || !khi || !klo || !d_job || !ka || !kb || !ia || !ib || !skh || !skl || !sjob || !ins || !insx ||
      !rep || !lbA || !src || !d_jobs || !d_cj || !d_aoff || !res)
    return ctx->fail(YRWI_E_NOMEM, "device allocation (add_postings)");
  int jbits = 1;
  while (((int64_t)1 << jbits) < nj) jbits++;
  const int ni = (int)n;
  size_t t1 = 0, t2 = 0, t3 = 0;
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, t1, ka, kb, ia, ib, ni, 0, 64, L->stream));
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, t2, kb, ka, ib, ia, ni, 0, 8 + jbits, L->stream));
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, t3, ins, insx, ni + 1, L->stream));
  const size_t tmpb = std::max(t1, std::max(t2, t3));
  void* tmp = L->arena.alloc(tmpb);
  if (!tmp) return ctx->fail(YRWI_E_NOMEM, "device allocation (add_postings sort)");
  // ---- upload, key and validate (the sortedness bit means nothing for a batch)
  const size_t extra = al256((size_t)n * 4) + 2 * al256((size_t)nj * sizeof(UpdJob)) + al256((size_t)nj * 4) +
                       al256((size_t)nj * 8) + 4096;
  if (int rc = stage_rows(ctx, L, rows40, (size_t)n * 40, d_rows, extra, &T)) return rc;
  if (int rc = upload(L, d_job, job, d_jobs, jobs)) return ctx->take(L, rc);
  HIPCHK(ctx, hipMemsetAsync(res, 0, (size_t)(1 + 2 * (int64_t)nj) * 8, L->stream));
  HIPCHK(ctx, hipMemsetAsync(ins + n, 0, 4, L->stream));
  T.launches += 3;
  if (launch_validate_rows(d_rows, n, khi, klo, reinterpret_cast<int32_t*>(res), L->stream))
    return ctx->fail(YRWI_E_HIP, "validate launch");
  // ---- sort by (job, url key, arrival)
  hipLaunchKernelGGL(k_upd_key_a, dim3(blocks(n)), dim3(256), 0, L->stream, khi, klo, n, ka, ia);
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(tmp, t1, ka, kb, ia, ib, ni, 0, 64, L->stream));
  hipLaunchKernelGGL(k_upd_key_b, dim3(blocks(n)), dim3(256), 0, L->stream, khi, d_job, ib, n, kb);
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(tmp, t2, kb, ka, ib, ia, ni, 0, 8 + jbits, L->stream));
  const uint32_t* perm = ia;
  hipLaunchKernelGGL(k_upd_gather, dim3(blocks(n)), dim3(256), 0, L->stream, khi, klo, d_job, perm, n, skh, skl, sjob);
  // ---- winners, lower bounds, one scan, one read-back
  hipLaunchKernelGGL(k_upd_pick, dim3(blocks(n)), dim3(256), 0, L->stream, d_jobs, d_rows, perm, skh, skl, sjob, n,
                     policy, ins, rep, lbA, src, reinterpret_cast<unsigned long long*>(res + 1));
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, t3, ins, insx, ni + 1, L->stream));
  HIPCHK(ctx, hipGetLastError());
  T.launches += 8;
  const int64_t* hres =
      reinterpret_cast<const int64_t*>(readback(L, &L->down_stage, res, 1 + 2 * (int64_t)nj, 8, 8));
  if (!hres) return ctx->take(L, YRWI_E_HIP);
  T.launches++;
  HIPCHK(ctx, lane_sync(L));
  T.syncs++;
  const int32_t herr = (int32_t)hres[0];
  if (herr & 1) return ctx->fail(YRWI_E_HASH, "url hash is not well-formed Base64");
  if (herr & 2) return ctx->fail(YRWI_E_NULL_LANGUAGE, "row with empty language cell (reference NPE)");
  // ---- one allocation round from index memory
  std::vector<int32_t> cj;
  std::vector<int64_t> aoff;
  int64_t atotal = 0;
  for (int j = 0; j < nj; j++) {
    const int64_t add = hres[1 + 2 * j], rp = hres[2 + 2 * j];
    S.added += add;
    S.replaced += rp;
    if (jobs[(size_t)j].an + add > MAX_LIST)
      return ctx->fail(YRWI_E_LIMIT, "list longer than 53,687,091 rows (RowSet.importRowSet)");
    if (add + rp == 0) continue;
    cj.push_back(j);
    aoff.push_back(atotal);
    atotal += jobs[(size_t)j].an;
  }
  S.dropped = n - S.added - S.replaced;
  if (cj.empty()) {  // every posting lost to an existing row
    put_stats(st, S, T);
    return 0;
  }
  for (int32_t j : cj) {
    UpdJob& J = jobs[(size_t)j];
    const size_t nn = (size_t)(J.an + hres[1 + 2 * j]);
    J.orows = ctx->index_mem.alloc(nn * 40);
    J.okhi = reinterpret_cast<uint64_t*>(ctx->index_mem.alloc(nn * 8));
    J.oklo = ctx->index_mem.alloc(nn);
    if (!J.orows || !J.okhi || !J.oklo) return ctx->fail(YRWI_E_NOMEM, "device index allocation failed");
  }
  // ---- place the old rows, then the batch's
  if (int rc = upload(L, d_jobs, jobs, d_cj, cj, d_aoff, aoff)) return ctx->take(L, rc);
  T.launches++;
  if (atotal > 0) {
    hipLaunchKernelGGL(k_upd_old, dim3(blocks(atotal)), dim3(256), 0, L->stream, d_jobs, d_cj, d_aoff, (int)cj.size(),
                       atotal, skh, skl, insx, rep);
    T.launches++;
  }
  hipLaunchKernelGGL(k_upd_new, dim3(blocks(n)), dim3(256), 0, L->stream, d_jobs, d_rows, n, skh, skl, sjob, ins, rep,
                     insx, lbA, src);
  T.launches++;
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, lane_sync(L));
  T.syncs++;
  // ---- bookkeeping: a pure add charges no dictionary churn (no key left a list)
  for (int32_t j : cj) {
    const UpdJob& J = jobs[(size_t)j];
    ListRec R;
    R.khi = J.okhi;
    R.klo = J.oklo;
    R.rows = J.orows;
    R.n = J.an + hres[1 + 2 * j];
    ctx->npostings += R.n - J.an;
    if (!old[(size_t)j]) S.new_terms++;
    ctx->lists[jkey[(size_t)j]] = R;
    index_changed(ctx, jkey[(size_t)j], 0, true);
    S.terms++;
  }
  put_stats(st, S, T);
  return 0;
}

extern "C" int yrwi_remove_postings(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* urls12,
                                    int64_t nurls, yrwi_update_stats* st) {
  if (!ctx || nterms < 0 || nurls < 0 || (nterms > 0 && !terms12) || (nurls > 0 && !urls12)) return YRWI_E_ARG;
  yrwi_update_stats S;
  std::memset(&S, 0, sizeof(S));
  Tally T;
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- the url set, sorted and deduplicated; the named lists, each once
  UrlSet U;
  if (int rc = url_set(ctx, urls12, nurls, &U)) return rc;
  ListSel sel;
  if (int rc = select_lists(ctx, terms12, nterms, false, &sel)) return rc;
  RmTable t;
  rm_table(sel, &t);
  if (U.uk.empty() || t.jobs.empty()) return 0;
  Lane* L = ctx->lanes[0];
  const int nj = (int)t.jobs.size();
  const int64_t nu = (int64_t)U.uk.size();
  // ---- one marking pass over the named lists' keys, the per-list counts read back once
  PassDev D;
  uint64_t* ukh = nullptr;
  uint8_t* ukl = nullptr;
  if (int rc = pass_begin(ctx, L, t, (size_t)nj * 8, "device allocation (remove_postings)", &D, &T, &ukh, U.kh, &ukl, U.kl))
    return rc;
  hipLaunchKernelGGL(k_rm_count, dim3(blocks(t.total)), dim3(256), 0, L->stream, D.jobs, D.off, nj, t.total, ukh, ukl,
                     nu, D.res);
  HIPCHK(ctx, hipGetLastError());
  T.launches++;
  const int64_t* hrem = nullptr;
  if (int rc = pass_end(ctx, L, D, nj, &hrem, &T)) return rc;
  // ---- compaction of only the lists that lost rows, and the bookkeeping
  const std::vector<int64_t> rem(hrem, hrem + nj);  // (the pinned landing buffer may be reused)
  auto flag = [&](const RmJob* dj, const int64_t* doff, int ncj, int64_t n, int32_t* keep, const ChunkAux&) {
    hipLaunchKernelGGL(k_rm_flag, dim3(blocks(n)), dim3(256), 0, L->stream, dj, doff, ncj, n, ukh, ukl, nu, keep);
  };
  if (int rc = compact_commit(ctx, L, t, rem, "device allocation (remove_postings compaction)", flag, &S, &T)) return rc;
  put_stats(st, S, T);
  return 0;
}

// ---------------------------------------------------------------- removal and counts by host
namespace {

// what both host calls start from: the host set and the selected lists, flattened
struct HostPass : RmTable {
  std::vector<uint64_t> in;  // the 36-bit key of every host given, in the caller's order
  std::vector<uint64_t> hk;  // the set: sorted, each once
  uint64_t* d_hk = nullptr;
  std::vector<int64_t> res;  // after host_mark: hits per selected list, then (count) postings per set slot
};

// arguments -> host set and selected lists (host only); waits for the batches in flight
int host_select(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6, int32_t nhosts,
                HostPass* P) {
  P->in.resize((size_t)nhosts);
  for (int32_t i = 0; i < nhosts; i++) {
    uint64_t x = 0;
    for (int j = 0; j < 6; j++) {  // key_of's rule, per character
      const int8_t v = AHP[hosts6[(size_t)i * 6 + j]];
      if (v < 0) return ctx->fail(YRWI_E_HASH, "host hash is not well-formed Base64");
      x = (x << 6) | (uint64_t)v;
    }
    P->in[(size_t)i] = x;
  }
  P->hk = P->in;
  std::sort(P->hk.begin(), P->hk.end());
  P->hk.erase(std::unique(P->hk.begin(), P->hk.end()), P->hk.end());
  ListSel sel;
  if (int rc = select_lists(ctx, terms12, nterms, false, &sel)) return rc;
  rm_table(sel, P);
  return 0;
}

// The marking pass on lane L (a new pass): the set and the list table uploaded once, one launch over
// the flattened keys, one read-back, one wait.  4 launches, 2 syncs, whatever was selected or given.
int host_mark(yrwi_ctx* ctx, Lane* L, HostPass* P, bool count, Tally* T) {
  const int nj = (int)P->jobs.size(), nh = (int)P->hk.size();
  const int64_t nres = (int64_t)nj + (count ? nh : 0);
  PassDev D;
  if (int rc = pass_begin(ctx, L, *P, (size_t)nres * 8, "device allocation (host marking pass)", &D, T, &P->d_hk, P->hk))
    return rc;
  const dim3 g(span_blocks(P->total)), b(256);
  const bool lds = nh <= HOST_LDS_MAX;
  if (lds && count)
    hipLaunchKernelGGL((k_host_mark<true, true>), g, b, 0, L->stream, D.jobs, D.off, nj, P->total, P->d_hk, nh, D.res, D.res + nj);
  else if (lds)
    hipLaunchKernelGGL((k_host_mark<true, false>), g, b, 0, L->stream, D.jobs, D.off, nj, P->total, P->d_hk, nh, D.res, D.res + nj);
  else if (count)
    hipLaunchKernelGGL((k_host_mark<false, true>), g, b, 0, L->stream, D.jobs, D.off, nj, P->total, P->d_hk, nh, D.res, D.res + nj);
  else
    hipLaunchKernelGGL((k_host_mark<false, false>), g, b, 0, L->stream, D.jobs, D.off, nj, P->total, P->d_hk, nh, D.res, D.res + nj);
  HIPCHK(ctx, hipGetLastError());
  T->launches++;
  const int64_t* h = nullptr;
  if (int rc = pass_end(ctx, L, D, nres, &h, T)) return rc;
  P->res.assign(h, h + nres);  // (the pinned landing buffer may be reused)
  return 0;
}

}  // namespace

extern "C" int yrwi_count_hosts(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6,
                                int32_t nhosts, int64_t* counts, int64_t* lists_hit) {
  if (!ctx || nterms < 0 || nhosts < 0 || (nterms > 0 && !terms12) || (nhosts > 0 && (!hosts6 || !counts)))
    return YRWI_E_ARG;
  HostPass P;
  if (int rc = host_select(ctx, terms12, nterms, hosts6, nhosts, &P)) return rc;
  for (int32_t i = 0; i < nhosts; i++) counts[i] = 0;
  if (lists_hit) *lists_hit = 0;
  if (P.hk.empty() || P.jobs.empty()) return 0;
  Tally T;
  if (int rc = host_mark(ctx, ctx->lanes[0], &P, true, &T)) return rc;
  const size_t nj = P.jobs.size();
  for (int32_t i = 0; i < nhosts; i++) {
    const size_t slot = (size_t)(std::lower_bound(P.hk.begin(), P.hk.end(), P.in[(size_t)i]) - P.hk.begin());
    counts[i] = P.res[nj + slot];
  }
  if (lists_hit)
    for (size_t j = 0; j < nj; j++) *lists_hit += P.res[j] > 0;
  return 0;
}

extern "C" int yrwi_remove_hosts(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6,
                                 int32_t nhosts, yrwi_update_stats* st) {
  if (!ctx || nterms < 0 || nhosts < 0 || (nterms > 0 && !terms12) || (nhosts > 0 && !hosts6)) return YRWI_E_ARG;
  yrwi_update_stats S;
  std::memset(&S, 0, sizeof(S));
  Tally T;
  if (st) std::memset(st, 0, sizeof(*st));
  HostPass P;
  if (int rc = host_select(ctx, terms12, nterms, hosts6, nhosts, &P)) return rc;
  if (P.hk.empty() || P.jobs.empty()) return 0;
  Lane* L = ctx->lanes[0];
  if (int rc = host_mark(ctx, L, &P, false, &T)) return rc;
  const int nh = (int)P.hk.size();
  auto flag = [&](const RmJob* dj, const int64_t* doff, int ncj, int64_t n, int32_t* keep, const ChunkAux&) {
    if (nh <= HOST_LDS_MAX)
      hipLaunchKernelGGL((k_host_flag<true>), dim3(span_blocks(n)), dim3(256), 0, L->stream, dj, doff, ncj, n, P.d_hk, nh, keep);
    else
      hipLaunchKernelGGL((k_host_flag<false>), dim3(span_blocks(n)), dim3(256), 0, L->stream, dj, doff, ncj, n, P.d_hk, nh, keep);
  };
  if (int rc = compact_commit(ctx, L, P, P.res, "device allocation (remove_hosts compaction)", flag, &S, &T)) return rc;
  put_stats(st, S, T);
  return 0;
}

// ---------------------------------------------------------------- census of the hosts
namespace {

constexpr int64_t CENSUS_SLOTS_DEFAULT = (int64_t)1 << 22;  // device table slots a call starts with at most (YRWI_CENSUS_SLOTS)
constexpr int64_t CENSUS_SLOTS_MAX = (int64_t)1 << 30;      // 16 GiB of table; the scan counts in int
constexpr int CENSUS_LDS_DEFAULT = 2048;                    // slots of a workgroup's LDS table (YRWI_CENSUS_LDS_SLOTS)
constexpr int CENSUS_LDS_PROBES = 64;                       // places a lane tries in the LDS table (all of a 64-slot table)
constexpr int CENSUS_PROBES = 128;                          // places an insert tries in the device table (at most all)
enum { CEN_OVERFLOW = 0, CEN_BYPASS = 1, CEN_HOSTS = 2, CEN_PASSING = 3, CEN_WORDS = 4 };

__device__ __forceinline__ uint64_t census_hash(uint64_t key1) { return key1 * 0x9E3779B97F4A7C15ull; }

// tab[2 p] = host36 + 1 (0: empty, as htab_insert's tables), tab[2 p + 1] = postings; linear probing from
// the key's place.  No place within the probes (or the pass has overflowed already): the overflow word is
// set and the postings are dropped; the host runs the pass again with a larger table.
__device__ __forceinline__ void census_add(unsigned long long* __restrict__ tab, uint64_t mask, uint64_t key1,
                                           unsigned long long n, unsigned long long* __restrict__ ctr) {
  uint64_t p = (census_hash(key1) >> 24) & mask;
  const uint64_t probes = std::min<uint64_t>(mask + 1, CENSUS_PROBES);
  for (uint64_t k = 0; k < probes; k++, p = (p + 1) & mask) {
    // a key never changes once set: only a slot read as empty needs the compare-and-swap
    unsigned long long cur = __hip_atomic_load(&tab[2 * p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) cur = atomicCAS(&tab[2 * p], 0ull, (unsigned long long)key1);
    if (cur == 0 || cur == key1) {
      atomicAdd(&tab[2 * p + 1], n);
      return;
    }
    if ((k & 63) == 63 && __hip_atomic_load(&ctr[CEN_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
  atomicOr(&ctr[CEN_OVERFLOW], 1ull);
}

// n postings of key1 into the workgroup's table (keys lk[S], counts lc[S]); false: no place within the probes
__device__ __forceinline__ bool census_lds_add(unsigned long long* lk, uint32_t* lc, uint32_t smask, uint64_t key1,
                                               uint32_t n) {
  uint32_t p = (uint32_t)(census_hash(key1) >> 52) & smask;
  for (int k = 0; k < CENSUS_LDS_PROBES; k++, p = (p + 1) & smask) {
    unsigned long long cur = *reinterpret_cast<volatile unsigned long long*>(&lk[p]);
    if (cur == 0) cur = atomicCAS(&lk[p], 0ull, (unsigned long long)key1);
    if (cur == 0 || cur == key1) {
      atomicAdd(&lc[p], n);
      return true;
    }
  }
  return false;
}

// a key tile -> its postings' host36 + 1 (0: past end, told by the posting's number: the census needs no list)
__device__ __forceinline__ void census_tile(SegCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                            int nj, int64_t total, int64_t base, int64_t end, uint64_t key1[4]) {
  int c[4];
  int64_t k[4];
  uint64_t h[4];
  uint32_t l[4];
  key_tile(s, jobs, off, nj, total, base, end, c, k, h, l);
#pragma unroll
  for (int u = 0; u < 4; u++) key1[u] = base + u * 256 + threadIdx.x < end ? host36(h[u], l[u]) + 1 : 0;
}

// Counting pass: a group-by of the selected postings on their host.  Grid and spans as k_host_mark.  Every
// workgroup sums in an LDS table of S slots (dynamic shared memory: S 8-B keys, then S 4-B counts) and adds
// its slots into the device table at the end of its span; a posting whose lane finds no place in LDS goes
// straight to the device table, equal keys of the wave as one add (counted in ctr[CEN_BYPASS]).  Every wave
// of a workgroup runs every step whole (the ballots); the only barriers are before the first and after the
// last step.
__global__ __launch_bounds__(256) void k_census(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off, int nj,
                                                int64_t total, int S, unsigned long long* __restrict__ tab,
                                                uint64_t mask, unsigned long long* __restrict__ ctr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char census_lds[];
  unsigned long long* lk = reinterpret_cast<unsigned long long*>(census_lds);
  uint32_t* lc = reinterpret_cast<uint32_t*>(census_lds + (size_t)S * 8);
  for (int i = threadIdx.x; i < S; i += blockDim.x) {
    lk[i] = 0;
    lc[i] = 0;
  }
  __syncthreads();
  const uint32_t smask = (uint32_t)S - 1;
  const int lane = threadIdx.x & 63;
  int64_t begin, end;
  span_of(total, &begin, &end);
  SegCursor cur;
  unsigned long long bypass = 0;  // the same in every lane of the wave
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    // the pass has overflowed and will be run again: the wave leaves (no barrier waits for it in here)
    if (__any(__hip_atomic_load(&ctr[CEN_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) break;
    uint64_t keys[4];
    census_tile(cur, jobs, off, nj, total, base, end, keys);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t key1 = keys[u];
      const bool live = key1 != 0;
      const uint64_t act = __ballot(live);
      // one host owns the wave's postings (a hot spot): one lane adds them all; else every lane its own
      const int lead = act ? __ffsll((unsigned long long)act) - 1 : 0;
      const uint64_t lkey = shfl64(key1, lead);
      const bool uni = __ballot(live && key1 != lkey) == 0;
      const uint32_t n = uni ? (uint32_t)__popcll(act) : 1u;
      bool pend = false;  // this lane's postings found no place in LDS
      if (uni ? (act && lane == lead) : live) pend = !census_lds_add(lk, lc, smask, key1, n);
      uint64_t left = __ballot(pend);
      while (left) {  // equal keys aggregated within the wave (wave_add_by, over 64-bit keys into a hash table)
        const int pl = __ffsll((unsigned long long)left) - 1;
        const uint64_t pk = shfl64(key1, pl);
        const uint64_t same = __ballot(pend && key1 == pk);
        const unsigned long long m = uni ? n : (unsigned long long)__popcll(same);
        if (lane == pl) census_add(tab, mask, pk, m, ctr);
        bypass += m;
        left &= ~same;
      }
    }
  }
  if (bypass && lane == 0) atomicAdd(&ctr[CEN_BYPASS], bypass);
  __syncthreads();
  if (__hip_atomic_load(&ctr[CEN_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  for (int i = threadIdx.x; i < S; i += blockDim.x)
    if (lk[i]) census_add(tab, mask, lk[i], (unsigned long long)lc[i], ctr);
}

// flag[i] = slot i holds a host with at least minp postings; flag[slots] = 0 (the scan's last element);
// ctr[CEN_HOSTS] += non-empty slots, ctr[CEN_PASSING] += flagged ones (one atomic each per wave)
__global__ __launch_bounds__(256) void k_census_flag(const unsigned long long* __restrict__ tab, int64_t slots,
                                                     unsigned long long minp, int32_t* __restrict__ flag,
                                                     unsigned long long* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool used = false, pass = false;
  if (i < slots) {
    const ulonglong2 s = *reinterpret_cast<const ulonglong2*>(tab + 2 * i);
    used = s.x != 0;
    pass = used && s.y >= minp;
  }
  if (i <= slots) flag[i] = pass ? 1 : 0;
  const uint64_t bu = __ballot(used), bp = __ballot(pass);
  if ((threadIdx.x & 63) == 0) {
    if (bu) atomicAdd(&ctr[CEN_HOSTS], (unsigned long long)__popcll(bu));
    if (bp) atomicAdd(&ctr[CEN_PASSING], (unsigned long long)__popcll(bp));
  }
}

__global__ void k_census_place(const unsigned long long* __restrict__ tab, int64_t slots,
                               const int32_t* __restrict__ flag, const int64_t* __restrict__ px,
                               uint64_t* __restrict__ okey, uint64_t* __restrict__ ocnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slots || !flag[i]) return;
  const ulonglong2 s = *reinterpret_cast<const ulonglong2*>(tab + 2 * i);
  okey[px[i]] = s.x - 1;
  ocnt[px[i]] = s.y;
}

int64_t pow2_floor(int64_t v) {
  int64_t p = 1;
  while (p <= v / 2) p *= 2;
  return p;
}

// environment knob `name`, read per call (tests reach the overflow paths with them): rounded down to a power
// of two within [lo, hi]
int64_t census_knob(const char* name, int64_t dflt, int64_t lo, int64_t hi) {
  const char* e = getenv(name);
  const int64_t v = e ? atoll(e) : dflt;
  return pow2_floor(std::min(std::max(v, lo), hi));
}

}  // namespace

extern "C" int yrwi_host_census(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t order,
                                int64_t min_postings, uint8_t* hosts6_out, int64_t* counts_out, int64_t cap,
                                int64_t* nout, yrwi_census_stats* st) {
  if (!ctx || nterms < 0 || (nterms > 0 && !terms12)) return YRWI_E_ARG;
  if (order != YRWI_CENSUS_BY_HOST && order != YRWI_CENSUS_BY_COUNT) return ctx->fail(YRWI_E_ARG, "unknown census order");
  if (cap < 0 || (cap > 0 && (!hosts6_out || !counts_out))) return ctx->fail(YRWI_E_ARG, "census capacity without buffers");
  const auto t_begin = std::chrono::steady_clock::now();
  yrwi_census_stats S;
  std::memset(&S, 0, sizeof(S));
  Tally T;
  ListSel sel;
  if (int rc = select_lists(ctx, terms12, nterms, false, &sel)) return rc;
  RmTable t;
  rm_table(sel, &t);
  auto finish = [&](int64_t n) {
    S.launches = T.launches;
    S.syncs = T.syncs;
    S.t_total_ns =
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
    if (nout) *nout = n;
    if (st) *st = S;
    return 0;
  };
  if (t.jobs.empty()) return finish(0);
  const int nj = (int)t.jobs.size();
  const int64_t total = t.total;
  const unsigned long long minp = (unsigned long long)std::max<int64_t>(min_postings, 1);
  S.lists = nj;
  S.postings = total;
  Lane* L = ctx->lanes[0];
  PassDev D;  // (the list table alone: every counting pass has a result block of its own)
  if (int rc = pass_begin(ctx, L, t, 0, "device allocation (host census)", &D, &T)) return rc;
  // ---- counting passes: the table sized and zeroed, one launch over the flattened keys, the table's
  //      hosts flagged and scanned, the four counters read back; on overflow again with four times the slots
  const int lds = (int)census_knob("YRWI_CENSUS_LDS_SLOTS", CENSUS_LDS_DEFAULT, 64, 4096);
  int64_t want = 1;
  while (want < 2 * total && want < CENSUS_SLOTS_MAX) want *= 2;
  int64_t slots = std::min(want, census_knob("YRWI_CENSUS_SLOTS", CENSUS_SLOTS_DEFAULT, 64, CENSUS_SLOTS_MAX));
  unsigned long long* tab = nullptr;
  int32_t* flag = nullptr;
  int64_t* px = nullptr;
  int64_t ctr[CEN_WORDS] = {0, 0, 0, 0};
  for (;; slots *= 4) {
    if (slots > CENSUS_SLOTS_MAX) return ctx->fail(YRWI_E_NOMEM, "host census table beyond 2^30 slots");
    // the counters sit in front of the table: one memset zeroes both
    unsigned long long* blk = arena_alloc<unsigned long long>(L, CEN_WORDS + 2 * slots);
    flag = arena_alloc<int32_t>(L, slots + 1);
    px = arena_alloc<int64_t>(L, slots + 1);
    size_t tb = 0;
    HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag, px, (int)(slots + 1), L->stream));
    void* tmp = L->arena.alloc(tb);
    if (!blk || !flag || !px || !tmp) return ctx->fail(YRWI_E_NOMEM, "device allocation (host census table)");
    unsigned long long* d_ctr = blk;
    tab = blk + CEN_WORDS;  // 32 B into a 256-B aligned block: 16-B slots
    HIPCHK(ctx, hipMemsetAsync(blk, 0, (size_t)(CEN_WORDS + 2 * slots) * 8, L->stream));
    hipEvent_t e0 = L->event(), e1 = L->event();
    HIPCHK(ctx, hipEventRecord(e0, L->stream));
    hipLaunchKernelGGL(k_census, dim3(span_blocks(total)), dim3(256), (size_t)lds * 12, L->stream, D.jobs, D.off, nj,
                       total, lds, tab, (uint64_t)(slots - 1), d_ctr);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(e1, L->stream));
    hipLaunchKernelGGL(k_census_flag, dim3(blocks(slots + 1)), dim3(256), 0, L->stream, tab, slots, minp, flag, d_ctr);
    HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tb, flag, px, (int)(slots + 1), L->stream));
    HIPCHK(ctx, hipGetLastError());
    const int64_t* h = reinterpret_cast<const int64_t*>(readback(L, &L->down_stage, d_ctr, CEN_WORDS, 8, 8));
    if (!h) return ctx->take(L, YRWI_E_HIP);
    T.launches += 5;
    HIPCHK(ctx, lane_sync(L));
    T.syncs++;
    std::memcpy(ctr, h, sizeof(ctr));  // (the pinned landing buffer is reused below)
    float msf = 0.f;
    if (hipEventElapsedTime(&msf, e0, e1) == hipSuccess) S.t_count_ns += (int64_t)((double)msf * 1e6);
    S.passes++;
    S.table_slots = slots;
    S.lds_bypass = ctr[CEN_BYPASS];
    if (!ctr[CEN_OVERFLOW]) break;
  }
  S.hosts = ctr[CEN_HOSTS];
  S.hosts_passing = ctr[CEN_PASSING];
  // ---- the passing hosts compacted and sorted; the first min(hosts_passing, cap) cross to the host
  const int64_t np = S.hosts_passing, nw = std::min(np, cap);
  const int ns = (int)std::max<int64_t>(np, 1);  // (no host passes: the sorts run over one unused element)
  uint64_t* okey = arena_alloc<uint64_t>(L, np);
  uint64_t* ocnt = arena_alloc<uint64_t>(L, np);
  uint64_t* skey = arena_alloc<uint64_t>(L, np);
  uint64_t* scnt = arena_alloc<uint64_t>(L, np);
  int cbits = 1;  // bits of a count: no host has more than `total` postings
  while (cbits < 64 && ((int64_t)1 << cbits) <= total) cbits++;
  size_t t1 = 0, t2 = 0;
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, t1, okey, skey, ocnt, scnt, ns, 0, 36, L->stream));
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(nullptr, t2, scnt, ocnt, skey, okey, ns, 0, cbits, L->stream));
  void* stmp = L->arena.alloc(std::max(t1, t2));
  if (!okey || !ocnt || !skey || !scnt || !stmp) return ctx->fail(YRWI_E_NOMEM, "device allocation (host census sort)");
  hipLaunchKernelGGL(k_census_place, dim3(blocks(slots)), dim3(256), 0, L->stream, tab, slots, flag, px, okey, ocnt);
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(stmp, t1, okey, skey, ocnt, scnt, ns, 0, 36, L->stream));
  const uint64_t *rkey = skey, *rcnt = scnt;
  if (order == YRWI_CENSUS_BY_COUNT) {  // stable: equal counts stay in host order
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(stmp, t2, scnt, ocnt, skey, okey, ns, 0, cbits, L->stream));
    rkey = okey;
    rcnt = ocnt;
    T.launches++;
  }
  HIPCHK(ctx, hipGetLastError());
  const uint64_t* hk = reinterpret_cast<const uint64_t*>(readback(L, &L->out_stage, rkey, nw, 8, 8));
  const int64_t* hc = reinterpret_cast<const int64_t*>(readback(L, &L->down_stage, rcnt, nw, 8, 8));
  if (!hk || !hc) return ctx->take(L, YRWI_E_HIP);
  T.launches += 4;
  HIPCHK(ctx, lane_sync(L));
  T.syncs++;
  for (int64_t i = 0; i < nw; i++) {
    for (int j = 0; j < 6; j++) hosts6_out[i * 6 + j] = (uint8_t)ALPHA[(hk[i] >> (6 * (5 - j))) & 63];
    counts_out[i] = hc[i];
  }
  return finish(nw);
}

// ---------------------------------------------------------------- census of the urls
//
// yrwi_url_census / yrwi_host_url_census: which urls the selected lists hold and in how many of them each
// (its references), and how many distinct urls and postings every host has (UNVERIFIED against a reference
// line: the reference has no method that groups the RWI by url).  A group-by over the 32-bit url ids
// (ListRec::uid, brought up to date first), never over the 9-byte keys: the key of an id is read from the
// dictionary (dkhi / dklo) only for the host test and for the urls that leave the device, and ascending id is
// ascending url hash, so YRWI_UCENSUS_BY_URL needs no sort.
//
// HIST (k_uc_hist): grid, spans and cursor of the other streaming passes over the uid of every selected
// posting, 4 B each (the lists' uid pointers are a table beside the list table); one 32-bit global atomic add
// per posting into a zeroed count per dictionary id.  The ids of a list ascend and are distinct, so a wave's
// adds collide only where it covers several short lists.  Its tail walks the dictionary.
// SORT (k_uc_gather): the selected ids into one array, radix-sorted over ceil(log2 dict_urls) bits; the heads
// of the runs of equal ids are flagged and scanned, and every head stores its id and its place: the
// references of a run are the distance to the next head.  Its cost follows the selected postings alone.
//
// One tail over the candidates of either path (UcCand: every dictionary id with its count, or every run):
// flag (references >= min, host in the sorted set: host_slot over the set staged in LDS or left in global
// memory), scan, compact to (id, refs) in id order; BY_REFS: one stable radix sort by refs descending;
// k_uc_place writes the characters of the first min(passing, cap) from their dictionary keys.
// The host form groups the compacted urls by host36 of their key: one radix sort of (host, refs) over 36
// bits, then the head flag, scan and run step of SORT over the hosts: a host's urls are its run's length, its
// postings the difference of the scanned refs at its run's ends; then the same flag, scan and compact over
// the runs, a stable sort by urls descending for BY_COUNT, and k_uc_hplace.  The postings are read once.
namespace {

// the call takes SORT when postings * UC_SORT_WEIGHT <= dict_urls.  UNMEASURED: tools/url_census.py has not
// run on the device yet; 8 is the placeholder the table is to replace
constexpr int64_t UC_SORT_WEIGHT = 8;
// the counters of a flagging pass
enum { UC_URLS = 0, UC_HOSTED = 1, UC_PASSING = 2, UC_MAXREFS = 3, UC_WORDS = 4 };

// a lane's place in the flattened lists and its list's url ids
struct UidCursor : SegCursor {
  const uint32_t* ids = nullptr;
};

// One step of a thread over the url ids, key_tile's counterpart: postings base + 256 u + thread (u < 4) below
// end -> their ids (live[u]: below end).  The four loads are issued before the caller's first use of one.
__device__ __forceinline__ void uid_tile(UidCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                         const uint32_t* const* __restrict__ uid, int nj, int64_t total, int64_t base,
                                         int64_t end, uint32_t id[4], bool live[4]) {
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int64_t i = base + u * 256 + threadIdx.x;
    live[u] = i < end;
    id[u] = 0;
    if (live[u]) {
      if (i >= s.hi) {
        seg_seek(s, jobs, off, nj, total, i);
        s.ids = uid[s.c];
      }
      id[u] = s.ids[i - s.lo];
    }
  }
}

// HIST: cnt[id] += 1 for every selected posting (cnt zeroed by the caller; an id is below nd)
__global__ __launch_bounds__(256) void k_uc_hist(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                 const uint32_t* const* __restrict__ uid, int nj, int64_t total,
                                                 int64_t nd, uint32_t* __restrict__ cnt) {
  int64_t begin, end;
  span_of(total, &begin, &end);
  UidCursor cur;
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    uint32_t id[4];
    bool live[4];
    uid_tile(cur, jobs, off, uid, nj, total, base, end, id, live);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (live[u] && (int64_t)id[u] < nd) atomicAdd(&cnt[id[u]], 1u);
  }
}

// SORT: out[i] = the url id of flattened posting i
__global__ __launch_bounds__(256) void k_uc_gather(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                   const uint32_t* const* __restrict__ uid, int nj, int64_t total,
                                                   uint32_t* __restrict__ out) {
  int64_t begin, end;
  span_of(total, &begin, &end);
  UidCursor cur;
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    uint32_t id[4];
    bool live[4];
    uid_tile(cur, jobs, off, uid, nj, total, base, end, id, live);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (live[u]) out[base + u * 256 + threadIdx.x] = id[u];
  }
}

// flag[i] = s[i] begins a run of equal keys of the ascending s[0, n); flag[n] = 0 (the scan's last element)
template <class K>
__global__ __launch_bounds__(256) void k_uc_heads(const K* __restrict__ s, int64_t n, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  flag[i] = i < n && (i == 0 || s[i] != s[i - 1]) ? 1 : 0;
}

// hx = the exclusive scan of flag: run r = hx[i] of head i gets its key and its place; *nruns = hx[n] and
// rpos[*nruns] = n, so run r holds rpos[r + 1] - rpos[r] elements
template <class K>
__global__ __launch_bounds__(256) void k_uc_runs(const K* __restrict__ s, int64_t n, const int32_t* __restrict__ flag,
                                                 const int64_t* __restrict__ hx, K* __restrict__ rkey,
                                                 uint32_t* __restrict__ rpos, int64_t* __restrict__ nruns) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    rpos[hx[n]] = (uint32_t)n;
    *nruns = hx[n];
  } else if (flag[i]) {
    rkey[hx[i]] = s[i];
    rpos[hx[i]] = (uint32_t)i;
  }
}

// The candidates of a flagging pass, i < m: (cnt) dictionary id i with cnt[i] references, none: no candidate;
// (rpos) run i of *nruns with the id rid[i] (rid null: i itself) and rpos[i + 1] - rpos[i] references.
struct UcCand {
  int64_t m;
  const uint32_t* cnt;
  const uint32_t* rid;
  const uint32_t* rpos;
  const int64_t* nruns;
};

template <bool RUNS>
__device__ __forceinline__ bool uc_cand(const UcCand& C, int64_t i, uint32_t* id, uint32_t* refs) {
  if (i >= C.m) return false;
  if (RUNS) {
    if (i >= *C.nruns) return false;
    *id = C.rid ? C.rid[i] : (uint32_t)i;
    *refs = C.rpos[i + 1] - C.rpos[i];
    return true;
  }
  *id = (uint32_t)i;
  *refs = C.cnt[i];
  return *refs != 0;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = std::max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

// flag[i] = candidate i has at least minr references and (nh > 0) the host of its dictionary key is in the
// set; flag[m] = 0.  ctr: candidates, of which with the host in the set, of which flagged, and the most
// references of one with the host in the set; one atomic each per wave.  At most SPAN_BLOCKS workgroups
// stride over the candidates, so the set is staged once per workgroup.
template <bool RUNS, bool LDS>
__global__ __launch_bounds__(256) void k_uc_flag(UcCand C, const uint64_t* __restrict__ dkhi,
                                                 const uint8_t* __restrict__ dklo, const uint64_t* __restrict__ hset,
                                                 int nh, uint32_t minr, int32_t* __restrict__ flag,
                                                 unsigned long long* __restrict__ ctr) {
  __shared__ uint64_t s_set[LDS ? HOST_LDS_MAX : 1];
  stage_set<LDS>(s_set, hset, nh);
  const uint64_t* hs = LDS ? s_set : hset;
  uint32_t n_url = 0, n_hosted = 0, n_pass = 0, most = 0;
  for (int64_t b = (int64_t)blockIdx.x * 256; b <= C.m; b += (int64_t)gridDim.x * 256) {
    const int64_t i = b + threadIdx.x;
    uint32_t id = 0, refs = 0;
    const bool url = uc_cand<RUNS>(C, i, &id, &refs);
    bool hosted = url;
    if (url && nh > 0) hosted = host_slot(hs, nh, host36(dkhi[id], dklo[id])) >= 0;
    const bool pass = hosted && refs >= minr;
    if (i <= C.m) flag[i] = pass ? 1 : 0;
    n_url += url;
    n_hosted += hosted;
    n_pass += pass;
    if (hosted) most = std::max(most, refs);
  }
  n_url = wave_sum(n_url);
  n_hosted = wave_sum(n_hosted);
  n_pass = wave_sum(n_pass);
  most = wave_max(most);
  if ((threadIdx.x & 63) == 0) {
    if (n_url) atomicAdd(&ctr[UC_URLS], (unsigned long long)n_url);
    if (n_hosted) atomicAdd(&ctr[UC_HOSTED], (unsigned long long)n_hosted);
    if (n_pass) atomicAdd(&ctr[UC_PASSING], (unsigned long long)n_pass);
    if (most) atomicMax(&ctr[UC_MAXREFS], (unsigned long long)most);
  }
}

// the flagged candidates, in their order: px = the exclusive scan of flag
template <bool RUNS>
__global__ __launch_bounds__(256) void k_uc_compact(UcCand C, const int32_t* __restrict__ flag,
                                                    const int64_t* __restrict__ px, uint32_t* __restrict__ oid,
                                                    uint32_t* __restrict__ oref) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.m || !flag[i]) return;
  uint32_t id = 0, refs = 0;
  uc_cand<RUNS>(C, i, &id, &refs);
  oid[px[i]] = id;
  oref[px[i]] = refs;
}

// result i < n: the 12 characters of the dictionary key of id[i] (key_chars' rule; three words) and its references
__global__ __launch_bounds__(256) void k_uc_place(const uint32_t* __restrict__ id, const uint32_t* __restrict__ refs,
                                                  int64_t n, const uint64_t* __restrict__ dkhi,
                                                  const uint8_t* __restrict__ dklo, uint32_t* __restrict__ urls12,
                                                  int64_t* __restrict__ refs_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t hi = dkhi[id[i]];
  const uint32_t lo = dklo[id[i]];
  const uint64_t x = hi >> 4;
  uint32_t w[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 12; j++) {
    const uint32_t v = j < 10 ? (uint32_t)(x >> (6 * (9 - j))) & 63u
                              : j == 10 ? (((uint32_t)hi & 15u) << 2) | (lo >> 6) : lo & 63u;
    w[j >> 2] |= b64_char(v) << (8 * (j & 3));
  }
#pragma unroll
  for (int k = 0; k < 3; k++) urls12[i * 3 + k] = w[k];
  refs_out[i] = (int64_t)refs[i];
}

// hk[i] = the host of url id[i]
__global__ __launch_bounds__(256) void k_uc_hostkeys(const uint32_t* __restrict__ id, int64_t n,
                                                     const uint64_t* __restrict__ dkhi,
                                                     const uint8_t* __restrict__ dklo, uint64_t* __restrict__ hk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) hk[i] = host36(dkhi[id[i]], dklo[id[i]]);
}

// result i < n: host run r = run[i]: its key, its urls (the run's length) and its postings (psum: the
// exclusive scan of the urls' references in host order), three words
__global__ __launch_bounds__(256) void k_uc_hplace(const uint32_t* __restrict__ run, int64_t n,
                                                   const uint64_t* __restrict__ rkey, const uint32_t* __restrict__ rpos,
                                                   const uint32_t* __restrict__ psum, uint64_t* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = run[i], lo = rpos[r], hi = rpos[r + 1];
  rec[i * 3] = rkey[r];
  rec[i * 3 + 1] = hi - lo;
  rec[i * 3 + 2] = psum[hi] - psum[lo];
}

// scratch of a flag / scan over m + 1 elements
struct UcScan {
  int32_t* flag = nullptr;
  int64_t* px = nullptr;
  void* tmp = nullptr;
  size_t tb = 0;
};

int uc_scan_alloc(yrwi_ctx* ctx, Lane* L, int64_t m, UcScan* X) {
  X->flag = arena_alloc<int32_t>(L, m + 1);
  X->px = arena_alloc<int64_t>(L, m + 1);
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, X->tb, X->flag, X->px, (int)(m + 1), L->stream));
  X->tmp = L->arena.alloc(X->tb);
  if (!X->flag || !X->px || !X->tmp) return ctx->fail(YRWI_E_NOMEM, "device allocation (url census scan)");
  return 0;
}

// flag, scan, the counters read back and waited for, the flagged candidates compacted: 4 launches, one sync.
// -> *oid / *oref: the np flagged candidates in their order (at least one element each), ctr: the counters
template <bool RUNS>
int uc_tail(yrwi_ctx* ctx, Lane* L, const UcCand& C, const uint64_t* d_hk, int nh, uint32_t minr, UcScan& X,
            unsigned long long* d_ctr, int64_t ctr[UC_WORDS], uint32_t** oid, uint32_t** oref, int64_t* np, Tally* T) {
  const dim3 g((unsigned)std::min<int64_t>(blocks(C.m + 1), SPAN_BLOCKS)), b(256);
  if (nh <= HOST_LDS_MAX)
    hipLaunchKernelGGL((k_uc_flag<RUNS, true>), g, b, 0, L->stream, C, ctx->dkhi, ctx->dklo, d_hk, nh, minr, X.flag, d_ctr);
  else
    hipLaunchKernelGGL((k_uc_flag<RUNS, false>), g, b, 0, L->stream, C, ctx->dkhi, ctx->dklo, d_hk, nh, minr, X.flag, d_ctr);
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(X.tmp, X.tb, X.flag, X.px, (int)(C.m + 1), L->stream));
  HIPCHK(ctx, hipGetLastError());
  const int64_t* h = reinterpret_cast<const int64_t*>(readback(L, &L->down_stage, d_ctr, UC_WORDS, 8, 8));
  if (!h) return ctx->take(L, YRWI_E_HIP);
  T->launches += 3;
  HIPCHK(ctx, lane_sync(L));
  T->syncs++;
  std::memcpy(ctr, h, UC_WORDS * sizeof(int64_t));  // (the pinned landing buffer is reused)
  *np = ctr[UC_PASSING];
  *oid = arena_alloc<uint32_t>(L, *np);
  *oref = arena_alloc<uint32_t>(L, *np);
  if (!*oid || !*oref) return ctx->fail(YRWI_E_NOMEM, "device allocation (url census result)");
  hipLaunchKernelGGL((k_uc_compact<RUNS>), dim3(std::max(blocks(C.m), 1u)), b, 0, L->stream, C, X.flag, X.px, *oid, *oref);
  HIPCHK(ctx, hipGetLastError());
  T->launches++;
  return 0;
}

int bits_for(int64_t values) {  // bits that hold 0 .. values - 1, at least one
  int b = 1;
  while (b < 63 && ((int64_t)1 << b) < values) b++;
  return b;
}

// What both calls share: arguments -> selection, url ids up to date, the counting pass on the chosen path and
// the tail over its candidates.  -> *done: nothing was selected (S holds the empty result); else *oid / *oref:
// the S->urls_passing urls with at least minr references and their host in the set, in id order.
struct UcCall {
  Tally T;
  yrwi_ucensus_stats S;
  HostPass P;
  Lane* L = nullptr;
  unsigned long long* d_ctr = nullptr;  // two counter blocks, zeroed: the urls' tail, the hosts' tail
  uint32_t *oid = nullptr, *oref = nullptr;
};

int uc_urls(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6, int32_t nhosts,
            int64_t min_refs, UcCall* U, bool* done) {
  std::memset(&U->S, 0, sizeof(U->S));
  yrwi_ucensus_stats& S = U->S;
  HostPass& P = U->P;
  *done = true;
  if (int rc = host_select(ctx, terms12, nterms, hosts6, nhosts, &P)) return rc;
  if (P.jobs.empty()) return 0;
  if (int rc = ensure_url_ids(ctx)) return rc;
  // the repack behind new ids may have moved the lists: they are flattened again, with their ids beside them
  ListSel sel;
  if (int rc = select_lists(ctx, terms12, nterms, false, &sel)) return rc;
  static_cast<RmTable&>(P) = RmTable();
  rm_table(sel, &P);
  std::vector<const uint32_t*> uids;
  for (const auto& s : sel) uids.push_back(s.second->uid);
  *done = false;
  const int nj = (int)P.jobs.size(), nh = (int)P.hk.size();
  const int64_t total = P.total, nd = ctx->nurls;
  if (total >= (int64_t)INT32_MAX || nd >= (int64_t)INT32_MAX)
    return ctx->fail(YRWI_E_LIMIT, "2^31 - 1 selected postings or dictionary urls or more");
  S.lists = nj;
  S.postings = total;
  S.dict_urls = nd;
  bool sort = total * UC_SORT_WEIGHT <= nd;
  const char* forced = getenv("YRWI_UCENSUS_PATH");
  if (forced && !strcmp(forced, "hist")) sort = false;
  if (forced && !strcmp(forced, "sort")) sort = true;
  S.path = sort ? YRWI_UCENSUS_SORT : YRWI_UCENSUS_HIST;
  Lane* L = U->L = ctx->lanes[0];
  const char* nomem = "device allocation (url census)";
  PassDev D;
  const uint32_t** d_uid = nullptr;
  uint64_t* d_hk = nullptr;
  if (int rc = pass_begin(ctx, L, P, 0, nomem, &D, &U->T, &d_uid, uids, &d_hk, P.hk)) return rc;
  Tally& T = U->T;
  const uint32_t minr = (uint32_t)std::min<int64_t>(std::max<int64_t>(min_refs, 1), (int64_t)UINT32_MAX);
  const int64_t m = sort ? total : nd;  // the candidates of the tail: runs (no more than postings) or ids
  // the counters sit in front of HIST's counts: one memset zeroes both
  unsigned long long* blk = arena_alloc<unsigned long long>(L, 2 * UC_WORDS + (sort ? 0 : (nd + 1) / 2));
  UcScan X;
  if (!blk) return ctx->fail(YRWI_E_NOMEM, nomem);
  if (int rc = uc_scan_alloc(ctx, L, m, &X)) return rc;
  U->d_ctr = blk;
  HIPCHK(ctx, hipMemsetAsync(blk, 0, (size_t)(2 * UC_WORDS + (sort ? 0 : (nd + 1) / 2)) * 8, L->stream));
  T.launches++;
  UcCand C{m, nullptr, nullptr, nullptr, nullptr};
  const dim3 g(span_blocks(total)), b(256);
  hipEvent_t e0 = L->event(), e1 = L->event();
  if (!sort) {
    uint32_t* cnt = reinterpret_cast<uint32_t*>(blk + 2 * UC_WORDS);
    HIPCHK(ctx, hipEventRecord(e0, L->stream));
    hipLaunchKernelGGL(k_uc_hist, g, b, 0, L->stream, D.jobs, D.off, d_uid, nj, total, nd, cnt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(e1, L->stream));
    T.launches++;
    C.cnt = cnt;
  } else {
    uint32_t* ids = arena_alloc<uint32_t>(L, total);
    uint32_t* sorted = arena_alloc<uint32_t>(L, total);
    uint32_t* rid = arena_alloc<uint32_t>(L, total);
    uint32_t* rpos = arena_alloc<uint32_t>(L, total + 1);
    size_t tb = 0;
    const int bits = bits_for(nd);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, tb, ids, sorted, (int)total, 0, bits, L->stream));
    void* tmp = L->arena.alloc(tb);
    int64_t* nruns = arena_alloc<int64_t>(L, 1);
    if (!ids || !sorted || !rid || !rpos || !tmp || !nruns) return ctx->fail(YRWI_E_NOMEM, nomem);
    HIPCHK(ctx, hipEventRecord(e0, L->stream));
    hipLaunchKernelGGL(k_uc_gather, g, b, 0, L->stream, D.jobs, D.off, d_uid, nj, total, ids);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(tmp, tb, ids, sorted, (int)total, 0, bits, L->stream));
    hipLaunchKernelGGL((k_uc_heads<uint32_t>), dim3(blocks(total + 1)), b, 0, L->stream, sorted, total, X.flag);
    HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(X.tmp, X.tb, X.flag, X.px, (int)(total + 1), L->stream));
    // (the number of runs stays on the device: the tail reads it there)
    hipLaunchKernelGGL((k_uc_runs<uint32_t>), dim3(blocks(total + 1)), b, 0, L->stream, sorted, total, X.flag, X.px, rid,
                       rpos, nruns);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(e1, L->stream));
    T.launches += 5;
    C.rid = rid;
    C.rpos = rpos;
    C.nruns = nruns;
  }
  int64_t ctr[UC_WORDS], np = 0;
  if (int rc = sort ? uc_tail<true>(ctx, L, C, d_hk, nh, minr, X, blk, ctr, &U->oid, &U->oref, &np, &T)
                    : uc_tail<false>(ctx, L, C, d_hk, nh, minr, X, blk, ctr, &U->oid, &U->oref, &np, &T))
    return rc;
  float msf = 0.f;
  if (hipEventElapsedTime(&msf, e0, e1) == hipSuccess) S.t_count_ns = (int64_t)((double)msf * 1e6);
  (void)hipGetLastError();  // a statistics event that could not be read is not the call's error
  S.urls = ctr[UC_URLS];
  S.urls_hosted = ctr[UC_HOSTED];
  S.urls_passing = ctr[UC_PASSING];
  S.max_refs = ctr[UC_MAXREFS];
  return 0;
}

void uc_finish(UcCall& U, std::chrono::steady_clock::time_point t_begin, int64_t n, int64_t* nout,
               yrwi_ucensus_stats* st) {
  U.S.launches = U.T.launches;
  U.S.syncs = U.T.syncs;
  U.S.t_total_ns =
      std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
  if (nout) *nout = n;
  if (st) *st = U.S;
}

}  // namespace

extern "C" int yrwi_url_census(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6,
                               int32_t nhosts, int32_t order, int64_t min_refs, uint8_t* urls12_out, int64_t* refs_out,
                               int64_t cap, int64_t* nout, yrwi_ucensus_stats* st) {
  if (!ctx || nterms < 0 || nhosts < 0 || (nterms > 0 && !terms12) || (nhosts > 0 && !hosts6)) return YRWI_E_ARG;
  if (order != YRWI_UCENSUS_BY_URL && order != YRWI_UCENSUS_BY_REFS) return ctx->fail(YRWI_E_ARG, "unknown url census order");
  if (cap < 0 || (cap > 0 && (!urls12_out || !refs_out))) return ctx->fail(YRWI_E_ARG, "url census capacity without buffers");
  const auto t_begin = std::chrono::steady_clock::now();
  UcCall U;
  bool done = false;
  if (int rc = uc_urls(ctx, terms12, nterms, hosts6, nhosts, min_refs, &U, &done)) return rc;
  if (done) {
    uc_finish(U, t_begin, 0, nout, st);
    return 0;
  }
  Lane* L = U.L;
  Tally& T = U.T;
  // ---- BY_REFS: one stable sort by references descending (equal references stay in url order); the first
  //      min(urls_passing, cap) get their characters and cross to the host
  const int64_t np = U.S.urls_passing, nw = std::min(np, cap);
  const int ns = (int)std::max<int64_t>(np, 1);  // (no url passes: the sort runs over one unused element)
  const uint32_t *rid = U.oid, *rref = U.oref;
  if (order == YRWI_UCENSUS_BY_REFS) {
    uint32_t* sid = arena_alloc<uint32_t>(L, ns);
    uint32_t* sref = arena_alloc<uint32_t>(L, ns);
    const int rb = bits_for(U.S.lists + 1);  // no url has more references than there are lists
    size_t tb = 0;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb, U.oref, sref, U.oid, sid, ns, 0, rb, L->stream));
    void* tmp = L->arena.alloc(tb);
    if (!sid || !sref || !tmp) return ctx->fail(YRWI_E_NOMEM, "device allocation (url census sort)");
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(tmp, tb, U.oref, sref, U.oid, sid, ns, 0, rb, L->stream));
    T.launches++;
    rid = sid;
    rref = sref;
  }
  uint32_t* d_urls = arena_alloc<uint32_t>(L, nw * 3);
  int64_t* d_refs = arena_alloc<int64_t>(L, nw);
  if (!d_urls || !d_refs) return ctx->fail(YRWI_E_NOMEM, "device allocation (url census output)");
  hipLaunchKernelGGL(k_uc_place, dim3(std::max(blocks(nw), 1u)), dim3(256), 0, L->stream, rid, rref, nw, ctx->dkhi,
                     ctx->dklo, d_urls, d_refs);
  HIPCHK(ctx, hipGetLastError());
  const uint8_t* hu = readback(L, &L->out_stage, d_urls, nw, 12, 12);
  const uint8_t* hr = readback(L, &L->down_stage, d_refs, nw, 8, 8);
  if (!hu || !hr) return ctx->take(L, YRWI_E_HIP);
  T.launches += 3;
  HIPCHK(ctx, lane_sync(L));
  T.syncs++;
  if (nw > 0) {
    std::memcpy(urls12_out, hu, (size_t)nw * 12);
    std::memcpy(refs_out, hr, (size_t)nw * 8);
  }
  uc_finish(U, t_begin, nw, nout, st);
  return 0;
}

extern "C" int yrwi_host_url_census(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t order,
                                    int64_t min_urls, uint8_t* hosts6_out, int64_t* urls_out, int64_t* postings_out,
                                    int64_t cap, int64_t* nout, yrwi_ucensus_stats* st) {
  if (!ctx || nterms < 0 || (nterms > 0 && !terms12)) return YRWI_E_ARG;
  if (order != YRWI_CENSUS_BY_HOST && order != YRWI_CENSUS_BY_COUNT) return ctx->fail(YRWI_E_ARG, "unknown census order");
  if (cap < 0 || (cap > 0 && (!hosts6_out || !urls_out || !postings_out)))
    return ctx->fail(YRWI_E_ARG, "url census capacity without buffers");
  const auto t_begin = std::chrono::steady_clock::now();
  UcCall U;
  bool done = false;
  if (int rc = uc_urls(ctx, terms12, nterms, nullptr, 0, 1, &U, &done)) return rc;
  if (done) {
    uc_finish(U, t_begin, 0, nout, st);
    return 0;
  }
  Lane* L = U.L;
  Tally& T = U.T;
  const char* nomem = "device allocation (host url census)";
  // ---- the nu distinct urls as (host, refs), sorted by host; the runs of a host: its urls; the scanned refs
  //      at a run's ends: its postings
  const int64_t nu = U.S.urls_passing;
  const int ns = (int)std::max<int64_t>(nu, 1);
  const dim3 b(256);
  uint64_t* hk = arena_alloc<uint64_t>(L, ns);
  uint64_t* hk2 = arena_alloc<uint64_t>(L, ns);
  uint32_t* ref2 = arena_alloc<uint32_t>(L, ns + 1);
  uint32_t* psum = arena_alloc<uint32_t>(L, ns + 1);
  uint64_t* rkey = arena_alloc<uint64_t>(L, ns);
  uint32_t* rpos = arena_alloc<uint32_t>(L, ns + 1);
  int64_t* nruns = arena_alloc<int64_t>(L, 1);
  UcScan X;
  if (int rc = uc_scan_alloc(ctx, L, nu, &X)) return rc;
  size_t t1 = 0, t2 = 0;
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, t1, hk, hk2, U.oref, ref2, ns, 0, 36, L->stream));
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, t2, ref2, psum, ns + 1, L->stream));
  void* tmp = L->arena.alloc(std::max(t1, t2));
  if (!hk || !hk2 || !ref2 || !psum || !rkey || !rpos || !nruns || !tmp) return ctx->fail(YRWI_E_NOMEM, nomem);
  hipLaunchKernelGGL(k_uc_hostkeys, dim3(std::max(blocks(nu), 1u)), b, 0, L->stream, U.oid, nu, ctx->dkhi, ctx->dklo, hk);
  HIPCHK(ctx, hipMemsetAsync(ref2, 0, (size_t)(ns + 1) * 4, L->stream));  // (the scan reads one element more than the sort writes)
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(tmp, t1, hk, hk2, U.oref, ref2, ns, 0, 36, L->stream));
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, t2, ref2, psum, ns + 1, L->stream));
  hipLaunchKernelGGL((k_uc_heads<uint64_t>), dim3(blocks(nu + 1)), b, 0, L->stream, hk2, nu, X.flag);
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(X.tmp, X.tb, X.flag, X.px, (int)(nu + 1), L->stream));
  hipLaunchKernelGGL((k_uc_runs<uint64_t>), dim3(blocks(nu + 1)), b, 0, L->stream, hk2, nu, X.flag, X.px, rkey, rpos,
                     nruns);
  HIPCHK(ctx, hipGetLastError());
  T.launches += 7;
  // ---- the hosts with at least min_urls urls: the tail of the urls over the runs (a run's "references" are its urls)
  const uint32_t minu = (uint32_t)std::min<int64_t>(std::max<int64_t>(min_urls, 1), (int64_t)UINT32_MAX);
  const UcCand C{nu, nullptr, nullptr, rpos, nruns};
  int64_t ctr[UC_WORDS], np = 0;
  uint32_t *orun = nullptr, *ourls = nullptr;
  if (int rc = uc_tail<true>(ctx, L, C, nullptr, 0, minu, X, U.d_ctr + UC_WORDS, ctr, &orun, &ourls, &np, &T)) return rc;
  U.S.hosts = ctr[UC_URLS];
  U.S.hosts_passing = np;
  const int64_t nw = std::min(np, cap);
  const int nr = (int)std::max<int64_t>(np, 1);
  const uint32_t* run = orun;  // already BY_HOST: the runs ascend by host
  if (order == YRWI_CENSUS_BY_COUNT) {  // stable: equal url counts stay in host order
    uint32_t* srun = arena_alloc<uint32_t>(L, nr);
    uint32_t* surls = arena_alloc<uint32_t>(L, nr);
    const int cb = bits_for(nu + 1);
    size_t tb = 0;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tb, ourls, surls, orun, srun, nr, 0, cb, L->stream));
    void* stmp = L->arena.alloc(tb);
    if (!srun || !surls || !stmp) return ctx->fail(YRWI_E_NOMEM, nomem);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(stmp, tb, ourls, surls, orun, srun, nr, 0, cb, L->stream));
    T.launches++;
    run = srun;
  }
  uint64_t* rec = arena_alloc<uint64_t>(L, nw * 3);
  if (!rec) return ctx->fail(YRWI_E_NOMEM, nomem);
  hipLaunchKernelGGL(k_uc_hplace, dim3(std::max(blocks(nw), 1u)), b, 0, L->stream, run, nw, rkey, rpos, psum, rec);
  HIPCHK(ctx, hipGetLastError());
  const uint64_t* hrec = reinterpret_cast<const uint64_t*>(readback(L, &L->out_stage, rec, nw, 24, 24));
  if (!hrec) return ctx->take(L, YRWI_E_HIP);
  T.launches += 2;
  HIPCHK(ctx, lane_sync(L));
  T.syncs++;
  for (int64_t i = 0; i < nw; i++) {
    for (int j = 0; j < 6; j++) hosts6_out[i * 6 + j] = (uint8_t)ALPHA[(hrec[i * 3] >> (6 * (5 - j))) & 63];
    urls_out[i] = (int64_t)hrec[i * 3 + 1];
    postings_out[i] = (int64_t)hrec[i * 3 + 2];
  }
  uc_finish(U, t_begin, nw, nout, st);
  return 0;
}

// ---------------------------------------------------------------- retention: age and cap
//
// yrwi_retain / yrwi_retention_count (UNVERIFIED against a reference line: the rules are this project's).
// The age rule removes every selected posting whose lastModified day (the `a` cell) is below min_day; the
// cap rule leaves a list that still has more than max_refs rows its max_refs newest, ties at the cut day
// kept in url-hash order.  One streaming pass over the a cells of the flattened selection (k_ret_mark, grid
// and spans of k_host_mark, 40 B per posting: the cell sits inside the row) counts the old rows per list,
// keeps the smallest and the largest day and, for the dry run, fills the histogram of the days: every
// workgroup counts in an LDS window of RET_WIN days around the day of its span's first posting and adds the
// window to the device table at the end of its span; a day outside the window goes straight to the device
// table, equal days of the wave as one add (hist_bypass).  The per-list counts are read back once, and the
// host then knows every list's final length.  The cut day d* and the quota q of the lists over the cap are
// found on the device by a two-level radix select over the flattened postings of those lists (k_ret_bins:
// 256 bins of the high byte per list, k_ret_pick, 256 bins of the low byte within the chosen bucket,
// k_ret_pick; only survivors of the age rule are counted; a wave sums a list's bins in LDS and adds them to
// the device bins on leaving the list) and
// are consumed by the flag kernels of compact_commit: with a cap a chunk is flagged in two steps, the marks
// a == d* scanned first for a row's rank among its list's rows of the cut day.
namespace {

constexpr int RET_WIN = 8192;  // days of a workgroup's LDS histogram window (32 KiB)
constexpr int RET_DAYS = 65536;
enum { RET_MINV = 0, RET_MAX1 = 1, RET_BYPASS = 2, RET_WORDS = 3 };

// a lane's place in the flattened lists and its list's rows
struct DayCursor : SegCursor {
  const uint8_t* rows = nullptr;
};

// -> the lane entered another list
__device__ __forceinline__ bool day_seek(DayCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                         int nj, int64_t total, int64_t i) {
  if (i < s.hi) return false;
  seg_seek(s, jobs, off, nj, total, i);
  s.rows = jobs[s.c].rows;
  return true;
}

// One step of a thread over the rows, key_tile's counterpart: postings base + 256 u + thread (u < 4) below end ->
// their a cells and lists (-1: past end).  The four loads are issued before the first use.  at(u, entered) is
// called for every posting below end with the cursor at it, entered: in another list than the lane's last.
template <class At>
__device__ __forceinline__ void day_tile(DayCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                         int nj, int64_t total, int64_t base, int64_t end, int a[4], int c[4], At at) {
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int64_t i = base + u * 256 + threadIdx.x;
    c[u] = -1;
    a[u] = -1;
    if (i < end) {
      at(u, day_seek(s, jobs, off, nj, total, i));
      c[u] = s.c;
      a[u] = (int)row_lm(s.rows + (i - s.lo) * YRWI_ROW_BYTES);
    }
  }
}

// Age pass: jage[c] += postings of list c with a < min_day (summed in the wave per list: ListTally);
// ctr[RET_MINV] = max(65536 - a), ctr[RET_MAX1] = max(a + 1) (0: no posting; one atomic each per wave);
// HIST: hist[d] += postings with a == d, through the workgroup's LDS window.  Every wave of a workgroup runs
// every step whole (the ballots).
template <bool HIST>
__global__ __launch_bounds__(256) void k_ret_mark(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                  int nj, int64_t total, int min_day,
                                                  unsigned long long* __restrict__ jage,
                                                  unsigned long long* __restrict__ ctr,
                                                  unsigned long long* __restrict__ hist) {
  __shared__ uint32_t s_win[HIST ? RET_WIN : 1];
  __shared__ int s_lo;
  const int lane = threadIdx.x & 63;
  int64_t begin, end;
  span_of(total, &begin, &end);
  if (HIST) {
    for (int i = threadIdx.x; i < RET_WIN; i += blockDim.x) s_win[i] = 0;
    if (threadIdx.x == 0) {
      int lo = 0;
      if (begin < end) {  // the window sits around the day of the span's first posting
        const int c = seg_of(off, 0, nj - 1, begin);
        lo = (int)row_lm(jobs[c].rows + (begin - off[c]) * YRWI_ROW_BYTES) - RET_WIN / 2;
      }
      s_lo = std::min(std::max(lo, 0), RET_DAYS - RET_WIN);
    }
    __syncthreads();
  }
  const int wlo = HIST ? s_lo : 0;
  DayCursor cur;
  ListTally per_list;
  int mn = RET_DAYS, mx = -1;
  unsigned long long bypass = 0;  // the same in every lane of the wave
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    int as[4], cs[4];
    day_tile(cur, jobs, off, nj, total, base, end, as, cs, [](int, bool) {});
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int a = as[u], c = cs[u];
      const bool live = c >= 0;
      const bool hit = live && a < min_day;
      if (live) {
        mn = std::min(mn, a);
        mx = std::max(mx, a);
      }
      per_list.add(hit, c, jage);
      if (HIST) {
        const uint64_t act = __ballot(live);
        // one day owns the wave's postings (lists written in one crawl): one add; else one per lane
        const int lead = act ? __ffsll((unsigned long long)act) - 1 : 0;
        const int la = __shfl(a, lead, 64);
        const bool inwin = live && (unsigned)(a - wlo) < (unsigned)RET_WIN;
        if (__ballot(live && a != la) == 0) {
          const bool lin = (unsigned)(la - wlo) < (unsigned)RET_WIN;
          if (act && lane == lead) {
            if (lin)
              atomicAdd(&s_win[la - wlo], (uint32_t)__popcll(act));
            else
              atomicAdd(&hist[la], (unsigned long long)__popcll(act));
          }
          if (!lin) bypass += (unsigned long long)__popcll(act);
        } else {
          if (inwin) atomicAdd(&s_win[a - wlo], 1u);
          bypass += wave_add_by(live && !inwin, a, hist);  // equal days aggregated within the wave
        }
      }
    }
  }
  per_list.flush(jage);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    mn = std::min(mn, __shfl_xor(mn, d, 64));
    mx = std::max(mx, __shfl_xor(mx, d, 64));
  }
  if (lane == 0 && mx >= 0) {
    atomicMax(&ctr[RET_MINV], (unsigned long long)(RET_DAYS - mn));
    atomicMax(&ctr[RET_MAX1], (unsigned long long)(mx + 1));
  }
  if (HIST) {
    if (bypass && lane == 0) atomicAdd(&ctr[RET_BYPASS], bypass);
    __syncthreads();
    for (int i = threadIdx.x; i < RET_WIN; i += blockDim.x)
      if (s_win[i]) atomicAdd(&hist[wlo + i], (unsigned long long)s_win[i]);
  }
}

// Cut-day search, one level: bins[512 c + 256 (LEVEL - 1) + b] += survivors of capped list c (a >= min_day) whose
// high byte is b (LEVEL 1), or whose high byte is the bucket level one chose (pick[2 c]) and whose low byte is
// b (LEVEL 2).  Flattened over the capped lists' postings.
template <int LEVEL>
__global__ __launch_bounds__(256) void k_ret_bins(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                  int nj, int64_t total, int min_day,
                                                  const int32_t* __restrict__ pick, uint32_t* __restrict__ bins) {
  // a wave sums the bins of the list it is in (acc_c) in its own 256 words of LDS and adds the non-zero ones
  // to the list's bins on leaving it: the days of a list fall into a few dozen high bytes, so a global atomic
  // per (list, bin) per step would hammer those few words from every wave (DESIGN.md §2 has both timings).
  // Only the wave touches its words, so no workgroup barrier is needed; the wave barriers keep the compiler
  // from moving the plain stores and the atomics across each other.
  __shared__ uint32_t s_bins[4][256];
  const int lane = threadIdx.x & 63;
  uint32_t* wb = s_bins[threadIdx.x >> 6];
#pragma unroll
  for (int k = 0; k < 4; k++) wb[lane + 64 * k] = 0;
  __builtin_amdgcn_wave_barrier();
  int acc_c = -1;
  auto flush = [&]() {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t v = atomicExch(&wb[lane + 64 * k], 0u);
      if (v) atomicAdd(&bins[(int64_t)acc_c * 512 + 256 * (LEVEL - 1) + lane + 64 * k], v);
    }
    __builtin_amdgcn_wave_barrier();
  };
  int64_t begin, end;
  span_of(total, &begin, &end);
  DayCursor cur;
  int b1 = 0;
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    int as[4], cs[4], bk[4] = {0, 0, 0, 0};
    day_tile(cur, jobs, off, nj, total, base, end, as, cs, [&](int u, bool entered) {
      if (LEVEL == 2) {  // the list's bucket, looked up where the lane enters a list
        if (entered) b1 = pick[2 * (int64_t)cur.c];
        bk[u] = b1;
      }
    });
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int a = as[u], c = cs[u];
      const bool in = c >= 0 && a >= min_day && (LEVEL == 1 || (a >> 8) == bk[u]);
      const int b = (LEVEL == 1 ? a >> 8 : a) & 255;
      uint64_t left = __ballot(in);
      while (left) {  // the wave's lists ascend: list by list, as ListTally::add, with bins to flush for a count
        const int pl = __ffsll((unsigned long long)left) - 1;
        const int lc = __shfl(c, pl, 64);
        const bool mine = in && c == lc;
        const uint64_t same = __ballot(mine);
        if (lc != acc_c) {
          if (acc_c >= 0) flush();
          acc_c = lc;
        }
        // one bin owns the list's rows of this step: one LDS add; else one per lane
        const int lb = __shfl(b, pl, 64);
        if (__ballot(mine && b != lb) == 0) {
          if (lane == pl) atomicAdd(&wb[lb], (uint32_t)__popcll(same));
        } else if (mine) {
          atomicAdd(&wb[b], 1u);
        }
        left &= ~same;
      }
    }
  }
  if (acc_c >= 0) flush();
}

// The bins of one level -> the bucket that holds the K-th largest survivor, one thread per capped list.
// LEVEL 1: K = max_refs; pick[2 c] = the high byte, pick[2 c + 1] = K - survivors in the buckets above.
// LEVEL 2: K = pick[2 c + 1]; cut[sel[c]] = (d*, q): the cut day and how many of its rows stay.
template <int LEVEL>
__global__ void k_ret_pick(int ncap, const uint32_t* __restrict__ bins, int32_t max_refs, int32_t* __restrict__ pick,
                           const int32_t* __restrict__ sel, int2* __restrict__ cut) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncap) return;
  const uint32_t* b = bins + (int64_t)c * 512 + 256 * (LEVEL - 1);
  const int64_t K = LEVEL == 1 ? max_refs : pick[2 * (int64_t)c + 1];
  int64_t above = 0;
  int at = 0;  // (the host has counted at least max_refs survivors: a bucket is found)
  for (int k = 255; k >= 0; k--) {
    const int64_t n = b[k];
    if (above + n >= K) {
      at = k;
      break;
    }
    above += n;
  }
  if (LEVEL == 1) {
    pick[2 * (int64_t)c] = at;
    pick[2 * (int64_t)c + 1] = (int32_t)(K - above);
  } else {
    cut[sel[c]] = make_int2((pick[2 * (int64_t)c] << 8) | at, (int32_t)(K - above));
  }
}

// The flag kernels of a compaction chunk.  MODE 0 (no cap): keep[i] = a >= min_day.  MODE 1: out[i] = posting
// i survives the age rule and sits on its list's cut day.  MODE 2: keep[i] = a >= min_day && (a > d* ||
// (a == d* && rank < q)), rank = tx[i] - tx[the list's first posting], tx = the exclusive sum of MODE 1's
// marks; a list without a cut (d* < 0) keeps its survivors.  out[total] = 0 (the scan's last element).
template <int MODE>
__global__ __launch_bounds__(256) void k_ret_flag(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                  int nj, int64_t total, int min_day, const int2* __restrict__ cut,
                                                  const int32_t* __restrict__ sel, const int64_t* __restrict__ tx,
                                                  int32_t* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[total] = 0;
  int64_t begin, end;
  span_of(total, &begin, &end);
  DayCursor cur;
  int2 dq = make_int2(-1, 0);
  int64_t tbase = 0;
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
#pragma unroll
    for (int u = 0; u < 4; u++) {  // (not day_tile: a posting's flag is stored before the next one's cell is loaded)
      const int64_t i = base + u * 256 + threadIdx.x;
      if (i >= end) continue;
      const bool entered = day_seek(cur, jobs, off, nj, total, i);
      if (MODE != 0 && entered) {
        dq = cut[sel[cur.c]];
        if (MODE == 2) tbase = tx[cur.lo];
      }
      const int a = (int)row_lm(cur.rows + (i - cur.lo) * YRWI_ROW_BYTES);
      const bool surv = a >= min_day;
      if (MODE == 0)
        out[i] = surv;
      else if (MODE == 1)
        out[i] = surv && a == dq.x;
      else
        out[i] = surv && (dq.x < 0 || a > dq.x || (a == dq.x && tx[i] - tbase < (int64_t)dq.y));
    }
  }
}

// both calls: the selection, the age pass and what the host derives from its per-list counts; apply: the
// cut-day search and the compaction
int retention(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t min_day, int64_t max_refs,
              int64_t* day_hist, bool apply, yrwi_update_stats* st, yrwi_retention_stats* rst) {
  if (!ctx || nterms < 0 || (nterms > 0 && !terms12)) return YRWI_E_ARG;
  if (min_day < 0 || min_day > RET_DAYS) return ctx->fail(YRWI_E_ARG, "min_day outside 0 .. 65536");
  if (max_refs < 0) return ctx->fail(YRWI_E_ARG, "max_refs below 0");
  if (max_refs > 0 && ctx->world > 1)
    return ctx->fail(YRWI_E_UNSUPPORTED, "the cap is of the whole container: not on a context of a shard group");
  const auto t_begin = std::chrono::steady_clock::now();
  yrwi_update_stats S;
  std::memset(&S, 0, sizeof(S));
  yrwi_retention_stats R;
  std::memset(&R, 0, sizeof(R));
  R.day_min = R.day_max = -1;
  Tally T;
  ListSel sel;
  if (int rc = select_lists(ctx, terms12, nterms, false, &sel)) return rc;
  if (st) std::memset(st, 0, sizeof(*st));
  if (day_hist) std::memset(day_hist, 0, sizeof(int64_t) * RET_DAYS);
  RmTable t;
  rm_table(sel, &t);
  auto finish = [&]() {
    R.launches = T.launches;
    R.syncs = T.syncs;
    R.t_total_ns =
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
    if (rst) *rst = R;
    put_stats(st, S, T);
    return 0;
  };
  if (t.jobs.empty() || (min_day == 0 && max_refs == 0 && !day_hist)) return finish();
  const int nj = (int)t.jobs.size();
  const int64_t total = t.total;
  const bool hist = day_hist != nullptr;
  Lane* L = ctx->lanes[0];
  // ---- the age pass: per-list counts, the day range, the bypass count and the histogram in one block, read back once
  const int64_t nres = (int64_t)nj + RET_WORDS + (hist ? RET_DAYS : 0);
  PassDev D;
  if (int rc = pass_begin(ctx, L, t, (size_t)nres * 8, "device allocation (retention age pass)", &D, &T)) return rc;
  hipEvent_t e0 = L->event(), e1 = L->event(), e2 = L->event(), e3 = L->event();
  HIPCHK(ctx, hipEventRecord(e0, L->stream));
  {
    const dim3 g(span_blocks(total)), b(256);
    unsigned long long* ctr = D.res + nj;
    if (hist)
      hipLaunchKernelGGL((k_ret_mark<true>), g, b, 0, L->stream, D.jobs, D.off, nj, total, min_day, D.res, ctr, ctr + RET_WORDS);
    else
      hipLaunchKernelGGL((k_ret_mark<false>), g, b, 0, L->stream, D.jobs, D.off, nj, total, min_day, D.res, ctr, ctr + RET_WORDS);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(e1, L->stream));
  T.launches++;
  const int64_t* h = nullptr;
  if (int rc = pass_end(ctx, L, D, nres, &h, &T)) return rc;
  float msf = 0.f;
  if (hipEventElapsedTime(&msf, e0, e1) == hipSuccess) R.t_mark_ns = (int64_t)((double)msf * 1e6);
  // ---- every list's final length: rem = age + max(0, n - age - max_refs)
  std::vector<int64_t> rem((size_t)nj);
  std::vector<RmJob> capj;
  std::vector<int64_t> capoff;  // (one entry more than lists: the total)
  std::vector<int32_t> capsel;
  int64_t ctotal = 0;
  R.lists = nj;
  R.postings = total;
  R.day_min = h[nj + RET_MINV] ? (int32_t)(RET_DAYS - h[nj + RET_MINV]) : -1;
  R.day_max = (int32_t)h[nj + RET_MAX1] - 1;
  R.hist_bypass = h[nj + RET_BYPASS];
  if (hist) std::memcpy(day_hist, h + nj + RET_WORDS, sizeof(int64_t) * RET_DAYS);
  for (int j = 0; j < nj; j++) {
    const int64_t n = t.jobs[(size_t)j].n, age = h[j];
    const int64_t over = max_refs > 0 ? std::max<int64_t>(0, n - age - max_refs) : 0;
    rem[(size_t)j] = age + over;
    R.removed_age += age;
    R.removed_cap += over;
    R.lists_age += age > 0;
    R.lists_cap += over > 0;
    R.emptied_terms += age == n;
    if (over > 0 && apply) {
      capj.push_back(t.jobs[(size_t)j]);
      capoff.push_back(ctotal);
      capsel.push_back(j);
      ctotal += n;
    }
  }
  capoff.push_back(ctotal);
  if (!apply) return finish();
  // ---- the cut day and the quota of every list over the cap, left on the device
  int2* cut = nullptr;
  if (max_refs > 0) {
    const int ncap = (int)capj.size();
    const int64_t nb = (int64_t)std::max(ncap, 1) * 512;
    RmJob* d_capj = arena_alloc<RmJob>(L, ncap);
    int64_t* d_capoff = arena_alloc<int64_t>(L, ncap + 1);
    int32_t* d_capsel = arena_alloc<int32_t>(L, ncap);
    uint32_t* bins = arena_alloc<uint32_t>(L, nb);
    int32_t* pick = arena_alloc<int32_t>(L, 2 * (int64_t)ncap);
    cut = arena_alloc<int2>(L, nj);
    if (!d_capj || !d_capoff || !d_capsel || !bins || !pick || !cut)
      return ctx->fail(YRWI_E_NOMEM, "device allocation (retention cut-day search)");
    if (int rc = upload(L, d_capj, capj, d_capoff, capoff, d_capsel, capsel)) return ctx->take(L, rc);
    HIPCHK(ctx, hipMemsetAsync(bins, 0, (size_t)nb * 4, L->stream));
    HIPCHK(ctx, hipMemsetAsync(cut, 0xFF, (size_t)nj * sizeof(int2), L->stream));  // d* = -1: no cut
    HIPCHK(ctx, hipEventRecord(e2, L->stream));
    const dim3 g(std::max(span_blocks(ctotal), 1u)), gp(std::max(blocks(ncap), 1u)), b(256);
    const int32_t K = (int32_t)std::min<int64_t>(max_refs, INT32_MAX);  // (a capped list is longer than max_refs)
    hipLaunchKernelGGL((k_ret_bins<1>), g, b, 0, L->stream, d_capj, d_capoff, ncap, ctotal, min_day, pick, bins);
    hipLaunchKernelGGL((k_ret_pick<1>), gp, b, 0, L->stream, ncap, bins, K, pick, d_capsel, cut);
    hipLaunchKernelGGL((k_ret_bins<2>), g, b, 0, L->stream, d_capj, d_capoff, ncap, ctotal, min_day, pick, bins);
    hipLaunchKernelGGL((k_ret_pick<2>), gp, b, 0, L->stream, ncap, bins, K, pick, d_capsel, cut);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(e3, L->stream));
    T.launches += 7;
  }
  // ---- compaction: with a cap a chunk is flagged in two steps (the cut-day marks scanned for the ranks)
  hipError_t ferr = hipSuccess;
  auto flag = [&](const RmJob* dj, const int64_t* doff, int ncj, int64_t n, int32_t* keep, const ChunkAux& x) {
    const dim3 g(span_blocks(n)), b(256);
    if (max_refs == 0) {
      hipLaunchKernelGGL((k_ret_flag<0>), g, b, 0, L->stream, dj, doff, ncj, n, min_day, cut, x.sel, x.kx, keep);
      return;
    }
    hipLaunchKernelGGL((k_ret_flag<1>), g, b, 0, L->stream, dj, doff, ncj, n, min_day, cut, x.sel, x.kx, keep);
    size_t tb = x.tb;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(x.tmp, tb, keep, x.kx, (int)(n + 1), L->stream);
    if (e != hipSuccess) ferr = e;
    hipLaunchKernelGGL((k_ret_flag<2>), g, b, 0, L->stream, dj, doff, ncj, n, min_day, cut, x.sel, x.kx, keep);
    T.launches += 2;
  };
  const int32_t syncs0 = T.syncs;
  if (int rc = compact_commit(ctx, L, t, rem, "device allocation (retention compaction)", flag, &S, &T, true)) return rc;
  if (ferr != hipSuccess) return ctx->fail(YRWI_E_HIP, std::string("retention rank scan: ") + hipGetErrorString(ferr));
  if (max_refs > 0 && T.syncs > syncs0 && hipEventElapsedTime(&msf, e2, e3) == hipSuccess)
    R.t_select_ns = (int64_t)((double)msf * 1e6);
  return finish();
}

}  // namespace

extern "C" int yrwi_retention_count(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t min_day,
                                    int64_t max_refs, int64_t* day_hist, yrwi_retention_stats* st) {
  return retention(ctx, terms12, nterms, min_day, max_refs, day_hist, false, nullptr, st);
}

extern "C" int yrwi_retain(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t min_day, int64_t max_refs,
                           yrwi_update_stats* st, yrwi_retention_stats* rst) {
  return retention(ctx, terms12, nterms, min_day, max_refs, nullptr, true, st, rst);
}

// ---------------------------------------------------------------- references of urls
//
// yrwi_url_references, the read-only form of yrwi_remove_postings (UNVERIFIED against a reference line: the
// reference has no such method).  Two ways to find the references, one way to deliver them.
//
// STREAM (k_ref_stream): the grid, spans, SegCursor and four loads in flight of k_host_mark over khi / klo of
// the selected lists in term order, 9 B per posting and no row read; the lookup is the slot of the 72-bit key
// in the sorted url set, staged in LDS (8 B + 1 B per url) up to REF_LDS_MAX urls and searched in global
// memory above.  Per-list hits are summed in the wave and added on leaving the list (ListTally); per-url
// hits take one atomic per distinct slot of a wave's step.
// PROBE (k_ref_probe): one thread per (list, slot) pair, list-major, searches the list for the url (lb_key).
//
// Both number their domain the way YRWI_REFS_BY_TERM orders the references (term, then url), so a hit's
// place is the hits before it: the count pass adds every wave's hits to its tile's count (1024 postings,
// 256 pairs), k_ref_scan turns the counts into 64-bit starts, and the pack pass (the same kernels, MODE
// REF_PACK) finds the hits of the tiles that have any again and writes each at its tile's start plus its rank
// in the tile.  The pack pass reads the total from device memory and returns when it exceeds the capacity.
// YRWI_REFS_BY_URL: the pack pass writes (slot, list << 32 | row) per reference instead (REF_KEYS), one
// stable radix sort by slot orders them, k_ref_place moves the rows.
namespace {

constexpr int REF_LDS_MAX = YRWI_REF_LDS_MAX;  // urls searched in LDS (9 B each)
constexpr int REF_PAIR_TILE = 256;             // (list, url) pairs per tile of PROBE: one per thread
// dispatch: one search step of PROBE is weighed as this many streamed keys of STREAM.  From the crossover of the
// two forced paths on C2: PROBE still wins at 4096 urls, where the estimate tips at 0.174,
// STREAM at 65,536, where it tips at 0.011 (a wave's searches of one list share their loads; a streamed key
// costs a search of the set as well)
constexpr double REF_PROBE_STEP_KEYS = 0.05;

enum { REF_COUNT = 0, REF_TILES = 1, REF_PACK = 2, REF_KEYS = 3 };  // what a finding kernel does with a hit

struct RefOut {  // where the pack pass writes (REF_PACK: rows, terms; REF_KEYS: skey, sval)
  const int64_t* tile_start;  // references before every tile; [tiles] = all of them
  int64_t tiles, cap;
  const uint32_t* lterm;  // the term hash of every selected list, three words each
  uint8_t* rows;
  uint32_t* terms;
  uint32_t* skey;
  uint64_t* sval;
};

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {
  return (uint32_t)__popcll(ballot & (((uint64_t)1 << (threadIdx.x & 63)) - 1));
}

// reference r = row k of list c, url slot `slot`
template <int MODE>
__device__ __forceinline__ void ref_emit(const RefOut& O, const RmJob* __restrict__ jobs, int64_t r, int c, int64_t k,
                                         int slot) {
  if (MODE == REF_PACK) {
    copy_row(O.rows + r * YRWI_ROW_BYTES, jobs[c].rows + k * YRWI_ROW_BYTES);
#pragma unroll
    for (int w = 0; w < 3; w++) O.terms[r * 3 + w] = O.lterm[(int64_t)c * 3 + w];
  } else {
    O.skey[r] = (uint32_t)slot;
    O.sval[r] = ((uint64_t)(uint32_t)c << 32) | (uint64_t)k;
  }
}

// a key tile -> its postings' slots in the url set (-1: not of the set, or past end), lists and rows
__device__ __forceinline__ void ref_tile(SegCursor& s, const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                         int nj, int64_t total, const uint64_t* kh, const uint8_t* kl, int nu,
                                         int64_t base, int64_t end, int slot[4], int c[4], int64_t k[4]) {
  uint64_t h[4];
  uint32_t l[4];
  key_tile(s, jobs, off, nj, total, base, end, c, k, h, l);
#pragma unroll
  for (int u = 0; u < 4; u++) slot[u] = c[u] >= 0 ? set_slot(kh, kl, nu, h[u], l[u]) : -1;
}

// STREAM.  REF_COUNT / REF_TILES: jcnt[c] += references in list c, ucnt[slot] += references of url slot,
// REF_TILES: tile_cnt[t] += references in tile t (the three zeroed by the caller).  REF_PACK / REF_KEYS: the
// references of every tile that has any go where O says.  Every wave of a workgroup runs every step whole.
template <bool LDS, int MODE>
__global__ __launch_bounds__(256) void k_ref_stream(const RmJob* __restrict__ jobs, const int64_t* __restrict__ off,
                                                    int nj, int64_t total, const uint64_t* __restrict__ ukh,
                                                    const uint8_t* __restrict__ ukl, int nu,
                                                    unsigned long long* __restrict__ jcnt,
                                                    unsigned long long* __restrict__ ucnt,
                                                    int32_t* __restrict__ tile_cnt, RefOut O) {
  __shared__ uint64_t s_kh[LDS ? REF_LDS_MAX : 1];
  __shared__ uint8_t s_kl[LDS ? REF_LDS_MAX : 1];
  __shared__ uint32_t s_w[16];
  if (MODE >= REF_PACK && O.tile_start[O.tiles] > O.cap) return;  // (the same in every thread of the grid)
  stage_set<LDS, true>(s_kh, ukh, nu, s_kl, ukl);
  const uint64_t* kh = LDS ? s_kh : ukh;
  const uint8_t* kl = LDS ? s_kl : ukl;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t begin, end;
  span_of(total, &begin, &end);
  SegCursor cur;
  ListTally per_list;
  for (int64_t base = begin; base < end; base += SPAN_TILE) {
    const int64_t t = base / SPAN_TILE;
    int64_t tstart = 0;
    if (MODE >= REF_PACK) {
      tstart = O.tile_start[t];
      if (O.tile_start[t + 1] == tstart) continue;  // (the same in every thread of the workgroup)
    }
    int slots[4], cs[4];
    int64_t ks[4];
    ref_tile(cur, jobs, off, nj, total, kh, kl, nu, base, end, slots, cs, ks);
    if (MODE <= REF_TILES) {
      uint32_t tile_n = 0;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool hit = slots[u] >= 0;
        tile_n += (uint32_t)__popcll(__ballot(hit));
        per_list.add(hit, cs[u], jcnt);
        wave_add_by(hit, slots[u], ucnt);
      }
      if (MODE == REF_TILES && tile_n && lane == 0) atomicAdd(&tile_cnt[t], (int32_t)tile_n);
    } else {
      // a hit's rank in the tile: the hits of the steps before, of the waves before in its step, of the lanes before
      uint64_t bal[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        bal[u] = __ballot(slots[u] >= 0);
        if (lane == 0) s_w[u * 4 + wave] = (uint32_t)__popcll(bal[u]);
      }
      __syncthreads();
      uint32_t run = 0;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        uint32_t mine = run;
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const uint32_t v = s_w[u * 4 + w];
          if (w < wave) mine += v;
          run += v;
        }
        if (slots[u] >= 0) ref_emit<MODE>(O, jobs, tstart + mine + lanes_below(bal[u]), cs[u], ks[u], slots[u]);
      }
      __syncthreads();  // (s_w is written again in the next tile that has hits)
    }
  }
  if (MODE <= REF_TILES) per_list.flush(jcnt);
}

// PROBE: pair p = list p / nu, slot p % nu; tile t = pairs [256 t, 256 t + 256).  Modes as k_ref_stream.
template <int MODE>
__global__ __launch_bounds__(REF_PAIR_TILE) void k_ref_probe(const RmJob* __restrict__ jobs,
                                                             const uint64_t* __restrict__ ukh,
                                                             const uint8_t* __restrict__ ukl, int nu, int64_t pairs,
                                                             unsigned long long* __restrict__ jcnt,
                                                             unsigned long long* __restrict__ ucnt,
                                                             int32_t* __restrict__ tile_cnt, RefOut O) {
  __shared__ uint32_t s_w[4];
  const int64_t t = blockIdx.x;
  int64_t tstart = 0;
  if (MODE >= REF_PACK) {
    if (O.tile_start[O.tiles] > O.cap) return;
    tstart = O.tile_start[t];
    if (O.tile_start[t + 1] == tstart) return;  // (the same in every thread of the workgroup)
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = t * REF_PAIR_TILE + threadIdx.x;
  bool hit = false;
  int c = 0, slot = 0;
  int64_t k = 0;
  if (p < pairs) {
    c = (int)(p / nu);
    slot = (int)(p - (int64_t)c * nu);
    const uint64_t* lkh = jobs[c].khi;
    const uint8_t* lkl = jobs[c].klo;
    const int64_t n = jobs[c].n;
    const uint64_t h = ukh[slot];
    const uint32_t l = ukl[slot];
    k = lb_key(lkh, lkl, 0, n, h, l);
    hit = k < n && lkh[k] == h && (uint32_t)lkl[k] == l;
  }
  const uint64_t bal = __ballot(hit);
  if (MODE <= REF_TILES) {
    wave_add_by(hit, c, jcnt);
    wave_add_by(hit, slot, ucnt);
    if (MODE == REF_TILES && bal && lane == 0) atomicAdd(&tile_cnt[t], (int32_t)__popcll(bal));
  } else {
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t mine = 0;
    for (int w = 0; w < wave; w++) mine += s_w[w];
    if (hit) ref_emit<MODE>(O, jobs, tstart + mine + lanes_below(bal), c, k, slot);
  }
}

// One workgroup walks the tile counts, 1024 at a time (four neighbours per thread) with a running 64-bit
// carry: tile_start[t] = references before tile t, tile_start[tiles] = *total = all of them.
__global__ __launch_bounds__(256) void k_ref_scan(const int32_t* __restrict__ tile_cnt, int64_t tiles,
                                                  int64_t* __restrict__ tile_start,
                                                  unsigned long long* __restrict__ total) {
  __shared__ uint64_t s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (int64_t b = 0; b < tiles; b += 1024) {
    const int64_t x = b + 4 * (int64_t)threadIdx.x;
    uint32_t v[4];
    uint64_t sum = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      v[u] = x + u < tiles ? (uint32_t)tile_cnt[x + u] : 0u;
      sum += v[u];
    }
    uint64_t inc = sum;  // inclusive sums over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t o = shfl64(inc, lane >= d ? lane - d : lane);
      if (lane >= d) inc += o;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint64_t before = carry + inc - sum, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      if (w < wave) before += s_w[w];
      all += s_w[w];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (x + u < tiles) tile_start[x + u] = (int64_t)before;
      before += v[u];
    }
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tile_start[tiles] = (int64_t)carry;
    *total = carry;
  }
}

// YRWI_REFS_BY_URL, after the sort: reference r is row (sval[r] & 2^32 - 1) of list sval[r] >> 32
__global__ __launch_bounds__(256) void k_ref_place(const RmJob* __restrict__ jobs, const uint32_t* __restrict__ lterm,
                                                   const uint64_t* __restrict__ sval, int64_t n,
                                                   uint8_t* __restrict__ rows, uint32_t* __restrict__ terms) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint64_t v = sval[r];
  const int64_t c = (int64_t)(v >> 32), k = (int64_t)(v & 0xFFFFFFFFull);
  copy_row(rows + r * YRWI_ROW_BYTES, jobs[c].rows + k * YRWI_ROW_BYTES);
#pragma unroll
  for (int w = 0; w < 3; w++) terms[r * 3 + w] = lterm[c * 3 + w];
}

struct RefPass {  // the device side of one call, as its finding kernels take it
  const RmJob* jobs;
  const int64_t* off;
  int nj, nu;
  int64_t total, pairs, tiles;
  const uint64_t* ukh;
  const uint8_t* ukl;
  unsigned long long *jcnt, *ucnt;
  int32_t* tile_cnt;
  bool probe;
};

template <int MODE>
void ref_find(const RefPass& P, const RefOut& O, hipStream_t s) {
  if (P.probe) {
    hipLaunchKernelGGL((k_ref_probe<MODE>), dim3((unsigned)P.tiles), dim3(REF_PAIR_TILE), 0, s, P.jobs, P.ukh, P.ukl,
                       P.nu, P.pairs, P.jcnt, P.ucnt, P.tile_cnt, O);
  } else if (P.nu <= REF_LDS_MAX) {
    hipLaunchKernelGGL((k_ref_stream<true, MODE>), dim3(span_blocks(P.total)), dim3(256), 0, s, P.jobs, P.off, P.nj,
                       P.total, P.ukh, P.ukl, P.nu, P.jcnt, P.ucnt, P.tile_cnt, O);
  } else {
    hipLaunchKernelGGL((k_ref_stream<false, MODE>), dim3(span_blocks(P.total)), dim3(256), 0, s, P.jobs, P.off, P.nj,
                       P.total, P.ukh, P.ukl, P.nu, P.jcnt, P.ucnt, P.tile_cnt, O);
  }
}

}  // namespace

extern "C" int yrwi_url_references(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* urls12,
                                   int64_t nurls, int32_t order, int64_t* counts, uint8_t* terms12_out,
                                   uint8_t* rows40_out, int64_t cap_refs, yrwi_ref_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  if (!ctx || nterms < 0 || nurls < 0 || (nterms > 0 && !terms12) || (nurls > 0 && !urls12)) return YRWI_E_ARG;
  if (order != YRWI_REFS_BY_TERM && order != YRWI_REFS_BY_URL) return ctx->fail(YRWI_E_ARG, "unknown reference order");
  if (cap_refs < 0 || (cap_refs > 0 && (!terms12_out || !rows40_out)))
    return ctx->fail(YRWI_E_ARG, "reference capacity without buffers");
  if (nurls > (int64_t)INT32_MAX) return ctx->fail(YRWI_E_LIMIT, "2^31 urls or more in one call");
  const auto t_begin = std::chrono::steady_clock::now();
  yrwi_ref_stats S;
  std::memset(&S, 0, sizeof(S));
  Tally T;
  // ---- the urls as given (for counts) and as a set, sorted and each once; the selected lists in term order
  UrlSet U;
  if (int rc = url_set(ctx, urls12, nurls, &U)) return rc;
  const std::vector<KeyT>&in = U.in, &uk = U.uk;
  ListSel sel;
  if (int rc = select_lists(ctx, terms12, nterms, true, &sel)) return rc;
  RmTable t;
  rm_table(sel, &t);
  const int nj = (int)t.jobs.size(), nu = (int)uk.size();
  const int64_t total = t.total;
  if (counts) std::fill(counts, counts + nurls, (int64_t)0);
  S.lists = nj;
  S.postings = total;
  S.urls = nu;
  Lane* L = ctx->lanes[0];
  const int64_t up0 = L->up_bytes, down0 = L->down_bytes;
  auto finish = [&](int rc) {
    S.launches = T.launches;
    S.syncs = T.syncs;
    S.bytes_h2d = L->up_bytes - up0;
    S.bytes_d2h = L->down_bytes - down0;
    S.t_total_ns =
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
    if (st) *st = S;
    return rc;
  };
  if (nu == 0 || nj == 0) return finish(0);
  // ---- the path: PROBE's search steps against STREAM's keys, unless the environment names one
  const int64_t pairs = (int64_t)nj * nu;
  int steps = 1;  // of one search: ceil(log2(mean list length + 1))
  while (steps < 63 && ((int64_t)1 << steps) < total / nj + 1) steps++;
  bool probe = (double)pairs * steps * REF_PROBE_STEP_KEYS <= (double)total;
  const char* forced = getenv("YRWI_REFS_PATH");
  if (forced && !strcmp(forced, "stream")) probe = false;
  if (forced && !strcmp(forced, "probe")) probe = true;
  const int64_t tiles = probe ? ceil_div(pairs, REF_PAIR_TILE) : ceil_div(total, SPAN_TILE);
  if (probe && tiles > (int64_t)INT32_MAX) return ctx->fail(YRWI_E_LIMIT, "2^39 (list, url) pairs or more on the probe path");
  S.path = probe ? YRWI_REFS_PROBE : YRWI_REFS_STREAM;
  const bool fetch = cap_refs > 0, by_url = order == YRWI_REFS_BY_URL;
  // no more references than postings or pairs: a larger cap_refs promises nothing the call could use
  const int64_t room = std::min(cap_refs, std::min(total, pairs));
  const bool direct = fetch && (reinterpret_cast<uintptr_t>(rows40_out) & 7) == 0 &&
                      ctx->hostreg.contains(rows40_out, (size_t)room * YRWI_ROW_BYTES);
  std::vector<uint32_t> lterm((size_t)nj * 3);  // the lists' term hashes, as the pack pass stores them
  for (int j = 0; j < nj; j++) key_chars(t.jkey[(size_t)j], reinterpret_cast<uint8_t*>(&lterm[(size_t)j * 3]));
  // ---- device tables; the counters (per list, per url, the total) and the tile counts are one block, zeroed at
  //      once; find: one upload, one memset, the count pass; fetch: the scan and, by term, the pack pass behind it
  const int64_t nres = (int64_t)nj + nu + 1;
  const size_t zero_bytes = (size_t)nres * 8 + (fetch ? (size_t)tiles * 4 : 0);
  const char* nomem = "device allocation (url references)";
  PassDev D;
  uint64_t* ukh = nullptr;
  uint8_t* ukl = nullptr;
  uint32_t* d_lterm = nullptr;
  if (int rc = pass_begin(ctx, L, t, zero_bytes, nomem, &D, &T, &ukh, U.kh, &ukl, U.kl, &d_lterm, lterm)) return rc;
  RmJob* d_jobs = D.jobs;
  unsigned long long* res = D.res;
  int64_t* tile_start = fetch ? arena_alloc<int64_t>(L, tiles + 1) : nullptr;
  if (fetch && !tile_start) return ctx->fail(YRWI_E_NOMEM, nomem);
  RefPass P{d_jobs, D.off, nj, nu, total, pairs, tiles, ukh, ukl, res, res + nj,
            reinterpret_cast<int32_t*>(res + nres), probe};
  RefOut O{tile_start, tiles, cap_refs, d_lterm, nullptr, nullptr, nullptr, nullptr};
  uint8_t* d_rows = nullptr;  // where the rows are written: the caller's pinned buffer or scratch
  auto out_buffers = [&](int64_t n) {
    if (direct) {
      if (hipHostGetDevicePointer(reinterpret_cast<void**>(&d_rows), rows40_out, 0) != hipSuccess) return false;
    } else {
      d_rows = arena_alloc<uint8_t>(L, n * YRWI_ROW_BYTES);
    }
    O.rows = d_rows;
    O.terms = arena_alloc<uint32_t>(L, n * 3);
    return d_rows && O.terms;
  };
  if (fetch && !by_url && !out_buffers(room)) return ctx->fail(YRWI_E_NOMEM, nomem);
  hipEvent_t e0 = L->event(), e1 = L->event();
  HIPCHK(ctx, hipEventRecord(e0, L->stream));
  if (fetch) ref_find<REF_TILES>(P, O, L->stream); else ref_find<REF_COUNT>(P, O, L->stream);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(e1, L->stream));
  T.launches++;
  if (fetch) {
    hipLaunchKernelGGL(k_ref_scan, dim3(1), dim3(256), 0, L->stream, P.tile_cnt, tiles, tile_start, res + nres - 1);
    T.launches++;
    if (!by_url) {
      ref_find<REF_PACK>(P, O, L->stream);
      T.launches++;
    }
    HIPCHK(ctx, hipGetLastError());
  }
  const int64_t* h = nullptr;
  if (int rc = pass_end(ctx, L, D, nres, &h, &T)) return rc;
  float msf = 0.f;
  if (hipEventElapsedTime(&msf, e0, e1) == hipSuccess) S.t_find_ns = (int64_t)((double)msf * 1e6);
  (void)hipGetLastError();  // a statistics event that could not be read is not the call's error
  // ---- the counts (the pinned landing buffer is reused below)
  for (int j = 0; j < nj; j++) {
    S.refs += h[j];
    S.lists_hit += h[j] > 0;
    S.lists_covered += h[j] == t.jobs[(size_t)j].n;
  }
  for (int i = 0; i < nu; i++) S.urls_found += h[nj + i] > 0;
  if (counts)
    for (int64_t i = 0; i < nurls; i++)
      counts[i] = h[nj + (std::lower_bound(uk.begin(), uk.end(), in[(size_t)i]) - uk.begin())];
  if (!fetch) return finish(0);
  const int64_t refs = S.refs;
  if (refs > cap_refs) {  // the pack pass saw the same total and stored nothing
    finish(0);
    return ctx->fail(YRWI_E_ARG, "reference capacity too small: st->refs references are needed");
  }
  const int64_t nout = std::max<int64_t>(refs, 1);  // (nothing found: the tail runs over one unused element)
  if (by_url) {
    // ---- the references alone, sorted stably by url slot, then placed
    if (refs > (int64_t)INT32_MAX) return ctx->fail(YRWI_E_LIMIT, "2^31 references or more by url");
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < nu) bits++;
    uint32_t* skey = arena_alloc<uint32_t>(L, nout);
    uint32_t* okey = arena_alloc<uint32_t>(L, nout);
    uint64_t* sval = arena_alloc<uint64_t>(L, nout);
    uint64_t* oval = arena_alloc<uint64_t>(L, nout);
    size_t tb = 0;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, skey, okey, sval, oval, (int)nout, 0, bits, L->stream));
    void* tmp = L->arena.alloc(tb);
    if (!skey || !okey || !sval || !oval || !tmp || !out_buffers(nout))
      return ctx->fail(YRWI_E_NOMEM, "device allocation (url references by url)");
    O.skey = skey;
    O.sval = sval;
    ref_find<REF_KEYS>(P, O, L->stream);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(tmp, tb, skey, okey, sval, oval, (int)nout, 0, bits, L->stream));
    hipLaunchKernelGGL(k_ref_place, dim3(blocks(nout)), dim3(256), 0, L->stream, d_jobs, d_lterm, oval, refs, d_rows,
                       O.terms);
    HIPCHK(ctx, hipGetLastError());
    T.launches += 3;
  }
  // ---- the terms, and the rows that were not written in place, leave through the pinned landing buffers
  const uint8_t* ht = readback(L, &L->down_stage, O.terms, nout, 12, 12);
  const uint8_t* hr = direct ? nullptr : readback(L, &L->out_stage, d_rows, nout, YRWI_ROW_BYTES, YRWI_ROW_BYTES);
  if (!ht || (!direct && !hr)) return ctx->take(L, YRWI_E_HIP);
  T.launches += direct ? 1 : 2;
  if (direct) L->down_bytes += refs * YRWI_ROW_BYTES;
  HIPCHK(ctx, lane_sync(L));
  T.syncs++;
  std::memcpy(terms12_out, ht, (size_t)refs * 12);
  if (!direct) std::memcpy(rows40_out, hr, (size_t)refs * YRWI_ROW_BYTES);
  S.direct = direct ? 1 : 0;
  return finish(0);
}
