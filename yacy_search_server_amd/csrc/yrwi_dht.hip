// yrwi_dht.hip -- the DHT send path: Dispatcher.selectContainersEnqueueToBuffer, i.e.
// selectContainers (whole containers in term order from a start hash, up to a container and a
// reference count), IndexCell.remove(termHash) of what was selected, and splitContainers /
// splitContainer by Distribution.verticalDHTPosition(urlhash) into 2^e partitions.
//
// The selection is host work over the term keys.  Every list is sorted by url hash and the
// partition of a posting is the top e bits of its url key, so a list's partitions are contiguous
// row ranges: the split is a boundary search per (list, partition) -- k_dht_bounds, one launch --
// and one device scan over the P * T cell counts in partition-major order.  One job table (row
// pointer, khi, n per selected list) goes up in one copy; the P * T + 1 offsets come back in one.
// k_dht_pack then writes the output, which is the cells' rows one after another, in windows of
// YRWI_DHT_WINDOW_ROWS rows into a device window; a copy lands the window in the caller's buffer
// (pinned and 8-byte aligned) or in a pinned window the host copies from, while the next window
// is packed (run_windows, yrwi_host.h).  Launches and host waits follow the number of windows,
// never the number of terms.
//
// k_dht_pack: a workgroup takes a 16 KiB slice of the window, finds the cells holding the slice's
// first and last row by binary search of the offsets (the last cell with off <= row: runs of
// empty cells are stepped over) and its threads search on between those two.  Every thread
// produces aligned 16-byte pieces and stores each with one 16-byte vector store.  Source and
// destination are both multiples of 40 from 256-byte aligned bases, so a source address is a
// multiple of 8: a piece inside one cell is one 16-byte load or two 8-byte halves; a piece whose
// second half is the first 8 bytes of the next cell's first row is put together from two 8-byte
// loads.  Nothing outside the rows of the selected lists is read.
//
// A sharded context selects from the lists it holds, i.e. its url range of every term; no
// collective is involved, and the cells of partitions outside its range come out empty.

#include <hipcub/hipcub.hpp>

#include "yrwi_device.h"
#include "yrwi_host.h"

using namespace yrwi;

namespace {

constexpr int ROW = YRWI_ROW_BYTES;
constexpr int PIECE = 16;
constexpr int PACK_THREADS = 256;
constexpr int PACK_ITERS = 4;
constexpr int64_t SLICE = (int64_t)PACK_THREADS * PIECE * PACK_ITERS;  // bytes per workgroup
constexpr int64_t DEFAULT_WINDOW_ROWS = (int64_t)1 << 20;
constexpr int64_t MIN_WINDOW_ROWS = 16, MAX_WINDOW_ROWS = (int64_t)1 << 24;
constexpr int32_t ALL_FLAGS = YRWI_DHT_ROT | YRWI_DHT_REMOVE | YRWI_DHT_SKIP_PRIVATE | YRWI_DHT_COUNT_ONLY;

struct DhtJob {  // one selected list
  const uint8_t* rows;
  const uint64_t* khi;
  int64_t n;
  int64_t pad;
};

// Cell (p, j), index p * T + j: srow = the first row of list j whose key's top e bits are >= p
// (the lower bound of p << (64 - e) in khi), cnt = its rows in partition p.  cnt has ncell + 1
// entries for the scan; the last is 0.
__global__ __launch_bounds__(256) void k_dht_bounds(const DhtJob* __restrict__ jobs, int64_t T, int32_t e,
                                                    int64_t ncell, int32_t* __restrict__ srow,
                                                    int64_t* __restrict__ cnt) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncell) return;
  if (c == ncell) {
    cnt[c] = 0;
    return;
  }
  const int64_t p = c / T, j = c - p * T;
  const gmem_u64* khi = (const gmem_u64*)(uintptr_t)jobs[j].khi;  // global, not flat, loads
  const int64_t n = jobs[j].n;
  const int64_t P = (int64_t)1 << e;
  int64_t b[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int64_t q = p + s;
    if (q == 0) {
      b[s] = 0;
    } else if (q == P) {
      b[s] = n;
    } else {  // 0 < q < P, so e >= 1
      const uint64_t key = (uint64_t)q << (64 - e);
      int64_t lo = 0, hi = n;  // first row with khi >= key
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (khi[mid] < key) lo = mid + 1; else hi = mid;
      }
      b[s] = lo;
    }
  }
  srow[c] = (int32_t)b[0];
  cnt[c] = b[1] - b[0];
}

// the address of row g's byte 8 k, g a row of the non-empty cell c
__device__ __forceinline__ const uint8_t* src_of(const DhtJob* __restrict__ jobs, const int32_t* __restrict__ srow,
                                                 const int64_t* __restrict__ off, int64_t T, int64_t c, int64_t g,
                                                 int k) {
  return jobs[c % T].rows + ((int64_t)srow[c] + (g - off[c])) * ROW + 8 * k;
}

// The cell of a row is the last one whose offset is <= the row (seg_of): the next offset is above
// it then, so the cell is not empty.
// Rows [w0, w0 + wrows) of the output -> dst (16-B aligned, room for 40 wrows rounded up to 16).
// off: ncell + 1 row offsets, off[ncell] = the total; w0 + wrows <= total.
__global__ __launch_bounds__(PACK_THREADS) void k_dht_pack(const int64_t* __restrict__ off,
                                                           const int32_t* __restrict__ srow,
                                                           const DhtJob* __restrict__ jobs, int64_t ncell, int64_t T,
                                                           int64_t w0, int64_t wrows, uint8_t* __restrict__ dst) {
  __shared__ int64_t s_c[2];
  const int64_t wbytes = wrows * ROW;
  const int64_t s0 = (int64_t)blockIdx.x * SLICE;  // slice start in the window (< wbytes by the grid)
  if (threadIdx.x == 0) {
    const int64_t last = (s0 + SLICE < wbytes ? s0 + SLICE : wbytes) - 1;
    s_c[0] = seg_of(off, (int64_t)0, ncell - 1, w0 + s0 / ROW);
    s_c[1] = seg_of(off, s_c[0], ncell - 1, w0 + last / ROW);
  }
  __syncthreads();
  int64_t c = s_c[0];
  const int64_t chi = s_c[1];
#pragma unroll 1
  for (int it = 0; it < PACK_ITERS; it++) {
    const int64_t ci = s0 + ((int64_t)it * PACK_THREADS + threadIdx.x) * PIECE;
    if (ci >= wbytes) break;
    const int64_t u = ci >> 3;  // 8-byte unit of the window; 5 to a row
    const int64_t r = u / 5;
    const int k = (int)(u - 5 * r);
    const int64_t g = w0 + r;                 // the row of the piece's first half (< w0 + wrows)
    const int64_t g1 = k == 4 ? g + 1 : g;    // and of its second half
    c = seg_of(off, c, chi, g);
    const uint8_t* s = src_of(jobs, srow, off, T, c, g, k);
    u32x4 o;
    if (g1 < off[c + 1]) {
      // both halves in cell c: 16 contiguous source bytes
      if (((uintptr_t)s & 15) == 0) {
        o = *(const gmem_u4*)(uintptr_t)s;
      } else {
        const u32x2 a = *(const gmem_u2*)(uintptr_t)s, b = *(const gmem_u2*)(uintptr_t)(s + 8);
        o = u32x4{a.x, a.y, b.x, b.y};
      }
    } else {
      // the second half is the start of the next cell's first row, or past the window's rows
      const u32x2 a = *(const gmem_u2*)(uintptr_t)s;
      u32x2 b = u32x2{0u, 0u};
      if (g1 < w0 + wrows) {  // a row of this slice: its cell is at most chi
        const int64_t c1 = seg_of(off, c + 1, chi, g1);
        b = *(const gmem_u2*)(uintptr_t)src_of(jobs, srow, off, T, c1, g1, 0);
      }
      o = u32x4{a.x, a.y, b.x, b.y};
    }
    *reinterpret_cast<u32x4*>(dst + ci) = o;
  }
}

// Word.isPrivate(termHash): the hash starts with YRWI_DHT_PRIVATE0, YRWI_DHT_PRIVATE1
bool is_private(const KeyT& k) {
  const uint64_t top12 = ((uint64_t)AHP[(uint8_t)YRWI_DHT_PRIVATE0] << 6) | (uint64_t)AHP[(uint8_t)YRWI_DHT_PRIVATE1];
  return (k.hi >> 52) == top12;
}

int64_t window_rows() {
  int64_t w = DEFAULT_WINDOW_ROWS;
  const char* e = getenv("YRWI_DHT_WINDOW_ROWS");  // read per call: tests force window boundaries with it
  if (e && *e) w = atoll(e);
  return std::max(MIN_WINDOW_ROWS, std::min(w, MAX_WINDOW_ROWS));
}

}  // namespace

extern "C" int yrwi_dht_select(yrwi_ctx* ctx, const uint8_t start[12], const uint8_t limit[12],
                               int32_t max_containers, int64_t max_refs, int32_t partition_exponent, int32_t flags,
                               uint8_t* terms12_out, int32_t cap_terms, int64_t* part_off, uint8_t* rows40_out,
                               int64_t cap_rows, yrwi_dht_stats* st) {
  if (!ctx) return YRWI_E_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  const int32_t e = partition_exponent;
  const bool count_only = (flags & YRWI_DHT_COUNT_ONLY) != 0;
  if (!start || !limit) return ctx->fail(YRWI_E_ARG, "start and limit hashes are required");
  if (e < 0 || e > YRWI_DHT_MAX_EXPONENT) return ctx->fail(YRWI_E_ARG, "partition exponent outside 0 .. 8");
  if (flags & ~ALL_FLAGS) return ctx->fail(YRWI_E_ARG, "unknown YRWI_DHT_* flag");
  if (!count_only && (cap_terms < 0 || cap_rows < 0 || !part_off || (cap_terms > 0 && !terms12_out) ||
                      (cap_rows > 0 && !rows40_out)))
    return ctx->fail(YRWI_E_ARG, "output buffers");
  KeyT ks, kl;
  if (!key_of(start, &ks) || !key_of(limit, &kl))
    return ctx->fail(YRWI_E_HASH, "start or limit hash is not well-formed Base64");
  yrwi_dht_stats S;
  std::memset(&S, 0, sizeof(S));
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- selectContainers: the non-empty lists in key order from the first term >= start
  ListSel all;
  if (int rc = select_lists(ctx, nullptr, 0, true, &all)) return rc;
  const size_t N = all.size();
  std::vector<size_t> sel;
  {
    size_t pos = (size_t)(std::lower_bound(all.begin(), all.end(), ks,
                                           [](const auto& a, const KeyT& k) { return a.first < k; }) -
                          all.begin());
    int64_t refs = 0;
    for (size_t seen = 0; seen < N; seen++, pos++) {  // at most one full cycle
      if (!((int64_t)sel.size() < (int64_t)max_containers && refs < max_refs)) break;
      if (pos == N) {
        if (!(flags & YRWI_DHT_ROT)) break;
        pos = 0;
        S.wrapped = 1;
      }
      const KeyT& k = all[pos].first;
      if ((flags & YRWI_DHT_SKIP_PRIVATE) && is_private(k)) {
        S.skipped_private++;
        continue;
      }
      if (!sel.empty() && !(k < kl)) break;
      sel.push_back(pos);
      refs += all[pos].second->n;
    }
    S.terms = (int64_t)sel.size();
    S.postings = refs;
  }
  const int64_t T = S.terms, total = S.postings, P = (int64_t)1 << e, ncell = P * T;
  auto finish = [&](int rc) {
    S.t_total_ns =
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
    if (st) *st = S;
    return rc;
  };
  if (count_only) return finish(0);
  if (cap_terms < T || cap_rows < total) {
    ctx->fail(YRWI_E_ARG, "cap_terms or cap_rows smaller than the selection (sizes in yrwi_dht_stats)");
    return finish(YRWI_E_ARG);
  }
  if (T == 0) {
    part_off[0] = 0;
    return finish(0);
  }
  if (ncell + 1 > (int64_t)INT32_MAX) return ctx->fail(YRWI_E_LIMIT, "2^e * terms does not fit the device scan");
  // ---- job table, boundary search, scan; the offsets come back in one copy
  std::vector<DhtJob> jobs((size_t)T);
  for (int64_t j = 0; j < T; j++) {
    const ListRec* R = all[sel[(size_t)j]].second;
    jobs[(size_t)j] = DhtJob{R->rows, R->khi, R->n, 0};
  }
  Lane* L = ctx->lanes[0];
  if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
  S.syncs++;
  const int64_t W = window_rows();
  const int64_t nwin = (total + W - 1) / W;
  const size_t wneed = ((size_t)W * ROW + 255) & ~(size_t)255;
  DhtJob* d_jobs = arena_alloc<DhtJob>(L, T);
  int32_t* d_srow = arena_alloc<int32_t>(L, ncell);
  int64_t* d_cnt = arena_alloc<int64_t>(L, ncell + 1);
  int64_t* d_off = arena_alloc<int64_t>(L, ncell + 1);
  size_t tb = 0;
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_cnt, d_off, (int)(ncell + 1), L->stream));
  void* tmp = L->arena.alloc(tb);
  if (!d_jobs || !d_srow || !d_cnt || !d_off || !tmp) return ctx->fail(YRWI_E_NOMEM, "device allocation (dht job table)");
  if (int rc = upload(L, d_jobs, jobs)) return ctx->take(L, rc);
  hipLaunchKernelGGL(k_dht_bounds, dim3((unsigned)((ncell + 1 + 255) / 256)), dim3(256), 0, L->stream, d_jobs, T, e,
                     ncell, d_srow, d_cnt);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tb, d_cnt, d_off, (int)(ncell + 1), L->stream));
  const int64_t* h_off = reinterpret_cast<const int64_t*>(readback(L, &L->down_stage, d_off, ncell + 1, 8, 8));
  if (!h_off) return ctx->take(L, YRWI_E_HIP);
  S.launches += 4;
  HIPCHK(ctx, lane_sync(L));
  S.syncs++;
  if (h_off[0] != 0 || h_off[ncell] != total) return ctx->fail(YRWI_E_HIP, "dht offsets do not add up to the selection");
  // ---- the rows, window by window
  const bool direct = ((uintptr_t)rows40_out & 7) == 0 && ctx->hostreg.contains(rows40_out, (size_t)total * ROW);
  WindowTally WT;
  const int wrc = run_windows(
      ctx, L, wneed, nwin, "dht", &WT,
      [&](int64_t i, uint8_t* dwin) {
        const int64_t w0 = i * W, len = std::min(W, total - w0);
        hipLaunchKernelGGL(k_dht_pack, dim3((unsigned)((len * ROW + SLICE - 1) / SLICE)), dim3(PACK_THREADS), 0,
                           L->stream, d_off, d_srow, d_jobs, ncell, T, w0, len, dwin);
      },
      [&](int64_t i, uint8_t* pinned, size_t* bytes) {
        *bytes = (size_t)std::min(W, total - i * W) * ROW;
        return direct ? rows40_out + (size_t)(i * W) * ROW : pinned;
      },
      [&](int64_t i, const uint8_t* p, size_t bytes) {  // staged rows to the caller's buffer
        if (!direct) std::memcpy(rows40_out + (size_t)(i * W) * ROW, p, bytes);
        return 0;
      });
  S.launches += WT.launches;
  S.syncs += WT.syncs;
  S.t_pack_ns = WT.t_pack_ns;
  S.windows = WT.windows;
  if (wrc) return wrc;
  for (int64_t j = 0; j < T; j++) key_chars(all[sel[(size_t)j]].first, terms12_out + (size_t)j * 12);
  std::memcpy(part_off, h_off, (size_t)(ncell + 1) * sizeof(int64_t));
  // ---- IndexCell.remove(termHash): the last row has landed; the bookkeeping of an emptied list
  if (flags & YRWI_DHT_REMOVE) {
    for (int64_t j = 0; j < T; j++) {
      const KeyT key = all[sel[(size_t)j]].first;
      auto it = ctx->lists.find(key);
      const int64_t n = it->second.n;
      index_changed(ctx, key, n, false);
      ctx->npostings -= n;
      ctx->lists.erase(it);
      S.removed += n;
    }
  }
  return finish(0);
}
