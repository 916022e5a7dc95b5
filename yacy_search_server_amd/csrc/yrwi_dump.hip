// yrwi_dump.hip -- the device index written to a YaCy BLOB heap file (the FlushThread dump of
// IndexCell, IndexCell.java:131-166, through HeapWriter.add, HeapWriter.java:114-124, and
// RowCollection.exportCollection, RowCollection.java:209-224).
//
// The file is the concatenation, in Base64Order of the term hashes, of one record per
// non-empty list: [int32 BE reclen = 12 + 14 + 40 n][12-B term hash][14-B export header][n rows
// of 40 B as stored].  Its image never exists in one piece: it is produced in fixed-size
// windows of the byte stream.  One job table (the selected terms in key order: row pointer, n,
// term hash, and the int64 file offset of every record, a prefix sum over 30 + 40 n) is uploaded
// in one copy; k_dump_pack then writes one window's bytes into a device window, and the host
// writes window i - 1 to the file while window i is packed and copied (run_windows,
// yrwi_host.h).  Launches follow the bytes and the window size, never the number of terms; the
// host waits once per window plus a constant.
//
// k_dump_pack: a workgroup takes a 16 KiB slice of the window, finds the record holding the
// slice start by binary search of the offset table and walks on from there.  Every thread
// produces aligned 16-byte pieces of the output and stores each with one 16-byte vector store.
// Row storage is 256-B aligned per list, a record's row area starts at an even file offset
// (30 + 40 n is even), so source and destination differ by an even amount mod 16: a piece that
// lies inside one record's rows is a funnel shift over two neighbouring aligned 16-byte loads;
// a piece that touches a reclen, key or export header, a record boundary or the end of the file
// is assembled from 2-byte units (every field starts at an even offset).
//
// A sharded context writes the lists it holds, i.e. its url-hash range of every term; no
// collective is involved, and the shards' files loaded together give the whole index.

#include <cerrno>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "yrwi_device.h"
#include "yrwi_host.h"

using namespace yrwi;

namespace {

constexpr int REC_HDR = 4 + YRWI_HASH_BYTES + 14;  // reclen, key, export header
constexpr int PIECE = 16;
constexpr int PACK_THREADS = 256;
constexpr int PACK_ITERS = 4;
constexpr int64_t SLICE = (int64_t)PACK_THREADS * PIECE * PACK_ITERS;  // bytes per workgroup
constexpr int SLICE_RECS = (int)(SLICE / (REC_HDR + YRWI_ROW_BYTES)) + 2;  // records a slice can touch
constexpr int64_t DEFAULT_WINDOW = (int64_t)32 << 20;
constexpr int64_t MAX_WINDOW = (int64_t)1 << 30;
constexpr int64_t MS_2000 = YRWI_DUMP_EPOCH_MS;
constexpr int64_t MS_DAY = 86400000ll;

struct DumpJob {  // one record of the file
  const uint8_t* rows;
  int64_t n;
  uint8_t key[YRWI_HASH_BYTES];
  uint32_t pad;
};

// byte h (0 .. 29) of a record's reclen, key and export header
__device__ __forceinline__ uint32_t hdr_byte(const DumpJob& J, int h, uint32_t days) {
  const uint32_t n = (uint32_t)J.n;
  if (h < 4) return ((uint32_t)(YRWI_HASH_BYTES + 14) + (uint32_t)YRWI_ROW_BYTES * n) >> (8 * (3 - h)) & 255u;
  if (h < 16) return J.key[h - 4];
  if (h < 20) return n >> (8 * (19 - h)) & 255u;              // size
  if (h < 24) return days >> (8 * (1 - ((h - 20) & 1))) & 255u;  // lastread, lastwrote
  if (h < 26) return h == 24 ? (uint32_t)YRWI_DUMP_ORDERKEY0 : (uint32_t)YRWI_DUMP_ORDERKEY1;
  return n >> (8 * (29 - h)) & 255u;                          // orderbound
}

// Window [w0, w0 + wlen) of the file image -> dst (16-B aligned, room for wlen rounded up to 16).
// off: nj + 1 record offsets (off[nj] = total, the file size); w0 is a multiple of 16.
__global__ __launch_bounds__(PACK_THREADS) void k_dump_pack(const int64_t* __restrict__ off,
                                                            const DumpJob* __restrict__ jobs, int64_t nj, int64_t w0,
                                                            int64_t wlen, int64_t total, uint32_t days,
                                                            uint8_t* __restrict__ dst) {
  __shared__ int64_t s_j0;
  const int64_t s0 = (int64_t)blockIdx.x * SLICE;  // slice start in the window (< wlen by the grid)
  if (threadIdx.x == 0) s_j0 = seg_of(off, (int64_t)0, nj - 1, w0 + s0);
  __syncthreads();
  int64_t j = s_j0;
  const int64_t jhi = j + SLICE_RECS < nj - 1 ? j + SLICE_RECS : nj - 1;
#pragma unroll 1
  for (int it = 0; it < PACK_ITERS; it++) {
    const int64_t ci = s0 + ((int64_t)it * PACK_THREADS + threadIdx.x) * PIECE;
    if (ci >= wlen) break;
    const int64_t c = w0 + ci;  // < total
    j = seg_of(off, j, jhi, c);
    const int64_t r = c - off[j];
    uint4 o;
    if (r >= REC_HDR && c + PIECE <= off[j + 1]) {
      // inside the rows of record j: funnel shift over two aligned 16-byte loads
      const uint8_t* s = jobs[j].rows + (r - REC_HDR);
      const int sh = (int)((uintptr_t)s & 15);
      const gmem_u4* a = (const gmem_u4*)(uintptr_t)(s - sh);  // global, not flat, loads
      const u32x4 lo = a[0];
      if (sh == 0) {
        o = make_uint4(lo.x, lo.y, lo.z, lo.w);
      } else {
        const u32x4 hi = a[1];  // ends at or before the 16-B round-up of the list's rows
        uint64_t q0 = ((uint64_t)lo.y << 32) | lo.x, q1 = ((uint64_t)lo.w << 32) | lo.z;
        uint64_t q2 = ((uint64_t)hi.y << 32) | hi.x;
        const uint64_t q3 = ((uint64_t)hi.w << 32) | hi.z;
        if (sh & 8) {
          q0 = q1;
          q1 = q2;
          q2 = q3;
        }
        const int bs = (sh & 7) * 8;  // 0, 16, 32 or 48
        if (bs) {
          q0 = (q0 >> bs) | (q1 << (64 - bs));
          q1 = (q1 >> bs) | (q2 << (64 - bs));
        }
        o = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
      }
    } else {
      // a header, a record boundary or the end of the file: 2-byte units
      uint32_t w[4] = {0, 0, 0, 0};
      int64_t jj = j;
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int64_t p = c + 2 * u;
        uint32_t v = 0;
        if (p < total) {
          while (p >= off[jj + 1]) jj++;
          const int64_t rr = p - off[jj];
          if (rr < REC_HDR) {
            v = hdr_byte(jobs[jj], (int)rr, days) | (hdr_byte(jobs[jj], (int)rr + 1, days) << 8);
          } else {
            v = *reinterpret_cast<const uint16_t*>(jobs[jj].rows + (rr - REC_HDR));
          }
        }
        w[u >> 1] |= v << (16 * (u & 1));
      }
      o = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(dst + ci) = o;
  }
}

int64_t window_bytes() {
  int64_t w = DEFAULT_WINDOW;
  const char* e = getenv("YRWI_DUMP_WINDOW");  // read per call: tests force window boundaries with it
  if (e && *e) w = atoll(e);
  w = std::min(w, MAX_WINDOW) & ~(int64_t)255;
  return std::max<int64_t>(w, 256);
}

int write_all(int fd, const uint8_t* p, size_t n) {
  while (n) {
    const ssize_t k = ::write(fd, p, n);
    if (k < 0) {
      if (errno == EINTR) continue;
      return -1;
    }
    p += k;
    n -= (size_t)k;
  }
  return 0;
}

// the temporary file: removed unless commit() renamed it onto the path
struct TmpFile {
  std::string tmp, path;
  int fd = -1;
  ~TmpFile() {
    if (fd >= 0) ::close(fd);
    if (!tmp.empty()) ::unlink(tmp.c_str());
  }
  int commit() {
    if (::fsync(fd) != 0) return -1;
    const int rc = ::close(fd);
    fd = -1;
    if (rc != 0) return -1;
    if (::rename(tmp.c_str(), path.c_str()) != 0) return -1;
    tmp.clear();
    return 0;
  }
};

int io_fail(yrwi_ctx* ctx, const std::string& what, const std::string& name) {
  return ctx->fail(YRWI_E_IO, what + " " + name + ": " + std::strerror(errno));
}

}  // namespace

extern "C" int yrwi_dump_heap(yrwi_ctx* ctx, const char* path, const uint8_t* terms12, int32_t nterms, int64_t now_ms,
                              yrwi_dump_stats* st) {
  if (!ctx || !path || !*path || nterms < 0 || (nterms > 0 && !terms12)) return YRWI_E_ARG;
  const auto t_begin = std::chrono::steady_clock::now();
  yrwi_dump_stats S;
  std::memset(&S, 0, sizeof(S));
  if (st) std::memset(st, 0, sizeof(*st));
  // ---- job table: the non-empty selected lists in key order (the selection is checked before
  //      anything is written), offsets a prefix sum over 30 + 40 n
  ListSel recs;
  if (int rc = select_lists(ctx, terms12, nterms, true, &recs)) return rc;
  const int64_t nj = (int64_t)recs.size();
  std::vector<DumpJob> jobs((size_t)nj);
  std::vector<int64_t> off((size_t)nj + 1);
  int64_t total = 0;
  for (int64_t j = 0; j < nj; j++) {
    DumpJob& J = jobs[(size_t)j];
    std::memset(&J, 0, sizeof(J));
    J.rows = recs[(size_t)j].second->rows;
    J.n = recs[(size_t)j].second->n;
    key_chars(recs[(size_t)j].first, J.key);
    off[(size_t)j] = total;
    total += REC_HDR + (int64_t)YRWI_ROW_BYTES * J.n;
    S.postings += J.n;
  }
  off[(size_t)nj] = total;
  S.terms = nj;
  S.bytes = total;
  if (now_ms == 0)
    now_ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch())
                 .count();
  int64_t d = now_ms - MS_2000;
  d = d >= 0 ? d / MS_DAY : -((-d + MS_DAY - 1) / MS_DAY);
  const uint32_t days = (uint32_t)d & 0xFFFFu;
  // ---- the temporary file
  TmpFile F;
  F.path = path;
  F.tmp = F.path + ".prt";
  F.fd = ::open(F.tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (F.fd < 0) {
    const int rc = io_fail(ctx, "cannot create", F.tmp);
    F.tmp.clear();  // nothing of ours to remove
    return rc;
  }
  const int64_t W = window_bytes();
  const int64_t nwin = (total + W - 1) / W;
  if (nwin > 0) {
    Lane* L = ctx->lanes[0];
    if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
    S.syncs++;
    int64_t* d_off = arena_alloc<int64_t>(L, nj + 1);
    DumpJob* d_jobs = arena_alloc<DumpJob>(L, nj);
    if (!d_off || !d_jobs) return ctx->fail(YRWI_E_NOMEM, "device allocation (dump job table)");
    if (int rc = upload(L, d_off, off, d_jobs, jobs)) return ctx->take(L, rc);
    S.launches++;
    WindowTally T;
    const int rc = run_windows(
        ctx, L, (size_t)W, nwin, "dump", &T,
        [&](int64_t i, uint8_t* dwin) {
          const int64_t w0 = i * W, len = std::min(W, total - w0);
          hipLaunchKernelGGL(k_dump_pack, dim3((unsigned)((len + SLICE - 1) / SLICE)), dim3(PACK_THREADS), 0, L->stream,
                             d_off, d_jobs, nj, w0, len, total, days, dwin);
        },
        [&](int64_t i, uint8_t* pinned, size_t* bytes) {
          *bytes = (size_t)std::min(W, total - i * W);
          return pinned;
        },
        [&](int64_t, const uint8_t* p, size_t bytes) {  // a landed window's bytes to the file
          return write_all(F.fd, p, bytes) != 0 ? io_fail(ctx, "cannot write", F.tmp) : 0;
        });
    S.launches += T.launches;
    S.syncs += T.syncs;
    S.t_pack_ns = T.t_pack_ns;
    S.windows = T.windows;
    if (rc) return rc;
  }
  if (F.commit() != 0) return io_fail(ctx, "cannot finish", F.path);
  S.t_total_ns =
      std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
  if (st) *st = S;
  return 0;
}
