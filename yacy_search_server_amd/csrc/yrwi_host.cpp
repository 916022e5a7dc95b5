// yrwi_host.cpp -- host runtime of libyrwi: index residency, query planning
// (the Java-side decisions of TermSearch / joinContainers / joinConstructive),
// batched device execution and the C ABI declared in include/yrwi.h.
//
// Planning rules restated here (paths relative to /root/reference/source/net/yacy):
//   J1  AbstractIndex.searchConjunction :96-128, TermSearch :42-70
//       (HandleSet: term hashes are a sorted set; a missing include term empties
//        the result, a missing exclude term disables exclusion)
//   J2  ReferenceContainer.joinContainers :334-366 (TreeMap key (int)(size*1000+i))
//   J3  ReferenceContainer.joinConstructive :406-416 (int-wrapping step counts)
// Everything per posting runs on the GPU (yrwi_kernels.hip).

#include "yrwi_host.h"
#include "yrwi_share.h"

using namespace yrwi;

// ===================================================================== profile
extern "C" void yrwi_profile_default(yrwi_profile* p) {
  std::memset(p, 0, sizeof(*p));
  p->coeff_appemph = 5; p->coeff_appurl = 12; p->coeff_app_dc_creator = 1;
  p->coeff_app_dc_description = 10; p->coeff_app_dc_subject = 2; p->coeff_app_dc_title = 14;
  p->coeff_authority = 5; p->coeff_cathasapp = 0; p->coeff_cathasaudio = 0; p->coeff_cathasimage = 0;
  p->coeff_cathasvideo = 0; p->coeff_catindexof = 0; p->coeff_date = 9; p->coeff_domlength = 10;
  p->coeff_hitcount = 1; p->coeff_language = 2; p->coeff_llocal = 0; p->coeff_lother = 7;
  p->coeff_phrasesintext = 0; p->coeff_posinphrase = 0; p->coeff_posintext = 4; p->coeff_posofphrase = 0;
  p->coeff_termfrequency = 8; p->coeff_urlcomps = 7; p->coeff_urllength = 6; p->coeff_worddistance = 10;
  p->coeff_wordsintext = 3; p->coeff_wordsintitle = 2; p->coeff_urlcompintoplist = 2;
  p->coeff_descrcompintoplist = 2; p->coeff_prefer = 0; p->coeff_citation = 10;
}

extern "C" void yrwi_profile_all_zero(yrwi_profile* p) { std::memset(p, 0, sizeof(*p)); }

// NumberTools.parseIntDecSubstring (NumberTools.java:91-124); false on NumberFormatException
static bool parse_int_dec(const std::string& s, size_t start, int32_t* out) {
  size_t end = s.size();
  if (end <= start) return false;
  size_t i = start;
  while (i < end && s[i] == ' ') i++;
  if (i >= end) return false;
  int64_t result = 0;
  bool neg = false;
  int64_t limit = -2147483647LL;
  char first = s[i];
  if (first < '0') {
    if (first == '-') { neg = true; limit = -2147483648LL; }
    else if (first != '+') return false;
    i++;
    if (i == end) return false;
  }
  int64_t multmin = limit / 10;
  while (i < end) {
    char c = s[i++];
    if (c < '0' || c > '9') break;
    int d = c - '0';
    if (result < multmin) return false;
    result *= 10;
    if (result < limit + d) return false;
    result -= d;
  }
  *out = (int32_t)(neg ? result : -result);
  return true;
}

// RankingProfile(String prefix, String profile) (RankingProfile.java:127-189)
extern "C" int yrwi_profile_parse(const char* prefix, const char* ext, yrwi_profile* out) {
  yrwi_profile_default(out);
  if (!ext || !*ext) return 0;
  std::string profile(ext);
  if (profile[0] == '{' && profile.back() == '}') profile = profile.substr(1, profile.size() - 2);
  auto trim = [](const std::string& x) {
    size_t a = 0, b = x.size();
    while (a < b && (unsigned char)x[a] <= ' ') a++;
    while (b > a && (unsigned char)x[b - 1] <= ' ') b--;
    return x.substr(a, b - a);
  };
  profile = trim(profile);
  std::vector<std::string> elts;
  char sep = (profile.find('&') != std::string::npos && profile.find('&') > 0) ? '&' : ',';
  {
    // String.split drops trailing empty strings; empty elements are harmless here
    size_t st = 0;
    while (true) {
      size_t p = profile.find(sep, st);
      elts.push_back(profile.substr(st, p == std::string::npos ? std::string::npos : p - st));
      if (p == std::string::npos) break;
      st = p + 1;
    }
  }
  std::string pre = prefix ? prefix : "";
  std::map<std::string, int32_t> coeff;
  for (auto& elt : elts) {
    std::string e = trim(elt);
    if (pre.empty() || e.compare(0, pre.size(), pre) == 0) {
      size_t p = e.find('=');
      if (p != std::string::npos && p > 0 && e.size() > p + 1) {
        int32_t v;
        if (parse_int_dec(e, p + 1, &v)) coeff[e.substr(pre.size(), p - pre.size())] = v;
      }
    }
  }
  struct F { const char* n; int32_t yrwi_profile::*f; };
  static const F fields[] = {
      {"domlength", &yrwi_profile::coeff_domlength}, {"date", &yrwi_profile::coeff_date},
      {"wordsintitle", &yrwi_profile::coeff_wordsintitle}, {"wordsintext", &yrwi_profile::coeff_wordsintext},
      {"phrasesintext", &yrwi_profile::coeff_phrasesintext}, {"llocal", &yrwi_profile::coeff_llocal},
      {"lother", &yrwi_profile::coeff_lother}, {"urllength", &yrwi_profile::coeff_urllength},
      {"urlcomps", &yrwi_profile::coeff_urlcomps}, {"hitcount", &yrwi_profile::coeff_hitcount},
      {"posintext", &yrwi_profile::coeff_posintext}, {"posofphrase", &yrwi_profile::coeff_posofphrase},
      {"posinphrase", &yrwi_profile::coeff_posinphrase}, {"authority", &yrwi_profile::coeff_authority},
      {"worddistance", &yrwi_profile::coeff_worddistance}, {"appurl", &yrwi_profile::coeff_appurl},
      {"appdescr", &yrwi_profile::coeff_app_dc_title}, {"appauthor", &yrwi_profile::coeff_app_dc_creator},
      {"apptags", &yrwi_profile::coeff_app_dc_subject}, {"appref", &yrwi_profile::coeff_app_dc_description},
      {"appemph", &yrwi_profile::coeff_appemph}, {"catindexof", &yrwi_profile::coeff_catindexof},
      {"cathasimage", &yrwi_profile::coeff_cathasimage}, {"cathasaudio", &yrwi_profile::coeff_cathasaudio},
      {"cathasvideo", &yrwi_profile::coeff_cathasvideo}, {"cathasapp", &yrwi_profile::coeff_cathasapp},
      {"tf", &yrwi_profile::coeff_termfrequency}, {"urlcompintoplist", &yrwi_profile::coeff_urlcompintoplist},
      {"descrcompintoplist", &yrwi_profile::coeff_descrcompintoplist}, {"prefer", &yrwi_profile::coeff_prefer},
      {"language", &yrwi_profile::coeff_language}, {"citation", &yrwi_profile::coeff_citation}};
  for (auto& f : fields) {
    auto it = coeff.find(f.n);
    if (it != coeff.end()) out->*(f.f) = it->second;
  }
  return 0;
}

// ===================================================================== context
extern "C" int yrwi_get_unique_id(uint8_t id[128]) {
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return YRWI_E_RCCL;
  static_assert(sizeof(u) == 128, "ncclUniqueId size");
  std::memcpy(id, &u, 128);
  return 0;
}

static void close_lanes(yrwi_ctx* ctx) {
  for (Lane* L : ctx->lanes) L->wait();
  for (Lane* L : ctx->lanes) {
    L->stop();
    if (L->stream) hipStreamSynchronize(L->stream);
    if (L->comm && L->comm != ctx->lanes[0]->comm) ncclCommDestroy(L->comm);
  }
  if (!ctx->lanes.empty() && ctx->lanes[0]->comm) ncclCommDestroy(ctx->lanes[0]->comm);
  for (Lane* L : ctx->lanes) {
    if (L->loop) loop_leave(L->loop);
    for (auto e : L->coll_ev)
      if (e) hipEventDestroy(e);
    L->arena.release();
    for (auto e : L->evpool) hipEventDestroy(e);
    if (L->stage.p) hipHostFree(L->stage.p);
    if (L->out_stage.p) hipHostFree(L->out_stage.p);
    if (L->down_stage.p) hipHostFree(L->down_stage.p);
    if (L->sync_ev) hipEventDestroy(L->sync_ev);
    if (L->stream && L->own_stream) hipStreamDestroy(L->stream);
    delete L;
  }
  ctx->lanes.clear();
}

// What a lane's first batch would otherwise set up inside the caller's first
// timed batches: its wait event, the pinned staging buffers (uploads, joined-size
// readbacks, result landing), the first scratch chunk and the stream's hardware
// queue (a first operation on it).  Runs on the lane's own thread at open.
static int warm_lane(Lane* L) {
  if (hipSetDevice(L->device) != hipSuccess) return L->fail(YRWI_E_HIP, "hipSetDevice");
  constexpr size_t kStage = (size_t)4 << 20;
  if (!stage_reserve(L, &L->stage, kStage, false) || !stage_reserve(L, &L->down_stage, kStage, false) ||
      !stage_reserve(L, &L->out_stage, kStage, false))
    return YRWI_E_HIP;
  uint8_t* p = L->arena.alloc(256);
  if (!p) return L->fail(YRWI_E_NOMEM, "scratch");
  HIPCHK(L, hipMemsetAsync(p, 0, 256, L->stream));
  HIPCHK(L, lane_sync(L));
  L->arena.reset();
  return 0;
}

// why the calling thread's last yrwi_open / yrwi_open_shard failed (no context to
// hold it): yrwi_last_error(NULL)
static thread_local std::string t_open_error;
static void set_open_error(const std::string& m) { t_open_error = m; }

static int open_common(int device, int rank, int world, yrwi_ctx** out) {
  *out = nullptr;
  t_open_error.clear();
  if (hipSetDevice(device) != hipSuccess) {
    set_open_error("hipSetDevice(" + std::to_string(device) + ") failed");
    return YRWI_E_HIP;
  }
  yrwi_ctx* ctx = new yrwi_ctx();
  ctx->device = device;
  ctx->rank = rank;
  ctx->world = world;
  // Eight lanes, sharded or not (C2, 400-step runs on one box: 0.76-0.80 ms per
  // batch with eight in flight, 0.80-0.86 with four, 1.0-1.25 with two: a lane's
  // host planning and its mid-batch wait for the joined sizes leave the device
  // idle unless enough other batches queue work).  The collectives of the lanes'
  // batch parts are enqueued in one total order on every rank (CollTurn,
  // yrwi_host.h).  Scratch: 128 GiB over all lanes (scratch_budget).
  const char* e = getenv("YRWI_LANES");
  const int nl = e ? std::max(1, std::min(16, atoi(e))) : 8;
  for (int l = 0; l < nl; l++) {
    Lane* L = new Lane();
    L->device = device;
    L->rank = rank;
    L->world = world;
    ctx->lanes.push_back(L);
    if (hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking) != hipSuccess) {
      close_lanes(ctx);
      delete ctx;
      set_open_error("hipStreamCreateWithFlags failed");
      return YRWI_E_HIP;
    }
    L->hostreg = &ctx->hostreg;
    L->turn = &ctx->turn;
    L->scratch_hint = &ctx->scratch_hint;
    L->scratch_total = &ctx->scratch_total;
    L->nlanes = nl;
    L->start_worker();
  }
  for (Lane* L : ctx->lanes) L->submit([L] { L->rc = warm_lane(L); });
  int wrc = 0;
  for (Lane* L : ctx->lanes) {
    L->wait();
    if (L->rc && !wrc) {
      wrc = L->rc;
      set_open_error("lane set-up: " + L->err);
    }
  }
  if (wrc) {
    close_lanes(ctx);
    delete ctx;
    return wrc;
  }
  ctx->stream = ctx->lanes[0]->stream;
  *out = ctx;
  return 0;
}

extern "C" int yrwi_open(int device, yrwi_ctx** out) { return open_common(device, 0, 1, out); }

extern "C" int yrwi_open_shard(int device, int rank, int world, const uint8_t nccl_id[128], yrwi_ctx** out) {
  if (world < 1 || (world & (world - 1)) || world > 64 || rank < 0 || rank >= world) return YRWI_E_ARG;
  int rc = open_common(device, rank, world, out);
  if (rc) return rc;
  yrwi_ctx* ctx = *out;
  const bool loop = world > 1 && std::memcmp(nccl_id, LOOP_TAG, sizeof(LOOP_TAG)) == 0;
  // YRWI_COLL_SELF=1: a world-1 context runs the sharded protocol over a real
  // 1-rank communicator (tests: RCCL on a one-GPU box; Lane::sharded)
  const char* cs = getenv("YRWI_COLL_SELF");
  ctx->sharded = world > 1 || (cs && atoi(cs));
  for (Lane* L : ctx->lanes) L->sharded = ctx->sharded;
  if (world > 1) {  // list-size exchanges through host shared memory (the ranks of one node)
    ctx->hostx = hostx_open(nccl_id, world, rank);
    for (Lane* L : ctx->lanes) L->hostx = ctx->hostx;
  }
  if (loop) {
    // in-process loopback group (tests: several shards on one GPU), one per lane
    bool ok = true;
    for (size_t l = 0; ok && l < ctx->lanes.size(); l++) {
      uint8_t id[128];
      std::memcpy(id, nccl_id, 128);
      id[127] ^= (uint8_t)l;
      ctx->lanes[l]->loop = loop_join(id, world, rank);
      ok = ctx->lanes[l]->loop != nullptr;
    }
    ctx->transport = YRWI_TRANSPORT_LOOPBACK;
    if (!ok) {
      yrwi_close(ctx);
      *out = nullptr;
      return YRWI_E_ARG;
    }
  } else if (ctx->sharded) {
    ctx->transport = YRWI_TRANSPORT_RCCL;
    // The transport is decided from facts every rank sees alike, before any
    // collective: ranks on ONE device (RCCL refuses a duplicate GPU) or an id
    // tagged YRWI-HOSTSTAGE exchange through host shared memory; ranks on
    // distinct devices use RCCL, and an RCCL failure there is an error, never a
    // silent switch to the host path.
    const bool staged = world > 1 && std::memcmp(nccl_id, STAGE_TAG, sizeof(STAGE_TAG)) == 0;
    int peers = -1;
    if (world > 1 && ctx->hostx) {
      char bus[32] = {0};
      int64_t devid = 0;
      if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) == hipSuccess) {
        uint64_t h = 1469598103934665603ull;  // FNV-1a of "dddd:bb:dd.f"
        for (const char* c = bus; *c; c++) h = (h ^ (uint8_t)*c) * 1099511628211ull;
        devid = (int64_t)(h >> 1) | 1;
      } else {
        devid = -(int64_t)rank - 1;  // unknown: distinct from every other rank's
      }
      peers = hostx_device_peers(ctx->hostx, devid, 120.0);
    }
    ctx->device_peers = peers;
    if (staged || peers > 0) {
      const char* why = staged ? "host-staged group id" : "ranks share a device";
      ctx->devx = (ctx->hostx && (staged ? hostx_wait_attached(ctx->hostx, 120.0) : true))
                      ? devx_open(nccl_id, world, rank, ctx->hostx) : nullptr;
      if (!ctx->devx) {
        set_open_error(std::string("host-staged collectives (") + why + ") unavailable: " +
                       (ctx->hostx ? "shared-memory segment" : "no host mailbox"));
        yrwi_close(ctx);
        *out = nullptr;
        return YRWI_E_RCCL;
      }
      for (Lane* L : ctx->lanes) L->devx = ctx->devx;
      ctx->transport = YRWI_TRANSPORT_HOSTSTAGED;
      if (!staged) fprintf(stderr, "yrwi: rank %d of %d: %s -- collectives host-staged through /dev/shm\n", rank,
                           world, why);
      return 0;
    }
    ncclUniqueId u;
    std::memcpy(&u, nccl_id, 128);
    ncclComm_t c0 = nullptr;
    const ncclResult_t irc = ncclCommInitRank(&c0, world, u, rank);
    if (irc != ncclSuccess) {
      set_open_error(std::string("ncclCommInitRank (rank ") + std::to_string(rank) + " of " + std::to_string(world) +
                     "): " + ncclGetErrorString(irc));
      yrwi_close(ctx);
      *out = nullptr;
      return YRWI_E_RCCL;
    }
    bool ok = true;
    ctx->lanes[0]->comm = c0;
    // the mailbox only works if every rank mapped the same segment (one node, one
    // /dev/shm): every rank opened it before the init above, so after it each
    // rank sees world attachments or not; all ranks agree (min over the ranks)
    // and drop the mailbox together if any one saw fewer (device all-gather then)
    if (world > 1) {
      int32_t* d_flag = nullptr;
      int32_t flag = hostx_attached(ctx->hostx) == world ? 1 : 0;
      ok = hipMalloc(&d_flag, 4) == hipSuccess;
      ok = ok && hipMemcpy(d_flag, &flag, 4, hipMemcpyHostToDevice) == hipSuccess;
      ok = ok && ncclAllReduce(d_flag, d_flag, 1, ncclInt32, ncclMin, c0, ctx->stream) == ncclSuccess;
      ok = ok && hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
      ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
      if (d_flag) hipFree(d_flag);
      if (ok && !flag && ctx->hostx) {
        hostx_close(ctx->hostx, rank == 0);  // some rank never mapped it: nobody else unlinks the name
        ctx->hostx = nullptr;
        for (Lane* L : ctx->lanes) L->hostx = nullptr;
      }
    }
    // one communicator per lane: lanes issue their collectives independently.  If
    // the split fails (the same way on every rank), the lanes share c0 -- still
    // safe: the collective turn lets one batch part at a time enqueue, in one
    // total order on every rank (close_lanes destroys c0 once).
    bool split = ok;
    for (size_t l = 1; split && l < ctx->lanes.size(); l++)
      split = ncclCommSplit(c0, 0, rank, &ctx->lanes[l]->comm, nullptr) == ncclSuccess;
    if (ok && !split)
      for (size_t l = 1; l < ctx->lanes.size(); l++) {
        if (ctx->lanes[l]->comm && ctx->lanes[l]->comm != c0) ncclCommDestroy(ctx->lanes[l]->comm);
        ctx->lanes[l]->comm = c0;
      }
    if (!ok) {
      set_open_error("RCCL group set-up after ncclCommInitRank failed (mailbox agreement all-reduce)");
      yrwi_close(ctx);
      *out = nullptr;
      return YRWI_E_RCCL;
    }
  }
  return 0;
}

extern "C" int yrwi_shard_info(yrwi_ctx* ctx, yrwi_transport_info* out) {
  if (!ctx || !out) return YRWI_E_ARG;
  std::memset(out, 0, sizeof(*out));
  out->transport = ctx->transport;
  out->rank = ctx->rank;
  out->world = ctx->world;
  out->lanes = (int32_t)ctx->lanes.size();
  out->device_peers = ctx->device_peers;
  out->mailbox = ctx->hostx ? 1 : 0;
  ncclComm_t c0 = ctx->lanes.empty() ? nullptr : ctx->lanes[0]->comm;
  if (c0) {
    int n = 0;
    if (ncclCommCount(c0, &n) == ncclSuccess) out->rccl_ranks = n;
    for (size_t l = 0; l < ctx->lanes.size(); l++)
      out->lanes_own_comm += ctx->lanes[l]->comm && (l == 0 || ctx->lanes[l]->comm != c0);
  }
  hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof(out->pci_bus_id), ctx->device);
  return 0;
}

extern "C" void yrwi_close(yrwi_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  close_lanes(ctx);
  // unlinked once every rank mapped it (hostx_open); rank 0 unlinks it again in
  // case some rank never did (ENOENT is harmless)
  hostx_close(ctx->hostx, ctx->rank == 0);
  ctx->hostx = nullptr;
  devx_close(ctx->devx, ctx->rank == 0);
  ctx->devx = nullptr;
  for (auto& b : ctx->ev_pool) hipFree(b.second);
  ctx->ev_pool.clear();
  // rows retained for events the caller left open (their handles die with the context)
  for (auto* b : ctx->local_blocks) {
    hipFree(b->mem);
    delete b;
  }
  ctx->local_blocks.clear();
  ctx->local_bytes = 0;
  if (ctx->win_dev) hipFree(ctx->win_dev);
  if (ctx->win_host) hipHostFree(ctx->win_host);
  if (ctx->host_key) hipFree(ctx->host_key);
  pair_cache_release(ctx);
  ctx->index_mem.release();
  if (ctx->uid_all) hipFree(ctx->uid_all);
  if (ctx->head_all) hipFree(ctx->head_all);
  if (ctx->bm_all) hipFree(ctx->bm_all);
  if (ctx->dkhi) hipFree(ctx->dkhi);
  if (ctx->dklo) hipFree(ctx->dklo);
  delete ctx;
}

extern "C" const char* yrwi_last_error(yrwi_ctx* ctx) {
  if (ctx) return ctx->err.c_str();
  return t_open_error.empty() ? "null context" : t_open_error.c_str();
}

// ======================================================================= index
extern "C" int yrwi_put_list(yrwi_ctx* ctx, const uint8_t term[12], const uint8_t* rows40, int64_t n, int sorted) {
  if (!ctx || !term || n < 0 || (n > 0 && !rows40)) return YRWI_E_ARG;
  KeyT tk;
  if (!key_of(term, &tk)) return ctx->fail(YRWI_E_HASH, "term hash is not well-formed Base64");
  if (n > MAX_LIST) return ctx->fail(YRWI_E_LIMIT, "list longer than 53,687,091 rows (RowSet.importRowSet)");
  hipSetDevice(ctx->device);
  drain(ctx);  // in-flight batches read the list table
  if (n == 0) {
    auto it = ctx->lists.find(tk);
    if (it != ctx->lists.end()) {
      index_changed(ctx, tk, it->second.n, false);
      ctx->npostings -= it->second.n;
      ctx->lists.erase(it);
    }
    return 0;
  }
  std::vector<uint8_t> tmp;
  const uint8_t* src = rows40;
  if (!sorted) {
    // RowSet sort; on duplicate url hashes the first occurrence wins (RowSet.mergeEnum)
    std::vector<std::pair<KeyT, int64_t>> ks((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      if (!key_of(rows40 + i * 40, &ks[(size_t)i].first)) return ctx->fail(YRWI_E_HASH, "malformed url hash");
      ks[(size_t)i].second = i;
    }
    std::stable_sort(ks.begin(), ks.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    tmp.reserve((size_t)n * 40);
    for (size_t i = 0; i < ks.size(); i++) {
      if (i > 0 && ks[i].first == ks[i - 1].first) continue;
      tmp.insert(tmp.end(), rows40 + ks[i].second * 40, rows40 + ks[i].second * 40 + 40);
    }
    src = tmp.data();
    n = (int64_t)(tmp.size() / 40);
  }
  ListRec L;
  L.n = n;
  L.rows = ctx->index_mem.alloc((size_t)n * 40);
  L.khi = reinterpret_cast<uint64_t*>(ctx->index_mem.alloc((size_t)n * 8));
  L.klo = ctx->index_mem.alloc((size_t)n);
  int32_t* derr = reinterpret_cast<int32_t*>(ctx->index_mem.alloc(4));
  if (!L.rows || !L.khi || !L.klo || !derr) return ctx->fail(YRWI_E_NOMEM, "device index allocation failed");
  HIPCHK(ctx, hipMemcpyAsync(L.rows, src, (size_t)n * 40, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(derr, 0, 4, ctx->stream));
  if (launch_validate_rows(L.rows, n, L.khi, L.klo, derr, ctx->stream)) return ctx->fail(YRWI_E_HIP, "validate launch");
  int32_t herr = 0;
  HIPCHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (herr & 1) return ctx->fail(YRWI_E_HASH, "url hash is not well-formed Base64");
  if (herr & 2) return ctx->fail(YRWI_E_NULL_LANGUAGE, "row with empty language cell (reference NPE)");
  if (herr & 4) return ctx->fail(YRWI_E_UNSORTED, "rows are not strictly ascending by url hash");
  auto it = ctx->lists.find(tk);
  const int64_t old_n = it != ctx->lists.end() ? it->second.n : 0;
  ctx->npostings -= old_n;
  ctx->lists[tk] = L;
  ctx->npostings += n;
  index_changed(ctx, tk, old_n, true);
  return 0;
}

extern "C" int yrwi_check_url_ids(yrwi_ctx* ctx, int64_t* bad, int64_t* nurls) {
  if (!ctx || !bad) return YRWI_E_ARG;
  hipSetDevice(ctx->device);
  drain(ctx);
  const int rc = check_url_ids(ctx, bad);
  if (nurls) *nurls = ctx->nurls;
  return rc;
}

extern "C" int yrwi_build_url_ids(yrwi_ctx* ctx) {
  if (!ctx) return YRWI_E_ARG;
  hipSetDevice(ctx->device);
  drain(ctx);
  return ensure_url_ids(ctx);
}

extern "C" int yrwi_list_size(yrwi_ctx* ctx, const uint8_t term[12], int64_t* n) {
  KeyT tk;
  if (!ctx || !n) return YRWI_E_ARG;
  if (!key_of(term, &tk)) return ctx->fail(YRWI_E_HASH, "term hash is not well-formed Base64");
  auto it = ctx->lists.find(tk);
  *n = it == ctx->lists.end() ? 0 : it->second.n;
  return 0;
}

extern "C" int yrwi_get_list(yrwi_ctx* ctx, const uint8_t term[12], uint8_t* rows40, int64_t cap, int64_t* n) {
  KeyT tk;
  if (!ctx || !n || cap < 0 || (cap > 0 && !rows40)) return YRWI_E_ARG;
  if (!key_of(term, &tk)) return ctx->fail(YRWI_E_HASH, "term hash is not well-formed Base64");
  // like put_list: no batch in flight (the copy below runs on lane 0's stream)
  drain(ctx);
  auto it = ctx->lists.find(tk);
  *n = it == ctx->lists.end() ? 0 : it->second.n;
  if (*n == 0) return 0;
  if (cap < *n) return ctx->fail(YRWI_E_ARG, "row buffer smaller than the list");
  hipSetDevice(ctx->device);
  HIPCHK(ctx, hipMemcpyAsync(rows40, it->second.rows, (size_t)*n * 40, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int64_t yrwi_realloc_events(void) { return g_realloc.load(); }

extern "C" int yrwi_index_info_get(yrwi_ctx* ctx, yrwi_index_info* info) {
  if (!ctx || !info) return YRWI_E_ARG;
  std::memset(info, 0, sizeof(*info));
  info->full_rebuilds = ctx->dict_full_builds;
  info->incremental_updates = ctx->dict_incremental;
  info->repacks = ctx->index_repacks;
  info->index_bytes = (int64_t)ctx->index_mem.capacity();
  info->index_bytes_used = (int64_t)ctx->index_mem.total_used;
  for (auto& kv : ctx->lists) info->bitmap_lists += kv.second.bm != nullptr;
  return 0;
}

extern "C" int yrwi_index_stats(yrwi_ctx* ctx, int64_t* nterms, int64_t* npostings, int64_t* device_bytes) {
  if (!ctx) return YRWI_E_ARG;
  if (nterms) *nterms = (int64_t)ctx->lists.size();
  if (npostings) *npostings = ctx->npostings;
  if (device_bytes) {
    // index memory, url ids, line heads, bitmaps, url dictionary, lane scratch, and the rows
    // open events retain from device-local arrivals
    size_t b = ctx->index_mem.capacity() + ctx->uid_cap * 4 + ctx->head_cap * 4 + ctx->bm_cap * 8 +
               ctx->dict_cap * 9 + ctx->local_bytes;
    for (Lane* L : ctx->lanes) b += L->arena.capacity();
    *device_bytes = (int64_t)b;
  }
  return 0;
}

// ================================================================== planning
// yrwi_filter -> FilterQ (device pointers left null), the sorted unique host keys
// of siteexcludes and the sorted unique url keys of the doublecheck seed set.
void yrwi::build_filterq(const yrwi_filter& F, FilterQ* Gp, std::vector<uint64_t>* siteex, std::vector<KeyT>* urls) {
  FilterQ& G = *Gp;
  std::memset(&G, 0, sizeof(G));
  std::memcpy(G.constraint, F.constraint, 4);
  G.has_constraint = F.has_constraint != 0;
  G.all_of = F.all_of_constraint != 0;
  G.contentdom = F.contentdom;
  G.strict = F.strict_contentdom != 0;
  const size_t ll = strnlen(F.language, sizeof(F.language));
  G.lang_len = (int32_t)ll;
  std::memcpy(G.lang, F.language, ll);
  auto host_key = [](const uint8_t* h, uint64_t* k) {
    uint64_t x = 0;
    for (int j = 0; j < 6; j++) {
      if (AHP[h[j]] < 0) return false;
      x = (x << 6) | (uint64_t)AHP[h[j]];
    }
    *k = x;
    return true;
  };
  // a host hash outside the alphabet matches no row (rows are validated)
  G.has_site = F.has_sitehash != 0;
  G.has_alt = F.has_alt_sitehash != 0 && host_key(F.alt_sitehash, &G.altsite);
  if (G.has_site && !host_key(F.sitehash, &G.site)) G.site = ~0ull;
  std::vector<uint64_t>& v = *siteex;
  v.clear();
  for (int i = 0; i < F.nsiteexcludes; i++) {
    uint64_t k;
    if (host_key(F.siteexcludes + 6 * i, &k)) v.push_back(k);
  }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  G.nsiteex = (int64_t)v.size();
  std::vector<KeyT>& u = *urls;
  u.clear();
  for (int i = 0; i < F.nurlhashes; i++) {
    KeyT k;
    if (key_of(F.urlhashes + 12 * i, &k)) u.push_back(k);
  }
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  G.nurl = (int64_t)u.size();
}

static int plan_query(const yrwi_ctx* ix, Lane* ctx, const yrwi_query_desc& d, Plan* P) {
  P->maxd = d.max_distance;
  P->k = std::min<int32_t>(std::max<int32_t>(d.k, 0), YRWI_MAX_K);
  if (d.profile) P->prof = *d.profile; else yrwi_profile_default(&P->prof);
  size_t ll = strnlen(d.language, sizeof(d.language));
  P->lang_ok = ll == 2;
  P->lang[0] = ll > 0 ? (uint8_t)d.language[0] : 0;
  P->lang[1] = ll > 1 ? (uint8_t)d.language[1] : 0;
  if (d.now_ms != 0) {
    P->now_ms = d.now_ms;
  } else {
    P->now_ms = (int64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
                    std::chrono::system_clock::now().time_since_epoch()).count();
  }
  if (d.nincl < 0 || d.nexcl < 0 || d.nincl > YRWI_MAX_TERMS || d.nexcl > YRWI_MAX_TERMS)
    return ctx->fail(YRWI_E_ARG, "too many terms");
  P->filter = d.filter;
  if (const yrwi_filter* F = d.filter) {
    if (F->nsiteexcludes < 0 || F->nurlhashes < 0 || (F->nsiteexcludes > 0 && !F->siteexcludes) ||
        (F->nurlhashes > 0 && !F->urlhashes))
      return ctx->fail(YRWI_E_ARG, "filter: bad siteexcludes / urlhashes");
  }
  // HandleSet: sorted (Base64Order) set of term hashes
  int ninc = 0, nexc = 0;
  for (int i = 0; i < d.nincl; i++)
    if (!key_of(d.incl + 12 * i, &P->inc[ninc++])) return ctx->fail(YRWI_E_HASH, "include term hash not well-formed");
  for (int i = 0; i < d.nexcl; i++)
    if (!key_of(d.excl + 12 * i, &P->exc[nexc++])) return ctx->fail(YRWI_E_HASH, "exclude term hash not well-formed");
  P->has_sel = d.urlselection != nullptr && d.nurlselection > 0;
  P->sel.clear();
  P->sel_uid.clear();
  if (d.nurlselection < 0 || (d.nurlselection > 0 && !d.urlselection))
    return ctx->fail(YRWI_E_ARG, "bad urlselection");
  if (P->has_sel) {  // HandleSet urlselection: a sorted set of url hashes
    P->sel.resize((size_t)d.nurlselection);
    for (int32_t i = 0; i < d.nurlselection; i++)
      if (!key_of(d.urlselection + 12 * (size_t)i, &P->sel[(size_t)i]))
        return ctx->fail(YRWI_E_HASH, "urlselection hash not well-formed");
    std::sort(P->sel.begin(), P->sel.end());
    P->sel.erase(std::unique(P->sel.begin(), P->sel.end()), P->sel.end());
  }
  std::sort(P->inc, P->inc + ninc);
  ninc = (int)(std::unique(P->inc, P->inc + ninc) - P->inc);
  std::sort(P->exc, P->exc + nexc);
  nexc = (int)(std::unique(P->exc, P->exc + nexc) - P->exc);
  P->ninc = ninc;
  P->nexc = nexc;
  auto local = [&](const KeyT& k) -> const ListRec* {
    auto it = ix->lists.find(k);
    return (it == ix->lists.end() || it->second.n == 0) ? nullptr : &it->second;
  };
  for (int i = 0; i < ninc; i++) P->linc[i] = local(P->inc[i]);
  for (int i = 0; i < nexc; i++) P->lexc[i] = local(P->exc[i]);
  P->empty = true;
  P->postings_in = 0;
  for (int i = 0; i < ninc; i++) P->postings_in += P->linc[i] ? P->linc[i]->n : 0;
  for (int i = 0; i < nexc; i++) P->postings_in += P->lexc[i] ? P->lexc[i]->n : 0;
  return 0;
}

// A list of a query term that this url-hash shard does not hold.
static const ListRec kAbsentList{};

// The size-dependent decisions of TermSearch / joinContainers, taken on the
// GLOBAL list sizes ng_inc / ng_exc (one context: its own sizes; url-hash
// shards: the sum over all shards, so every shard takes the decisions the single
// container would -- AbstractIndex.java:108-127, ReferenceContainer.java:334-366):
//   J1  any include term without postings empties the result; any exclude term
//       without postings disables the exclusion;
//   J2  fold order by (int)(size*1000 + count), a later put overwriting an
//       equal key.
// The lists joined are the shard's own (absent ones are empty).
static void plan_finish(Plan* P, const int64_t* ng_inc, const int64_t* ng_exc) {
  P->empty = true;
  P->seq.clear();
  P->seq_ng.clear();
  P->excl.clear();
  if (P->ninc == 0) return;
  for (int i = 0; i < P->ninc; i++)
    if (ng_inc[i] == 0) return;  // conjunction: any missing term -> empty
  bool use_excl = P->nexc > 0;
  for (int i = 0; i < P->nexc; i++)
    if (ng_exc[i] == 0) use_excl = false;
  P->nexcl_g = use_excl ? P->nexc : 0;
  if (use_excl)
    for (int i = 0; i < P->nexc; i++)
      if (P->lexc[i]) P->excl.push_back(P->lexc[i]);
  // joinContainers: TreeMap<Long>((int)(size*1000 + count)); put overwrites equal keys
  std::pair<int32_t, int> tm[YRWI_MAX_TERMS];
  for (int c = 0; c < P->ninc; c++) tm[c] = {add32(mul32((int32_t)ng_inc[c], 1000), c), c};
  std::stable_sort(tm, tm + P->ninc, [](const std::pair<int32_t, int>& a, const std::pair<int32_t, int>& b) {
    return a.first < b.first;
  });
  for (int i = 0; i < P->ninc; i++) {
    if (i + 1 < P->ninc && tm[i + 1].first == tm[i].first) continue;  // the later put wins
    const int c = tm[i].second;
    P->seq_term[P->seq.size()] = c;
    P->seq.push_back(P->linc[c] ? P->linc[c] : &kAbsentList);
    P->seq_ng.push_back(ng_inc[c]);
  }
  P->empty = false;
}

int yrwi::allsum_host(Lane* L, std::vector<int64_t>& v) {
  if (!L->sharded || v.empty()) return 0;
  const int hx = hostx_allsum(L, v);  // the node's shared-memory mailbox (no device collective, no turn)
  if (hx <= 0) return hx;
  const size_t n = v.size();
  int64_t* d_v = arena_alloc<int64_t>(L, (int64_t)n);
  int64_t* d_all = arena_alloc<int64_t>(L, (int64_t)n * L->world);
  if (!d_v || !d_all) return L->fail(YRWI_E_NOMEM, "arena");
  if (upload(L, d_v, v)) return YRWI_E_HIP;
  if (int rc = coll_allgather(L, d_v, d_all, n * sizeof(int64_t))) return rc;
  const uint8_t* hb = readback(L, &L->down_stage, d_all, (int64_t)n * L->world, 8, 8);
  if (!hb) return YRWI_E_HIP;
  HIPCHK(L, lane_sync(L));
  std::vector<int64_t> all(n * (size_t)L->world);
  std::memcpy(all.data(), hb, all.size() * sizeof(int64_t));
  for (size_t i = 0; i < n; i++) {
    int64_t s = 0;
    for (int r = 0; r < L->world; r++) s += all[(size_t)r * n + i];
    v[i] = s;
  }
  return 0;
}

// TermSearch's urlselection (yrwi_query_desc.urlselection): every selection
// query's url ids on this shard (from the url dictionary; urls it does not hold
// can match nothing) and the local sizes of its include and exclude lists
// restricted to them -- the sizes ReferenceContainerCache.get(key, urlselection)
// gives (ReferenceContainerCache.java:448-470), on which J1 / J2 / J3 decide.
static int resolve_selections(Lane* L, std::vector<Plan>& plans) {
  std::vector<size_t> qs;
  for (size_t q = 0; q < plans.size(); q++)
    if (plans[q].has_sel) qs.push_back(q);
  if (qs.empty()) return 0;
  if (begin_pass(L)) return YRWI_E_HIP;
  std::vector<uint64_t> hi;
  std::vector<uint8_t> lo;
  std::vector<size_t> off{0};
  for (size_t q : qs) {
    for (const KeyT& k : plans[q].sel) {
      hi.push_back(k.hi);
      lo.push_back((uint8_t)k.lo);
    }
    off.push_back(hi.size());
  }
  const int64_t n = (int64_t)hi.size();
  uint64_t* d_hi = arena_alloc<uint64_t>(L, n);
  uint8_t* d_lo = arena_alloc<uint8_t>(L, n);
  uint32_t* d_uid = arena_alloc<uint32_t>(L, n);
  if (!d_hi || !d_lo || !d_uid) return L->fail(YRWI_E_NOMEM, "arena");
  if (upload(L, d_hi, hi, d_lo, lo)) return YRWI_E_HIP;
  if (launch_sel_lookup(d_hi, d_lo, n, L->dkhi, L->dklo, L->dkhi ? L->nurls : 0, d_uid, L->stream))
    return L->fail(YRWI_E_HIP, "selection lookup launch");
  const uint8_t* hb = readback(L, &L->down_stage, d_uid, n, 4, 4);
  if (!hb) return YRWI_E_HIP;
  HIPCHK(L, lane_sync(L));
  std::vector<uint32_t> uids((size_t)n);
  std::memcpy(uids.data(), hb, (size_t)n * 4);
  std::vector<uint32_t> all;  // every query's ids, concatenated (ascending per query: ids keep key order)
  std::vector<int64_t> aoff;
  for (size_t i = 0; i < qs.size(); i++) {
    Plan& P = plans[qs[i]];
    P.sel_uid.clear();
    for (size_t j = off[i]; j < off[i + 1]; j++)
      if (uids[j] != 0xFFFFFFFFu) P.sel_uid.push_back(uids[j]);
    aoff.push_back((int64_t)all.size());
    all.insert(all.end(), P.sel_uid.begin(), P.sel_uid.end());
  }
  uint32_t* d_all = arena_alloc<uint32_t>(L, (int64_t)all.size());
  if (!d_all) return L->fail(YRWI_E_NOMEM, "arena");
  std::vector<SelCount> jobs;
  std::vector<std::pair<size_t, int>> who;  // (plan, list: include i or YRWI_MAX_TERMS + exclude i)
  int64_t* d_cnt = arena_alloc<int64_t>(L, (int64_t)qs.size() * 2 * YRWI_MAX_TERMS);
  if (!d_cnt) return L->fail(YRWI_E_NOMEM, "arena");
  for (size_t i = 0; i < qs.size(); i++) {
    Plan& P = plans[qs[i]];
    for (int t = 0; t < YRWI_MAX_TERMS; t++) P.sel_ninc[t] = P.sel_nexc[t] = 0;
    for (int li = 0; li < P.ninc + P.nexc; li++) {
      const ListRec* R = li < P.ninc ? P.linc[li] : P.lexc[li - P.ninc];
      if (!R || P.sel_uid.empty()) continue;
      SelCount c{};
      c.L = chain_list(R);
      c.sel = d_all + aoff[i];
      c.nsel = (int64_t)P.sel_uid.size();
      c.out = d_cnt + (int64_t)jobs.size();
      jobs.push_back(c);
      who.push_back({qs[i], li < P.ninc ? li : YRWI_MAX_TERMS + (li - P.ninc)});
    }
  }
  if (jobs.empty()) return 0;
  SelCount* d_jobs = arena_alloc<SelCount>(L, (int64_t)jobs.size());
  if (!d_jobs) return L->fail(YRWI_E_NOMEM, "arena");
  if (upload(L, d_all, all, d_jobs, jobs)) return YRWI_E_HIP;
  if (launch_sel_count(d_jobs, (int32_t)jobs.size(), L->stream)) return L->fail(YRWI_E_HIP, "selection count launch");
  const uint8_t* cb = readback(L, &L->down_stage, d_cnt, (int64_t)jobs.size(), 8, 8);
  if (!cb) return YRWI_E_HIP;
  HIPCHK(L, lane_sync(L));
  for (size_t j = 0; j < jobs.size(); j++) {
    int64_t c;
    std::memcpy(&c, cb + 8 * j, 8);
    Plan& P = plans[who[j].first];
    if (who[j].second < YRWI_MAX_TERMS) P.sel_ninc[who[j].second] = c;
    else P.sel_nexc[who[j].second - YRWI_MAX_TERMS] = c;
  }
  return 0;
}

// plan_finish for a batch: global term sizes from one exchange of the local
// sizes of the batch's distinct terms (sharded), or the local sizes (one context).
static int plan_batch(Lane* L, std::vector<Plan>& plans) {
  // a query with a url selection sees its lists restricted to it (resolve_selections)
  auto inc_n = [](const Plan& P, int i) -> int64_t { return P.has_sel ? P.sel_ninc[i] : P.linc[i] ? P.linc[i]->n : 0; };
  auto exc_n = [](const Plan& P, int i) -> int64_t { return P.has_sel ? P.sel_nexc[i] : P.lexc[i] ? P.lexc[i]->n : 0; };
  if (!L->sharded) {  // one context: its own sizes are the global ones
    for (Plan& P : plans) {
      int64_t gi[YRWI_MAX_TERMS], ge[YRWI_MAX_TERMS];
      for (int i = 0; i < P.ninc; i++) P.inc_allbm[i] = !P.has_sel && P.linc[i] && P.linc[i]->bm;
      for (int i = 0; i < P.ninc; i++) gi[i] = inc_n(P, i);
      for (int i = 0; i < P.nexc; i++) ge[i] = exc_n(P, i);
      plan_finish(&P, gi, ge);
    }
    return 0;
  }
  // every slot carries size * 128 + (this shard's list has a url-id bitmap): the
  // sum over the shards is the global size * 128 + the shards with a bitmap (< 128)
  std::unordered_map<KeyT, size_t, KeyHash> slot;
  std::vector<int64_t> sz;
  auto slot_of = [&](const KeyT& k, const ListRec* l) {
    auto it = slot.find(k);
    if (it != slot.end()) return it->second;
    slot.emplace(k, sz.size());
    sz.push_back(l ? l->n * 128 + (l->bm ? 1 : 0) : 0);
    return sz.size() - 1;
  };
  auto own_slot = [&](int64_t n) {  // a selection query's restricted size: a slot of its own
    sz.push_back(n * 128);
    return sz.size() - 1;
  };
  // first-appearance order over the batch's queries: identical on every rank
  std::vector<std::array<size_t, 2 * YRWI_MAX_TERMS>> idx(plans.size());
  for (size_t q = 0; q < plans.size(); q++) {
    Plan& P = plans[q];
    for (int i = 0; i < P.ninc; i++)
      idx[q][(size_t)i] = P.has_sel ? own_slot(inc_n(P, i)) : slot_of(P.inc[i], P.linc[i]);
    for (int i = 0; i < P.nexc; i++)
      idx[q][(size_t)(YRWI_MAX_TERMS + i)] = P.has_sel ? own_slot(exc_n(P, i)) : slot_of(P.exc[i], P.lexc[i]);
  }
  if (int rc = allsum_host(L, sz)) return rc;
  for (size_t q = 0; q < plans.size(); q++) {
    Plan& P = plans[q];
    int64_t gi[YRWI_MAX_TERMS], ge[YRWI_MAX_TERMS];
    for (int i = 0; i < P.ninc; i++) {
      const int64_t v = sz[idx[q][(size_t)i]];
      gi[i] = v >> 7;
      P.inc_allbm[i] = !P.has_sel && (v & 127) == L->world;
    }
    for (int i = 0; i < P.nexc; i++) ge[i] = sz[idx[q][(size_t)(YRWI_MAX_TERMS + i)]] >> 7;
    plan_finish(&P, gi, ge);
  }
  return 0;
}

static int64_t now_ns() {
  return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Plan and run queries q[0, nq) on lane L; results at out (row stride kmax).
// Every field of *st is this part's own (the caller sums parts).
// Upper bound of the arena bytes one query takes in a pass: per fold step the
// join's tile descriptors (~1 B per 64 input postings), its matched pairs (12 B
// each, at most the smaller side) and the joined container (url id + 32-byte
// record: 36 B per row, at most the smallest list), then the rank phase over
// that container (exclusion marks, chunk summaries, candidates: ~48 B per row).
// Scratch bytes a query is expected to take in a pass: 48 B per slot of its
// smallest list and fold step (a step-by-step container at its bound min(nA, nB);
// a chained fold's pair slots, later-list rows, tile arrays and output), plus the
// ranked container.  (A tighter estimate for chained folds -- pairs and rows
// once, the output from the lists' densities -- put C4's eight lanes past the
// device's memory as their outputs grew the arenas: profiles/archive/r04_c4_host.txt.)
static int64_t scratch_estimate(const Plan& P) {
  if (P.empty || P.seq.empty()) return 4096;
  int64_t sum = 0, nmin = INT64_MAX;
  for (const ListRec* l : P.seq) {
    sum += l->n;
    nmin = std::min(nmin, l->n);
  }
  for (const ListRec* l : P.excl) sum += l->n;
  return sum / 64 + (48 * (int64_t)(P.seq.size() - 1) + 48) * nmin + 65536;
}

// Scratch budget of one pass (YRWI_SCRATCH_GB per lane, default 192 GiB / lanes).  A
// batch whose queries need more runs as consecutive passes over query ranges;
// sharded contexts never split (every rank must issue the same collectives, and
// the estimate depends on the local shard), so they keep one pass per batch.
static int64_t scratch_budget(const Lane* L) {
  if (L->sharded) return INT64_MAX;
  // per lane: YRWI_SCRATCH_GB, else the device memory left beside the resident
  // index (measured after it was built, ensure_url_ids: free memory + the lanes'
  // arenas then - 8 GiB headroom) shared by the lanes, at most 192 GiB in all (C4:
  // 16 GiB per lane ran 7 passes a batch at 10.3 ms/step, 24 GiB 9.86, 32 GiB 9.73
  // -- the passes' fixed kernels and syncs; profiles/archive/r04_scratch_c4.txt)
  const char* e = getenv("YRWI_SCRATCH_GB");
  if (e) return (int64_t)(std::max(atof(e), 0.001) * (double)(1ll << 30));
  const int64_t cap = (int64_t)192 << 30;
  const int64_t tot = L->scratch_total ? L->scratch_total->load() : 0;
  const int64_t all = tot > 0 ? std::min(tot, cap) : cap;
  return std::max<int64_t>(all / std::max(1, L->nlanes), (int64_t)256 << 20);
}

// the scratch budget's base (scratch_budget): device memory free beside the index,
// dictionary and bitmaps, plus what the lanes' arenas hold now, minus headroom
void yrwi::measure_scratch(CtxBase* ctx) {
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  int64_t arenas = 0;
  for (Lane* L : ctx->lanes) arenas += (int64_t)L->arena.capacity();
  ctx->scratch_total = std::max<int64_t>((int64_t)fr + arenas - ((int64_t)8 << 30), (int64_t)1 << 30);
}

// ================================================================ pair cache
void yrwi::pair_cache_invalidate(CtxBase* ctx) {
  std::lock_guard<std::mutex> lk(ctx->pcache.mu);
  ctx->pcache.tab.invalidate();
}

void yrwi::pair_cache_release(CtxBase* ctx) {
  PairCache& C = ctx->pcache;
  std::lock_guard<std::mutex> lk(C.mu);
  C.tab.reset(0);
  if (C.block) hipFree(C.block);
  C.block = nullptr;
  for (hipEvent_t e : C.ev)
    if (e) hipEventDestroy(e);
  C.ev.clear();
  C.ready.clear();
}

void yrwi::pair_cache_reserve(CtxBase* ctx) {
  PairCache& C = ctx->pcache;
  std::lock_guard<std::mutex> lk(C.mu);
  const size_t want = ctx->sharded || !pair_cache_enabled() ? 0 : pair_cache_budget();
  if (want == C.tab.capacity()) return;
  C.tab.reset(0);  // (nothing is in flight: no entry is pinned)
  if (C.block) hipFree(C.block);
  C.block = nullptr;
  if (want == 0) return;
  note_realloc("pair cache", want);
  void* p = nullptr;
  if (hipMalloc(&p, want) != hipSuccess) {
    (void)hipGetLastError();  // no block: the cache stays off (yrwi_pair_cache_info_get reports it)
    return;
  }
  C.block = static_cast<uint8_t*>(p);
  C.tab.reset(want);
}

static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// an entry's block: the records, the url ids, the pieces, each from a 256-B boundary
static size_t pair_entry_bytes(int64_t rows, int64_t ntiles) {
  return al256((size_t)rows * FEAT_BYTES) + al256((size_t)rows * 4) + al256((size_t)ntiles * sizeof(ChunkSum));
}

int yrwi::pair_cache_lookup(Lane* L, std::vector<Plan>& plans) {
  PairCache* C = L->pcache;
  if (!C) return 0;
  const int64_t min_rows = pair_cache_min_rows();
  // hits whose fill is not known to be complete: (slot, its event); looked at outside the lock
  std::vector<std::pair<int32_t, hipEvent_t>> fresh;
  std::unique_lock<std::mutex> lk(C->mu);
  if (!C->block) return 0;
  for (Plan& P : plans) {
    P.pc_slot = -1;
    P.pc_fill = false;
    // two distinct include terms and nothing else; a last step that gets pieces (no authority counts)
    if (P.empty || P.rep >= 0 || P.chain || P.seq.size() != 2 || P.ninc != 2 || P.nexc != 0 || P.filter ||
        P.has_sel || P.maxd != YRWI_MAX_DISTANCE_ANY || P.prof.coeff_authority > 12 || P.now_ms < 0)
      continue;
    if (std::min(P.seq[0]->n, P.seq[1]->n) < min_rows) continue;  // its container cannot reach the minimum
    P.pc_key = pair_key(P.inc[0].hi, P.inc[0].lo, P.inc[1].hi, P.inc[1].lo, P.now_ms / DAY_MS);
    const int32_t s = C->tab.lookup(P.pc_key);
    if (s < 0) {
      P.pc_fill = true;
      continue;
    }
    L->pc_pins.push_back(s);
    if (!C->ready[(size_t)s]) fresh.push_back({s, C->ev[(size_t)s]});
    const PairEntry& e = C->tab.at(s);
    uint8_t* base = C->block + e.off;
    uint64_t* feat = reinterpret_cast<uint64_t*>(base);
    uint32_t* uid = reinterpret_cast<uint32_t*>(base + al256((size_t)e.rows * FEAT_BYTES));
    const ChunkSum* ps = reinterpret_cast<const ChunkSum*>(base + al256((size_t)e.rows * FEAT_BYTES) +
                                                           al256((size_t)e.rows * 4));
    P.cont = DList{nullptr, nullptr, nullptr, e.rows, uid, feat, nullptr, nullptr, 0};
    P.pieces = ps;
    P.npieces = e.ntiles;
    P.pc_slot = s;
  }
  lk.unlock();
  // Filled a moment ago, maybe by another lane: this lane's stream goes behind the fill's event
  // (the pin keeps slot and event this entry's).  The table's lock is held for table calls only.
  std::vector<int32_t> done;
  for (auto& f : fresh) {
    if (hipEventQuery(f.second) == hipSuccess) {
      done.push_back(f.first);
    } else {
      (void)hipGetLastError();
      HIPCHK(L, hipStreamWaitEvent(L->stream, f.second, 0));
    }
  }
  if (!done.empty()) {
    lk.lock();
    for (int32_t s : done) C->ready[(size_t)s] = 1;
  }
  return 0;
}

int yrwi::pair_cache_fill(Lane* L, std::vector<Plan>& plans, const std::vector<JoinQ>& jobs,
                          const std::vector<int>& owner, const std::vector<int64_t>& mh) {
  PairCache* C = L->pcache;
  if (!C) return 0;
  bool any = false;
  for (size_t j = 0; j < jobs.size(); j++) any |= plans[(size_t)owner[j]].pc_fill;
  if (!any) return 0;
  const int64_t min_rows = pair_cache_min_rows();
  std::lock_guard<std::mutex> lk(C->mu);
  if (!C->block) return 0;
  const size_t budget = std::min(pair_cache_budget(), C->tab.capacity());
  PairFill f{};
  std::vector<int32_t> filled;
  // an error: the entries reserved here and not yet published go (PairTable::abort), so that their
  // keys can be filled again; their pins go with them
  auto give_up = [&](const char* what) {
    for (int32_t s : filled) {
      if (C->tab.at(s).published) continue;
      C->tab.abort(s);
      L->pc_pins.erase(std::find(L->pc_pins.begin(), L->pc_pins.end(), s));
    }
    return L->fail(YRWI_E_HIP, what);
  };
  for (size_t j = 0; j < jobs.size(); j++) {
    const JoinQ& J = jobs[j];
    Plan& P = plans[(size_t)owner[j]];
    if (!P.pc_fill || J.count_only || J.chained || !J.psum || !J.out_uid || !J.out_feat || J.out_tup ||
        mh[j] < min_rows)
      continue;
    P.pc_fill = false;
    const int64_t rows = mh[j];
    // (a key another lane filled meanwhile: the insert is dropped)
    const int32_t s = C->tab.insert(P.pc_key, rows, J.ntiles, pair_entry_bytes(rows, J.ntiles), budget);
    if (s < 0) continue;
    if ((size_t)s >= C->ev.size()) {
      C->ev.resize((size_t)s + 1, nullptr);
      C->ready.resize((size_t)s + 1, 0);
    }
    if (!C->ev[(size_t)s] && hipEventCreateWithFlags(&C->ev[(size_t)s], hipEventDisableTiming) != hipSuccess) {
      C->ev[(size_t)s] = nullptr;
      C->tab.abort(s);
      return give_up("pair cache event");
    }
    L->pc_pins.push_back(s);  // until this pass ends: the copy below is complete by then
    filled.push_back(s);
    C->ready[(size_t)s] = 0;
    uint8_t* base = C->block + C->tab.at(s).off;
    const size_t fb = (size_t)rows * FEAT_BYTES, ub = (size_t)rows * 4, pb = (size_t)J.ntiles * sizeof(ChunkSum);
    const uint8_t* src[3] = {reinterpret_cast<const uint8_t*>(J.out_feat), reinterpret_cast<const uint8_t*>(J.out_uid),
                             reinterpret_cast<const uint8_t*>(J.psum)};
    uint8_t* dst[3] = {base, base + al256(fb), base + al256(fb) + al256(ub)};
    const size_t nb[3] = {fb, ub, pb};
    if (f.n + 3 > PAIR_FILL_MAX) {
      if (launch_pair_fill(f, L->stream)) return give_up("pair cache fill launch");
      f = PairFill{};
    }
    for (int k = 0; k < 3; k++) {
      f.src[f.n] = src[k];
      f.dst[f.n] = dst[k];
      f.bytes[f.n] = nb[k];
      f.n++;
    }
  }
  if (f.n && launch_pair_fill(f, L->stream)) return give_up("pair cache fill launch");
  // visible to the other lanes only now, behind an event on this lane's stream
  for (int32_t s : filled) {
    if (hipEventRecord(C->ev[(size_t)s], L->stream) != hipSuccess) return give_up("pair cache event record");
    C->tab.publish(s);
  }
  return 0;
}

void yrwi::pair_cache_unpin(Lane* L) {
  if (L->pcache && !L->pc_pins.empty()) {
    std::lock_guard<std::mutex> lk(L->pcache->mu);
    for (int32_t s : L->pc_pins) L->pcache->tab.unpin(s);
  }
  L->pc_pins.clear();
}

extern "C" int yrwi_pair_cache_info_get(yrwi_ctx* ctx, yrwi_pair_cache_info* out) {
  if (!ctx || !out) return YRWI_E_ARG;
  std::memset(out, 0, sizeof(*out));
  PairCache& C = ctx->pcache;
  std::lock_guard<std::mutex> lk(C.mu);
  const PairCounters& c = C.tab.counters();
  out->enabled = !ctx->sharded && pair_cache_enabled() && C.block != nullptr ? 1 : 0;
  out->capacity_bytes = (int64_t)C.tab.capacity();
  out->budget_bytes = (int64_t)std::min(pair_cache_budget(), C.tab.capacity());
  out->min_rows = pair_cache_min_rows();
  out->entries = C.tab.entries();
  out->pieces = C.tab.pieces();
  out->bytes = (int64_t)C.tab.bytes_used();
  out->hits = c.hits;
  out->misses = c.misses;
  out->fills = c.fills;
  out->dropped = c.dropped;
  out->evictions = c.evictions;
  out->invalidations = c.invalidations;
  out->rows_served = c.rows_served;
  return 0;
}

static int run_batch_part_(const yrwi_ctx* ix, Lane* L, const yrwi_query_desc* q, int32_t nq, int32_t kmax,
                           yrwi_hit* out, uint8_t* rows, int32_t* nout, yrwi_stats* st);

// rows: the 40-byte row of every hit (stride kmax rows per query), or nullptr
static int run_batch_part(const yrwi_ctx* ix, Lane* L, const yrwi_query_desc* q, int32_t nq, int32_t kmax,
                          yrwi_hit* out, uint8_t* rows, int32_t* nout, yrwi_stats* st) {
  L->enter();
  const int64_t seq = L->seq;  // (passing the turn after the final collective clears L->seq)
  const int rc = run_batch_part_(ix, L, q, nq, kmax, out, rows, nout, st);
  if (rc && !L->pc_pins.empty()) (void)lane_sync(L);  // a failed pass: nothing of it reads a cached entry any more
  pair_cache_unpin(L);
  L->pcache = nullptr;
  // peers waiting on this part's exchanges fail fast; later parts are unaffected
  if (rc && L->hostx) hostx_abort(L->hostx, seq);
  turn_release(L);  // error paths, parts without collectives: the turn still passes in order
  L->release_after_final = false;
  L->leave();
  return rc;
}

static int run_batch_part_(const yrwi_ctx* ix, Lane* L, const yrwi_query_desc* q, int32_t nq, int32_t kmax,
                           yrwi_hit* out, uint8_t* rows, int32_t* nout, yrwi_stats* st) {
  const int64_t t0 = now_ns();
  const int64_t r0 = t_realloc;
  int64_t tp = 0, tj = 0, tr = 0, w0 = L->wait_ns, wj = 0;
  std::vector<Plan> all((size_t)nq);
  for (int i = 0; i < nq; i++) {
    int rc = plan_query(ix, L, q[i], &all[(size_t)i]);
    if (rc) return rc;
    if (st) st->postings_in += all[(size_t)i].postings_in;
  }
  // url selections: restricted list sizes first (J1/J2/J3 decide on them)
  if (int rc = resolve_selections(L, all)) return rc;
  // J1/J2 on global list sizes (one exchange of the batch's term sizes when sharded,
  // through this lane's arena and staging)
  if (L->sharded && begin_pass(L)) return YRWI_E_HIP;
  if (int rc = plan_batch(L, all)) return rc;
  // Identical queries of a pass run once (yrwi_share.h): group[i] names the part's earliest query
  // with query i's key; a pass's first member of a group represents its later ones.  Not on a
  // sharded context (the ranks resolve "now" apart, and the collectives count queries).
  const bool share = !L->sharded && share_enabled();
  std::vector<int32_t> group;
  if (share && share_groups(all, &group) == 0) group.clear();  // no repeats: nothing to look up
  for (size_t i = 0; i < group.size(); i++)
    if (group[i] < 0) group[i] = (int32_t)i;
  std::vector<int32_t> pass_rep(group.size(), -1);  // by group: its first member in the running pass
  tp = now_ns() - t0;
  const int64_t budget = scratch_budget(L);
  int npass = 0;
  for (int g0 = 0; g0 < nq;) {
    npass++;
    int g1 = g0;
    int64_t need = 0;
    while (g1 < nq) {
      // a repeat joins and ranks nothing: the floor of the estimate
      const bool repeat = !group.empty() && pass_rep[(size_t)group[(size_t)g1]] >= g0;
      const int64_t e = repeat ? 4096 : scratch_estimate(all[(size_t)g1]);
      if (g1 > g0 && need + e > budget) break;
      need += e;
      if (repeat) {
        all[(size_t)g1].rep = pass_rep[(size_t)group[(size_t)g1]] - g0;
        if (st) {
          st->queries_shared++;
          st->postings_shared += all[(size_t)g1].postings_in;
        }
      } else if (!group.empty()) {
        pass_rep[(size_t)group[(size_t)g1]] = g1;
      }
      g1++;
    }
    std::vector<Plan> plans(std::make_move_iterator(all.begin() + g0), std::make_move_iterator(all.begin() + g1));
    L->release_after_final = g1 >= nq;
    if (begin_pass(L)) return YRWI_E_HIP;
    // the pair cache serves query batches on one context (knobs read per pass)
    L->pcache = !L->sharded && pair_cache_enabled() ? &const_cast<yrwi_ctx*>(ix)->pcache : nullptr;
    // HIP events (per-kernel timing) only when the caller asked for statistics
    Timing tm;
    Timing* tmp = st ? &tm : nullptr;
    if (tmp) {
      tm.t0 = L->event();
      hipEventRecord(tm.t0, L->stream);
    }
    const int64_t tj0 = now_ns(), wj0 = L->wait_ns;
    int rc = run_join_phase(L, plans, st, tmp);
    if (rc) return rc;
    tj += now_ns() - tj0;
    wj += L->wait_ns - wj0;
    const int64_t tr0 = now_ns();
    if (tmp) {
      tm.tj = L->event();
      hipEventRecord(tm.tj, L->stream);
    }
    // (a pass's rows leave its arena here, before the next pass reuses it, at its queries' own positions)
    rc = run_rank_phase(L, plans, kmax, out + (size_t)g0 * kmax, nout + g0, nullptr, st, tmp, /*collective=*/true,
                        rows ? rows + (size_t)YRWI_ROW_BYTES * (size_t)g0 * kmax : nullptr);
    if (rc) return rc;
    pair_cache_unpin(L);  // the pass's results are complete (run_rank_phase waited for them)
    tr += now_ns() - tr0;
    if (st) {
      if (g1 < nq) HIPCHK(L, lane_sync(L));  // the pass's events must be complete before they are reused
      float ms = 0;
      for (auto& ev : tm.kjoin) {
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st->t_join_ns += (int64_t)(ms * 1e6);
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) {
          st->t_probe_ns += (int64_t)(ms * 1e6);
          st->t_probe_all_ns += (int64_t)(ms * 1e6);
        }
      }
      for (auto& ev : tm.kexcl)
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st->t_probe_all_ns += (int64_t)(ms * 1e6);
      for (auto& ev : tm.kcompact)
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st->t_compact_ns += (int64_t)(ms * 1e6);
      for (auto& ev : tm.spans)
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st->t_kernels_ns += (int64_t)(ms * 1e6);
      for (auto& ev : tm.kreduce)
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st->t_reduce_ns += (int64_t)(ms * 1e6);
      for (auto& ev : tm.kscore)
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st->t_scorek_ns += (int64_t)(ms * 1e6);
      for (auto& ev : tm.kchain)
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st->t_chain_ns += (int64_t)(ms * 1e6);
      if (tm.tn && hipEventElapsedTime(&ms, tm.tj, tm.tn) == hipSuccess) st->t_norm_ns += (int64_t)(ms * 1e6);
      if (tm.ts && tm.tn && hipEventElapsedTime(&ms, tm.tn, tm.ts) == hipSuccess) st->t_score_ns += (int64_t)(ms * 1e6);
      // a statistics event that could not be read is not the batch's error: it must
      // not linger as this thread's last HIP error (a later launch check reads it)
      (void)hipGetLastError();
    }
    g0 = g1;
  }
  // An arena that had to grow consolidates now, while this batch's caller still
  // waits for it, not at the start of the lane's next batch (one hipFree +
  // hipMalloc of the whole scratch costs milliseconds).
  if (L->arena.chunks.size() > 1) {
    HIPCHK(L, lane_sync(L));
    L->arena.reset();
    // busy lanes take this size at their next pass (begin_pass)
    size_t h = L->scratch_hint ? L->scratch_hint->load() : 0;
    while (L->scratch_hint && h < L->arena.capacity() &&
           !L->scratch_hint->compare_exchange_weak(h, L->arena.capacity())) {
    }
    // the lanes share one workload: idle lanes take the same size now, so their
    // first batch does not pay for growing (single-lane sharded contexts: none)
    for (Lane* o : ix->lanes)
      if (o != L) o->try_reserve(L->arena.capacity());
  }
  if (st) {
    st->t_total_ns = now_ns() - t0;
    st->n_realloc = (int32_t)(t_realloc - r0);
  }
  return 0;
}

static int check_batch_args(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax, yrwi_hit* out,
                            int32_t* nout) {
  if (!ctx || (nq > 0 && (!q || !out || !nout)) || nq < 0 || kmax < 1 || kmax > YRWI_MAX_K) return YRWI_E_ARG;
  return 0;
}

extern "C" int yrwi_settle_scratch(yrwi_ctx* ctx) {
  if (!ctx) return YRWI_E_ARG;
  hipSetDevice(ctx->device);
  drain(ctx);
  size_t a = ctx->scratch_hint.load(), s0 = 0, s1 = 0, s2 = 0;
  for (Lane* L : ctx->lanes) {
    a = std::max(a, L->arena.capacity());
    s0 = std::max(s0, L->stage.cap);
    s1 = std::max(s1, L->out_stage.cap);
    s2 = std::max(s2, L->down_stage.cap);
  }
  for (Lane* L : ctx->lanes) {
    L->arena.reserve(a);  // one chunk of the largest scratch any lane has needed
    if ((s0 && !stage_reserve(L, &L->stage, s0, true)) || (s1 && !stage_reserve(L, &L->out_stage, s1, true)) ||
        (s2 && !stage_reserve(L, &L->down_stage, s2, true)))
      return ctx->take(L, YRWI_E_HIP);
    if (a && L->arena.capacity() < a) return ctx->fail(YRWI_E_NOMEM, "scratch reservation");
  }
  ctx->scratch_hint = a;
  return 0;
}

// wait until no asynchronous batch is in flight (their statuses stay recorded)
void yrwi::drain(CtxBase* ctx) {
  for (Lane* L : ctx->lanes) L->wait();
}

int yrwi::select_lists(CtxBase* ctx, const uint8_t* terms12, int32_t nterms, bool sorted, ListSel* sel) {
  std::vector<KeyT> tks;
  std::unordered_set<KeyT, KeyHash> seen;
  for (int32_t i = 0; i < nterms; i++) {
    KeyT tk;
    if (!key_of(terms12 + (size_t)i * 12, &tk)) return ctx->fail(YRWI_E_HASH, "term hash is not well-formed Base64");
    if (seen.insert(tk).second) tks.push_back(tk);
  }
  hipSetDevice(ctx->device);
  drain(ctx);
  sel->clear();
  if (nterms == 0) {
    sel->reserve(ctx->lists.size());
    for (auto& kv : ctx->lists)
      if (kv.second.n > 0) sel->emplace_back(kv.first, &kv.second);
  } else {
    for (const KeyT& tk : tks) {
      auto it = ctx->lists.find(tk);
      if (it != ctx->lists.end() && it->second.n > 0) sel->emplace_back(tk, &it->second);
    }
  }
  if (sorted) std::sort(sel->begin(), sel->end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  return 0;
}

// an authority profile in the batch (ReferenceOrder.cardinal, coeff_authority > 12)
static bool wants_authority(const yrwi_query_desc* q, int32_t nq) {
  for (int32_t i = 0; i < nq; i++)
    if (q[i].profile && q[i].profile->coeff_authority > 12) return true;
  return false;
}

extern "C" int yrwi_query_batch(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax, yrwi_hit* out,
                                int32_t* nout, yrwi_stats* st) {
  return yrwi_query_batch_rows(ctx, q, nq, kmax, out, nullptr, nout, st);
}

extern "C" int yrwi_query_batch_rows(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax, yrwi_hit* out,
                                     uint8_t* rows, int32_t* nout, yrwi_stats* st) {
  if (int rc = check_batch_args(ctx, q, nq, kmax, out, nout)) return rc;
  if (nq == 0) {
    if (st) std::memset(st, 0, sizeof(*st));
    return 0;
  }
  hipSetDevice(ctx->device);
  drain(ctx);
  if (int rc = ensure_url_ids(ctx)) return rc;
  if (wants_authority(q, nq))
    if (int rc = ensure_host_ids(ctx)) return rc;
  const int64_t t0 = now_ns();
  // contiguous parts of equal query count, one per lane, each planned and run
  // by its lane's thread (every rank splits a sharded batch identically)
  const int nl = (int)std::min<int64_t>((int64_t)ctx->lanes.size(), nq);
  std::vector<yrwi_stats> pst((size_t)nl);
  for (auto& p : pst) std::memset(&p, 0, sizeof(p));
  auto cut = [&](int l) { return (int32_t)((int64_t)nq * l / nl); };
  const int64_t seq0 = ctx->coll_seq;  // collective order of the parts (CollTurn)
  ctx->coll_seq += nl;
  for (int l = 0; l < nl; l++) {
    ctx->lanes[(size_t)l]->seq = seq0 + l;
    ctx->lanes[(size_t)l]->xcall = 0;
    ctx->lanes[(size_t)l]->dcall = 0;
  }
  auto part = [=, &pst](int l) {
    Lane* L = ctx->lanes[(size_t)l];
    L->rc = run_batch_part(ctx, L, q + cut(l), cut(l + 1) - cut(l), kmax, out + (size_t)cut(l) * kmax,
                           rows ? rows + (size_t)YRWI_ROW_BYTES * (size_t)cut(l) * kmax : nullptr, nout + cut(l),
                           st ? &pst[(size_t)l] : nullptr);
  };
  for (int l = 1; l < nl; l++) ctx->lanes[(size_t)l]->submit([=] { part(l); });
  part(0);  // lane 0 on the calling thread (its worker is idle after drain)
  int rc = 0;
  for (int l = 0; l < nl; l++) {
    Lane* L = ctx->lanes[(size_t)l];
    if (l > 0) L->wait();
    if (L->rc && !rc) rc = ctx->take(L, L->rc);
  }
  if (rc) return rc;
  if (st) {
    std::memset(st, 0, sizeof(*st));
    for (const yrwi_stats& p : pst) {
      st->postings_in += p.postings_in;
      st->joined += p.joined;
      st->bytes_alg += p.bytes_alg;
      st->bytes_join += p.bytes_join;
      st->bytes_probe += p.bytes_probe;
      st->bytes_probe_loaded += p.bytes_probe_loaded;
      st->bytes_probe_capped += p.bytes_probe_capped;
      st->bytes_features += p.bytes_features;
      st->bytes_join_capped += p.bytes_join_capped;
      st->bytes_alg_capped += p.bytes_alg_capped;
      st->t_join_ns += p.t_join_ns;
      st->t_probe_ns += p.t_probe_ns;
      st->bytes_compact += p.bytes_compact;
      st->t_compact_ns += p.t_compact_ns;
      st->t_kernels_ns += p.t_kernels_ns;
      st->t_norm_ns += p.t_norm_ns;
      st->t_score_ns += p.t_score_ns;
      st->n_join_launches += p.n_join_launches;
      st->n_enum_steps += p.n_enum_steps;
      st->n_test_steps += p.n_test_steps;
      st->n_realloc += p.n_realloc;
      st->n_probe_dispatches += p.n_probe_dispatches;
      st->t_probe_all_ns += p.t_probe_all_ns;
      st->n_rank_passes += p.n_rank_passes;
      st->t_reduce_ns += p.t_reduce_ns;
      st->t_scorek_ns += p.t_scorek_ns;
      st->bytes_reduce += p.bytes_reduce;
      st->bytes_score += p.bytes_score;
      st->n_chain_launches += p.n_chain_launches;
      st->t_chain_ns += p.t_chain_ns;
      st->bytes_chain += p.bytes_chain;
      st->queries_shared += p.queries_shared;
      st->postings_shared += p.postings_shared;
      st->joined_shared += p.joined_shared;
    }
    st->t_total_ns = now_ns() - t0;
  }
  return 0;
}

extern "C" int yrwi_query_batch_submit(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax,
                                       yrwi_hit* out, int32_t* nout, yrwi_stats* st, int64_t* ticket) {
  return yrwi_query_batch_rows_submit(ctx, q, nq, kmax, out, nullptr, nout, st, ticket);
}

extern "C" int yrwi_query_batch_rows_submit(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax,
                                            yrwi_hit* out, uint8_t* rows, int32_t* nout, yrwi_stats* st,
                                            int64_t* ticket) {
  if (int rc = check_batch_args(ctx, q, nq, kmax, out, nout)) return rc;
  if (!ticket) return YRWI_E_ARG;
  hipSetDevice(ctx->device);
  if (ctx->uid_dirty) {  // the index changed: nothing can be in flight (put_list drained)
    drain(ctx);
    if (int rc = ensure_url_ids(ctx)) return rc;
  }
  if (!ctx->host_ids && wants_authority(q, nq)) {  // the first authority batch since the index changed
    drain(ctx);
    if (int rc = ensure_host_ids(ctx)) return rc;
  }
  const int64_t t = ctx->next_ticket;
  Lane* L = ctx->lanes[(size_t)(t % (int64_t)ctx->lanes.size())];
  L->wait();  // the lane's previous batch (its status is already recorded)
  ctx->next_ticket++;
  L->seq = ctx->coll_seq++;  // collective order (CollTurn): submission order, the same on every rank
  L->xcall = 0;
  L->dcall = 0;
  L->submit([=] {
    if (st) std::memset(st, 0, sizeof(*st));
    const int rc = nq == 0 ? 0 : run_batch_part(ctx, L, q, nq, kmax, out, rows, nout, st);
    turn_release(L);  // nq == 0: nothing ran, the turn passes all the same
    {
      std::lock_guard<std::mutex> lk(ctx->st_mu);
      ctx->status[t] = {rc, rc ? L->err : std::string()};
    }
    L->done = t;
  });
  *ticket = t;
  return 0;
}

extern "C" int yrwi_query_batch_wait(yrwi_ctx* ctx, int64_t ticket) {
  if (!ctx || ticket < 0 || ticket >= ctx->next_ticket) return YRWI_E_ARG;
  Lane* L = ctx->lanes[(size_t)(ticket % (int64_t)ctx->lanes.size())];
  L->wait();  // a lane runs its tickets in order; the next one is not submitted before this returns
  std::lock_guard<std::mutex> lk(ctx->st_mu);
  auto it = ctx->status.find(ticket);
  if (it == ctx->status.end()) return ctx->fail(YRWI_E_ARG, "unknown or already collected ticket");
  const int rc = it->second.first;
  if (rc) ctx->err = it->second.second;
  ctx->status.erase(it);
  return rc;
}

extern "C" int yrwi_host_alloc(yrwi_ctx* ctx, size_t bytes, void** p) {
  if (!ctx || !p || bytes == 0) return YRWI_E_ARG;
  hipSetDevice(ctx->device);
  void* h = nullptr;
  if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) return ctx->fail(YRWI_E_NOMEM, "hipHostMalloc");
  std::lock_guard<std::mutex> lk(ctx->hostreg.mu);
  ctx->hostreg.bufs.push_back({static_cast<uint8_t*>(h), bytes});
  *p = h;
  return 0;
}

extern "C" int yrwi_host_free(yrwi_ctx* ctx, void* p) {
  if (!ctx || !p) return YRWI_E_ARG;
  drain(ctx);
  std::lock_guard<std::mutex> lk(ctx->hostreg.mu);
  auto& v = ctx->hostreg.bufs;
  for (size_t i = 0; i < v.size(); i++)
    if (v[i].first == p) {
      hipHostFree(p);
      v.erase(v.begin() + (long)i);
      return 0;
    }
  return ctx->fail(YRWI_E_ARG, "not a yrwi_host_alloc buffer");
}

extern "C" int yrwi_query(yrwi_ctx* ctx, const yrwi_query_desc* q, yrwi_hit* out, int32_t* nout, yrwi_stats* st) {
  if (!q) return YRWI_E_ARG;
  int32_t kmax = std::max<int32_t>(1, std::min<int32_t>(q->k, YRWI_MAX_K));
  return yrwi_query_batch(ctx, q, 1, kmax, out, nout, st);
}

extern "C" int yrwi_query_rows(yrwi_ctx* ctx, const yrwi_query_desc* q, yrwi_hit* out, uint8_t* rows, int32_t* nout,
                               yrwi_stats* st) {
  if (!q) return YRWI_E_ARG;
  int32_t kmax = std::max<int32_t>(1, std::min<int32_t>(q->k, YRWI_MAX_K));
  return yrwi_query_batch_rows(ctx, q, 1, kmax, out, rows, nout, st);
}

extern "C" int yrwi_score_nodes(yrwi_ctx* ctx, const yrwi_node* nodes, int64_t n, const yrwi_profile* prof,
                                const char* language, int32_t maxdomcount, int64_t* scores) {
  if (!ctx || n < 0 || (n > 0 && (!nodes || !scores))) return YRWI_E_ARG;
  if (n == 0) return 0;
  hipSetDevice(ctx->device);
  drain(ctx);
  Lane* L = ctx->lanes[0];
  if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
  yrwi_profile p;
  if (prof) p = *prof; else yrwi_profile_default(&p);
  char lang[8] = {0};
  if (language) std::strncpy(lang, language, 7);  // ReferenceOrder.language (a String; longer never equals)
  if (language && std::strlen(language) > 7) std::memset(lang, 0xFF, 7);
  yrwi_node* d_nodes = arena_alloc<yrwi_node>(L, n);
  yrwi_profile* d_prof = arena_alloc<yrwi_profile>(L, 1);
  int64_t* d_sc = arena_alloc<int64_t>(L, n);
  if (!d_nodes || !d_prof || !d_sc) return ctx->fail(YRWI_E_NOMEM, "arena");
  HIPCHK(ctx, hipMemcpyAsync(d_nodes, nodes, sizeof(yrwi_node) * (size_t)n, hipMemcpyHostToDevice, L->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_prof, &p, sizeof(p), hipMemcpyHostToDevice, L->stream));
  if (launch_score_nodes(d_nodes, n, d_prof, lang, maxdomcount, d_sc, L->stream))
    return ctx->fail(YRWI_E_HIP, "score_nodes launch");
  HIPCHK(ctx, hipMemcpyAsync(scores, d_sc, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, L->stream));
  HIPCHK(ctx, lane_sync(L));
  return 0;
}

extern "C" int yrwi_join_exclude(yrwi_ctx* ctx, const uint8_t* incl, int32_t nincl, const uint8_t* excl,
                                 int32_t nexcl, int32_t max_distance, int64_t now_ms, uint8_t* rows_out,
                                 int64_t cap_rows, int64_t* m) {
  yrwi_query_desc d{};
  d.incl = incl;
  d.nincl = nincl;
  d.excl = excl;
  d.nexcl = nexcl;
  d.max_distance = max_distance;
  d.k = 1;
  d.now_ms = now_ms;
  return yrwi_term_search(ctx, &d, rows_out, cap_rows, m);
}

extern "C" int yrwi_term_search(yrwi_ctx* ctx, const yrwi_query_desc* q, uint8_t* rows_out, int64_t cap_rows,
                                int64_t* m) {
  if (!ctx || !m || !q) return YRWI_E_ARG;
  *m = 0;
  hipSetDevice(ctx->device);
  yrwi_query_desc d = *q;
  d.k = 1;
  d.filter = nullptr;
  drain(ctx);
  if (int rc0 = ensure_url_ids(ctx)) return rc0;
  Lane* L = ctx->lanes[0];
  std::vector<Plan> plans(1);
  int rc = ctx->take(L, plan_query(ctx, L, d, &plans[0]));
  if (rc) return rc;
  if ((rc = ctx->take(L, resolve_selections(L, plans)))) return rc;
  if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
  if ((rc = ctx->take(L, plan_batch(L, plans)))) return rc;
  rc = ctx->take(L, run_join_phase(L, plans, nullptr, nullptr));
  if (rc) return rc;
  const Plan& P = plans[0];
  if (P.empty || P.cont.n == 0) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
  }
  std::vector<uint8_t> rows((size_t)P.cont.n * 40), rem;
  const uint8_t* src = P.cont.rows;  // a single include list is returned as it is stored (:355-370)
  if (!src) {  // a joined container: its rows as toRowEntry re-encodes them (J6)
    uint8_t* d_rows = arena_alloc<uint8_t>(L, P.cont.n * 40);
    if (!d_rows) return ctx->fail(YRWI_E_NOMEM, "arena");
    if (launch_feat_rows(P.cont.feat, P.cont.uid, ctx->dkhi, ctx->dklo, P.cont.n, plans[0].now_ms, d_rows, L->stream))
      return ctx->fail(YRWI_E_HIP, "row launch");
    src = d_rows;
  }
  HIPCHK(ctx, hipMemcpyAsync(rows.data(), src, rows.size(), hipMemcpyDeviceToHost, ctx->stream));
  if (P.removed) {
    rem.resize((size_t)P.cont.n);
    HIPCHK(ctx, hipMemcpyAsync(rem.data(), P.removed, rem.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int64_t k = 0;
  for (int64_t i = 0; i < P.cont.n; i++) {
    if (!rem.empty() && rem[(size_t)i]) continue;
    if (k >= cap_rows) return ctx->fail(YRWI_E_ARG, "rows_out capacity too small");
    std::memcpy(rows_out + k * 40, rows.data() + i * 40, 40);
    k++;
  }
  *m = k;
  return 0;
}

int yrwi::join_containers(yrwi_ctx* ctx, Lane* L, const yrwi_query_desc* const* q, int32_t nq,
                          std::vector<Plan>* plans_out) {
  if (int rc0 = ensure_url_ids(ctx)) return rc0;
  std::vector<Plan>& plans = *plans_out;
  plans.assign((size_t)nq, Plan());
  L->err_query = -1;
  for (int32_t i = 0; i < nq; i++) {
    yrwi_query_desc d = *q[i];
    d.k = 1;
    d.filter = nullptr;
    L->err_query = i;
    if (int rc = ctx->take(L, plan_query(ctx, L, d, &plans[(size_t)i]))) return rc;
  }
  L->err_query = -1;
  int rc;
  if ((rc = ctx->take(L, resolve_selections(L, plans)))) return rc;
  if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
  if ((rc = ctx->take(L, plan_batch(L, plans)))) return rc;
  return ctx->take(L, run_join_phase(L, plans, nullptr, nullptr));
}

extern "C" int yrwi_normalize_score(yrwi_ctx* ctx, const uint8_t* rows40, int64_t m, const yrwi_profile* prof,
                                    const char* language, int64_t now_ms, int64_t* score_out) {
  if (!ctx || (m > 0 && (!rows40 || !score_out))) return YRWI_E_ARG;
  if (m <= 0) return 0;
  if (m > MAX_LIST) return ctx->fail(YRWI_E_LIMIT, "container longer than 53,687,091 rows");
  hipSetDevice(ctx->device);
  drain(ctx);
  Lane* L = ctx->lanes[0];
  if (begin_pass(L)) return ctx->take(L, YRWI_E_HIP);
  uint8_t* rows = arena_alloc<uint8_t>(L, m * 40);
  uint64_t* khi = arena_alloc<uint64_t>(L, m);
  uint8_t* klo = arena_alloc<uint8_t>(L, m);
  int32_t* derr = arena_alloc<int32_t>(L, 1);
  if (!rows || !khi || !klo || !derr) return ctx->fail(YRWI_E_NOMEM, "arena");
  HIPCHK(ctx, hipMemcpyAsync(rows, rows40, (size_t)m * 40, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(derr, 0, 4, ctx->stream));
  if (launch_validate_rows(rows, m, khi, klo, derr, ctx->stream)) return ctx->fail(YRWI_E_HIP, "validate launch");
  int32_t herr = 0;
  HIPCHK(ctx, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (herr & 1) return ctx->fail(YRWI_E_HASH, "url hash is not well-formed Base64");
  if (herr & 2) return ctx->fail(YRWI_E_NULL_LANGUAGE, "row with empty language cell (reference NPE)");
  if (herr & 4) return ctx->fail(YRWI_E_UNSORTED, "container rows are not strictly ascending by url hash");
  std::vector<Plan> plans(1);
  Plan& P = plans[0];
  P.empty = false;
  uint64_t* feat = arena_alloc<uint64_t>(L, m * FEAT_WORDS);
  if (!feat) return ctx->fail(YRWI_E_NOMEM, "arena");
  if (launch_features(rows, m, feat, ctx->stream)) return ctx->fail(YRWI_E_HIP, "features launch");
  P.cont = DList{khi, klo, rows, m, nullptr, feat};
  P.removed = nullptr;
  if (prof) P.prof = *prof; else yrwi_profile_default(&P.prof);
  size_t ll = language ? strnlen(language, 8) : 0;
  P.lang_ok = ll == 2;
  P.lang[0] = ll > 0 ? (uint8_t)language[0] : 0;
  P.lang[1] = ll > 1 ? (uint8_t)language[1] : 0;
  P.now_ms = now_ms != 0 ? now_ms
                         : (int64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
                               std::chrono::system_clock::now().time_since_epoch()).count();
  P.k = 1;
  return ctx->take(L, run_rank_phase(L, plans, 1, nullptr, nullptr, score_out, nullptr, nullptr, /*collective=*/false,
                                     nullptr));
}
