// yrwi_rank.cpp -- the rank phase of a batch part (run_rank_phase): the joined
// containers' normalisation (with the cross-shard exchanges), then either every
// element's score (yrwi_normalize_score) or score + top-k, the hits' way into the
// caller's buffers and their rows.  Planning, batching and the C entry points are
// in yrwi_host.cpp, the join phase in yrwi_join.cpp.

#include "yrwi_host.h"

using namespace yrwi;

// What the steps of one rank pass share on the host.
struct RankPass {
  Lane* ctx;
  std::vector<Plan>& plans;
  yrwi_stats* st;
  Timing* tm;
  int nq;
  int W;     // shards whose summaries are combined (1: the pass is not collective)
  bool shx;  // the url-hash-shard protocol
  std::vector<RankQ> rq;
  std::vector<int64_t> chunk_base, slot_base;  // every query's first chunk, first authority host-table slot
  int64_t chunks = 0, nslots = 0;
  bool any_auth = false, any_dd = false;
  uint64_t* d_hkeys = nullptr;  // authority host tables of all queries (nslots)
  uint32_t* d_hcnt = nullptr;
  std::vector<int> fidx;  // every query's FilterQ (-1: none) among the pass's nf
  int nf = 0;
  int32_t* d_flag = nullptr;  // 32 flag counters per FilterQ (nullptr: no query counts flags)
  int32_t keff = 1;           // the largest k of the pass: the stride of the top-k passes' lists
  int32_t* d_zero = nullptr;  // d_zero[0]: a zero count (queries without chunks); d_zero[1]: k_score's redo count
  RankStep S;

  RankPass(Lane* L, std::vector<Plan>& p, yrwi_stats* s, Timing* t, bool collective)
      : ctx(L), plans(p), st(s), tm(t), nq((int)p.size()), W(collective ? L->world : 1),
        shx(collective && L->sharded), rq(p.size()), chunk_base(p.size()), slot_base(p.size() + 1),
        fidx(p.size(), -1) {}
};

// Where the hits of a pass go.  Results go straight into pinned host memory -- the
// caller's buffer when it came from yrwi_host_alloc, else this lane's landing buffer
// (then copied out per query).  One GPU: k_emit writes them (doubledom queries:
// their stacks, ordered by k_pull).  Sharded: every shard's stack is gathered, merged
// on the device (k_gmerge_*) and pulled (k_pull); every rank ends with the same lists.
struct RankDest {
  yrwi_hit* h_hits;
  int32_t* h_nout;
  uint8_t* h_rows;  // the hits' rows (yrwi_query_*_rows) or nullptr
  int32_t kmax;
  int32_t kint = 0;  // stack stride
  size_t hb = 0, hb_al = 0, nb = 0, land_rows = 0;  // hit and count bytes; the rows' offset in the landing buffer
  bool direct = false, rows_direct = false;         // the caller's buffers are pinned: written in place
  uint8_t* land = nullptr;
  HitList out;     // device address of the pinned destination (stride kmax)
  uint8_t* d_rows = nullptr;
  HitList pulled;  // what k_pull writes: `out`, or with rows device memory that k_hit_rows reads and forwards
  HitRowQ* d_hq = nullptr;
  const uint8_t* hD_land = nullptr;  // sharded: max-distance fold state per query (overflow check)
};

// The RankQ of every query, the chunk and host-table layout, the containers' statistics.
static void build_queries(RankPass& R) {
  Lane* ctx = R.ctx;
  for (int qi = 0; qi < R.nq; qi++) {
    Plan& P = R.plans[(size_t)qi];
    RankQ& Q = R.rq[(size_t)qi];
    std::memset(&Q, 0, sizeof(Q));
    if (P.rep >= 0) {
      // A repeat of an earlier query of the pass: no chunks, no pieces, no host table -- it is not
      // normalised, scored or selected.  Its RankQ names the representative's container (key_at),
      // upload_final gives it the representative's final list and rows, and k_emit / k_hit_rows
      // write its own slots of the results.
      const RankQ& Rq = R.rq[(size_t)P.rep];
      Q.feat = Rq.feat;
      Q.uid = Rq.uid;
      Q.ekhi = Rq.ekhi;
      Q.eklo = Rq.eklo;
      Q.dkhi = Rq.dkhi;
      Q.dklo = Rq.dklo;
      Q.removed = Rq.removed;
      Q.n = Rq.n;
      Q.chunk_base = R.chunks;
      R.chunk_base[(size_t)qi] = R.chunks;
      Q.prof = Rq.prof;
      Q.lang[0] = Rq.lang[0];
      Q.lang[1] = Rq.lang[1];
      Q.lang_ok = Rq.lang_ok;
      Q.now_ms = Rq.now_ms;
      Q.k = Rq.k;
      Q.kout = Rq.kout;
      Q.host_rec = Rq.host_rec;
      R.slot_base[(size_t)qi] = R.nslots;
      if (R.st) {  // per-query meaning: the rows of its result; no bytes, nobody read them again
        R.st->joined += Q.n;
        R.st->joined_shared += Q.n;
      }
      continue;
    }
    Q.feat = P.cont.feat;
    Q.uid = P.cont.uid;
    Q.ekhi = P.cont.uid ? nullptr : P.cont.khi;
    Q.eklo = P.cont.uid ? nullptr : P.cont.klo;
    Q.dkhi = ctx->dkhi;
    Q.dklo = ctx->dklo;
    Q.removed = P.removed;
    Q.n = P.empty ? 0 : P.cont.n;
    Q.pieces = P.empty || P.removed ? nullptr : P.pieces;
    Q.npieces = Q.pieces ? P.npieces : 0;
    Q.ngroups = ceil_div(Q.npieces, 64);
    Q.nchunks = ceil_div(Q.n, CHUNK);
    Q.chunk_base = R.chunks;
    R.chunk_base[(size_t)qi] = R.chunks;
    R.chunks += Q.nchunks;
    Q.prof = P.prof;
    Q.lang[0] = P.lang[0];
    Q.lang[1] = P.lang[1];
    Q.lang_ok = P.lang_ok;
    Q.now_ms = P.now_ms;
    Q.k = P.k;
    Q.want_authority = P.prof.coeff_authority > 12 && Q.n > 0;
    Q.idx_tag = R.shx ? (uint32_t)ctx->rank << 28 : 0u;
    Q.doubledom = P.filter && P.filter->skip_double_dom ? 1 : 0;
    Q.host_rec = ctx->host_ids && P.cont.uid != nullptr ? 1 : 0;  // index records: dense host ids
    Q.kout = P.k;
    if (Q.doubledom) Q.k = YRWI_MAX_K;  // pullOneRWI draws from the whole rwiStack (max_results_rwi)
    if (Q.doubledom) R.any_dd = true;
    // identical on every rank (same queries): decides the collective host-count exchange
    if (P.prof.coeff_authority > 12) R.any_auth = true;
    R.slot_base[(size_t)qi] = R.nslots;
    if (Q.want_authority) {
      uint64_t cap = 1;
      while (cap < (uint64_t)(2 * Q.n)) cap <<= 1;
      Q.hmask = cap - 1;
      R.nslots += (int64_t)cap;
    }
    R.keff = std::max(R.keff, Q.k);
    if (R.st) {
      R.st->joined += Q.n;
      R.st->bytes_alg += 23 * (int64_t)P.seq.size() * Q.n;  // ranking feature bytes per surviving posting and term
      R.st->bytes_features += 23 * (int64_t)P.seq.size() * Q.n;
      R.st->bytes_alg_capped += 23 * (int64_t)P.seq.size() * Q.n;
    }
  }
  R.slot_base[(size_t)R.nq] = R.nslots;
}

// authority host tables of all queries, one allocation
static int alloc_host_tables(RankPass& R) {
  Lane* ctx = R.ctx;
  if (R.nslots <= 0) return 0;
  R.d_hkeys = arena_alloc<uint64_t>(ctx, R.nslots);
  R.d_hcnt = arena_alloc<uint32_t>(ctx, R.nslots);
  if (!R.d_hkeys || !R.d_hcnt) return ctx->fail(YRWI_E_NOMEM, "arena");
  HIPCHK(ctx, hipMemsetAsync(R.d_hkeys, 0, (size_t)R.nslots * 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(R.d_hcnt, 0, (size_t)R.nslots * 4, ctx->stream));
  for (int qi = 0; qi < R.nq; qi++) {
    RankQ& Q = R.rq[(size_t)qi];
    if (!Q.want_authority) continue;
    Q.hkeys = R.d_hkeys + R.slot_base[(size_t)qi];
    Q.hcnt = R.d_hcnt + R.slot_base[(size_t)qi];
  }
  return 0;
}

// authority by partition (RankQ::ecnt; one context, records with host ids): each
// query's hosts hashed into ~HPART_TARGET-element buckets, per-element counts
static int plan_host_part(RankPass& R) {
  Lane* ctx = R.ctx;
  RankStep& S = R.S;
  int64_t hp_hist = 0, hp_elems = 0, hp_buckets = 0;
  std::vector<int2> bq;
  const char* hpm = getenv("YRWI_HPART_MAXB");  // (tests: fewer buckets, so large queries overflow the LDS tables)
  const int64_t maxb = hpm ? std::max(1, std::min(HPART_MAXS, atoi(hpm))) : HPART_MAXS;
  for (int qi = 0; qi < R.nq; qi++) {
    RankQ& Q = R.rq[(size_t)qi];
    if (!Q.want_authority || !Q.host_rec || R.shx) continue;
    Q.hp_nb = (int32_t)std::min<int64_t>(maxb, std::max<int64_t>(1, ceil_div(Q.n, HPART_TARGET)));
    Q.hp_hoff = hp_hist;
    hp_hist += Q.nchunks * Q.hp_nb;
    for (int32_t s = 0; s < Q.hp_nb; s++) bq.push_back(make_int2(qi, s));
    hp_buckets += Q.hp_nb;
  }
  if (hp_buckets == 0) return 0;
  for (const RankQ& Q : R.rq)
    if (Q.hp_nb) hp_elems += Q.n;
  S.hp_any = true;
  S.nhist = hp_hist;
  S.nbuckets = (int32_t)hp_buckets;
  S.tmp_bytes = host_part_tmp_bytes(hp_hist);
  S.d_hist = arena_alloc<int32_t>(ctx, hp_hist + 1);
  S.d_hoffs = arena_alloc<int32_t>(ctx, hp_hist + 1);
  int32_t* d_ecnt = arena_alloc<int32_t>(ctx, hp_elems);
  S.d_part = arena_alloc<uint2>(ctx, hp_elems);
  int2* d_bq = arena_alloc<int2>(ctx, hp_buckets);
  S.d_tmp = arena_alloc<uint8_t>(ctx, (int64_t)std::max<size_t>(S.tmp_bytes, 1));
  if (!S.d_hist || !S.d_hoffs || !d_ecnt || !S.d_part || !d_bq || !S.d_tmp) return ctx->fail(YRWI_E_NOMEM, "arena");
  S.d_bq = d_bq;
  HIPCHK(ctx, hipMemsetAsync(S.d_hist + hp_hist, 0, 4, ctx->stream));  // the scan's extra entry: the total
  int64_t eb = 0;
  for (RankQ& Q : R.rq) {
    if (!Q.hp_nb) continue;
    Q.ecnt = d_ecnt + eb;
    Q.hp_hist = S.d_hist;
    eb += Q.n;
  }
  return upload(ctx, d_bq, bq) ? YRWI_E_HIP : 0;
}

// addRWIs constraints: one FilterQ per filtered query, key arrays and flag counters
static int upload_filters(RankPass& R) {
  Lane* ctx = R.ctx;
  const int nq = R.nq;
  bool any_flagcount = false;
  for (int qi = 0; qi < nq; qi++) {
    if (R.plans[(size_t)qi].filter) R.fidx[(size_t)qi] = R.nf++;
    if (R.plans[(size_t)qi].filter && R.plans[(size_t)qi].filter->flagcount) any_flagcount = true;
  }
  const int nf = R.nf;
  if (nf == 0) return 0;
  std::vector<FilterQ> fq((size_t)nf);
  std::vector<uint64_t> sx, uh;
  std::vector<uint8_t> ul;
  std::vector<int64_t> sx0((size_t)nf), uh0((size_t)nf);
  for (int qi = 0; qi < nq; qi++) {
    const int f = R.fidx[(size_t)qi];
    if (f < 0) continue;
    std::vector<uint64_t> v;
    std::vector<KeyT> u;
    build_filterq(*R.plans[(size_t)qi].filter, &fq[(size_t)f], &v, &u);
    sx0[(size_t)f] = (int64_t)sx.size();
    sx.insert(sx.end(), v.begin(), v.end());
    uh0[(size_t)f] = (int64_t)uh.size();
    for (auto& k : u) { uh.push_back(k.hi); ul.push_back((uint8_t)k.lo); }
  }
  FilterQ* d_fq = arena_alloc<FilterQ>(ctx, nf);
  uint64_t* d_sx = arena_alloc<uint64_t>(ctx, (int64_t)sx.size());
  uint64_t* d_uh = arena_alloc<uint64_t>(ctx, (int64_t)uh.size());
  uint8_t* d_ul = arena_alloc<uint8_t>(ctx, (int64_t)ul.size());
  R.d_flag = any_flagcount ? arena_alloc<int32_t>(ctx, (int64_t)nf * 32) : nullptr;
  if (!d_fq || !d_sx || !d_uh || !d_ul || (any_flagcount && !R.d_flag)) return ctx->fail(YRWI_E_NOMEM, "arena");
  if (R.d_flag) HIPCHK(ctx, hipMemsetAsync(R.d_flag, 0, (size_t)nf * 32 * 4, ctx->stream));
  for (int qi = 0; qi < nq; qi++) {
    const int f = R.fidx[(size_t)qi];
    if (f < 0) continue;
    FilterQ& G = fq[(size_t)f];
    G.siteex = d_sx + sx0[(size_t)f];
    G.url_hi = d_uh + uh0[(size_t)f];
    G.url_lo = d_ul + uh0[(size_t)f];
    G.flagcount = R.plans[(size_t)qi].filter->flagcount ? R.d_flag + (int64_t)f * 32 : nullptr;
    R.rq[(size_t)qi].filt = d_fq + f;
  }
  return upload(ctx, d_fq, fq, d_sx, sx, d_uh, uh, d_ul, ul) ? YRWI_E_HIP : 0;
}

// flag counters back to the callers' filters (summed over the shards)
static int flagcounts_out(RankPass& R) {
  Lane* ctx = R.ctx;
  if (!R.d_flag) return 0;
  if (R.shx)
    if (int rc = coll_allreduce_i32(ctx, R.d_flag, (size_t)R.nf * 32, false)) return rc;
  const uint8_t* hf = readback(ctx, &ctx->down_stage, R.d_flag, (int64_t)R.nf * 32, 4, 4);
  if (!hf) return YRWI_E_HIP;
  HIPCHK(ctx, lane_sync(ctx));
  for (int qi = 0; qi < R.nq; qi++)
    if (R.fidx[(size_t)qi] >= 0 && R.plans[(size_t)qi].filter->flagcount)
      std::memcpy(R.plans[(size_t)qi].filter->flagcount, hf + (size_t)R.fidx[(size_t)qi] * 32 * 4, 32 * 4);
  return 0;
}

// The summaries' buffers and the groups of the compaction's pieces; the query table,
// complete by now, goes up with the chunk tables in one copy.
static int upload_queries(RankPass& R) {
  Lane* ctx = R.ctx;
  RankStep& S = R.S;
  const int nq = R.nq;
  RankQ* d_q = arena_alloc<RankQ>(ctx, nq);
  int64_t* d_cb = arena_alloc<int64_t>(ctx, nq);
  S.d_chunks = arena_alloc<ChunkSum>(ctx, R.chunks);
  S.d_shard = arena_alloc<ShardSum>(ctx, nq);
  S.d_all = R.shx ? arena_alloc<ShardSum>(ctx, (int64_t)nq * R.W) : S.d_shard;
  S.d_norm = arena_alloc<NormState>(ctx, nq);
  if (!d_q || !d_cb || !S.d_chunks || !S.d_shard || !S.d_all || !S.d_norm) return ctx->fail(YRWI_E_NOMEM, "arena");
  std::vector<int32_t> chunk_q((size_t)R.chunks);
  for (int qi = 0; qi < nq; qi++)
    for (int64_t c = 0; c < R.rq[(size_t)qi].nchunks; c++) chunk_q[(size_t)(R.chunk_base[(size_t)qi] + c)] = qi;
  int32_t* d_cq = arena_alloc<int32_t>(ctx, R.chunks);
  if (!d_cq) return ctx->fail(YRWI_E_NOMEM, "arena");
  // groups of the compaction's pieces (k_piece_merge): (query, group) of each
  std::vector<int2> group_q;
  for (int qi = 0; qi < nq; qi++)
    for (int64_t g = 0; g < R.rq[(size_t)qi].ngroups; g++) group_q.push_back(make_int2(qi, (int32_t)g));
  if (!group_q.empty()) {
    ChunkSum* d_groups = arena_alloc<ChunkSum>(ctx, (int64_t)group_q.size());
    int2* d_gq = arena_alloc<int2>(ctx, (int64_t)group_q.size());
    if (!d_groups || !d_gq) return ctx->fail(YRWI_E_NOMEM, "arena");
    int64_t gb = 0;
    for (RankQ& Q : R.rq) {
      Q.groups = Q.ngroups ? d_groups + gb : nullptr;
      gb += Q.ngroups;
    }
    if (upload(ctx, d_gq, group_q)) return YRWI_E_HIP;
    S.d_group_q = d_gq;
  }
  if (upload(ctx, d_q, R.rq, d_cb, R.chunk_base, d_cq, chunk_q)) return YRWI_E_HIP;
  HIPCHK(ctx, hipMemsetAsync(S.d_shard, 0, sizeof(ShardSum) * nq, ctx->stream));
  S.d_q = d_q;
  S.d_chunk_base = d_cb;
  S.d_chunk_q = d_cq;
  S.nq = nq;
  S.chunks = R.chunks;
  S.world = R.W;
  S.ngroups = (int64_t)group_q.size();
  for (const RankQ& Q : R.rq) S.reduce |= !Q.pieces && Q.nchunks > 0;  // a query without the compaction's pieces
  return 0;
}

// Global host counts for authority (ReferenceOrder.java:176-216) across url-hash
// shards: (query, host, count) messages to the host's owner rank, summed there,
// totals sent back; the per-query max count is all-reduced.  Collective.
static int exchange_host_counts(const RankPass& R) {
  Lane* ctx = R.ctx;
  const int nq = R.nq;
  const int64_t nslots = R.nslots;
  uint64_t* d_hkeys = R.d_hkeys;
  uint32_t* d_hcnt = R.d_hcnt;
  const int W = ctx->world, me = ctx->rank;
  uint32_t* d_ocnt = arena_alloc<uint32_t>(ctx, W);
  uint32_t* d_M = arena_alloc<uint32_t>(ctx, (int64_t)W * W);
  int64_t* d_sb = arena_alloc<int64_t>(ctx, nq + 1);
  int32_t* d_gmax = arena_alloc<int32_t>(ctx, nq);
  if (!d_ocnt || !d_M || !d_sb || !d_gmax) return ctx->fail(YRWI_E_NOMEM, "arena");
  HIPCHK(ctx, hipMemsetAsync(d_ocnt, 0, W * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_gmax, 0, nq * 4, ctx->stream));
  if (upload(ctx, d_sb, R.slot_base)) return YRWI_E_HIP;
  const uint64_t* hkey = ctx->host_ids ? ctx->host_key : nullptr;  // tables of dense host ids (build_queries)
  if (launch_host_count(d_hkeys, nslots, W, d_ocnt, ctx->stream, hkey)) return ctx->fail(YRWI_E_HIP, "host count");
  if (int rc = coll_allgather(ctx, d_ocnt, d_M, (size_t)W * 4)) return rc;
  const uint8_t* hm = readback(ctx, &ctx->down_stage, d_M, (int64_t)W * W, 4, 4);
  if (!hm) return YRWI_E_HIP;
  HIPCHK(ctx, lane_sync(ctx));
  std::vector<uint32_t> M((size_t)W * W);
  std::memcpy(M.data(), hm, M.size() * 4);
  // row s of M = what rank s sends to each owner
  std::vector<int64_t> soff((size_t)W + 1, 0), roff((size_t)W + 1, 0);
  for (int p = 0; p < W; p++) {
    soff[(size_t)p + 1] = soff[(size_t)p] + M[(size_t)me * W + p];
    roff[(size_t)p + 1] = roff[(size_t)p] + M[(size_t)p * W + me];
  }
  const int64_t nsend = soff[(size_t)W], nrecv = roff[(size_t)W];
  std::vector<uint32_t> cur((size_t)W);
  for (int p = 0; p < W; p++) cur[(size_t)p] = (uint32_t)soff[(size_t)p];
  uint32_t* d_cur = arena_alloc<uint32_t>(ctx, W);
  HostMsg* d_send = arena_alloc<HostMsg>(ctx, nsend);
  uint64_t* d_sslot = arena_alloc<uint64_t>(ctx, nsend);
  HostMsg* d_recv = arena_alloc<HostMsg>(ctx, nrecv);
  uint32_t* d_reply = arena_alloc<uint32_t>(ctx, nrecv);
  uint32_t* d_back = arena_alloc<uint32_t>(ctx, nsend);
  uint64_t ocap = 1;
  while (ocap < (uint64_t)(2 * std::max<int64_t>(nrecv, 1))) ocap <<= 1;
  uint64_t* d_okeys = arena_alloc<uint64_t>(ctx, (int64_t)ocap);
  uint32_t* d_ovals = arena_alloc<uint32_t>(ctx, (int64_t)ocap);
  if (!d_cur || !d_send || !d_sslot || !d_recv || !d_reply || !d_back || !d_okeys || !d_ovals)
    return ctx->fail(YRWI_E_NOMEM, "arena");
  if (upload(ctx, d_cur, cur)) return YRWI_E_HIP;
  HIPCHK(ctx, hipMemsetAsync(d_okeys, 0, ocap * 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_ovals, 0, ocap * 4, ctx->stream));
  if (launch_host_pack(d_hkeys, d_hcnt, d_sb, nq, nslots, W, d_cur, d_send, d_sslot, ctx->stream, hkey))
    return ctx->fail(YRWI_E_HIP, "host pack");
  {
    std::vector<Xfer> snd, rcv;
    for (int p = 0; p < W; p++) {
      snd.push_back({p, d_send + soff[(size_t)p], (size_t)(soff[(size_t)p + 1] - soff[(size_t)p]) * sizeof(HostMsg)});
      rcv.push_back({p, d_recv + roff[(size_t)p], (size_t)(roff[(size_t)p + 1] - roff[(size_t)p]) * sizeof(HostMsg)});
    }
    if (int rc = coll_exchange(ctx, snd, rcv)) return rc;
  }
  if (launch_host_owner(d_recv, nrecv, d_okeys, d_ovals, ocap - 1, d_gmax, d_reply, ctx->stream))
    return ctx->fail(YRWI_E_HIP, "host owner");
  if (int rc = coll_allreduce_i32(ctx, d_gmax, (size_t)nq, true)) return rc;
  {
    std::vector<Xfer> snd, rcv;  // replies to what p sent me; totals for what I sent p
    for (int p = 0; p < W; p++) {
      snd.push_back({p, d_reply + roff[(size_t)p], (size_t)(roff[(size_t)p + 1] - roff[(size_t)p]) * 4});
      rcv.push_back({p, d_back + soff[(size_t)p], (size_t)(soff[(size_t)p + 1] - soff[(size_t)p]) * 4});
    }
    if (int rc = coll_exchange(ctx, snd, rcv)) return rc;
  }
  if (launch_host_apply(d_back, d_sslot, nsend, d_hcnt, R.S.d_shard, d_gmax, nq, ctx->stream))
    return ctx->fail(YRWI_E_HIP, "host apply");
  return 0;
}

// Normalise: every shard's summaries (k_reduce / the compaction's pieces, authority
// host counts), their exchange between the shards, the combined NormState per query.
static int normalize(RankPass& R) {
  Lane* ctx = R.ctx;
  Timing* tm = R.tm;
  const RankStep& S = R.S;
  hipEvent_t sp = span_open(ctx, tm);
  hipEvent_t rmid = tm ? ctx->event() : nullptr;  // after k_reduce, before k_shard_fin
  if (launch_reduce(S, ctx->stream, rmid)) return ctx->fail(YRWI_E_HIP, "reduce launch");
  if (S.hp_any && launch_host_part(S, ctx->stream)) return ctx->fail(YRWI_E_HIP, "host count launch");
  span_close(ctx, tm, sp);
  if (tm) tm->kreduce.push_back({sp, rmid});  // k_reduce alone: the population rocprofv3 averages
  if (R.st) {
    R.st->n_rank_passes++;
    for (int qi = 0; qi < R.nq; qi++) {
      const RankQ& Q = R.rq[(size_t)qi];
      if (R.plans[(size_t)qi].rep >= 0) continue;  // a repeat: nothing of it is reduced or scored
      if (!Q.pieces) R.st->bytes_reduce += (int64_t)FEAT_BYTES * Q.n + (Q.removed ? Q.n : 0);
      R.st->bytes_score += (int64_t)FEAT_BYTES * Q.n + (Q.removed ? Q.n : 0);
    }
  }
  if (R.shx && R.any_auth)
    if (int rc = exchange_host_counts(R)) return rc;
  if (R.shx)
    if (int rc = coll_allgather(ctx, S.d_shard, S.d_all, sizeof(ShardSum) * R.nq)) return rc;
  sp = span_open(ctx, tm);
  if (launch_combine(S, ctx->stream)) return ctx->fail(YRWI_E_HIP, "combine launch");
  span_close(ctx, tm, sp);
  if (tm) { tm->tn = ctx->event(); hipEventRecord(tm->tn, ctx->stream); }
  return 0;
}

// yrwi_normalize_score: the score of every element of the single query, no top-k
static int scores_all(RankPass& R, int64_t* h_scores_all) {
  Lane* ctx = R.ctx;
  R.S.d_scores = arena_alloc<int64_t>(ctx, R.rq[0].n);
  if (!R.S.d_scores) return ctx->fail(YRWI_E_NOMEM, "arena");
  if (launch_score_all(R.S, ctx->stream)) return ctx->fail(YRWI_E_HIP, "score launch");
  HIPCHK(ctx, hipMemcpyAsync(h_scores_all, R.S.d_scores, sizeof(int64_t) * R.rq[0].n, hipMemcpyDeviceToHost,
                             ctx->stream));
  HIPCHK(ctx, lane_sync(ctx));
  NormState nsh;
  HIPCHK(ctx, hipMemcpy(&nsh, R.S.d_norm, sizeof(nsh), hipMemcpyDeviceToHost));
  if (nsh.D < 0) return ctx->fail(YRWI_E_UNSUPPORTED, "distance fold summary overflow");
  return 0;
}

// chunk order for k_score: every query's chunk 0, then every chunk 1, ... so that
// a big query's later chunks run after its threshold is set (PruneP)
static std::vector<int32_t> chunk_order(const RankPass& R) {
  std::vector<int32_t> order((size_t)R.chunks * 2);  // (chunk, query) pairs
  // counting sort by chunk index c (stable in query order): O(chunks + max chunks)
  int64_t maxc = 0;
  for (auto& Q : R.rq) maxc = std::max(maxc, Q.nchunks);
  std::vector<int64_t> at((size_t)maxc + 1, 0);
  for (auto& Q : R.rq)
    for (int64_t c = 0; c < Q.nchunks; c++) at[(size_t)c + 1]++;
  for (int64_t c = 0; c < maxc; c++) at[(size_t)c + 1] += at[(size_t)c];
  for (int qi = 0; qi < R.nq; qi++)
    for (int64_t c = 0; c < R.rq[(size_t)qi].nchunks; c++) {
      const size_t o = (size_t)at[(size_t)c]++;
      order[2 * o] = (int32_t)(R.chunk_base[(size_t)qi] + c);
      order[2 * o + 1] = qi;
    }
  return order;
}

// score + per-chunk top-k
static int score_chunks(RankPass& R) {
  Lane* ctx = R.ctx;
  Timing* tm = R.tm;
  RankStep& S = R.S;
  S.kc = std::min<int32_t>(R.keff, CHUNK);  // per-chunk candidate list stride
  S.d_cand = arena_alloc<Cand>(ctx, std::max<int64_t>(R.chunks, 1) * S.kc);
  S.d_cand_cnt = arena_alloc<int32_t>(ctx, std::max<int64_t>(R.chunks, 1));
  if (!S.d_cand || !S.d_cand_cnt) return ctx->fail(YRWI_E_NOMEM, "arena");
  R.d_zero = arena_alloc<int32_t>(ctx, 2);
  S.d_redo = arena_alloc<int32_t>(ctx, std::max<int64_t>(R.chunks, 1));
  if (!R.d_zero || !S.d_redo) return ctx->fail(YRWI_E_NOMEM, "arena");
  S.d_nredo = R.d_zero + 1;
  HIPCHK(ctx, hipMemsetAsync(R.d_zero, 0, 2 * sizeof(int32_t), ctx->stream));
  hipEvent_t sp = span_open(ctx, tm);
  const std::vector<int32_t> order = chunk_order(R);
  int32_t* d_order = arena_alloc<int32_t>(ctx, 2 * R.chunks);
  S.d_tq = arena_alloc<unsigned long long>(ctx, R.nq);
  S.d_qtab = arena_alloc<uint8_t>(ctx, (int64_t)R.nq * (int64_t)score_qtab_bytes());
  if (!d_order || !S.d_tq || !S.d_qtab) return ctx->fail(YRWI_E_NOMEM, "arena");
  if (upload(ctx, d_order, order)) return YRWI_E_HIP;
  S.d_order = d_order;
  HIPCHK(ctx, hipMemsetAsync(S.d_tq, 0, sizeof(unsigned long long) * (size_t)R.nq, ctx->stream));
  // the k_score launch alone (the population rocprofv3 averages): from right
  // before it to before k_score_full
  hipEvent_t s0 = span_open(ctx, tm);
  hipEvent_t smid = tm ? ctx->event() : nullptr;
  if (launch_score(S, ctx->stream, smid)) return ctx->fail(YRWI_E_HIP, "score launch");
  span_close(ctx, tm, sp);
  if (tm) tm->kscore.push_back({s0, smid});
  return 0;
}

// top-k passes over groups of candidate lists until one list per query; a query
// with a single list (one chunk) is final as it stands.  fptr / fcnt: every
// query's final list and its count.
static int topk_ladder(RankPass& R, std::vector<const Cand*>* fptr, std::vector<const int32_t*>* fcnt) {
  Lane* ctx = R.ctx;
  const RankStep& S = R.S;
  const int nq = R.nq;
  const int32_t keff = R.keff;
  fptr->resize((size_t)nq);
  fcnt->resize((size_t)nq);
  std::vector<int64_t> lists((size_t)nq), lbase((size_t)nq);
  for (int qi = 0; qi < nq; qi++) {
    lists[(size_t)qi] = R.rq[(size_t)qi].nchunks;
    lbase[(size_t)qi] = R.chunk_base[(size_t)qi];
    (*fptr)[(size_t)qi] = S.d_cand + R.chunk_base[(size_t)qi] * S.kc;
    (*fcnt)[(size_t)qi] = lists[(size_t)qi] ? S.d_cand_cnt + R.chunk_base[(size_t)qi] : R.d_zero;
  }
  TopqPass T;  // a pass reads the lists the one before wrote
  T.keff = keff;
  T.d_in = S.d_cand;
  T.d_in_cnt = S.d_cand_cnt;
  T.in_stride = S.kc;
  while (true) {
    const int64_t G = std::max<int64_t>(2, std::min<int64_t>(64, topq_capacity(keff) / T.in_stride));
    std::vector<int64_t> gb;
    std::vector<int32_t> gn, gk;
    std::vector<int> part;
    for (int qi = 0; qi < nq; qi++) {
      const int64_t L = lists[(size_t)qi];
      if (L <= 1) continue;
      const int64_t ng = ceil_div(L, G);
      const int64_t first = (int64_t)gb.size();
      for (int64_t g = 0; g < ng; g++) {
        gb.push_back(lbase[(size_t)qi] + g * G);
        gn.push_back((int32_t)std::min<int64_t>(G, L - g * G));
        gk.push_back(R.rq[(size_t)qi].k);
      }
      lists[(size_t)qi] = ng;
      lbase[(size_t)qi] = first;
      part.push_back(qi);
    }
    if (gb.empty()) break;
    T.ngroups = (int64_t)gb.size();
    int64_t* d_gb = arena_alloc<int64_t>(ctx, T.ngroups);
    int32_t* d_gn = arena_alloc<int32_t>(ctx, T.ngroups);
    int32_t* d_gk = arena_alloc<int32_t>(ctx, T.ngroups);
    T.d_out = arena_alloc<Cand>(ctx, T.ngroups * keff);
    T.d_out_cnt = arena_alloc<int32_t>(ctx, T.ngroups);
    if (!d_gb || !d_gn || !d_gk || !T.d_out || !T.d_out_cnt) return ctx->fail(YRWI_E_NOMEM, "arena");
    if (upload(ctx, d_gb, gb, d_gn, gn, d_gk, gk)) return YRWI_E_HIP;
    T.d_gbase = d_gb;
    T.d_gn = d_gn;
    T.d_gk = d_gk;
    hipEvent_t sq = span_open(ctx, R.tm);
    if (launch_topq(T, ctx->stream)) return ctx->fail(YRWI_E_HIP, "top-k launch");
    span_close(ctx, R.tm, sq);
    for (int qi : part) {
      (*fptr)[(size_t)qi] = T.d_out + lbase[(size_t)qi] * keff;
      (*fcnt)[(size_t)qi] = T.d_out_cnt + lbase[(size_t)qi];
    }
    T.in_stride = keff;
    T.d_in = T.d_out;
    T.d_in_cnt = T.d_out_cnt;
  }
  return 0;
}

// Destination binding: hits, counts and rows each go to the caller's buffer when it
// is pinned, else to the landing buffer; the device addresses the emit kernels write.
static int bind_dest(RankPass& R, RankDest* D) {
  Lane* ctx = R.ctx;
  const int32_t kmax = D->kmax;
  D->kint = R.any_dd ? YRWI_MAX_K : kmax;
  D->hb = sizeof(yrwi_hit) * (size_t)R.nq * kmax;
  D->hb_al = (D->hb + 255) & ~(size_t)255;
  D->nb = sizeof(int32_t) * (size_t)R.nq;
  D->direct = ctx->hostreg && ctx->hostreg->contains(D->h_hits, D->hb) && ctx->hostreg->contains(D->h_nout, D->nb);
  // the hits' rows (yrwi_query_*_rows) go the same way: into the caller's buffer when it is
  // pinned and 8-byte aligned (k_hit_rows stores 8-byte words), else behind the hits in the
  // landing buffer
  uint8_t* h_rows = D->h_rows;
  const size_t rb = h_rows ? (size_t)YRWI_ROW_BYTES * (size_t)R.nq * kmax : 0;
  D->rows_direct = h_rows && ctx->hostreg && (reinterpret_cast<uintptr_t>(h_rows) & 7) == 0 &&
                   ctx->hostreg->contains(h_rows, rb);
  D->land_rows = D->direct ? 0 : (D->hb_al + D->nb + 255) & ~(size_t)255;
  void* hp = D->h_hits;
  void* np = D->h_nout;
  void* rp = h_rows;
  if (!D->direct || (h_rows && !D->rows_direct)) {
    const size_t bytes = h_rows && !D->rows_direct ? D->land_rows + rb : D->hb_al + D->nb;
    D->land = stage_reserve(ctx, &ctx->out_stage, bytes, true);
    if (!D->land) return YRWI_E_HIP;
  }
  if (!D->direct) {
    hp = D->land;
    np = D->land + D->hb_al;
  }
  if (h_rows && !D->rows_direct) rp = D->land + D->land_rows;
  if (h_rows) HIPCHK(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&D->d_rows), rp, 0));
  // the emit kernels write the pinned destination directly (a DMA copy from a
  // device buffer instead measured 1.17 vs 1.07 ms per C2 step)
  HIPCHK(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&D->out.hits), hp, 0));
  HIPCHK(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&D->out.cnt), np, 0));
  D->out.stride = kmax;
  D->pulled = D->out;
  return 0;
}

// The final-list pointers go up.  Rows asked for: k_pull (doubledom, sharded) leaves its hits in
// device memory, where k_hit_rows reads them, looks their rows up and forwards them to the pinned
// destination.
static int upload_final(RankPass& R, RankDest* D, std::vector<const Cand*>& fptr, std::vector<const int32_t*>& fcnt) {
  Lane* ctx = R.ctx;
  const int nq = R.nq;
  const Cand** d_fptr = arena_alloc<const Cand*>(ctx, nq);
  const int32_t** d_fcnt = arena_alloc<const int32_t*>(ctx, nq);
  if (!d_fptr || !d_fcnt) return ctx->fail(YRWI_E_NOMEM, "arena");
  R.S.d_final = d_fptr;
  R.S.d_final_cnt = d_fcnt;
  // a repeat's final list is its representative's (an earlier query of the pass)
  for (int qi = 0; qi < nq; qi++) {
    const int32_t r = R.plans[(size_t)qi].rep;
    if (r < 0) continue;
    fptr[(size_t)qi] = fptr[(size_t)r];
    fcnt[(size_t)qi] = fcnt[(size_t)r];
  }
  if (!D->h_rows) return upload(ctx, d_fptr, fptr, d_fcnt, fcnt) ? YRWI_E_HIP : 0;
  std::vector<HitRowQ> hq((size_t)nq);
  int own_shift = -1;
  if (R.shx) {
    own_shift = 6;
    for (int w = ctx->world; w > 1; w >>= 1) own_shift--;
  }
  for (int qi = 0; qi < nq; qi++) {
    const Plan& P = R.plans[(size_t)qi];
    HitRowQ& H = hq[(size_t)qi];
    const Plan& C = P.rep >= 0 ? R.plans[(size_t)P.rep] : P;  // whose container the hits were ranked from
    H.rows = C.empty ? nullptr : C.cont.rows;
    H.now_ms = P.now_ms;
    H.src = R.shx || R.rq[(size_t)qi].doubledom ? HR_HITS : HR_CAND;
    H.own_shift = own_shift;
    H.own_rank = ctx->rank;
    H.pad = 0;
  }
  D->d_hq = arena_alloc<HitRowQ>(ctx, nq);
  if (!D->d_hq) return ctx->fail(YRWI_E_NOMEM, "arena");
  // (the rows' descriptors ride in the candidate lists' copy kernel: no launch of their own)
  if (upload(ctx, d_fptr, fptr, d_fcnt, fcnt, D->d_hq, hq)) return YRWI_E_HIP;
  if (R.shx || R.any_dd) {
    D->pulled.hits = arena_alloc<yrwi_hit>(ctx, (int64_t)nq * D->kmax);
    D->pulled.cnt = arena_alloc<int32_t>(ctx, nq);
    if (!D->pulled.hits || !D->pulled.cnt) return ctx->fail(YRWI_E_NOMEM, "arena");
  }
  return 0;
}

// One GPU: k_emit writes the hits; doubledom queries' stacks are emitted apart and pulled.
static int emit_single(RankPass& R, const RankDest& D) {
  Lane* ctx = R.ctx;
  Timing* tm = R.tm;
  hipEvent_t sp = span_open(ctx, tm);
  if (launch_emit(R.S, D.out, 0, ctx->stream)) return ctx->fail(YRWI_E_HIP, "emit launch");
  span_close(ctx, tm, sp);
  if (!R.any_dd) return 0;
  HitList stack;
  stack.hits = arena_alloc<yrwi_hit>(ctx, (int64_t)R.nq * D.kint);
  stack.cnt = arena_alloc<int32_t>(ctx, R.nq);
  stack.stride = D.kint;
  if (!stack.hits || !stack.cnt) return ctx->fail(YRWI_E_NOMEM, "arena");
  sp = span_open(ctx, tm);
  if (launch_emit(R.S, stack, 2, ctx->stream) || launch_pull(R.S, stack, 1, D.pulled, ctx->stream))
    return ctx->fail(YRWI_E_HIP, "doubledom launch");
  span_close(ctx, tm, sp);
  return 0;
}

// Sharded: every shard's stacks gathered, merged (TreeSet in shard order) and pulled;
// NormState::D of every query read back for the overflow check.
static int emit_sharded(RankPass& R, RankDest* D) {
  Lane* ctx = R.ctx;
  Timing* tm = R.tm;
  const int nq = R.nq, W = R.W;
  const int32_t kint = D->kint;
  HitList mine, all, stack;
  mine.stride = all.stride = stack.stride = kint;
  mine.hits = arena_alloc<yrwi_hit>(ctx, (int64_t)nq * kint);
  mine.cnt = arena_alloc<int32_t>(ctx, nq);
  all.hits = arena_alloc<yrwi_hit>(ctx, (int64_t)nq * kint * W);
  all.cnt = arena_alloc<int32_t>(ctx, (int64_t)nq * W);
  uint32_t* d_slot = arena_alloc<uint32_t>(ctx, (int64_t)nq * kint * W);
  uint8_t* d_dup = arena_alloc<uint8_t>(ctx, (int64_t)nq * kint * W);
  stack.hits = arena_alloc<yrwi_hit>(ctx, (int64_t)nq * kint);
  stack.cnt = arena_alloc<int32_t>(ctx, nq);
  if (!mine.hits || !mine.cnt || !all.hits || !all.cnt || !d_slot || !d_dup || !stack.hits || !stack.cnt)
    return ctx->fail(YRWI_E_NOMEM, "arena");
  hipEvent_t sp = span_open(ctx, tm);
  if (launch_emit(R.S, mine, 1, ctx->stream)) return ctx->fail(YRWI_E_HIP, "emit launch");
  span_close(ctx, tm, sp);
  if (int rc = coll_allgather(ctx, mine.hits, all.hits, sizeof(yrwi_hit) * (size_t)nq * kint)) return rc;
  if (int rc = coll_allgather(ctx, mine.cnt, all.cnt, sizeof(int32_t) * (size_t)nq)) return rc;
  if (ctx->release_after_final) turn_release(ctx);  // the next batch part's collectives may follow now
  sp = span_open(ctx, tm);
  if (launch_gmerge(R.S, all, d_slot, d_dup, stack, ctx->stream) || launch_pull(R.S, stack, 0, D->pulled, ctx->stream))
    return ctx->fail(YRWI_E_HIP, "shard merge launch");
  span_close(ctx, tm, sp);
  D->hD_land = readback(ctx, &ctx->down_stage, reinterpret_cast<const uint8_t*>(R.S.d_norm) + offsetof(NormState, D),
                        nq, 4, (int64_t)sizeof(NormState));
  return D->hD_land ? 0 : YRWI_E_HIP;
}

// Wait for the pass, check the distance fold, copy out of the landing buffer what went there.
static int finish(RankPass& R, const RankDest& D) {
  Lane* ctx = R.ctx;
  const int32_t kmax = D.kmax;
  if (R.tm) { R.tm->ts = ctx->event(); hipEventRecord(R.tm->ts, ctx->stream); }
  HIPCHK(ctx, lane_sync(ctx));
  for (int qi = 0; D.hD_land && qi < R.nq; qi++) {
    int32_t maxdist;
    std::memcpy(&maxdist, D.hD_land + (size_t)qi * 4, 4);
    if (maxdist < 0) return ctx->fail(YRWI_E_UNSUPPORTED, "distance fold summary overflow");
  }
  if (!D.direct) {
    std::memcpy(D.h_nout, D.land + D.hb_al, D.nb);
    for (int qi = 0; qi < R.nq; qi++)
      std::memcpy(D.h_hits + (size_t)qi * kmax, D.land + sizeof(yrwi_hit) * (size_t)qi * kmax,
                  sizeof(yrwi_hit) * (size_t)std::max(0, std::min(D.h_nout[qi], kmax)));
  }
  if (D.h_rows && !D.rows_direct)
    for (int qi = 0; qi < R.nq; qi++)
      std::memcpy(D.h_rows + (size_t)YRWI_ROW_BYTES * (size_t)qi * kmax,
                  D.land + D.land_rows + (size_t)YRWI_ROW_BYTES * (size_t)qi * kmax,
                  (size_t)YRWI_ROW_BYTES * (size_t)std::max(0, std::min(D.h_nout[qi], kmax)));
  return 0;
}

int yrwi::run_rank_phase(Lane* ctx, std::vector<Plan>& plans, int32_t kmax, yrwi_hit* h_hits, int32_t* h_nout,
                         int64_t* h_scores_all, yrwi_stats* st, Timing* tm, bool collective, uint8_t* h_rows) {
  RankPass R(ctx, plans, st, tm, collective);
  build_queries(R);
  if (int rc = alloc_host_tables(R)) return rc;
  if (int rc = plan_host_part(R)) return rc;
  if (int rc = upload_filters(R)) return rc;
  if (int rc = upload_queries(R)) return rc;
  if (int rc = normalize(R)) return rc;
  if (h_scores_all) return scores_all(R, h_scores_all);
  if (int rc = score_chunks(R)) return rc;
  std::vector<const Cand*> fptr;
  std::vector<const int32_t*> fcnt;
  if (int rc = topk_ladder(R, &fptr, &fcnt)) return rc;
  RankDest D{h_hits, h_nout, h_rows, kmax};
  if (int rc = bind_dest(R, &D)) return rc;
  if (int rc = upload_final(R, &D, fptr, fcnt)) return rc;
  if (int rc = R.shx ? emit_sharded(R, &D) : emit_single(R, D)) return rc;
  if (h_rows) {
    hipEvent_t sp = span_open(ctx, tm);
    if (launch_hit_rows(R.S, D.d_hq, D.pulled, D.out, D.d_rows, ctx->stream))
      return ctx->fail(YRWI_E_HIP, "hit rows launch");
    span_close(ctx, tm, sp);
  }
  if (int rc = finish(R, D)) return rc;
  return flagcounts_out(R);
}
