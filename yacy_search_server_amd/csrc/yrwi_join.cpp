// yrwi_join.cpp -- the join / exclusion phase of a batch part (run_join_phase):
// every fold step's dispatch (J3, yrwi_host.cpp), its jobs' layout, launches and
// byte accounting, chained folds and the exclusion step.  Planning and the C
// entry points are in yrwi_host.cpp, the rank phase in yrwi_rank.cpp.

#include "yrwi_host.h"

using namespace yrwi;

// joinConstructive dispatch (ReferenceContainer.java:406-416); returns JoinMode
static int32_t dispatch_mode(int64_t n1, int64_t n2) {
  int32_t s1 = (int32_t)n1, s2 = (int32_t)n2;
  int32_t high = s1 > s2 ? s1 : s2, low = s1 > s2 ? s2 : s1;
  int32_t steps_enum = mul32(10, add32(add32(high, low), -1));
  int32_t steps_test = mul32(mul32(12, log2j(high)), low);
  if (steps_enum > steps_test) return s1 < s2 ? JM_TEST_LARGE_B : JM_TEST_LARGE_A;
  return JM_ENUM;
}

// algorithmic bytes of one join step
static int64_t step_bytes(int32_t mode, int64_t na, int64_t nb) {
  if (mode == JM_ENUM) return 12 * (na + nb);
  int64_t ns = std::min(na, nb), nl = std::max(na, nb);
  if (ns <= 0) return 0;  // by test with an empty smaller side: nothing is probed
  int64_t lg = 0;
  while ((ns << lg) < nl) lg++;  // ceil(log2(nl/ns))
  return 12 * (ns + std::min(nl, ns * (lg + 1)));
}

// bytes a probe of `acc` url ids into a list of n loads: the ids and one 16-B
// bitmap word per id (bm: the list has a bitmap); else the ids and the list's
// range, or a 128-B leaf line per id, whichever is less
static int64_t probe_bytes(bool bm, int64_t acc, int64_t n) {
  return bm ? 20 * acc : 4 * acc + std::min(4 * n, 128 * acc);
}

// bytes a join job's kernel loads (yrwi_stats.bytes_alg_capped): merge tiles
// stream both sides' 4-B url ids; a probe reads the smaller side's ids into the
// larger list (probe_bytes; layout_jobs has set J.algo)
static int64_t loaded_bytes(const JoinQ& J) {
  const int64_t ns = std::min(J.A.n, J.B.n), nl = std::max(J.A.n, J.B.n);
  if (J.algo == JA_MERGE) return 4 * (ns + nl);
  if (J.algo == JA_BMAND) return (J.bm3 ? 48 : 32) * J.bm_words;  // every bitmap's 16-B units
  return probe_bytes((J.small_is_A ? J.B.bm : J.A.bm) != nullptr, ns, nl);
}

// §8(d) K of a step's jobs as the reference dispatches them
static void account_jobs(yrwi_stats* st, const std::vector<JoinQ>& jobs) {
  for (const JoinQ& J : jobs) {
    const int64_t K = step_bytes(J.mode, J.A.n, J.B.n), loaded = loaded_bytes(J);
    (J.algo == JA_MERGE ? st->bytes_join : st->bytes_probe) += K;
    (J.algo == JA_MERGE ? st->bytes_join_capped : st->bytes_probe_capped) += std::min(K, loaded);
    if (J.algo != JA_MERGE) st->bytes_probe_loaded += loaded;
    st->bytes_alg_capped += std::min(K, loaded);
  }
}

// k_compact per joined row (mh: every job's joined rows): pair + id read, the records it gathers
// (32 B, + 16 B of the joined side for enumeration steps, + the deferred rows' sources and
// records), record + id written; deferred output: A's sources read, sources + id written;
// chained: the rows of every list of the fold (4 B each beyond the pair), the records of the
// fold (32 B + 16 B per enumeration step)
static void account_compact(yrwi_stats* st, const std::vector<JoinQ>& jobs, const std::vector<int>& owner,
                            const std::vector<ChainQ>* chq, const std::vector<int64_t>& mh) {
  for (size_t j = 0; j < jobs.size(); j++) {
    const JoinQ& J = jobs[j];
    const int64_t atw = J.A.tup ? J.A.tw : 0;
    if (J.count_only) continue;
    if (J.chain) {
      const int64_t t = 2 + (*chq)[(size_t)owner[j]].npos;
      st->bytes_compact += mh[j] * (12 + 4 * (t - 2) + 32 + 24 * (t - 1) + 36);
      continue;
    }
    st->bytes_compact += mh[j] * (J.out_tup ? 12 + 4 * atw + 4 + 4 * (int64_t)J.out_tw
                                            : (J.mode == JM_ENUM ? 96 : 80) + 4 * atw + (atw > 1 ? 24 * (atw - 1) : 0));
  }
}

// a chained fold's steps after the first: their K (acc: this shard's container before each),
// charged min(K, the bytes the chain tests load for them)
static void account_chain_steps(yrwi_stats* st, const Plan& P, const int64_t* acc) {
  for (size_t l = 2; l < P.seq.size(); l++) {
    const int64_t n = P.seq[l]->n;
    const int32_t m = P.step_mode[l - 1];
    const int64_t K = step_bytes(m, acc[l - 2], n);
    const int64_t loaded = probe_bytes(P.seq[l]->bm != nullptr, acc[l - 2], n);
    st->bytes_alg += K;
    st->bytes_chain += std::min(K, loaded);
    st->bytes_alg_capped += std::min(K, loaded);
    if (m == JM_ENUM) st->n_enum_steps++; else st->n_test_steps++;
  }
}

// exclusions of a chained query: the bytes k_chain loads for them (pre: the rows that reach them)
static void account_chain_excl(yrwi_stats* st, const ChainQ& C, int64_t pre) {
  for (int l = C.ninc; l < C.nl; l++) {
    const int64_t b = std::min<int64_t>(12 * C.l[l].n, probe_bytes(C.l[l].bm != nullptr, pre, C.l[l].n));
    st->bytes_alg_capped += b;
    st->bytes_chain += b;
  }
}

// Give every job its algorithm and tile count, put merge jobs first and lay out
// the global tile index space: merge tiles [0, merge_tiles), probe tiles after
// (S: the step's job and tile counts and long_tiles).
static void layout_jobs(int64_t probe_ratio, int64_t nurls, std::vector<JoinQ>& jobs, std::vector<int>& owner,
                        std::vector<int64_t>& tile_base, JoinStep* S) {
  S->long_tiles = false;
  std::vector<size_t> order(jobs.size());
  for (size_t i = 0; i < jobs.size(); i++) {
    JoinQ& J = jobs[i];
    // a counted-only join of two lists with bitmaps: popcounts of their words
    if (J.count_only && J.A.bm && J.B.bm && nurls > 0) {
      J.algo = JA_BMAND;
      J.small_is_A = 1;
      J.ptile = BMAND_WORDS;
      J.bm_words = bm_units(nurls);
      J.ntiles = ceil_div(J.bm_words, BMAND_WORDS);
      J.chain_bm = nullptr;
      order[i] = i;
      continue;
    }
    // a sparse list's bitmap (below 1/64 of the url ids: k_chain's tests and the
    // selections use it) does not take a join: its probes search the list, where
    // a tile's staged range costs less than a bitmap line per key
    if (J.A.bm && J.A.n * 64 < nurls) J.A.bm = nullptr;
    if (J.B.bm && J.B.n * 64 < nurls) J.B.bm = nullptr;
    const int64_t ns = std::min(J.A.n, J.B.n), nl = std::max(J.A.n, J.B.n);
    J.small_is_A = J.A.n <= J.B.n;
    // skewed sizes: probe the large list; a large list with a url-id bitmap is
    // probed at any ratio (the small side's ids stream, the bitmap stays in L2)
    const bool bm = (J.small_is_A ? J.B.bm : J.A.bm) != nullptr;
    J.algo = (bm || nl > probe_ratio * ns) ? JA_PROBE : JA_MERGE;
    // long bitmap tiles only where no record is gathered per match (a deferred
    // step writes sources, an exclusion marks): a final step's compaction keeps
    // its band order per 1024-id tile (C2 k_compact 220 -> 236 us with 2048)
    // A chained probe job whose first later include list has a bitmap (J.chain_bm,
    // set by the caller) tests it inside k_probe -- a bitmap probe on BM_TILE
    // tiles (the long tiles' registers leave no room for it), a range probe on its
    // usual tiles; merge jobs leave it to k_chain.
    if (J.algo == JA_MERGE) J.chain_bm = nullptr;
    const bool light = J.out_tup != nullptr || J.mode == JM_MARK || (J.chained && !J.chain_bm);
    J.ptile = bm ? (light && ns >= BM_LARGE_MIN ? KPT_LARGE * PROBE_TILE : BM_TILE) : PROBE_TILE;
    if (J.ptile == KPT_LARGE * PROBE_TILE) S->long_tiles = true;
    J.ntiles = J.algo == JA_MERGE ? ceil_div(J.A.n + J.B.n, JOIN_TILE) : ceil_div(ns, J.ptile);
    order[i] = i;
  }
  // Within each algorithm, jobs that share their larger list run back to back:
  // queries sample terms by df, so the big lists recur across a batch, and
  // consecutive tiles over the same list hit in L2 / MALL instead of HBM.  Job
  // order only changes the schedule (every job owns its output slots).
  auto big = [&](const JoinQ& J) { return (uintptr_t)(J.A.n >= J.B.n ? J.A.uid : J.B.uid); };
  auto small = [&](const JoinQ& J) { return (uintptr_t)(J.A.n >= J.B.n ? J.B.uid : J.A.uid); };
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    const JoinQ &x = jobs[a], &y = jobs[b];
    if (x.algo != y.algo) return x.algo < y.algo;
    if (big(x) != big(y)) return big(x) < big(y);
    return small(x) < small(y);
  });
  std::vector<JoinQ> js;
  std::vector<int> ow;
  tile_base.clear();
  S->njobs = (int32_t)jobs.size();
  S->nmerge = 0;
  S->merge_tiles = 0;
  S->tiles = 0;
  for (size_t i : order) {
    JoinQ J = jobs[i];
    J.tile_base = S->tiles;
    tile_base.push_back(S->tiles);
    S->tiles += J.ntiles;
    if (J.algo == JA_MERGE) { S->nmerge++; S->merge_tiles = S->tiles; }
    js.push_back(J);
    if (!owner.empty()) ow.push_back(owner[i]);
  }
  jobs.swap(js);
  if (!owner.empty()) owner.swap(ow);
}

// band-major compaction schedule of a step's tiles (BandOrder, k_order_hist /
// k_order_scatter):
// scratch for the tile keys and the order; job order when disabled
static BandOrder band_order(Lane* ctx, int64_t tiles, int64_t merge_tiles, bool compact) {
  BandOrder bo;
  if (tiles <= 0 || tiles > INT32_MAX) return bo;
  bo.tile_job = arena_alloc<int32_t>(ctx, tiles);
  if (!ctx->band_order || tiles <= 1 || !bo.tile_job) return bo;
  bo.hist = arena_alloc<int32_t>(ctx, (int64_t)ORDER_HIST_SLICES * 4096);
  if (compact) {
    bo.key = arena_alloc<uint32_t>(ctx, tiles);
    bo.perm = arena_alloc<int2>(ctx, tiles);
  }
  if (tiles - merge_tiles > 1) {
    bo.pkey = arena_alloc<uint32_t>(ctx, tiles - merge_tiles);
    bo.pperm = arena_alloc<int2>(ctx, tiles - merge_tiles);
  }
  if (!bo.hist || (compact && (!bo.key || !bo.perm)) || (bo.pkey && !bo.pperm)) {
    bo.key = bo.pkey = nullptr;
    return bo;
  }
  int bits = 0;  // url ids < 2^bits; 2^12 bands for compaction, 2^4 for the probe
  while (bits < 32 && ((int64_t)1 << bits) < ctx->nurls) bits++;
  bo.shift = std::max(0, bits - 12);
  bo.pshift = std::max(0, bits - 4);
  return bo;
}

// A laid-out step's job table, tile descriptors and band order; unless it only
// marks (S->mark), also the bitmap-probe tiles' short descriptors and its pair
// run of npairs.
static int alloc_step(Lane* ctx, JoinStep* S, int64_t npairs) {
  const int64_t probe_tiles = S->tiles - S->merge_tiles;
  S->d_jobs = arena_alloc<JoinQ>(ctx, S->njobs);
  S->d_tile_base = arena_alloc<int64_t>(ctx, S->njobs);
  S->d_desc = arena_alloc<TileDesc>(ctx, S->merge_tiles);
  S->d_pdesc = arena_alloc<ProbeDesc>(ctx, probe_tiles);
  if (!S->d_jobs || !S->d_tile_base || !S->d_desc || !S->d_pdesc) return ctx->fail(YRWI_E_NOMEM, "arena");
  if (!S->mark) {
    S->d_fast = arena_alloc<BmFast>(ctx, probe_tiles);
    S->d_fast_perm = arena_alloc<BmFast>(ctx, probe_tiles);
    S->d_pairs = arena_alloc<uint2>(ctx, npairs);
    S->d_pair_uid = arena_alloc<uint32_t>(ctx, npairs);
    S->d_tile_src = arena_alloc<int64_t>(ctx, S->tiles);
    S->d_tile_cnt = arena_alloc<int32_t>(ctx, S->tiles);
    S->d_tile_off = arena_alloc<int64_t>(ctx, S->tiles);
    if (!S->d_fast || !S->d_fast_perm || !S->d_pairs || !S->d_pair_uid || !S->d_tile_src || !S->d_tile_cnt ||
        !S->d_tile_off)
      return ctx->fail(YRWI_E_NOMEM, "arena");
  }
  S->bo = band_order(ctx, S->tiles, S->merge_tiles, !S->mark);
  return 0;
}

// The queries' last steps that summarise their containers as they compact them
// (JoinQ::want_sum): one ChunkSum per tile of the step, the job's run from its
// first tile.  Sets S->sum.
static int alloc_pieces(Lane* ctx, std::vector<JoinQ>& jobs, const std::vector<int64_t>& tile_base, JoinStep* S) {
  bool any_want = false;
  for (const JoinQ& J : jobs) any_want |= J.want_sum != 0;
  if (any_want) {
    ChunkSum* d_psum = arena_alloc<ChunkSum>(ctx, S->tiles);
    if (!d_psum) return ctx->fail(YRWI_E_NOMEM, "arena");
    for (size_t j = 0; j < jobs.size(); j++)
      if (jobs[j].want_sum) jobs[j].psum = d_psum + tile_base[j];
  }
  bool any = false, all = true;
  for (const JoinQ& J : jobs) {
    if (J.count_only) continue;
    any |= J.psum != nullptr;
    all &= J.psum != nullptr;
  }
  S->sum = any ? (all ? 1 : 2) : 0;
  return 0;
}

// The host side of a chained step's tables, uploaded with its job table.
struct ChainTables {
  std::vector<ChainQ> cq;  // the chained jobs' ChainQ (JoinQ::chain points into d_cq)
  ChainQ* d_cq = nullptr;
  std::vector<int2> cgrp;  // JoinStep::d_cgrp
  // Lane::chain_groups_on_device: one entry per chained job instead, expanded by k_chain_groups
  std::vector<ChainGroupJob> cgj;
  ChainGroupJob* d_cgj = nullptr;
};

// Chained jobs: their chain groups, their ChainQ (chq by plan; level counts into
// the landing buffer at d_level, the later include lists' rows in slot-indexed
// arrays beside the pairs), per-tile level counts and the list ranges of
// k_chain_part.
static int chain_setup(Lane* ctx, std::vector<JoinQ>& jobs, const std::vector<int>& owner,
                       const std::vector<int64_t>& tile_base, const std::vector<ChainQ>& chq, int64_t npairs,
                       int64_t* d_level, JoinStep* S, ChainTables* T) {
  const int64_t nurls = std::max<int64_t>(1, ctx->nurls);
  // a group holds about 640 expected matches (independent lists: nA nB / nurls
  // per job), so a workgroup tests close to one round of 768
  for (size_t j = 0; j < jobs.size(); j++) {
    const JoinQ& J = jobs[j];
    if (!J.chained || J.ntiles <= 0) continue;
    double per_tile = (double)J.A.n * (double)J.B.n / (double)nurls / (double)J.ntiles;
    const ChainQ& Cq = chq[(size_t)owner[j]];
    if (J.chain_bm)  // the probe already thinned the matches by the first later include
      per_tile *= std::min(1.0, (double)Cq.l[0].n / (double)nurls);
    const int G = (int)std::max(1.0, std::min((double)CHAIN_GMAX, 640.0 / std::max(1.0, per_tile)));
    if (ctx->chain_groups_on_device)
      T->cgj.push_back(ChainGroupJob{(int32_t)T->cgrp.size(), (int32_t)tile_base[j], (int32_t)J.ntiles, G});
    for (int64_t t = 0; t < J.ntiles; t += G)
      T->cgrp.push_back(make_int2((int32_t)(tile_base[j] + t), (int32_t)std::min<int64_t>(G, J.ntiles - t)));
  }
  S->ngroups = (int64_t)T->cgrp.size();
  S->d_tile_lvl = arena_alloc<int32_t>(ctx, S->tiles * CHAIN_LVL);
  S->d_crange = arena_alloc<ProbeDesc>(ctx, S->ngroups * CHAIN_MAXL);
  S->d_cgrp = arena_alloc<int2>(ctx, S->ngroups);
  T->d_cq = arena_alloc<ChainQ>(ctx, S->njobs);
  if (!S->d_tile_lvl || !S->d_crange || !S->d_cgrp || !T->d_cq) return ctx->fail(YRWI_E_NOMEM, "arena");
  int maxi = 0;
  for (size_t j = 0; j < jobs.size(); j++)
    if (jobs[j].chained) maxi = std::max(maxi, chq[(size_t)owner[j]].npos);
  int32_t* d_tup[CHAIN_MAXI] = {nullptr, nullptr};  // rows in the later include lists, indexed like d_pairs
  for (int l = 0; l < maxi; l++)
    if (!(d_tup[l] = arena_alloc<int32_t>(ctx, npairs))) return ctx->fail(YRWI_E_NOMEM, "arena");
  for (size_t j = 0; j < jobs.size(); j++) {
    JoinQ& J = jobs[j];
    if (!J.chained) continue;  // (a count-first fold's counted job is not)
    ChainQ C = chq[(size_t)owner[j]];
    C.level = d_level + (int64_t)j * CHAIN_LVL;
    for (int l = 0; l < CHAIN_MAXI; l++) C.tup[l] = l < C.npos ? d_tup[l] : nullptr;
    // a bitmap probe tests the first later include list itself when that list
    // has a bitmap (no selection before it): only its survivors reach k_chain
    C.pre = J.chain_bm != nullptr ? 1 : 0;  // (layout_jobs kept it for bitmap probes only)
    J.chain_tup0 = C.pre ? C.tup[0] : nullptr;
    J.chain_fill = C.pre && C.ninc == 1 ? 2 : 0;
    J.chain = T->d_cq + (int64_t)T->cq.size();
    T->cq.push_back(C);
  }
  if (ctx->chain_groups_on_device && !(T->d_cgj = arena_alloc<ChainGroupJob>(ctx, (int64_t)T->cgj.size())))
    return ctx->fail(YRWI_E_NOMEM, "arena");
  return 0;
}

// Jobs + tile bases (+ a chained step's ChainQs and its groups, or the group
// jobs k_chain_groups expands) in one copy.
static int upload_step(Lane* ctx, const JoinStep& S, const std::vector<JoinQ>& jobs,
                       const std::vector<int64_t>& tile_base, const ChainTables& T) {
  if (!S.chain) return upload(ctx, S.d_jobs, jobs, S.d_tile_base, tile_base);
  if (!ctx->chain_groups_on_device)
    return upload(ctx, S.d_jobs, jobs, S.d_tile_base, tile_base, T.d_cq, T.cq, S.d_cgrp, T.cgrp);
  if (upload(ctx, S.d_jobs, jobs, S.d_tile_base, tile_base, T.d_cq, T.cq, T.d_cgj, T.cgj)) return YRWI_E_HIP;
  if (launch_chain_groups(T.d_cgj, (int32_t)T.cgj.size(), S.d_cgrp, S.ngroups, ctx->stream))
    return ctx->fail(YRWI_E_HIP, "chain groups launch");
  return 0;
}

// A chained step whose compaction waits for the fold's dispatch modes (k_chain
// counts the intersections they depend on): what launch_compact needs.
struct PendingCompact {
  bool active = false;
  JoinStep step;
  std::vector<std::array<int64_t, CHAIN_LVL>> level;  // per job (layout order): k_chain's level counts
  std::vector<int64_t> mh;  // per job: its joined rows (the pair cache fills from them after the compaction)
};

// One fold step's join jobs: layout, launch, joined sizes back to the plans.
// chq (indexed by plan): the ChainQ of every chained query; a step with chained
// jobs runs k_chain and leaves its compaction to the caller (pend).
static int run_join_jobs(Lane* ctx, std::vector<Plan>& plans, std::vector<JoinQ>& jobs, std::vector<int>& owner,
                         yrwi_stats* st, Timing* tm, const std::vector<ChainQ>* chq, PendingCompact* pend) {
  if (chq)  // candidates for the probe's own test of the first later include (layout_jobs)
    for (size_t j = 0; j < jobs.size(); j++) {
      const ChainQ& Cq = (*chq)[(size_t)owner[j]];
      jobs[j].chain_bm = jobs[j].chained && Cq.pos0 == 0 && Cq.ninc >= 1 ? Cq.l[0].bm : nullptr;
    }
  JoinStep S;
  std::vector<int64_t> tile_base;
  layout_jobs(ctx->probe_ratio, ctx->nurls, jobs, owner, tile_base, &S);
  const int nj = S.njobs;
  if (st) account_jobs(st, jobs);
  if (chq)
    for (const JoinQ& J : jobs) S.chain |= J.chained != 0;
  // joined sizes (and chained jobs' level counts) land in pinned host memory:
  // k_scan_tiles writes them through its device address (no copy engine), the host
  // reads them after the step's sync
  const size_t land_words = (size_t)nj * (S.chain ? 1 + CHAIN_LVL : 1);
  uint8_t* land = stage_reserve(ctx, &ctx->down_stage, land_words * sizeof(int64_t), true);
  if (!land) return YRWI_E_HIP;
  int64_t* d_mout = nullptr;
  HIPCHK(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&d_mout), land, 0));
  // pair runs: a job matches at most min(nA, nB) postings (both sides strictly
  // ascending); merge tiles bound theirs by min(na, nb + 1), at most one more per tile
  int64_t npairs = 0;
  for (int j = 0; j < nj; j++) {
    JoinQ& J = jobs[(size_t)j];
    J.m_out = d_mout + j;
    J.pair_base = npairs;
    if (!J.count_only) npairs += std::min(J.A.n, J.B.n) + (J.algo == JA_MERGE ? J.ntiles : 0);
  }
  if (int rc = alloc_step(ctx, &S, npairs)) return rc;
  if (int rc = alloc_pieces(ctx, jobs, tile_base, &S)) return rc;
  ChainTables ct;
  if (S.chain)
    if (int rc = chain_setup(ctx, jobs, owner, tile_base, *chq, npairs, d_mout + nj, &S, &ct)) return rc;
  if (int rc = upload_step(ctx, S, jobs, tile_base, ct)) return rc;
  hipEvent_t e0 = tm ? ctx->event() : nullptr, em = tm ? ctx->event() : nullptr, e1 = tm ? ctx->event() : nullptr;
  hipEvent_t c0 = tm ? ctx->event() : nullptr, c1 = tm ? ctx->event() : nullptr;
  hipEvent_t sp = span_open(ctx, tm);
  if (launch_join_step(S, ctx->stream, JoinEvents{e0, em, e1, c0, c1})) return ctx->fail(YRWI_E_HIP, "join launch");
  if (tm) {
    tm->kjoin.push_back({e0, em, e1});
    // the span ends after k_scan_tiles (chained steps: compaction comes later)
    hipEvent_t se = ctx->event();
    hipEventRecord(se, ctx->stream);
    if (S.chain) {
      // c0 / c1 bracket k_chain alone; a step without chain groups launched none
      if (S.ngroups > 0) tm->kchain.push_back({c0, c1});
    } else {
      tm->kcompact.push_back({c0, c1});
    }
    tm->spans.push_back({sp, se});
  }
  if (st) {
    st->n_join_launches++;
    st->n_probe_dispatches += S.tiles > S.merge_tiles;
    st->n_chain_launches += S.chain && S.ngroups > 0 ? 1 : 0;  // k_chain launches (timed in t_chain_ns)
  }
  std::vector<int64_t> mh((size_t)nj, 0);
  HIPCHK(ctx, lane_sync(ctx));
  std::memcpy(mh.data(), land, (size_t)nj * sizeof(int64_t));
  if (st) account_compact(st, jobs, owner, chq, mh);
  if (S.chain) {  // chained jobs' containers, sized by their survivors; the job table again for k_compact
    for (int j = 0; j < nj; j++) {
      JoinQ& J = jobs[(size_t)j];
      if (!J.chain) continue;
      J.out_uid = arena_alloc<uint32_t>(ctx, mh[(size_t)j]);
      J.out_feat = arena_alloc<uint64_t>(ctx, mh[(size_t)j] * FEAT_WORDS);
      if (!J.out_uid || !J.out_feat) return ctx->fail(YRWI_E_NOMEM, "arena");
    }
    if (upload(ctx, S.d_jobs, jobs)) return YRWI_E_HIP;
  }
  for (int j = 0; j < nj; j++) {
    Plan& P = plans[(size_t)owner[(size_t)j]];
    const JoinQ& J = jobs[(size_t)j];
    if (J.count_only) {
      (J.bm3 ? P.cf_count2 : P.cf_count) = mh[(size_t)j];
      continue;
    }
    P.cont = DList{nullptr, nullptr, nullptr, mh[(size_t)j], J.out_uid, J.out_feat, nullptr, J.out_tup,
                   J.out_tup ? J.out_tw : 0};
    P.pieces = J.psum;
    P.npieces = J.psum ? J.ntiles : 0;
  }
  // the containers of the queries the pair cache missed become its entries (a chained step's
  // jobs are compacted later: finish_chained_step fills then)
  if (!S.chain)
    if (int rc = pair_cache_fill(ctx, plans, jobs, owner, mh)) return rc;
  if (S.chain && pend) {
    pend->active = true;
    pend->step = S;
    pend->mh = mh;
    pend->level.assign((size_t)nj, {0, 0, 0, 0, 0});
    const int64_t* hl = reinterpret_cast<const int64_t*>(land) + nj;
    for (int j = 0; j < nj; j++)
      if (jobs[(size_t)j].chain)
        for (int l = 0; l < CHAIN_LVL; l++) pend->level[(size_t)j][(size_t)l] = hl[(int64_t)j * CHAIN_LVL + l];
  }
  return 0;
}

// exclusion (excludeContainers :373-388): mark container rows present in an exclude list
static int run_exclusion(Lane* ctx, std::vector<Plan>& plans, yrwi_stats* st, Timing* tm) {
  std::vector<JoinQ> jobs;
  std::vector<int> owner;
  std::vector<int64_t> tile_base;
  for (auto& P : plans) {
    P.removed = nullptr;
    if (P.empty || P.cont.n == 0 || P.excl.empty()) continue;
    P.removed = arena_alloc<uint8_t>(ctx, P.cont.n);
    if (!P.removed) return ctx->fail(YRWI_E_NOMEM, "arena");
    HIPCHK(ctx, hipMemsetAsync(P.removed, 0, (size_t)P.cont.n, ctx->stream));
    for (auto* E : P.excl) {
      JoinQ J{};
      J.A = P.cont;
      J.B = E->dl();
      J.mode = JM_MARK;
      J.maxd = YRWI_MAX_DISTANCE_ANY;
      J.removed = P.removed;
      if (st) st->bytes_alg += 12 * E->n;
      jobs.push_back(J);
    }
  }
  if (jobs.empty()) return 0;
  JoinStep S;
  S.mark = true;
  layout_jobs(ctx->probe_ratio, ctx->nurls, jobs, owner, tile_base, &S);
  if (st)
    for (const JoinQ& J : jobs) st->bytes_alg_capped += std::min<int64_t>(12 * J.B.n, loaded_bytes(J));
  if (int rc = alloc_step(ctx, &S, 0)) return rc;
  if (upload(ctx, S.d_jobs, jobs, S.d_tile_base, tile_base)) return YRWI_E_HIP;
  hipEvent_t sp = span_open(ctx, tm);
  hipEvent_t pm = tm ? ctx->event() : nullptr, p1 = tm ? ctx->event() : nullptr;
  if (launch_join_step(S, ctx->stream, JoinEvents{nullptr, pm, p1})) return ctx->fail(YRWI_E_HIP, "exclude launch");
  span_close(ctx, tm, sp);
  if (tm) tm->kexcl.push_back({pm, p1});
  if (st) st->n_probe_dispatches += S.tiles > S.merge_tiles;
  return 0;
}

// a query steps at s while it has a list left and its global container (acc_g) is not empty
// (a pair-cache hit has its container already: it never steps)
static bool steps_at(const Plan& P, int64_t acc_g, size_t s) {
  return !P.empty && P.pc_slot < 0 && P.seq.size() > s + 1 && acc_g > 0 && !(P.chain && s > 0);
}

// url selections (resolve_selections): their ids for this pass's kernels (dsel,
// by plan); a single include list is restricted right here (k_sel_pick), a fold of
// two or more chains the selection as its first test (ChainQ)
static int pick_selections(Lane* ctx, std::vector<Plan>& plans, std::vector<uint32_t*>& dsel) {
  std::vector<SelPick> picks;
  for (size_t qi = 0; qi < plans.size(); qi++) {
    Plan& P = plans[qi];
    if (!P.has_sel || P.empty) continue;
    if (!P.sel_uid.empty()) {
      if (!(dsel[qi] = arena_alloc<uint32_t>(ctx, (int64_t)P.sel_uid.size()))) return ctx->fail(YRWI_E_NOMEM, "arena");
      if (upload(ctx, dsel[qi], P.sel_uid)) return YRWI_E_HIP;
    }
    if (P.seq.size() == 1) {  // ReferenceContainer.java:355-370: the one (restricted) container, rows as stored
      const int64_t m = P.sel_ninc[P.seq_term[0]];
      P.cont = DList{nullptr, nullptr, nullptr, 0};
      if (m == 0 || P.seq[0]->n == 0) continue;
      SelPick k{};
      k.L = chain_list(P.seq[0]);
      k.feat = P.seq[0]->feat;
      k.rows = P.seq[0]->rows;
      k.sel = dsel[qi];
      k.nsel = (int64_t)P.sel_uid.size();
      k.out_uid = arena_alloc<uint32_t>(ctx, m);
      k.out_feat = arena_alloc<uint64_t>(ctx, m * FEAT_WORDS);
      k.out_rows = arena_alloc<uint8_t>(ctx, m * YRWI_ROW_BYTES);
      if (!k.out_uid || !k.out_feat || !k.out_rows) return ctx->fail(YRWI_E_NOMEM, "arena");
      P.cont = DList{nullptr, nullptr, k.out_rows, m, k.out_uid, k.out_feat, nullptr, nullptr, 0};
      picks.push_back(k);
    }
  }
  if (!picks.empty()) {
    SelPick* d_pk = arena_alloc<SelPick>(ctx, (int64_t)picks.size());
    if (!d_pk) return ctx->fail(YRWI_E_NOMEM, "arena");
    if (upload(ctx, d_pk, picks)) return YRWI_E_HIP;
    if (launch_sel_pick(d_pk, (int32_t)picks.size(), ctx->stream)) return ctx->fail(YRWI_E_HIP, "selection launch");
  }
  return 0;
}

// Chained folds (ChainQ): every query with lists after its first join step --
// later includes (t <= 4) and / or exclusions -- and no maxDistance filter.  The
// decision rests on global facts only (fold length, exclusion terms in effect),
// so every shard takes it alike.  YRWI_NO_CHAIN=1: the step-by-step fold.
// Sets P.chain / P.cf / P.cf3 and the ChainQ (chq, by plan) of every chained query.
static int plan_chains(Lane* ctx, std::vector<Plan>& plans, const std::vector<int64_t>& acc_g,
                       const std::vector<uint32_t*>& dsel, yrwi_stats* st, std::vector<ChainQ>& chq,
                       bool* any_chain) {
  const char* nc = getenv("YRWI_NO_CHAIN");  // read per call: tests compare both paths in one process
  const bool chain_on = !(nc && atoi(nc));
  // YRWI_CHAIN_CF: 0 never count-first, 2 every 3-term chained fold (tests), default 1 (list 2 the smallest)
  const char* cfe = getenv("YRWI_CHAIN_CF");
  const int cf_mode = cfe ? atoi(cfe) : 1;
  *any_chain = false;
  for (size_t qi = 0; qi < plans.size(); qi++) {
    Plan& P = plans[qi];
    P.chain = false;
    const int t = (int)P.seq.size(), ni = t - 2, ns = P.has_sel ? 1 : 0;
    const bool can = chain_on && !P.empty && P.maxd >= 65535 && acc_g[qi] > 0 && t >= 2 && ni <= CHAIN_MAXI &&
                     ns + ni + P.nexcl_g > 0 && ns + ni + P.nexcl_g <= CHAIN_MAXL;
    if (P.has_sel && !P.empty && t >= 2 && !can) {
      ctx->err_query = (int32_t)qi;
      return ctx->fail(YRWI_E_UNSUPPORTED, "urlselection: a fold of more than four include terms or with a "
                                           "maxDistance filter");
    }
    if (!can) continue;
    ChainQ& C = chq[qi];
    std::memset(&C, 0, sizeof(C));
    C.nl = 0;
    // Count-first (t = 3 whose list 2 is the smallest -- J2's int-wrapped keys put
    // big lists first: C3's 52 such queries make 85 of its 98 M first-step
    // matches): list 0 x list 1 is only counted (its size is step 1's dispatch),
    // the survivors are chained from list 2 (probing list 0, then testing list 1)
    // (t = 4 too: the chain's first test, list 1, leaves |list 0..2| -- step 2's
    // dispatch -- and list 3 follows)
    // (lists 0..2 with bitmaps on every shard -- the planning exchange decides it
    // alike on every rank -- so every shard counts by popcounts)
    P.cf3 = cf_mode != 0 && t == 4 && !ns && P.inc_allbm[P.seq_term[0]] && P.inc_allbm[P.seq_term[1]] &&
            P.inc_allbm[P.seq_term[2]] &&
            (cf_mode == 2 || (P.seq_ng[3] < P.seq_ng[0] && P.seq_ng[3] < P.seq_ng[1] && P.seq_ng[3] < P.seq_ng[2]));
    P.cf = !P.cf3 && cf_mode != 0 && (t == 3 || t == 4) && !ns &&
           (cf_mode == 2 || (P.seq_ng[2] < P.seq_ng[0] && P.seq_ng[2] < P.seq_ng[1]));
    if (ns)  // the selection first: its ids, no heads, no bitmap
      C.l[C.nl++] = ChainList{dsel[qi], nullptr, nullptr, (int64_t)P.sel_uid.size()};
    if (P.cf) {
      C.l[C.nl++] = chain_list(P.seq[1]);
      if (t == 4) C.l[C.nl++] = chain_list(P.seq[3]);
    } else if (P.cf3) {
      C.l[C.nl++] = chain_list(P.seq[1]);
      C.l[C.nl++] = chain_list(P.seq[2]);
    } else {
      for (int l = 0; l < ni; l++) C.l[C.nl++] = chain_list(P.seq[(size_t)l + 2]);
    }
    C.ninc = C.nl;
    C.pos0 = ns;
    C.npos = ni;
    C.perm = P.cf ? 1 : P.cf3 ? 2 : 0;
    for (const ListRec* E : P.excl) C.l[C.nl++] = chain_list(E);  // this shard's lists of the exclusion terms
    if (st)
      for (const ListRec* E : P.excl) st->bytes_alg += 12 * E->n;
    P.excl.clear();  // excluded inside k_chain: no marks, no exclusion step
    P.chain = true;
    *any_chain = true;
  }
  return 0;
}

// The jobs of one fold step and the plan that owns each.
struct StepJobs {
  std::vector<JoinQ> jobs;
  std::vector<int> owner;
  bool any = false, more = false;  // some query steps now / after this step (global decisions)
  // chained queries with a job in this step (plan index): their fold programs
  // (d_cfold, cfold_of[plan] the query's slot or -1) are written once the modes are known
  std::vector<int> chain_q;
  std::vector<int> cfold_of;
  FoldSrc* d_cfold = nullptr;
};

// The JoinQs of fold step s: count-first jobs, deferred or materialised outputs,
// want_sum and the fold programs of the jobs whose A is deferred.
static int build_step_jobs(Lane* ctx, std::vector<Plan>& plans, const std::vector<int64_t>& acc_g,
                           const std::vector<ChainQ>& chq, size_t s, yrwi_stats* st, StepJobs* out) {
  std::vector<JoinQ>& jobs = out->jobs;
  std::vector<int>& owner = out->owner;
  std::vector<FoldSrc> fold;
  std::vector<int> fold_job;
  for (size_t qi = 0; qi < plans.size(); qi++) {
    Plan& P = plans[qi];
    if (!steps_at(P, acc_g[qi], s)) continue;
    out->any = true;
    if (P.seq.size() > s + 2 && !P.chain) out->more = true;
    const DList B = P.seq[s + 1]->dl();
    if (P.chain) P.step_mode[s] = dispatch_mode(acc_g[qi], P.seq_ng[s + 1]);
    if (P.cont.n == 0 || B.n == 0) {  // nothing of this shard survives the step
      P.cont = DList{nullptr, nullptr, nullptr, 0};
      continue;
    }
    JoinQ J{};
    J.A = P.cont;
    J.B = B;
    J.mode = dispatch_mode(acc_g[qi], P.seq_ng[s + 1]);
    J.maxd = P.maxd;
    J.now_ms = P.now_ms;
    J.chained = P.chain ? 1 : 0;
    P.step_mode[s] = J.mode;
    if (P.cf || P.cf3) {  // count-first: list 0 x list 1 counted, the chained job probes list 2 (3) into list 0
      JoinQ K = J;
      K.chained = 0;
      K.count_only = 1;
      if (st) st->bytes_alg += step_bytes(K.mode, K.A.n, K.B.n);
      jobs.push_back(K);
      owner.push_back((int)qi);
      if (P.cf3) {  // and list 0 x list 1 x list 2 (a three-way popcount)
        K.bm3 = P.seq[2]->bm;
        jobs.push_back(K);
        owner.push_back((int)qi);
      }
      const DList L2 = P.seq[P.cf3 ? 3 : 2]->dl();
      if (L2.n == 0) {  // nothing of this shard survives (its count still goes in)
        P.cont = DList{nullptr, nullptr, nullptr, 0};
        continue;
      }
      J.A = L2;
      J.B = P.cont;
      J.mode = JM_ENUM;  // (the chained job's records are folded by fold_chain with the fold's modes)
    }
    int64_t cap = std::min(J.A.n, J.B.n);
    // a chained job's output is allocated once k_chain has counted its survivors
    // (run_join_jobs): its capacity bound min(nA, nB) is far above them
    J.out_uid = P.chain ? nullptr : arena_alloc<uint32_t>(ctx, cap);
    // Deferred multi-term folds: a step before the fold's last writes sources only.
    // It keeps its rows deferred (the rows of lists 0..s+1 they join, no records):
    // the next step joins on url ids alone, and only the last step gathers and
    // folds the records of the rows that survive.
    // A maxDistance filter needs every step's joined features: materialised.
    // A chained query's first step is its only one.
    const bool last = P.seq.size() == s + 2 || P.chain;
    if (!last && P.maxd >= 65535) {
      J.out_tw = (int32_t)s + 2;
      J.out_tup = arena_alloc<int32_t>(ctx, cap * J.out_tw);
      if (!J.out_tup) return ctx->fail(YRWI_E_NOMEM, "arena");
    } else {
      J.out_feat = P.chain ? nullptr : arena_alloc<uint64_t>(ctx, cap * FEAT_WORDS);
      if (!J.out_feat && !P.chain) return ctx->fail(YRWI_E_NOMEM, "arena");
      // the container the rank phase reads: summarised by the compaction unless
      // exclusion marks (run_exclusion, after this) or host counts need a pass over
      // it.  Not a chained fold with exclusions inside the chain: its survivors are
      // sparse in their tiles, and k_compact, four tiles per workgroup, packs them
      // (C3 1.23 -> 1.37 ms/step through k_compact_sum); the chained folds without
      // take the pieces (C4 9.59-9.69 -> 9.24-9.26 ms/step against pieces only for
      // those averaging 64 survivors per tile, 9.47-9.52 at 16)
      const bool chain_excl = P.chain && chq[qi].nl > chq[qi].ninc;
      J.want_sum = last && P.excl.empty() && !chain_excl && P.prof.coeff_authority <= 12 ? 1 : 0;
      if (P.chain) {
        out->chain_q.push_back((int)qi);
      } else if (J.A.tup) {
        FoldSrc F{};
        for (int l = 0; l < J.A.tw; l++) {
          F.feat[l] = P.seq[(size_t)l]->feat;
          F.j5[l] = P.seq[(size_t)l]->j5;
        }
        for (size_t t = 0; t < s; t++) F.mode[t] = P.step_mode[t];
        fold.push_back(F);
        fold_job.push_back((int)jobs.size());
      }
    }
    if (!J.out_uid && !P.chain) return ctx->fail(YRWI_E_NOMEM, "arena");
    if (st) {
      st->bytes_alg += step_bytes(J.mode, J.A.n, J.B.n);
      if (J.mode == JM_ENUM) st->n_enum_steps++; else st->n_test_steps++;
    }
    jobs.push_back(J);
    owner.push_back((int)qi);
  }
  if (!fold.empty()) {  // the fold programs of the jobs whose A is deferred
    FoldSrc* d_fold = arena_alloc<FoldSrc>(ctx, (int64_t)fold.size());
    if (!d_fold) return ctx->fail(YRWI_E_NOMEM, "arena");
    if (upload(ctx, d_fold, fold)) return YRWI_E_HIP;
    for (size_t f = 0; f < fold.size(); f++) jobs[(size_t)fold_job[f]].fold = d_fold + f;
  }
  out->cfold_of.assign(plans.size(), -1);
  if (!out->chain_q.empty()) {
    out->d_cfold = arena_alloc<FoldSrc>(ctx, (int64_t)out->chain_q.size());
    if (!out->d_cfold) return ctx->fail(YRWI_E_NOMEM, "arena");
    for (size_t k = 0; k < out->chain_q.size(); k++) out->cfold_of[(size_t)out->chain_q[k]] = (int)k;
    for (size_t j = 0; j < jobs.size(); j++)
      if (out->cfold_of[(size_t)owner[j]] >= 0) jobs[j].fold = out->d_cfold + out->cfold_of[(size_t)owner[j]];
  }
  return 0;
}

// After the chained step (the first): the fold's later steps take their dispatch
// (J3) from the GLOBAL intersection sizes (k_chain's level counts summed over the
// shards), then the fold programs are written and the step is compacted.
static int finish_chained_step(Lane* ctx, std::vector<Plan>& plans, const std::vector<int64_t>& acc_g,
                               const std::vector<ChainQ>& chq, const StepJobs& J, const PendingCompact& pend,
                               yrwi_stats* st, Timing* tm) {
  const size_t nq = plans.size();
  std::vector<int> cqs;
  for (size_t qi = 0; qi < nq; qi++)
    if (plans[qi].chain && steps_at(plans[qi], acc_g[qi], 0)) cqs.push_back((int)qi);
  std::vector<int> job_of(nq, -1);
  for (size_t j = 0; j < J.jobs.size(); j++)
    if (!J.jobs[j].count_only) job_of[(size_t)J.owner[j]] = (int)j;
  std::vector<int64_t> v(cqs.size() * 2, 0);
  for (size_t k = 0; k < cqs.size(); k++) {
    const Plan& P = plans[(size_t)cqs[k]];
    const int j = job_of[(size_t)cqs[k]];
    if (P.cf3) {  // from list 3: both sizes counted apart
      v[2 * k] = P.cf_count;
      v[2 * k + 1] = P.cf_count2;
    } else if (P.cf) {  // count-first: |list 0 x list 1| counted apart, then |list 0..2|
      v[2 * k] = P.cf_count;
      if (j >= 0 && pend.active) v[2 * k + 1] = pend.level[(size_t)j][1];
    } else if (j >= 0 && pend.active) {  // the intersection sizes after the selection (if any) and include 2
      const int o = chq[(size_t)cqs[k]].pos0;
      v[2 * k] = pend.level[(size_t)j][(size_t)o];
      v[2 * k + 1] = pend.level[(size_t)j][(size_t)o + 1];
    }
  }
  const std::vector<int64_t> loc = v;
  if (int rc = allsum_host(ctx, v)) return rc;
  std::vector<FoldSrc> cf(J.chain_q.size());
  for (size_t k = 0; k < cqs.size(); k++) {
    Plan& P = plans[(size_t)cqs[k]];
    const int t = (int)P.seq.size();
    if (t >= 3) P.step_mode[1] = dispatch_mode(v[2 * k], P.seq_ng[2]);
    if (t >= 4) P.step_mode[2] = dispatch_mode(v[2 * k + 1], P.seq_ng[3]);
    if (st) account_chain_steps(st, P, &loc[2 * k]);
    const int f = J.cfold_of[(size_t)cqs[k]];
    if (f < 0) continue;  // no job of this query on this shard
    FoldSrc& F = cf[(size_t)f];
    for (int l = 0; l < t; l++) {
      F.feat[l] = P.seq[(size_t)l]->feat;
      F.j5[l] = P.seq[(size_t)l]->j5;
    }
    for (int l = 0; l + 1 < t; l++) F.mode[l] = P.step_mode[l];
  }
  if (!cf.empty() && upload(ctx, J.d_cfold, cf)) return YRWI_E_HIP;
  if (pend.active) {
    hipEvent_t c0 = tm ? ctx->event() : nullptr, c1 = tm ? ctx->event() : nullptr;
    if (c0) hipEventRecord(c0, ctx->stream);
    if (launch_compact(pend.step, true, ctx->stream)) return ctx->fail(YRWI_E_HIP, "compact launch");
    if (c1) {
      hipEventRecord(c1, ctx->stream);
      tm->kcompact.push_back({c0, c1});
      tm->spans.push_back({c0, c1});
    }
    if (int rc = pair_cache_fill(ctx, plans, J.jobs, J.owner, pend.mh)) return rc;
  }
  if (st)
    for (size_t k = 0; k < cqs.size(); k++) {
      const int j = job_of[(size_t)cqs[k]];
      const ChainQ& C = chq[(size_t)cqs[k]];
      account_chain_excl(st, C, (j >= 0 && pend.active) ? pend.level[(size_t)j][(size_t)C.ninc] : 0);
    }
  return 0;
}

// the accumulated containers' global sizes decide the next step's dispatch
static int exchange_sizes(Lane* ctx, const std::vector<Plan>& plans, size_t s, std::vector<int64_t>& acc_g) {
  const size_t nq = plans.size();
  std::vector<int64_t> v(nq, 0);
  std::vector<char> stepped(nq, 0);
  for (size_t qi = 0; qi < nq; qi++)
    if (steps_at(plans[qi], acc_g[qi], s)) { v[qi] = plans[qi].cont.n; stepped[qi] = 1; }
  if (int rc = allsum_host(ctx, v)) return rc;
  for (size_t qi = 0; qi < nq; qi++)
    if (stepped[qi]) acc_g[qi] = v[qi];
  return 0;
}

int yrwi::run_join_phase(Lane* ctx, std::vector<Plan>& plans, yrwi_stats* st, Timing* tm) {
  const size_t nq = plans.size();
  std::vector<int64_t> acc_g(nq, 0);  // global size of each query's accumulated container
  for (size_t qi = 0; qi < nq; qi++) {
    Plan& P = plans[qi];
    // (a repeat of an earlier query of the pass, Plan::rep: no step, no chain, no exclusion -- its
    // container stays empty here and the rank phase hands it its representative's)
    if (P.empty || P.rep >= 0) { P.cont = DList{nullptr, nullptr, nullptr, 0}; continue; }
    P.cont = P.seq[0]->dl();  // (a single list under a url selection: restricted by pick_selections)
    acc_g[qi] = P.seq_ng[0];
  }
  std::vector<uint32_t*> dsel(nq, nullptr);
  if (int rc = pick_selections(ctx, plans, dsel)) return rc;
  std::vector<ChainQ> chq(nq);
  bool any_chain = false;
  if (int rc = plan_chains(ctx, plans, acc_g, dsel, st, chq, &any_chain)) return rc;
  // two-term queries whose joined container the pair cache holds take it and join nothing
  if (int rc = pair_cache_lookup(ctx, plans)) return rc;
  for (Plan& P : plans) {
    if (P.pc_slot < 0) continue;
    P.step_mode[0] = dispatch_mode(acc_g[(size_t)(&P - plans.data())], P.seq_ng[1]);
    if (st) {  // the reference's work for the query, as a miss accounts it; no kernel loaded a byte
      st->bytes_alg += step_bytes(P.step_mode[0], P.seq[0]->n, P.seq[1]->n);
      if (P.step_mode[0] == JM_ENUM) st->n_enum_steps++; else st->n_test_steps++;
    }
  }
  for (size_t s = 0;; s++) {
    StepJobs J;
    if (int rc = build_step_jobs(ctx, plans, acc_g, chq, s, st, &J)) return rc;
    if (!J.any) break;
    PendingCompact pend;
    if (!J.jobs.empty())
      if (int rc = run_join_jobs(ctx, plans, J.jobs, J.owner, st, tm, any_chain ? &chq : nullptr, &pend)) return rc;
    if (s == 0 && any_chain) {
      if (int rc = finish_chained_step(ctx, plans, acc_g, chq, J, pend, st, tm)) return rc;
    } else if (pend.active) {
      return ctx->fail(YRWI_E_HIP, "chained step outside the first fold step");
    }
    if (!J.more) break;
    if (int rc = exchange_sizes(ctx, plans, s, acc_g)) return rc;
  }
  return run_exclusion(ctx, plans, st, tm);
}
