// yrwi_facets.cpp -- yrwi_host_facets_batch: per query of a call the hosts of its joined container
// and how many postings each has (the "results by domain" navigator of a result page).
// Planning, join and the kept-row test are those of yrwi_term_search_batch (join_containers,
// LocalJob, launch_tsb_rows with no output for the per-query row counts); behind them one
// group-by over (query, host) of every container of the call (yrwi_facets.hip).  Only the
// (host, count, url) triples that the caller asked for cross PCIe.
#include "yrwi_host.h"

using namespace yrwi;

extern "C" int yrwi_host_facets_batch(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t order,
                                      int32_t max_hosts, uint8_t* hosts6_out, int64_t* counts_out, uint8_t* urls12_out,
                                      int64_t cap, int64_t* host_off, int64_t* nhosts, int64_t* nrows,
                                      yrwi_facet_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  if (!ctx || nq < 0 || (nq > 0 && (!q || !host_off))) return YRWI_E_ARG;
  if (order != YRWI_FACETS_BY_HOST && order != YRWI_FACETS_BY_COUNT) return ctx->fail(YRWI_E_ARG, "unknown facet order");
  if (max_hosts < 0) return ctx->fail(YRWI_E_ARG, "max_hosts is negative");
  if (cap < 0) return ctx->fail(YRWI_E_ARG, "cap is negative");
  const bool count_only = !hosts6_out && !counts_out;
  if (!count_only && (!hosts6_out || !counts_out))
    return ctx->fail(YRWI_E_ARG, "hosts6_out and counts_out go together");
  if (count_only && urls12_out) return ctx->fail(YRWI_E_ARG, "urls12_out without hosts6_out and counts_out");
  if (nq > (1 << 27)) return ctx->fail(YRWI_E_LIMIT, "more than 2^27 queries in one call");
  if (ctx->world > 1)
    return ctx->fail(YRWI_E_UNSUPPORTED, "host facets on a shard: a shard holds only its url range of a container");
  if (nq == 0) {
    if (host_off) host_off[0] = 0;
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipSetDevice(ctx->device);
  drain(ctx);
  Lane* L = ctx->lanes[0];
  const int64_t up0 = L->up_bytes, down0 = L->down_bytes, realloc0 = t_realloc;
  std::vector<const yrwi_query_desc*> qs((size_t)nq);
  for (int32_t i = 0; i < nq; i++) qs[(size_t)i] = q + i;
  std::vector<Plan> plans;
  L->chain_groups_on_device = true;  // no table of the join phase grows with the lists
  const int jrc = join_containers(ctx, L, qs.data(), nq, &plans);
  L->chain_groups_on_device = false;
  if (jrc) {
    if (L->err_query >= 0) ctx->err = "query " + std::to_string(L->err_query) + ": " + ctx->err;
    return jrc;
  }
  int32_t tail = 0;  // launches and copies from here on
  const int64_t sync0 = L->n_sync;  // and the host waits from here on

  // one job per container that has rows before the exclusion, in query order (the tables of
  // yrwi_term_search_batch, padded to nq entries), and the rows before each job
  std::vector<LocalJob> ljobs;
  std::vector<int64_t> tile_base, row_base, qtile((size_t)nq + 1);
  int64_t joined = 0, tiles = 0;
  for (int32_t i = 0; i < nq; i++) {
    const Plan& P = plans[(size_t)i];
    const int64_t n = P.empty ? 0 : P.cont.n;
    qtile[(size_t)i] = tiles;
    if (n <= 0) continue;
    LocalJob J{};
    J.rows = P.cont.rows;
    J.feat = P.cont.feat;
    J.uid = P.cont.uid;
    J.removed = P.removed;
    J.n = n;
    J.now_ms = P.now_ms;
    J.tile0 = tiles;
    J.evjob = i;  // k_facet_keys: the query of the job's rows
    tile_base.push_back(tiles);
    row_base.push_back(joined);
    ljobs.push_back(J);
    tiles += (n + LR_TILE - 1) / LR_TILE;
    joined += n;
  }
  qtile[(size_t)nq] = tiles;
  const int32_t nlj = (int32_t)ljobs.size();
  ljobs.resize((size_t)nq);
  tile_base.resize((size_t)nq, tiles);
  row_base.resize((size_t)nq, joined);
  if (tiles > 0x7FFFFFFFLL || joined >= 0x7FFFFFFFLL)
    return ctx->fail(YRWI_E_LIMIT, "2^31 or more container rows in one call");

  int64_t group_ns = 0;
  auto finish = [&](int64_t kept, int64_t hosts, int64_t hosts_out) {
    if (!st) return;
    st->rows_joined = joined;
    st->rows_kept = kept;
    st->hosts = hosts;
    st->hosts_out = hosts_out;
    st->bytes_h2d = L->up_bytes - up0;
    st->bytes_d2h = L->down_bytes - down0;
    st->launches_tail = tail;
    st->syncs = (int32_t)(L->n_sync - sync0);
    st->device_allocs = t_realloc - realloc0;
    st->t_group_ns = group_ns;
    st->t_total_ns =
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  };
  if (tiles == 0) {  // every container is empty before its exclusion
    std::fill(host_off, host_off + nq + 1, (int64_t)0);
    if (nhosts) std::fill(nhosts, nhosts + nq, (int64_t)0);
    if (nrows) std::fill(nrows, nrows + nq, (int64_t)0);
    finish(0, 0, 0);
    return 0;
  }

  FacetDev F;
  F.njobs = nlj;
  F.nq = nq;
  F.max_hosts = max_hosts;
  F.tiles = tiles;
  F.n = joined;
  F.dkhi = ctx->dkhi;
  F.dklo = ctx->dklo;
  F.tmp_bytes = facet_tmp_bytes(joined, nq);
  if (!F.tmp_bytes) return ctx->fail(YRWI_E_HIP, "host facets scratch size");
  LocalJob* d_ljobs = arena_alloc<LocalJob>(L, nq);
  int64_t* d_tb = arena_alloc<int64_t>(L, nq);
  int64_t* d_rb = arena_alloc<int64_t>(L, nq);
  int64_t* d_qtile = arena_alloc<int64_t>(L, (int64_t)nq + 1);
  int32_t* d_tcnt = arena_alloc<int32_t>(L, tiles);
  int64_t* d_tstart = arena_alloc<int64_t>(L, tiles + 1);
  // what the host reads back, in one block: host_off (nq + 1), nhosts (nq), the kept-row offsets (nq + 1)
  const int64_t nres = 3 * (int64_t)nq + 2;
  int64_t* d_res = arena_alloc<int64_t>(L, nres);
  F.key = arena_alloc<uint64_t>(L, joined);
  F.skey = arena_alloc<uint64_t>(L, joined);
  F.val = arena_alloc<uint32_t>(L, joined);
  F.sval = arena_alloc<uint32_t>(L, joined);
  F.flag = arena_alloc<int32_t>(L, joined + 1);
  F.hx = arena_alloc<int64_t>(L, joined + 1);
  F.rkey = arena_alloc<uint64_t>(L, joined + 1);
  F.rpos = arena_alloc<uint32_t>(L, joined + 1);
  F.ruid = arena_alloc<uint32_t>(L, joined + 1);
  F.qstart = arena_alloc<int64_t>(L, (int64_t)nq + 1);
  F.nwrite = arena_alloc<int64_t>(L, (int64_t)nq + 1);
  F.tmp = L->arena.alloc(F.tmp_bytes);
  if (!d_ljobs || !d_tb || !d_rb || !d_qtile || !d_tcnt || !d_tstart || !d_res || !F.key || !F.skey || !F.val ||
      !F.sval || !F.flag || !F.hx || !F.rkey || !F.rpos || !F.ruid || !F.qstart || !F.nwrite || !F.tmp)
    return ctx->fail(YRWI_E_NOMEM, "arena");
  F.jobs = d_ljobs;
  F.tile_base = d_tb;
  F.row_base = d_rb;
  F.host_off = d_res;
  F.nhosts = d_res + nq + 1;
  int64_t* d_rowoff = d_res + 2 * (int64_t)nq + 1;
  hipStream_t s = L->stream;
  if (upload(L, d_ljobs, ljobs, d_tb, tile_base, d_rb, row_base, d_qtile, qtile)) return ctx->take(L, YRWI_E_HIP);
  tail += 1;
  // the per-query kept rows: the counting form of the batched term search (its pack kernel stores nothing)
  if (launch_tsb_rows(d_ljobs, d_tb, nlj, tiles, ctx->dkhi, ctx->dklo, d_qtile, nq, d_tcnt, d_tstart, d_rowoff, 0,
                      nullptr, s))
    return ctx->fail(YRWI_E_HIP, "host facets row count launch");
  tail += 3;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
  if (st) {
    e0 = L->event();
    e1 = L->event();
    e2 = L->event();
    e3 = L->event();
    HIPCHK(ctx, hipEventRecord(e0, s));
  }
  if (launch_facet_group(F, s)) return ctx->fail(YRWI_E_HIP, "host facets group launch");
  tail += FACET_GROUP_LAUNCHES;
  if (st) HIPCHK(ctx, hipEventRecord(e1, s));
  const uint8_t* hb = readback(L, &L->down_stage, d_res, nres, 8, 8);
  if (!hb) return ctx->take(L, YRWI_E_HIP);
  tail += 1;
  HIPCHK(ctx, lane_sync(L));
  auto elapsed = [&](hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) group_ns += (int64_t)((double)ms * 1e6);
    (void)hipGetLastError();  // a statistics event that could not be read is not the call's error
  };
  if (st) elapsed(e0, e1);
  const int64_t* res = reinterpret_cast<const int64_t*>(hb);
  std::memcpy(host_off, res, ((size_t)nq + 1) * sizeof(int64_t));
  const int64_t* h_nh = res + nq + 1;
  const int64_t* h_ro = res + 2 * (int64_t)nq + 1;
  int64_t nruns = 0;
  for (int32_t i = 0; i < nq; i++) {
    nruns += h_nh[i];
    if (nhosts) nhosts[i] = h_nh[i];
    if (nrows) nrows[i] = h_ro[i + 1] - h_ro[i];
  }
  const int64_t kept = h_ro[nq], total = host_off[nq];
  if (count_only || total == 0) {
    finish(kept, nruns, total);
    return 0;
  }
  if (total > cap) {
    finish(kept, nruns, total);
    return ctx->fail(YRWI_E_ARG, "facet capacity too small: host_off[nq] hosts are needed");
  }
  if (nruns > joined) return ctx->fail(YRWI_E_HIP, "host facets: more runs than rows");

  uint8_t* d_h6 = arena_alloc<uint8_t>(L, total * 6);
  int64_t* d_cnt = arena_alloc<int64_t>(L, total);
  uint8_t* d_u12 = urls12_out ? arena_alloc<uint8_t>(L, total * 12) : nullptr;
  if (!d_h6 || !d_cnt || (urls12_out && !d_u12)) return ctx->fail(YRWI_E_NOMEM, "arena");
  if (st) HIPCHK(ctx, hipEventRecord(e2, s));
  if (order == YRWI_FACETS_BY_COUNT) {
    const size_t ob = facet_order_tmp_bytes(nruns, nq);
    void* otmp = ob ? L->arena.alloc(ob) : nullptr;
    if (!otmp) return ctx->fail(YRWI_E_NOMEM, "arena");
    if (launch_facet_order(F, nruns, otmp, ob, s)) return ctx->fail(YRWI_E_HIP, "host facets order launch");
    tail += 2;
  }
  if (launch_facet_pack(F, total, order == YRWI_FACETS_BY_COUNT, d_h6, d_cnt, d_u12, s))
    return ctx->fail(YRWI_E_HIP, "host facets pack launch");
  tail += 1;
  if (st) HIPCHK(ctx, hipEventRecord(e3, s));
  HIPCHK(ctx, hipMemcpyAsync(hosts6_out, d_h6, (size_t)total * 6, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(counts_out, d_cnt, (size_t)total * 8, hipMemcpyDeviceToHost, s));
  tail += 2;
  L->down_bytes += total * 14;
  if (urls12_out) {
    HIPCHK(ctx, hipMemcpyAsync(urls12_out, d_u12, (size_t)total * 12, hipMemcpyDeviceToHost, s));
    tail += 1;
    L->down_bytes += total * 12;
  }
  HIPCHK(ctx, lane_sync(L));
  if (st) elapsed(e2, e3);
  finish(kept, nruns, total);
  return 0;
}
