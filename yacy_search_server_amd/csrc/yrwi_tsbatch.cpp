// yrwi_tsbatch.cpp -- yrwi_term_search_batch: TermSearch.joined() of many descriptors in one
// pass, for callers that want the rows (GpuTermSearch / GpuReferenceOrder keep addRWIs in Java).
// Planning and join are those of yrwi_term_search over the whole call (join_containers); the
// rows an exclusion removes are dropped on the device and the kept rows of every container go
// into one packed image (k_local_count, k_tsb_scan, k_tsb_pack in yrwi_kernels.hip) that the
// pack kernel writes into the caller's pinned buffer, or that leaves device scratch in one copy.
#include "yrwi_host.h"

using namespace yrwi;

extern "C" int yrwi_term_search_batch(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, uint8_t* rows40_out,
                                      int64_t cap_rows, int64_t* row_off, yrwi_tsb_stats* st) {
  if (st) std::memset(st, 0, sizeof(*st));
  if (!ctx || nq < 0 || (nq > 0 && (!q || !row_off))) return YRWI_E_ARG;
  if (rows40_out && cap_rows < 0) return ctx->fail(YRWI_E_ARG, "cap_rows is negative");
  if (ctx->world > 1)
    return ctx->fail(YRWI_E_UNSUPPORTED, "batched term search on a shard: a shard holds only its url range of a container");
  if (nq == 0) {
    if (row_off) row_off[0] = 0;
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipSetDevice(ctx->device);
  drain(ctx);
  Lane* L = ctx->lanes[0];
  const int64_t sync0 = L->n_sync, up0 = L->up_bytes, down0 = L->down_bytes, realloc0 = t_realloc;
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

  // one job per container that has rows before the exclusion, in query order; the tables are
  // padded to nq entries so that the bytes uploaded depend on nq alone
  std::vector<LocalJob> ljobs;
  std::vector<int64_t> tile_base, qtile((size_t)nq + 1);
  int64_t joined = 0, tiles = 0;
  for (int32_t i = 0; i < nq; i++) {
    const Plan& P = plans[(size_t)i];
    const int64_t n = P.empty ? 0 : P.cont.n;
    qtile[(size_t)i] = tiles;
    if (n <= 0) continue;
    LocalJob J{};
    J.rows = P.cont.rows;  // a single include list is taken as it is stored (:355-370)
    J.feat = P.cont.feat;
    J.uid = P.cont.uid;
    J.removed = P.removed;
    J.n = n;
    J.now_ms = P.now_ms;
    J.tile0 = tiles;
    J.evjob = i;
    tile_base.push_back(tiles);
    ljobs.push_back(J);
    tiles += (n + LR_TILE - 1) / LR_TILE;
    joined += n;
  }
  qtile[(size_t)nq] = tiles;
  const int32_t nlj = (int32_t)ljobs.size();
  ljobs.resize((size_t)nq);
  tile_base.resize((size_t)nq, tiles);
  if (tiles > 0x7FFFFFFFLL) return ctx->fail(YRWI_E_LIMIT, "more than 2^31 tiles of container rows in one call");

  auto finish = [&](int64_t rows_out, int32_t direct, int64_t pack_ns) {
    if (!st) return;
    st->rows_joined = joined;
    st->rows_out = rows_out;
    st->bytes_h2d = L->up_bytes - up0;
    st->bytes_d2h = L->down_bytes - down0;
    st->launches_tail = tail;
    st->syncs = (int32_t)(L->n_sync - sync0);
    st->direct = direct;
    st->device_allocs = t_realloc - realloc0;
    st->t_pack_ns = pack_ns;
    st->t_total_ns =
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  };
  if (tiles == 0) {  // every container is empty before its exclusion
    std::fill(row_off, row_off + nq + 1, (int64_t)0);
    finish(0, 0, 0);
    return 0;
  }

  // at most `joined` rows are kept: a larger cap_rows promises nothing the call could use
  const int64_t room = rows40_out ? std::min(cap_rows, joined) : 0;
  const bool direct = room > 0 && (reinterpret_cast<uintptr_t>(rows40_out) & 7) == 0 &&
                      ctx->hostreg.contains(rows40_out, (size_t)room * YRWI_ROW_BYTES);
  LocalJob* d_ljobs = arena_alloc<LocalJob>(L, nq);
  int64_t* d_tb = arena_alloc<int64_t>(L, nq);
  int64_t* d_qtile = arena_alloc<int64_t>(L, (int64_t)nq + 1);
  int32_t* d_tcnt = arena_alloc<int32_t>(L, tiles);
  int64_t* d_tstart = arena_alloc<int64_t>(L, tiles + 1);
  int64_t* d_off = arena_alloc<int64_t>(L, (int64_t)nq + 1);
  uint8_t* d_rows = nullptr;  // where the pack kernel stores: nullptr counts only
  if (direct) {
    HIPCHK(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&d_rows), rows40_out, 0));
  } else if (room > 0) {
    if (!(d_rows = arena_alloc<uint8_t>(L, room * YRWI_ROW_BYTES))) return ctx->fail(YRWI_E_NOMEM, "arena");
  }
  if (!d_ljobs || !d_tb || !d_qtile || !d_tcnt || !d_tstart || !d_off) return ctx->fail(YRWI_E_NOMEM, "arena");
  hipStream_t s = L->stream;
  if (upload(L, d_ljobs, ljobs, d_tb, tile_base, d_qtile, qtile)) return ctx->take(L, YRWI_E_HIP);
  tail += 1;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (st) {
    e0 = L->event();
    e1 = L->event();
    HIPCHK(ctx, hipEventRecord(e0, s));
  }
  if (launch_tsb_rows(d_ljobs, d_tb, nlj, tiles, ctx->dkhi, ctx->dklo, d_qtile, nq, d_tcnt, d_tstart, d_off,
                      rows40_out ? cap_rows : 0, d_rows, s))
    return ctx->fail(YRWI_E_HIP, "term search batch launch");
  tail += 3;
  if (st) HIPCHK(ctx, hipEventRecord(e1, s));
  const uint8_t* hb = readback(L, &L->down_stage, d_off, (int64_t)nq + 1, 8, 8);
  if (!hb) return ctx->take(L, YRWI_E_HIP);
  tail += 1;
  HIPCHK(ctx, lane_sync(L));
  int64_t pack_ns = 0;
  if (st) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) pack_ns = (int64_t)((double)ms * 1e6);
    (void)hipGetLastError();  // a statistics event that could not be read is not the call's error
  }
  std::memcpy(row_off, hb, ((size_t)nq + 1) * sizeof(int64_t));
  const int64_t total = row_off[nq];
  if (rows40_out && total > cap_rows) {  // k_tsb_pack saw the same total and stored nothing
    finish(total, 0, pack_ns);
    return ctx->fail(YRWI_E_ARG, "rows40_out capacity too small: row_off[nq] rows are needed");
  }
  if (rows40_out && !direct && total > 0) {
    HIPCHK(ctx, hipMemcpyAsync(rows40_out, d_rows, (size_t)total * YRWI_ROW_BYTES, hipMemcpyDeviceToHost, s));
    tail += 1;
    L->down_bytes += total * YRWI_ROW_BYTES;
    HIPCHK(ctx, lane_sync(L));
  }
  if (direct) L->down_bytes += total * YRWI_ROW_BYTES;
  finish(total, rows40_out && direct ? 1 : 0, pack_ns);
  return 0;
}
