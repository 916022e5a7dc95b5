// yrwi_share.h -- identical queries of one pass run once: the
// canonical key of a planned query and the grouping of a pass's plans by it.
// No HIP dependency: PlanT is yrwi_host.h's Plan, or a test's stand-in with the
// same members (tests/share_key_main.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/yrwi.h"

namespace yrwi {

// What decides a query's result on one context, as plan_query / plan_finish leave
// it in the plan: the sorted unique include and exclude keys, maxDistance, k, the
// profile by value, the language and the resolved "now".
struct ShareKey {
  int32_t ninc = 0, nexc = 0;
  uint64_t inc_hi[YRWI_MAX_TERMS] = {}, exc_hi[YRWI_MAX_TERMS] = {};
  uint32_t inc_lo[YRWI_MAX_TERMS] = {}, exc_lo[YRWI_MAX_TERMS] = {};
  int32_t maxd = 0, k = 0;
  int32_t prof[sizeof(yrwi_profile) / sizeof(int32_t)] = {};
  uint8_t lang[2] = {0, 0};
  int32_t lang_ok = 0;
  int64_t now_ms = 0;
};
static_assert(sizeof(yrwi_profile) % sizeof(int32_t) == 0, "yrwi_profile: int32 coefficients only");

// A query with a filter (its flagcount and doubledom order are per query) or a
// url selection never shares.
template <class PlanT>
inline bool share_candidate(const PlanT& P) {
  return P.filter == nullptr && !P.has_sel;
}

template <class PlanT>
inline ShareKey share_key(const PlanT& P) {
  ShareKey K;
  K.ninc = P.ninc;
  K.nexc = P.nexc;
  for (int i = 0; i < P.ninc; i++) { K.inc_hi[i] = P.inc[i].hi; K.inc_lo[i] = P.inc[i].lo; }
  for (int i = 0; i < P.nexc; i++) { K.exc_hi[i] = P.exc[i].hi; K.exc_lo[i] = P.exc[i].lo; }
  K.maxd = P.maxd;
  K.k = P.k;
  std::memcpy(K.prof, &P.prof, sizeof(K.prof));
  K.lang[0] = P.lang[0];
  K.lang[1] = P.lang[1];
  K.lang_ok = P.lang_ok;
  K.now_ms = P.now_ms;
  return K;
}

// total order of the keys, field by field (no padding bytes compared)
inline int share_cmp(const ShareKey& a, const ShareKey& b) {
  auto c = [](auto x, auto y) { return x < y ? -1 : y < x ? 1 : 0; };
  if (int r = c(a.ninc, b.ninc)) return r;
  if (int r = c(a.nexc, b.nexc)) return r;
  for (int i = 0; i < a.ninc; i++) {
    if (int r = c(a.inc_hi[i], b.inc_hi[i])) return r;
    if (int r = c(a.inc_lo[i], b.inc_lo[i])) return r;
  }
  for (int i = 0; i < a.nexc; i++) {
    if (int r = c(a.exc_hi[i], b.exc_hi[i])) return r;
    if (int r = c(a.exc_lo[i], b.exc_lo[i])) return r;
  }
  if (int r = c(a.maxd, b.maxd)) return r;
  if (int r = c(a.k, b.k)) return r;
  if (int r = std::memcmp(a.prof, b.prof, sizeof(a.prof))) return r;
  if (int r = std::memcmp(a.lang, b.lang, sizeof(a.lang))) return r;
  if (int r = c(a.lang_ok, b.lang_ok)) return r;
  return c(a.now_ms, b.now_ms);
}

// YRWI_SHARE=0 turns the sharing off (read per call; tests and A/B measurements)
inline bool share_enabled() {
  const char* e = getenv("YRWI_SHARE");
  return !(e && e[0] == '0');
}

// a hash of the key's terms and scalars (equal keys hash alike; share_cmp decides)
inline uint64_t share_hash(const ShareKey& K) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  auto mix = [&h](uint64_t v) {
    h ^= v;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  };
  mix(((uint64_t)(uint32_t)K.ninc << 32) | (uint32_t)K.nexc);
  for (int i = 0; i < K.ninc; i++) { mix(K.inc_hi[i]); mix(K.inc_lo[i]); }
  for (int i = 0; i < K.nexc; i++) { mix(K.exc_hi[i]); mix(K.exc_lo[i]); }
  mix(((uint64_t)(uint32_t)K.maxd << 32) | (uint32_t)K.k);
  mix((uint64_t)K.now_ms);
  return h;
}

// rep[i]: the earliest of `plans` with plan i's key, or -1 when that is plan i
// itself (or plan i never shares).  Returns the number of plans with rep >= 0.
// `plans` is a pass, or a batch part before its passes are cut (the caller then
// keeps a group's members of one pass together, run_batch_part_).
template <class PlanT>
inline int64_t share_groups(const std::vector<PlanT>& plans, std::vector<int32_t>* rep) {
  const size_t n = plans.size();
  rep->assign(n, -1);
  std::vector<ShareKey> key(n);
  std::vector<std::pair<uint64_t, int32_t>> idx;  // (hash, plan): equal keys side by side, in plan order
  for (size_t i = 0; i < n; i++)
    if (share_candidate(plans[i])) {
      key[i] = share_key(plans[i]);
      idx.push_back({share_hash(key[i]), (int32_t)i});
    }
  std::sort(idx.begin(), idx.end());
  int64_t shared = 0;
  for (size_t r0 = 0; r0 < idx.size();) {
    size_t r1 = r0 + 1;
    while (r1 < idx.size() && idx[r1].first == idx[r0].first) r1++;
    // one hash (a few plans): every member takes the first earlier member with its key
    for (size_t j = r0 + 1; j < r1; j++)
      for (size_t f = r0; f < j; f++) {
        if ((*rep)[(size_t)idx[f].second] >= 0) continue;  // itself a repeat: its representative comes earlier
        if (share_cmp(key[(size_t)idx[f].second], key[(size_t)idx[j].second]) != 0) continue;
        (*rep)[(size_t)idx[j].second] = idx[f].second;
        shared++;
        break;
      }
    r0 = r1;
  }
  return shared;
}

}  // namespace yrwi
