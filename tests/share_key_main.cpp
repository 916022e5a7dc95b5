// Stand-alone check of yrwi_share.h (tests/test_share_key.py compiles it with the
// address and undefined-behaviour sanitizers and runs it): which plans of a pass
// are repeats of which.  SharePlan carries the members of yrwi_host.h's Plan that
// the key reads, filled the way plan_query leaves them (terms sorted and unique).

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../yacy_search_server_amd/csrc/yrwi_share.h"

struct Key {
  uint64_t hi;
  uint32_t lo;
  bool operator<(const Key& o) const { return hi < o.hi || (hi == o.hi && lo < o.lo); }
  bool operator==(const Key& o) const { return hi == o.hi && lo == o.lo; }
};

struct SharePlan {
  int ninc = 0, nexc = 0;
  Key inc[YRWI_MAX_TERMS], exc[YRWI_MAX_TERMS];
  int32_t maxd = YRWI_MAX_DISTANCE_ANY, k = 10;
  yrwi_profile prof{};
  uint8_t lang[2] = {'e', 'n'};
  int32_t lang_ok = 1;
  int64_t now_ms = 1792000000000ll;
  const yrwi_filter* filter = nullptr;
  bool has_sel = false;
};

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                             \
    }                                                         \
  } while (0)

// plan_query's HandleSet: sorted, unique
static SharePlan plan(std::vector<uint32_t> inc, std::vector<uint32_t> exc = {}) {
  SharePlan P;
  std::memset(&P.prof, 0, sizeof(P.prof));
  P.prof.coeff_date = 9;
  P.prof.coeff_termfrequency = 8;
  auto put = [](std::vector<uint32_t>& v, Key* out) {
    int n = 0;
    for (uint32_t t : v) out[n++] = Key{0x1234500000000000ull + t / 3, t % 3};
    std::sort(out, out + n);
    return (int)(std::unique(out, out + n) - out);
  };
  P.ninc = put(inc, P.inc);
  P.nexc = put(exc, P.exc);
  return P;
}

static std::vector<int32_t> groups(const std::vector<SharePlan>& v, int64_t* shared = nullptr) {
  std::vector<int32_t> rep;
  const int64_t s = yrwi::share_groups(v, &rep);
  if (shared) *shared = s;
  int64_t c = 0;
  for (int32_t r : rep) c += r >= 0;
  CHECK(c == s);
  CHECK(rep.size() == v.size());
  return rep;
}

int main() {
  // reordered and duplicated include terms are one query; the earliest represents
  {
    std::vector<SharePlan> v{plan({5, 9}), plan({7}), plan({9, 5}), plan({5, 9, 5}), plan({5}), plan({9, 9, 5, 5})};
    int64_t s = 0;
    const std::vector<int32_t> rep = groups(v, &s);
    CHECK(s == 3);
    CHECK(rep[0] == -1 && rep[1] == -1 && rep[4] == -1);
    CHECK(rep[2] == 0 && rep[3] == 0 && rep[5] == 0);
  }
  // every field of the key splits a group
  {
    const SharePlan base = plan({5, 9}, {11});
    std::vector<SharePlan> v{base};
    SharePlan p = base; p.k = 11; v.push_back(p);
    p = base; p.maxd = 1; v.push_back(p);
    p = base; p.lang[1] = 'o'; v.push_back(p);
    p = base; p.lang[0] = 'd'; v.push_back(p);
    p = base; p.lang_ok = 0; v.push_back(p);
    p = base; p.now_ms += 1; v.push_back(p);
    v.push_back(plan({5, 9}, {12}));
    v.push_back(plan({5, 9}, {11, 12}));
    v.push_back(plan({5, 9}));
    v.push_back(plan({5, 9, 11}));
    v.push_back(plan({5}, {9, 11}));
    // include and exclude sets swapped: the same keys in other roles
    v.push_back(plan({11}, {5, 9}));
    // two keys that differ in the low part only
    v.push_back(plan({3}));
    v.push_back(plan({4}));
    const size_t nprof = sizeof(yrwi_profile) / sizeof(int32_t);
    for (size_t f = 0; f < nprof; f++) {  // any profile field
      p = base;
      reinterpret_cast<int32_t*>(&p.prof)[f] += 1;
      v.push_back(p);
    }
    int64_t s = -1;
    const std::vector<int32_t> rep = groups(v, &s);
    CHECK(s == 0);
    for (int32_t r : rep) CHECK(r == -1);
    // and a true copy of every one of them is found, each by its own first occurrence
    const size_t n = v.size();
    for (size_t i = 0; i < n; i++) v.push_back(v[n - 1 - i]);
    const std::vector<int32_t> rep2 = groups(v, &s);
    CHECK(s == (int64_t)n);
    for (size_t i = 0; i < n; i++) {
      CHECK(rep2[i] == -1);
      CHECK(rep2[n + i] == (int32_t)(n - 1 - i));
    }
  }
  // a filter or a url selection never shares, neither as a repeat nor as a representative
  {
    yrwi_filter F;
    std::memset(&F, 0, sizeof(F));
    SharePlan f = plan({5, 9});
    f.filter = &F;
    SharePlan s = plan({5, 9});
    s.has_sel = true;
    std::vector<SharePlan> v{f, s, plan({5, 9}), f, s, plan({9, 5})};
    int64_t n = 0;
    const std::vector<int32_t> rep = groups(v, &n);
    CHECK(n == 1);
    CHECK(rep[0] == -1 && rep[1] == -1 && rep[2] == -1 && rep[3] == -1 && rep[4] == -1);
    CHECK(rep[5] == 2);
  }
  // the representative is always the earliest member, and never itself a repeat
  {
    std::vector<SharePlan> v;
    for (int i = 0; i < 600; i++) v.push_back(plan({(uint32_t)(i * 7 % 13), (uint32_t)(i * 5 % 11)}));
    v.push_back(plan({}));  // no include term at all: a query like any other
    v.push_back(plan({}));
    const std::vector<int32_t> rep = groups(v);
    for (size_t i = 0; i < v.size(); i++) {
      int32_t first = -1;
      for (size_t j = 0; j < i && first < 0; j++)
        if (yrwi::share_cmp(yrwi::share_key(v[j]), yrwi::share_key(v[i])) == 0) first = (int32_t)j;
      CHECK(rep[i] == first);
      if (rep[i] >= 0) CHECK(rep[(size_t)rep[i]] == -1);
    }
  }
  // nothing to group
  {
    std::vector<SharePlan> v;
    int64_t s = -1;
    CHECK(groups(v, &s).empty() && s == 0);
  }
  if (failures) return 1;
  std::printf("share_key: OK\n");
  return 0;
}
