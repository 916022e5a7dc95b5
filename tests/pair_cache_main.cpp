// The pair cache's table (csrc/yrwi_pair_cache.h) on the CPU: key, insert / hit /
// double insert, LRU eviction under a byte budget, pins, generations, the block
// allocator.  Built with the sanitizers and run by tests/test_pair_cache_table.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../yacy_search_server_amd/csrc/yrwi_pair_cache.h"

using namespace yrwi;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                               \
    }                                                         \
  } while (0)

// the pair of terms a and b (each term's low word follows from its high word), in the order given
static PairKey K(uint64_t a, uint64_t b, int64_t day = 20741) {
  return pair_key(a, (uint32_t)(a * 7 % 251), b, (uint32_t)(b * 7 % 251), day);
}

// the blocks of the live slots lie inside the block and do not overlap
static bool disjoint(const PairTable& T, const std::vector<int32_t>& slots) {
  std::vector<std::pair<size_t, size_t>> r;
  for (int32_t s : slots) r.push_back({T.at(s).off, T.at(s).off + T.at(s).bytes});
  for (size_t i = 0; i < r.size(); i++) {
    if (r[i].second > T.capacity()) return false;
    for (size_t j = i + 1; j < r.size(); j++)
      if (r[i].first < r[j].second && r[j].first < r[i].second) return false;
  }
  return true;
}

static int test_key() {
  // the terms in either order are one key; the day and each term are part of it
  CHECK(pair_key(5, 1, 9, 2, 7) == pair_key(9, 2, 5, 1, 7));
  CHECK(!(pair_key(5, 1, 9, 2, 7) == pair_key(5, 1, 9, 2, 8)));
  CHECK(!(pair_key(5, 1, 9, 2, 7) == pair_key(5, 1, 9, 3, 7)));
  CHECK(!(pair_key(5, 1, 9, 2, 7) == pair_key(6, 1, 9, 2, 7)));
  CHECK(pair_key(5, 3, 5, 1, 7).a_lo == 1);  // equal high words: the low word orders
  CHECK(PairKeyHash()(pair_key(5, 1, 9, 2, 7)) == PairKeyHash()(pair_key(9, 2, 5, 1, 7)));
  return 0;
}

static int test_insert_hit() {
  PairTable T;
  T.reset(1 << 20);
  CHECK(T.lookup(K(1, 2)) < 0);
  CHECK(T.counters().misses == 1);
  const int32_t s = T.insert(K(1, 2), 1000, 3, 40000, 1 << 20);
  CHECK(s >= 0 && T.at(s).pins == 1 && T.at(s).rows == 1000 && T.at(s).ntiles == 3);
  CHECK(T.at(s).bytes == 40192 && T.at(s).off % 256 == 0);  // rounded up to 256
  // not visible before it is published; a second insert of the key is dropped either way
  CHECK(T.lookup(K(1, 2)) < 0);
  CHECK(T.insert(K(2, 1), 1000, 3, 40000, 1 << 20) < 0);
  CHECK(T.counters().dropped == 1 && T.counters().fills == 1);
  T.publish(s);
  CHECK(T.insert(K(1, 2), 1000, 3, 40000, 1 << 20) < 0);
  CHECK(T.counters().dropped == 2);
  const int32_t h = T.lookup(K(2, 1));
  CHECK(h == s && T.at(s).pins == 2);
  CHECK(T.counters().hits == 1 && T.counters().rows_served == 1000 && T.entries() == 1);
  CHECK(T.bytes_used() == 40192);
  T.unpin(s);
  T.unpin(s);
  CHECK(T.at(s).pins == 0 && T.at(s).used && T.entries() == 1);
  // the clamp day is part of the key
  CHECK(T.lookup(K(1, 2, 20743)) < 0);
  const int32_t d = T.insert(K(1, 2, 20743), 1000, 3, 40000, 1 << 20);
  CHECK(d >= 0 && d != s && T.entries() == 2);
  CHECK(disjoint(T, {s, d}));
  // larger than the block or the budget: refused, nothing evicted
  CHECK(T.insert(K(7, 8), 1, 1, (1 << 20) + 1, 1 << 21) < 0);
  CHECK(T.insert(K(7, 8), 1, 1, 4096, 1024) < 0);
  CHECK(T.entries() == 2 && T.counters().evictions == 0);
  return 0;
}

static int test_lru_budget() {
  PairTable T;
  T.reset(1 << 20);
  const size_t budget = 4 * 65536;  // four entries of 64 KiB
  int32_t s[6];
  for (int i = 0; i < 4; i++) {
    s[i] = T.insert(K(10 + i, 100), 10, 1, 65536, budget);
    CHECK(s[i] >= 0);
    T.publish(s[i]);
    T.unpin(s[i]);
  }
  CHECK(T.bytes_used() == budget && T.counters().evictions == 0);
  // touch 0: 1 is now the least recently used
  int32_t h = T.lookup(K(10, 100));
  CHECK(h == s[0]);
  T.unpin(h);
  s[4] = T.insert(K(14, 100), 10, 1, 65536, budget);
  CHECK(s[4] >= 0 && T.counters().evictions == 1);
  T.publish(s[4]);
  T.unpin(s[4]);
  CHECK(T.lookup(K(11, 100)) < 0);  // evicted
  h = T.lookup(K(10, 100));
  CHECK(h == s[0]);
  T.unpin(h);
  CHECK(T.bytes_used() == budget && T.entries() == 4);
  // an entry of two units evicts the two least recently used: 2 and 3
  s[5] = T.insert(K(15, 100), 10, 1, 2 * 65536, budget);
  CHECK(s[5] >= 0 && T.counters().evictions == 3);
  T.publish(s[5]);
  T.unpin(s[5]);
  CHECK(T.lookup(K(12, 100)) < 0 && T.lookup(K(13, 100)) < 0);
  CHECK(T.bytes_used() == budget && T.entries() == 3);
  CHECK(disjoint(T, {s[0], s[4], s[5]}));
  return 0;
}

static int test_pinned() {
  PairTable T;
  T.reset(3 * 4096);
  int32_t a = T.insert(K(1, 2), 1, 1, 4096, 3 * 4096), b = T.insert(K(3, 4), 1, 1, 4096, 3 * 4096),
          c = T.insert(K(5, 6), 1, 1, 4096, 3 * 4096);
  CHECK(a >= 0 && b >= 0 && c >= 0);
  T.publish(a);
  T.publish(b);
  T.publish(c);
  // every entry pinned: nothing to evict, the insert fails and the entries stay
  CHECK(T.insert(K(7, 8), 1, 1, 4096, 3 * 4096) < 0);
  CHECK(T.entries() == 3 && T.counters().evictions == 0);
  // b unpinned: b goes although a is older
  T.unpin(b);
  const int32_t d = T.insert(K(7, 8), 1, 1, 4096, 3 * 4096);
  CHECK(d >= 0 && T.counters().evictions == 1);
  CHECK(T.lookup(K(3, 4)) < 0);
  int32_t h = T.lookup(K(1, 2));
  CHECK(h == a && T.at(a).pins == 2);
  T.unpin(h);
  // every entry pinned again and the budget full: no room for two units
  CHECK(T.insert(K(9, 9), 1, 1, 2 * 4096, 3 * 4096) < 0);
  T.unpin(a);
  T.unpin(c);
  T.unpin(d);
  const int32_t e = T.insert(K(9, 9), 1, 1, 3 * 4096, 3 * 4096);  // the whole block: the freed blocks coalesce
  CHECK(e >= 0 && T.at(e).off == 0 && T.entries() == 1 && T.counters().evictions == 4);
  return 0;
}

static int test_generation() {
  PairTable T;
  T.reset(1 << 16);
  const int32_t a = T.insert(K(1, 2), 5, 1, 4096, 1 << 16), b = T.insert(K(3, 4), 6, 1, 4096, 1 << 16);
  T.publish(a);
  T.publish(b);
  T.unpin(b);  // a stays pinned: a pass reads it
  const uint64_t g = T.generation();
  T.invalidate();
  CHECK(T.generation() == g + 1 && T.counters().invalidations == 1);
  CHECK(T.entries() == 0);
  CHECK(T.lookup(K(1, 2)) < 0 && T.lookup(K(3, 4)) < 0);  // hidden, pinned or not
  CHECK(T.bytes_used() == 4096);                          // b freed at once, a's block still held
  CHECK(T.at(a).used && T.at(a).pins == 1);
  // the key can be filled again at the new generation while the stale entry is still read
  const int32_t a2 = T.insert(K(1, 2), 7, 1, 4096, 1 << 16);
  CHECK(a2 >= 0 && a2 != a && T.at(a2).gen == g + 1);
  CHECK(disjoint(T, {a, a2}));
  T.publish(a2);
  const int32_t h = T.lookup(K(1, 2));
  CHECK(h == a2 && T.at(h).rows == 7);
  T.unpin(a);  // the stale entry's last pin: freed
  CHECK(!T.at(a).used && T.bytes_used() == 4096);
  T.unpin(a2);
  T.unpin(h);
  T.invalidate();
  CHECK(T.bytes_used() == 0 && T.entries() == 0 && T.counters().invalidations == 2);
  // an evicted entry is never pinned, so eviction frees at once; a stale one frees with its pin
  const int32_t w = T.insert(K(9, 9), 1, 1, 1 << 16, 1 << 16);
  CHECK(w >= 0 && T.at(w).off == 0 && T.pieces() == 1);
  // a fill that could not be enqueued: the entry goes, its key and its block are free again
  const int64_t fills = T.counters().fills;
  T.abort(w);
  CHECK(!T.at(w).used && T.entries() == 0 && T.bytes_used() == 0 && T.pieces() == 0);
  CHECK(T.counters().fills == fills - 1 && T.counters().dropped == 0);
  const int32_t w2 = T.insert(K(9, 9), 1, 3, 1 << 16, 1 << 16);
  CHECK(w2 >= 0 && T.at(w2).off == 0 && T.pieces() == 3);
  T.publish(w2);
  T.abort(w2);  // a published entry is not aborted
  CHECK(T.entries() == 1);
  T.unpin(w2);
  // a bump that finds nothing to drop moves the generation and is not counted
  T.invalidate();
  const uint64_t g2 = T.generation();
  T.invalidate();
  CHECK(T.generation() == g2 + 1 && T.counters().invalidations == 3);
  return 0;
}

// random inserts, hits, unpins and invalidations: blocks never overlap, the budget holds
static int test_random() {
  PairTable T;
  const size_t cap = 1 << 20, budget = 3 << 18;
  T.reset(cap);
  std::vector<int32_t> pinned;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&x]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int it = 0; it < 20000; it++) {
    const uint64_t r = rnd() % 100;
    const PairKey k = K(rnd() % 40, 1000 + rnd() % 3, 20741 + (int64_t)(rnd() % 2));
    if (r < 45) {
      const int32_t s = T.lookup(k);
      if (s >= 0) pinned.push_back(s);
    } else if (r < 80) {
      const int32_t s = T.insert(k, (int64_t)(rnd() % 5000), 1 + (int64_t)(rnd() % 9), 1 + rnd() % 200000, budget);
      if (s >= 0) {
        T.publish(s);
        pinned.push_back(s);
      }
    } else if (r < 98) {
      if (!pinned.empty()) {
        const size_t i = rnd() % pinned.size();
        T.unpin(pinned[i]);
        pinned[i] = pinned.back();
        pinned.pop_back();
      }
    } else {
      T.invalidate();
    }
    CHECK(T.bytes_used() <= budget);
    if (it % 64 == 0) {
      std::set<int32_t> live(pinned.begin(), pinned.end());
      std::vector<int32_t> v(live.begin(), live.end());
      for (int32_t s : v) CHECK(T.at(s).used && T.at(s).pins > 0);
      CHECK(disjoint(T, v));
    }
  }
  for (int32_t s : pinned) T.unpin(s);
  T.invalidate();
  CHECK(T.bytes_used() == 0 && T.entries() == 0);
  const int32_t w = T.insert(K(1, 1), 1, 1, cap, cap);  // everything coalesced back into one block
  CHECK(w >= 0);
  return 0;
}

int main() {
  if (test_key() || test_insert_hit() || test_lru_budget() || test_pinned() || test_generation() || test_random())
    return 1;
  std::printf("pair_cache: OK\n");
  return 0;
}
