// yrwi_pair_cache.h -- the table of the pair cache: the joined
// containers of hot two-term queries, kept across query calls in one device
// block.  This is the host-side bookkeeping only -- key, block allocation, LRU,
// pins, index generation, byte budget -- with no HIP dependency: the owner
// (yrwi_host.h PairCache) holds the device block and the fill events, and a test
// drives the table alone (tests/pair_cache_main.cpp).  Not thread-safe: the owner
// serialises every call.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <iterator>
#include <map>
#include <unordered_map>
#include <vector>

namespace yrwi {

// What a pair's joined container is a function of, beside the index itself (its
// generation is the entry's): the two term keys, sorted, and the day "now" falls
// on (J6 clamps lastModified to it; the normalisation pieces carry the clamped days).
struct PairKey {
  uint64_t a_hi = 0, b_hi = 0;
  uint32_t a_lo = 0, b_lo = 0;
  int64_t day = 0;
  bool operator==(const PairKey& o) const {
    return a_hi == o.a_hi && b_hi == o.b_hi && a_lo == o.a_lo && b_lo == o.b_lo && day == o.day;
  }
};
struct PairKeyHash {
  size_t operator()(const PairKey& k) const {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint64_t v : {k.a_hi, k.b_hi, ((uint64_t)k.a_lo << 32) | k.b_lo, (uint64_t)k.day}) {
      h ^= v;
      h *= 0xFF51AFD7ED558CCDull;
      h ^= h >> 32;
    }
    return (size_t)h;
  }
};
// (t1, t2) in either order, each a 72-bit term key as (hi, lo)
inline PairKey pair_key(uint64_t hi1, uint32_t lo1, uint64_t hi2, uint32_t lo2, int64_t day) {
  const bool swap = hi2 < hi1 || (hi2 == hi1 && lo2 < lo1);
  PairKey k;
  k.a_hi = swap ? hi2 : hi1;
  k.a_lo = swap ? lo2 : lo1;
  k.b_hi = swap ? hi1 : hi2;
  k.b_lo = swap ? lo1 : lo2;
  k.day = day;
  return k;
}

struct PairEntry {
  PairKey key;
  uint64_t gen = 0;       // the index generation it was joined from
  int64_t rows = 0;       // joined rows of the container
  int64_t ntiles = 0;     // its normalisation pieces (one per tile of the join job)
  size_t off = 0;         // its block: [off, off + bytes) of the owner's device block
  size_t bytes = 0;
  int32_t pins = 0;       // passes in flight that read (or fill) it
  uint64_t stamp = 0;     // LRU: the tick of its last use
  bool used = false;      // the slot holds an entry
  bool published = false; // its fill is enqueued and its event recorded: lookups may return it
  bool indexed = false;   // the key map names it (false: stale or evicted, freed once unpinned)
};

struct PairCounters {
  int64_t hits = 0, misses = 0, fills = 0, dropped = 0, evictions = 0, rows_served = 0;
  int64_t invalidations = 0;  // generation bumps that found entries to drop
};

class PairTable {
 public:
  // A block of `bytes` to allocate from; drops every entry (none may be pinned).
  void reset(size_t bytes) {
    slots_.clear();
    free_slots_.clear();
    map_.clear();
    free_.clear();
    if (bytes) free_[0] = bytes;
    capacity_ = bytes;
    used_ = 0;
    live_ = 0;
    pieces_ = 0;
  }
  size_t capacity() const { return capacity_; }
  size_t bytes_used() const { return used_; }  // of every block not yet freed (pinned stale ones included)
  int64_t entries() const { return live_; }    // entries a lookup can find
  int64_t pieces() const { return pieces_; }   // their normalisation pieces (tiles), summed
  const PairCounters& counters() const { return c_; }
  const PairEntry& at(int32_t slot) const { return slots_[(size_t)slot]; }

  // The published entry of `key` at the current generation, pinned and touched; -1: none.
  int32_t lookup(const PairKey& key) {
    auto it = map_.find(key);
    if (it == map_.end() || !slots_[(size_t)it->second].published) {
      c_.misses++;
      return -1;
    }
    PairEntry& e = slots_[(size_t)it->second];
    e.pins++;
    e.stamp = ++tick_;
    c_.hits++;
    c_.rows_served += e.rows;
    return it->second;
  }

  // Reserve `bytes` for a new entry of `key` while at most `budget` bytes are in
  // use, evicting unpinned entries, least recently used first.  Returns its slot,
  // pinned and not yet published, or -1: the key already has an entry (a second
  // insert is dropped), or the bytes cannot be had.  align: a power of two.
  int32_t insert(const PairKey& key, int64_t rows, int64_t ntiles, size_t bytes, size_t budget, size_t align = 256) {
    if (map_.count(key)) {
      c_.dropped++;
      return -1;
    }
    bytes = (bytes + align - 1) & ~(align - 1);
    if (bytes == 0 || bytes > capacity_ || bytes > budget) return -1;
    size_t off = 0;
    while (used_ + bytes > budget || !take(bytes, &off)) {
      const int32_t v = lru_victim();
      if (v < 0) return -1;
      unindex(v);
      c_.evictions++;
      release(v);
    }
    int32_t s;
    if (!free_slots_.empty()) {
      s = free_slots_.back();
      free_slots_.pop_back();
    } else {
      s = (int32_t)slots_.size();
      slots_.emplace_back();
    }
    PairEntry& e = slots_[(size_t)s];
    e = PairEntry{};
    e.key = key;
    e.gen = gen_;
    e.rows = rows;
    e.ntiles = ntiles;
    e.off = off;
    e.bytes = bytes;
    e.pins = 1;
    e.stamp = ++tick_;
    e.used = true;
    e.indexed = true;
    map_[key] = s;
    used_ += bytes;
    live_++;
    pieces_ += ntiles;
    c_.fills++;
    return s;
  }

  // The fill of `slot` is enqueued and its event recorded: lookups may return it.
  void publish(int32_t slot) { slots_[(size_t)slot].published = true; }

  // The fill of `slot` (just inserted, not published, pinned by the filler alone) could not be
  // enqueued: the entry goes, its key can be filled again, the fill is not counted.
  void abort(int32_t slot) {
    PairEntry& e = slots_[(size_t)slot];
    if (!e.used || e.published) return;
    unindex(slot);
    e.pins = 0;
    release(slot);
    c_.fills--;
  }

  // One pin less; an entry that is stale or evicted by then is freed with its last pin.
  void unpin(int32_t slot) {
    PairEntry& e = slots_[(size_t)slot];
    if (e.pins > 0) e.pins--;
    if (e.pins == 0 && !e.indexed) release(slot);
  }

  // The index changed: no entry of an earlier generation is found again; the
  // unpinned ones are freed now, the others with their last pin.
  void invalidate() {
    gen_++;
    if (map_.empty()) return;
    c_.invalidations++;
    std::vector<int32_t> all;
    for (auto& kv : map_) all.push_back(kv.second);
    for (int32_t s : all) {
      unindex(s);
      if (slots_[(size_t)s].pins == 0) release(s);
    }
  }
  uint64_t generation() const { return gen_; }

 private:
  bool take(size_t bytes, size_t* off) {  // first fit
    for (auto it = free_.begin(); it != free_.end(); ++it) {
      if (it->second < bytes) continue;
      *off = it->first;
      const size_t rest = it->second - bytes;
      const size_t at = it->first + bytes;
      free_.erase(it);
      if (rest) free_[at] = rest;
      return true;
    }
    return false;
  }
  void give(size_t off, size_t bytes) {  // coalescing with both neighbours
    auto nx = free_.lower_bound(off);
    if (nx != free_.begin()) {
      auto pv = std::prev(nx);
      if (pv->first + pv->second == off) {
        off = pv->first;
        bytes += pv->second;
        free_.erase(pv);
      }
    }
    if (nx != free_.end() && off + bytes == nx->first) {
      bytes += nx->second;
      free_.erase(nx);
    }
    free_[off] = bytes;
  }
  int32_t lru_victim() const {
    int32_t v = -1;
    for (auto& kv : map_) {
      const PairEntry& e = slots_[(size_t)kv.second];
      if (e.pins == 0 && (v < 0 || e.stamp < slots_[(size_t)v].stamp)) v = kv.second;
    }
    return v;
  }
  void unindex(int32_t s) {
    PairEntry& e = slots_[(size_t)s];
    if (!e.indexed) return;
    map_.erase(e.key);
    e.indexed = false;
    e.published = false;
    live_--;
    pieces_ -= e.ntiles;
  }
  void release(int32_t s) {  // unindexed and unpinned: its block and its slot are free again
    PairEntry& e = slots_[(size_t)s];
    if (!e.used) return;
    give(e.off, e.bytes);
    used_ -= e.bytes;
    e.used = false;
    free_slots_.push_back(s);
  }

  std::vector<PairEntry> slots_;
  std::vector<int32_t> free_slots_;
  std::unordered_map<PairKey, int32_t, PairKeyHash> map_;
  std::map<size_t, size_t> free_;  // free blocks: offset -> bytes
  size_t capacity_ = 0, used_ = 0;
  int64_t live_ = 0, pieces_ = 0;
  uint64_t gen_ = 0, tick_ = 0;
  PairCounters c_;
};

}  // namespace yrwi
