// tsx_pool_map.hpp -- the bookkeeping of libtsx's device memory pool (tsx_pool.hip): which bytes of which slab are handed out.
// Plain C++, no HIP: every byte of every slab belongs to exactly one piece; pieces are ordered by address; a request takes the
// smallest free piece that holds it (best fit) and splits it; a returned piece is merged with free neighbours of the SAME slab.
// A piece may carry red zones (TSX_POOL_POISON, tsx_pool.hip): kZone bytes in front of what the caller gets and, behind it, the
// rest of the piece (the rounding slack + kZone).  The caller holds the USER pointer: the piece's start, or start + kZone if zoned.
// tests/c/pool_map_test.cpp (CPU, `-m "not gpu"`) runs random request sequences against the invariants.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

struct TsxPiece {
  size_t bytes;
  int slab;
  bool free;
  size_t user = 0;      // zoned: the bytes the caller asked for
  bool zoned = false;   // red zones around the caller's bytes (free pieces never are)
};
struct TsxPieceMap {
  static constexpr size_t kAlign = 256;
  static constexpr size_t kZone = 4096;
  using It = std::map<char *, TsxPiece>::iterator;
  std::map<char *, TsxPiece> pieces;
  std::vector<std::pair<char *, size_t>> slabs;
  size_t bytes = 0, live = 0;

  static size_t rounded(size_t n) { return ((n ? n : 1) + kAlign - 1) & ~(kAlign - 1); }
  static size_t zoned_bytes(size_t req) { return kZone + rounded(req) + kZone; }
  static char *user_of(const std::pair<char *const, TsxPiece> &kv) { return kv.second.zoned ? kv.first + kZone : kv.first; }
  size_t free_total() const {
    size_t t = 0;
    for (auto &kv : pieces)
      if (kv.second.free) t += kv.second.bytes;
    return t;
  }
  void add_slab(char *base, size_t n) {
    slabs.emplace_back(base, n);
    bytes += n;
    pieces[base] = TsxPiece{n, (int)slabs.size() - 1, true};
  }
  // -> pointer, or nullptr if no free piece holds `need` (already rounded) bytes
  char *take(size_t need) {
    auto best = pieces.end();
    for (auto it = pieces.begin(); it != pieces.end(); ++it)
      if (it->second.free && it->second.bytes >= need && (best == pieces.end() || it->second.bytes < best->second.bytes)) best = it;
    if (best == pieces.end()) return nullptr;
    const TsxPiece pc = best->second;
    char *p = best->first;
    if (pc.bytes > need) pieces[p + need] = TsxPiece{pc.bytes - need, pc.slab, true};
    best->second = TsxPiece{need, pc.slab, false};
    live += need;
    return p;
  }
  // a zoned piece of zoned_bytes(req) bytes; -> its user pointer (start + kZone), or nullptr
  char *take_zoned(size_t req) {
    char *p = take(zoned_bytes(req));
    if (!p) return nullptr;
    TsxPiece &pc = pieces[p];
    pc.zoned = true;
    pc.user = req;
    return p + kZone;
  }
  // the piece whose user pointer is `u` (a plain piece's start -- free ones too -- or a live zoned piece's start + kZone), or end().
  // Unambiguous: a live zoned piece covers its own user pointer, so no other piece starts there.
  It find_user(const char *u) {
    auto it = pieces.find(const_cast<char *>(u));
    if (it != pieces.end() && !it->second.zoned) return it;
    if ((uintptr_t)u < kZone) return pieces.end();
    it = pieces.find(const_cast<char *>(u) - kZone);
    return it != pieces.end() && it->second.zoned && !it->second.free ? it : pieces.end();
  }
  bool owns(const char *u) { return find_user(u) != pieces.end(); }
  // false: not the user pointer of a live piece of this map
  bool give(char *u) {
    auto it = find_user(u);
    if (it == pieces.end() || it->second.free) return false;
    it->second.free = true;
    it->second.zoned = false;
    it->second.user = 0;
    live -= it->second.bytes;
    auto nx = std::next(it);
    if (nx != pieces.end() && nx->second.free && nx->second.slab == it->second.slab && nx->first == it->first + it->second.bytes) {
      it->second.bytes += nx->second.bytes;
      pieces.erase(nx);
    }
    if (it != pieces.begin()) {
      auto pv = std::prev(it);
      if (pv->second.free && pv->second.slab == it->second.slab && pv->first + pv->second.bytes == it->first) {
        pv->second.bytes += it->second.bytes;
        pieces.erase(it);
      }
    }
    return true;
  }
};
