// One window of the backtrack's walk (enc_parse.hip backtrack_kernel), for all 64 lanes at
// once.  Host and device: the kernel runs it on a wave (lane x holds the node at offset x from
// the window's top; a gather is a ds_bpermute), tests/backtrack_window_host_main.cpp on arrays
// of 64 -- the same text, so the arithmetic the sanitizers and the exhaustive check run is the
// product's.
//
// A window is 64 positions, offset 0 at its top (the highest position); the walk goes down.
// Node x is a copy's end when len[x] != 0 and a literal's otherwise: its successor on a
// backward path is x + max(len[x], 1).  Offsets at or beyond nvalid lie outside (before the
// segment's start, or simply in the next window): the caller passes len = 0 there.  The path
// from the entry x0 < nvalid is x0, next(x0), next(next(x0)), ...; lane k ends up with its
// k-th node:
//   - next^(2^i) for i = 0..5 by pointer doubling (a gather of next at next), 64 absorbing;
//   - lane k composes the powers of k's set bits from x0 (a gather each);
//   - lane k gathers len at its node.
// The path's nodes rise strictly, so the lanes whose node is inside the window are 0..npath-1,
// and the ballot of "inside and a copy" lists the window's copy nodes in walk order.  The
// literals between two consecutive copy nodes at path indices k < k' number k' - k - 1 (every
// path node between them is a literal's), those before the first copy its index, those after
// the last one npath - 1 - its index.  The path leaves the window at the last inside node's
// successor (not clamped: a copy may leave by any amount).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MIB_BT_HD __host__ __device__ __forceinline__
#else
#define MIB_BT_HD inline
#endif

namespace mib {
namespace enc {

struct BtWindow {
  uint64_t copies;   // bit k: the path's k-th node is inside the window and a copy's end
  uint32_t npath;    // path nodes inside the window (>= 1: x0 is one)
  uint32_t exit;     // the offset at which the path leaves the window (>= nvalid)
};

// W: the lanes.  W::Reg is a value per lane; W::at(r, x) lane x's (on the device: the calling
// lane's own); w.each(f) the Reg of f(lane); w.gather(idx, v) lane idx's v, idx < 64 (any lane
// for another idx); w.ballot(r) the lanes with r != 0; w.read(r, x) lane x's r as a scalar.
// node, nlen: lane k's path node (64: the path has left the 64 offsets) and the copy length
// there (0: a literal's node, or outside the window).
template <class W>
MIB_BT_HD BtWindow bt_window(const W &w, const typename W::Reg &len, uint32_t x0, uint32_t nvalid, typename W::Reg &node,
                             typename W::Reg &nlen) {
  using R = typename W::Reg;
  R nx = w.each([&](uint32_t x) {
    const uint32_t l = W::at(len, x), n = x + (l ? l : 1u);
    return n < 64u ? n : 64u;
  });
  R p = w.each([&](uint32_t) { return x0; });
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 6; i++) {
    const R t = w.gather(p, nx);   // next^(2^i) at the node so far
    p = w.each([&](uint32_t k) {
      const uint32_t q = W::at(p, k);
      return ((k >> i) & 1u) && q < 64u ? W::at(t, k) : q;
    });
    if (i < 5) {
      const R u = w.gather(nx, nx);
      nx = w.each([&](uint32_t x) { return W::at(nx, x) < 64u ? W::at(u, x) : 64u; });
    }
  }
  const R l = w.gather(p, len);
  nlen = w.each([&](uint32_t k) { return W::at(p, k) < nvalid ? W::at(l, k) : 0u; });
  node = p;
  const uint64_t inside = w.ballot(w.each([&](uint32_t k) { return W::at(p, k) < nvalid ? 1u : 0u; }));
  BtWindow r;
  r.copies = w.ballot(nlen);
  r.npath = (uint32_t)__builtin_popcountll(inside);
  const R succ = w.each([&](uint32_t k) {
    const uint32_t c = W::at(nlen, k);
    return W::at(p, k) + (c ? c : 1u);
  });
  r.exit = w.read(succ, r.npath - 1u);
  return r;
}

// What a copy node at path index k makes of the window's ballot (k < 64, bit k of copies set
// for the first two):
// its rank among the window's copy nodes, in walk order
MIB_BT_HD uint32_t bt_rank(uint64_t copies, uint32_t k) { return (uint32_t)__builtin_popcountll(copies & ((1ull << k) - 1ull)); }
// the literals the walk passes after it: to the next copy node, or (the last) to the path's
// leaving the window
MIB_BT_HD uint32_t bt_lits_after(uint64_t copies, uint32_t npath, uint32_t k) {
  const uint64_t rest = k < 63u ? copies >> (k + 1u) : 0ull;
  return rest ? (uint32_t)__builtin_ctzll(rest) : npath - 1u - k;
}
MIB_BT_HD uint32_t bt_first(uint64_t copies) { return (uint32_t)__builtin_ctzll(copies); }        // copies != 0
MIB_BT_HD uint32_t bt_last(uint64_t copies) { return 63u - (uint32_t)__builtin_clzll(copies); }   // copies != 0

// ---------------------------------------------------------------- arrays of 64 as the lanes
struct BtHostWave {
  struct Reg {
    uint32_t v[64];
  };
  static uint32_t at(const Reg &r, uint32_t x) { return r.v[x]; }
  template <class F>
  Reg each(F f) const {
    Reg r;
    for (uint32_t x = 0; x < 64; x++) r.v[x] = f(x);
    return r;
  }
  Reg gather(const Reg &idx, const Reg &v) const {
    Reg r;
    for (uint32_t x = 0; x < 64; x++) r.v[x] = v.v[idx.v[x] & 63u];   // (ds_bpermute wraps too)
    return r;
  }
  uint64_t ballot(const Reg &r) const {
    uint64_t m = 0;
    for (uint32_t x = 0; x < 64; x++) m |= (uint64_t)(r.v[x] != 0) << x;
    return m;
  }
  uint32_t read(const Reg &r, uint32_t x) const { return r.v[x]; }
};

// The window as the kernel consumes it, spelled out: the copy nodes in walk order, the
// literals before each (lits[j]: between copy j - 1, or the entry, and copy j), the literals
// after the last (all the path's, with no copy) and the exit.
struct BtWalk {
  uint32_t ncopy, node[64], lits[64], trail, exit;
};
inline BtWalk bt_walk_window(const uint32_t len[64], uint32_t x0, uint32_t nvalid) {
  BtHostWave w;
  BtHostWave::Reg l, node, nlen;
  for (uint32_t x = 0; x < 64; x++) l.v[x] = x < nvalid ? len[x] : 0u;
  const BtWindow r = bt_window(w, l, x0, nvalid, node, nlen);
  BtWalk o{};
  o.exit = r.exit;
  o.trail = r.npath;
  for (uint32_t k = 0; k < 64; k++)
    if ((r.copies >> k) & 1ull) {
      const uint32_t j = bt_rank(r.copies, k);
      o.node[j] = node.v[k];
      if (j == 0) o.lits[0] = bt_first(r.copies);
      const uint32_t after = bt_lits_after(r.copies, r.npath, k);
      if (k == bt_last(r.copies)) o.trail = after;
      else o.lits[j + 1] = after;
      o.ncopy++;
    }
  return o;
}

}  // namespace enc
}  // namespace mib
