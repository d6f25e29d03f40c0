// The backtrack's window arithmetic (brotli-lib_amd/csrc/backtrack_window.h: the path through a
// window of 64 nodes by pointer doubling, as backtrack_kernel runs it on a wave) as host code,
// against the plain walk node by node.  Built twice by tests/test_backtrack_window_host.py,
// plain and with AddressSanitizer and UBSan.
//
//   backtrack_window_host exhaustive FULL SMALL PART OF
//       windows of 1..FULL positions with every length that behaves differently at each position
//       (0, every length that lands inside, the one that leaves exactly at the window's end, one
//       and 64 beyond it); windows of FULL+1..SMALL positions with every pattern of the lengths
//       0, 2 and 3; every entry of each.  Part PART of OF (0-based): the windows are dealt out
//       in turn, so that the parts can run side by side
//   backtrack_window_host random SEED ROUNDS
//       windows of 64 positions, every nvalid in 1..64 and every entry below it ROUNDS times:
//       lengths drawn from {0, 1, 2, 3, 63, 64, 65, 200, 255, 65535} at several densities, windows
//       without a copy, windows of copies of length 2 only, and a copy on the path that leaves
//       the window by exactly 0, 1 and 64 positions
// Prints "ok <checks>" last and returns 0, or a line saying what failed and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "backtrack_window.h"

using namespace mib::enc;

static long g_checks = 0;

// the walk as the kernel's scalar loop makes it: a node at a time
static BtWalk plain_walk(const uint32_t len[64], uint32_t x0, uint32_t nvalid) {
  BtWalk o{};
  uint32_t x = x0, lits = 0;
  while (x < nvalid) {
    if (len[x]) {
      o.node[o.ncopy] = x;
      o.lits[o.ncopy] = lits;
      o.ncopy++;
      lits = 0;
      x += len[x];
    } else {
      lits++;
      x++;
    }
  }
  o.trail = lits;
  o.exit = x;
  return o;
}

static void check(const uint32_t len[64], uint32_t x0, uint32_t nvalid) {
  const BtWalk want = plain_walk(len, x0, nvalid), got = bt_walk_window(len, x0, nvalid);
  g_checks++;
  bool same = want.ncopy == got.ncopy && want.trail == got.trail && want.exit == got.exit;
  for (uint32_t j = 0; same && j < want.ncopy; j++) same = want.node[j] == got.node[j] && want.lits[j] == got.lits[j];
  if (same) return;
  printf("FAILED: nvalid %u, entry %u: %u copies, trail %u, exit %u; the plain walk has %u, %u, %u\nlen:", nvalid, x0, got.ncopy,
         got.trail, got.exit, want.ncopy, want.trail, want.exit);
  for (uint32_t x = 0; x < nvalid; x++) printf(" %u", len[x]);
  printf("\n");
  exit(1);
}

static uint32_t g_part = 0, g_of = 1;
static unsigned long g_window = 0;

static void entries(const uint32_t len[64], uint32_t nvalid) {
  for (uint32_t x0 = 0; x0 < nvalid; x0++) check(len, x0, nvalid);
}

// every window of n positions whose position x takes each of choices(x)'s lengths
template <class F>
static void patterns(uint32_t n, F choices) {
  uint32_t len[64] = {0}, idx[64] = {0}, vals[64][80], cnt[64];
  for (uint32_t x = 0; x < n; x++) cnt[x] = choices(x, vals[x]);
  for (;;) {
    for (uint32_t x = 0; x < n; x++) len[x] = vals[x][idx[x]];
    // (beyond the window: what a neighbouring window's nodes would be, which no path may read)
    for (uint32_t x = n; x < 64; x++) len[x] = 7;
    if (g_window++ % g_of == g_part) entries(len, n);
    uint32_t x = 0;
    while (x < n && ++idx[x] == cnt[x]) idx[x++] = 0;
    if (x == n) return;
  }
}

static void exhaustive(uint32_t full, uint32_t small) {
  for (uint32_t n = 1; n <= full; n++)
    patterns(n, [n](uint32_t x, uint32_t *v) {
      uint32_t c = 0;
      for (uint32_t l = 0; l <= n - x + 1; l++) v[c++] = l;   // 0, inside, exactly the end, one beyond
      v[c++] = n - x + 64;
      return c;
    });
  for (uint32_t n = full + 1; n <= small; n++)
    patterns(n, [](uint32_t, uint32_t *v) {
      v[0] = 0, v[1] = 2, v[2] = 3;
      return 3u;
    });
}

static uint32_t g_rng;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

static void random_windows(uint32_t seed, uint32_t rounds) {
  static const uint32_t kLens[10] = {0, 1, 2, 3, 63, 64, 65, 200, 255, 65535};
  g_rng = seed ? seed : 1u;
  uint32_t len[64];
  for (uint32_t round = 0; round < rounds; round++)
    for (uint32_t nvalid = 1; nvalid <= 64; nvalid++) {
      // drawn lengths: a copy at one position in 1, 2, 4 or 16; short copies more often than long
      for (uint32_t x = 0; x < 64; x++) {
        const uint32_t every = 1u << ((round & 3u) == 3u ? 4u : (round & 3u));
        len[x] = rnd() % every ? 0u : kLens[rnd() & 1u ? 1u + rnd() % 3u : rnd() % 10u];
      }
      entries(len, nvalid);
      for (uint32_t x = 0; x < 64; x++) len[x] = kLens[rnd() % 10u];
      entries(len, nvalid);
      memset(len, 0, sizeof(len));   // no copy
      entries(len, nvalid);
      for (uint32_t x = 0; x < 64; x++) len[x] = 2;
      entries(len, nvalid);
      // a copy at the entry, or two literals below it, that leaves the window by exactly 0, 1, 64
      for (uint32_t x0 = 0; x0 < nvalid; x0++)
        for (uint32_t by : {0u, 1u, 64u})
          for (uint32_t at : {x0, x0 + 2u}) {
            if (at >= nvalid) continue;
            for (uint32_t x = 0; x < 64; x++) len[x] = rnd() % 3u ? 0u : 2u + rnd() % 2u;
            if (at != x0) len[x0] = len[x0 + 1] = 0;
            len[at] = nvalid - at + by;
            check(len, x0, nvalid);
          }
    }
}

int main(int argc, char **argv) {
  if (argc == 6 && !strcmp(argv[1], "exhaustive")) {
    g_part = (uint32_t)atoi(argv[4]);
    g_of = (uint32_t)atoi(argv[5]);
    if (g_of == 0 || g_part >= g_of) return 1;
    exhaustive((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]));
  } else if (argc == 4 && !strcmp(argv[1], "random")) {
    random_windows((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]));
  } else {
    printf("usage: %s exhaustive FULL SMALL PART OF | random SEED ROUNDS\n", argv[0]);
    return 1;
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
