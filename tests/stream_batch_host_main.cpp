// The planning of a batch of streaming decoder sessions (brotli-lib_amd/csrc/stream_batch.h)
// driven with seeded random session states, stand-alone so that it runs under AddressSanitizer
// and UBSan (tests/test_stream_batch_host.py).  The kernels' walks are replayed on the host:
// which bytes each (block, tile, thread) of a move or copy launch touches is plain arithmetic.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "stream_batch.h"
#include "stream_session.h"

using namespace mib;

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 7;
  g_seed ^= g_seed << 17;
  return g_seed;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

#include "stream_copy_walk.h"

// one tile of copy_tile (decode_stream.hip): the destination offsets thread `tid` stores
static void tile_bytes(uint64_t mis, uint64_t n, uint64_t tile, int threads, int tid, int64_t *lo, int64_t *hi) {
  const uint64_t g = tile * (uint64_t)threads + (uint64_t)tid;
  int64_t a = (int64_t)(16 * g) - (int64_t)mis, b = a + 16;
  if (a < 0) a = 0;
  if (b > (int64_t)n) b = (int64_t)n;
  *lo = a;
  *hi = b > a ? b : a;
}

// the move launch replayed on a host buffer: units in any order of blocks (here: reversed, the
// worst case for an overlapping move were it split), tiles of a unit ascending, a tile loaded
// whole before it is stored
static void test_moves(int rounds) {
  for (int r = 0; r < rounds; r++) {
    const size_t k = 1 + below(12);
    std::vector<std::vector<uint8_t>> mem(k), want(k);
    std::vector<MoveDesc> d(k);
    for (size_t i = 0; i < k; i++) {
      const uint64_t mis = below(3) ? 0 : below(16);
      uint64_t n = below(4) == 0 ? below(40) : below(5 * kMoveTile);
      uint64_t src = below(4) == 0 ? below(64) : below(3 * kMoveTile);
      if (below(9) == 0) n = 0;
      if (below(9) == 0) src = 0;
      if (below(3) == 0) src = n + below(100);   // no overlap
      mem[i].resize(mis + src + n + 32);
      for (auto &b : mem[i]) b = (uint8_t)rnd();
      want[i] = mem[i];
      if (src && n) memmove(want[i].data() + mis, want[i].data() + mis + src, n);
      d[i] = MoveDesc{mem[i].data() + mis, src, n};
      // (the kernel takes the misalignment from the address: make the host buffer's match)
      CHECK(((uintptr_t)mem[i].data() & 15) == 0);
    }
    std::vector<MoveUnit> units;
    plan_moves(d.data(), k, units);
    std::vector<int> blocks(k, 0);
    for (const MoveUnit &u : units) {
      CHECK(u.desc < k);
      blocks[u.desc]++;
    }
    for (size_t i = 0; i < k; i++) {
      const uint64_t tiles = tiles_of((uintptr_t)d[i].buf, d[i].n, kMoveTile);
      if (d[i].n == 0 || d[i].src == 0) CHECK(blocks[i] == 0);
      else if (d[i].src < d[i].n) CHECK(blocks[i] == 1);   // an overlapping move never has two blocks
      else CHECK(blocks[i] >= 1 && (uint64_t)blocks[i] <= std::min<uint64_t>(tiles, kMoveSpread));
    }
    std::vector<std::vector<uint8_t>> written(k);
    for (size_t i = 0; i < k; i++) written[i].assign(d[i].n, 0);
    for (size_t b = units.size(); b-- > 0;) {
      const MoveUnit u = units[b];
      const MoveDesc &m = d[u.desc];
      const uint64_t mis = (uintptr_t)m.buf & 15;
      const uint64_t tiles = tiles_of(mis, m.n, kMoveTile);
      CHECK(u.step >= 1 && u.tile0 < u.step);
      for (uint64_t t = u.tile0; t < tiles; t += u.step) {
        std::vector<uint8_t> regs(kMoveTile);
        for (int tid = 0; tid < kMoveThreads; tid++) {
          int64_t lo, hi;
          tile_bytes(mis, m.n, t, kMoveThreads, tid, &lo, &hi);
          for (int64_t x = lo; x < hi; x++) regs[(size_t)tid * 16 + (size_t)(x - lo)] = m.buf[m.src + (uint64_t)x];
        }
        for (int tid = 0; tid < kMoveThreads; tid++) {
          int64_t lo, hi;
          tile_bytes(mis, m.n, t, kMoveThreads, tid, &lo, &hi);
          for (int64_t x = lo; x < hi; x++) {
            CHECK((uint64_t)x < m.n);
            m.buf[x] = regs[(size_t)tid * 16 + (size_t)(x - lo)];
            written[u.desc][(size_t)x]++;
          }
        }
      }
    }
    for (size_t i = 0; i < k; i++) {
      if (d[i].src && d[i].n)
        for (uint64_t x = 0; x < d[i].n; x++) CHECK(written[i][x] == 1);   // every byte once
      CHECK(mem[i] == want[i]);
    }
  }
  printf("moves: %d batches ok\n", rounds);
}

// A host call's delivery: plan_gather lays the sessions' ranges out in the staging span, one
// CopyDesc per range goes through plan_copies, and the copy kernel's walk is replayed.  Every
// span byte of every range is written exactly once with its source byte, nothing is written
// outside the ranges, and ranges start on 16-byte boundaries.  Sources have any alignment, as a
// session's `deliv` has in its buffer.
static void test_gather(int rounds) {
  for (int r = 0; r < rounds; r++) {
    const size_t k = 1 + below(40);
    std::vector<uint64_t> len(k), dst(k), sat(k);
    uint64_t stotal = 0;
    for (size_t i = 0; i < k; i++) {
      len[i] = below(3) == 0 ? 0 : below(4) == 0 ? below(50) : below(6 * kGatherTile);
      if (r % 20 == 3 && i == 0) len[i] = (kGatherSpread + 1) * kGatherTile + 1;   // more tiles than blocks
      sat[i] = stotal + below(16);
      stotal = sat[i] + len[i];
    }
    const uint64_t total = plan_gather(len.data(), k, dst.data());
    uint64_t prev_end = 0;
    for (size_t i = 0; i < k; i++) {
      CHECK(dst[i] % 16 == 0);
      CHECK(dst[i] >= prev_end);             // no two ranges overlap
      CHECK(dst[i] + len[i] <= total);       // inside the span
      prev_end = dst[i] + len[i];
    }
    CHECK(total % 16 == 0 && total < prev_end + 16);
    // a 16-byte aligned span, as the device allocation is, with room to see a store outside it
    std::vector<uint8_t> mem(total + 48, 0xC5), cover(total + 48, 0), smem(stotal + 32);
    uint8_t *span = mem.data() + 16 + ((16 - ((uintptr_t)mem.data() & 15)) & 15);
    for (auto &b : smem) b = (uint8_t)rnd();
    std::vector<CopyDesc> d(k);
    for (size_t i = 0; i < k; i++) d[i] = CopyDesc{smem.data() + sat[i], span + dst[i], len[i]};
    std::vector<CopyLaunch> ls;
    plan_copies(d.data(), k, r % 3 == 0 ? 1 + below(5) : kGatherMaxDescs, ls);
    size_t next = 0;
    for (const CopyLaunch &l : ls) {
      CHECK(l.first == next && l.count >= 1);
      CHECK(l.blocks >= 1 && l.blocks <= kGatherSpread);
      // the grid is the one the lengths alone give: ranges start on granules
      uint64_t most = 1;
      for (size_t y = 0; y < l.count; y++) most = std::max(most, tiles_of(0, len[l.first + y], kGatherTile));
      CHECK(l.blocks == std::min<uint64_t>(most, kGatherSpread));
      next += l.count;
    }
    CHECK(next == k);
    replay_copies(d.data(), ls, mem.data(), cover);
    std::vector<uint8_t> want(mem.size(), 0xC5), wcover(mem.size(), 0);
    for (size_t i = 0; i < k; i++)
      for (uint64_t x = 0; x < len[i]; x++) {
        want[(size_t)(span + dst[i] + x - mem.data())] = smem[sat[i] + x];
        wcover[(size_t)(span + dst[i] + x - mem.data())] = 1;
      }
    CHECK(mem == want);
    CHECK(cover == wcover);
  }
  printf("gather: %d batches ok\n", rounds);
}

// which sessions enter a round, the grid, the read-back layout
static void test_rounds(int rounds) {
  for (int r = 0; r < rounds; r++) {
    const uint64_t in_len = below(1 << 20), need = below(3) ? 0 : below(1 << 20);
    CHECK(stream_enters_round(true, in_len, need));
    CHECK(stream_enters_round(false, in_len, need) == (in_len >= need));
    const size_t jobs = below(5000);
    const int cus = (int)below(300), per_cu = (int)below(6), cap = (int)below(4) ? 0 : (int)below(40);
    const int grid = stream_batch_grid(jobs, cus, per_cu, cap);
    if (jobs == 0) {
      CHECK(grid == 0);
    } else {
      CHECK(grid >= 1 && (size_t)grid <= jobs);
      CHECK((uint64_t)grid <= (uint64_t)std::max(cus, 1) * (uint64_t)std::max(per_cu, 1));
      if (cap > 0) CHECK(grid <= cap);
      if (cap == 0 && jobs <= (size_t)std::max(cus, 1)) CHECK((size_t)grid == jobs);
    }
    const size_t k = 1 + below(3000);
    const uint64_t at = stream_heads_offset(k, sizeof(StreamJob));
    CHECK(at % 16 == 0 && at >= k * sizeof(StreamJob) && at < k * sizeof(StreamJob) + 16);
  }
  // a round's sessions in buffer terms: the history move of each and its output range stay
  // inside the session buffer
  for (int r = 0; r < rounds; r++) {
    const int lgwin = 10 + (int)below(15);
    const uint64_t window = stream_clamp_window(below(2) ? 0 : below(1ull << 27));
    const uint64_t cap = stream_buf_cap(lgwin, window);
    uint64_t pos = below((1ull << lgwin) + window + kStreamMaxMlen);
    const uint64_t delta = stream_compact_delta(pos, lgwin);
    const MoveDesc m{nullptr, delta, pos - delta};
    CHECK(m.src + m.n <= cap);
    pos -= delta;
    CHECK(pos <= (1ull << lgwin));
    CHECK(pos + window + kStreamSlack <= cap);   // the launch's out_limit and slack
  }
  printf("rounds: %d states ok\n", rounds);
}

int main() {
  static_assert(sizeof(MoveDesc) == 24 && sizeof(MoveUnit) == 16 && sizeof(CopyDesc) == 24, "descriptor layouts");
  static_assert(sizeof(CopyDesc) <= sizeof(StreamJob), "copy descriptors reuse the jobs' place");
  test_moves(60);
  test_gather(60);
  test_rounds(20000);
  return 0;
}
