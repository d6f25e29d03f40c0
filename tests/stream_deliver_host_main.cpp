// The planning of the device-resident session calls (brotli-lib_amd/csrc/stream_batch.h: how much
// a slot delivers, what stays held, when it launches and with which output limit, the copy
// launches' grids and their split) driven with seeded random sessions and rooms, stand-alone so
// that it runs under AddressSanitizer and UBSan (tests/test_stream_deliver_host.py).  The rounds
// of runtime.cpp are replayed over a model session whose "launch" decodes up to the output limit
// plus a random overshoot; the copy kernel's walk is replayed on host memory.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "stream_batch.h"
#include "stream_session.h"

using namespace mib;

static uint64_t g_seed = 0xD1B54A32D192ED03ull;
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

// A model session: `total` bytes of output, of which the input so far determines `avail`.
struct Model {
  uint64_t total = 0, avail = 0;      // stream positions
  uint64_t decoded = 0, given = 0;    // bytes launches have produced / calls have handed out
  uint64_t deliv = 0, held_to = 0;    // the session's held range (buffer positions)
  uint64_t pos = 0;                   // the checkpoint's buffer position
  uint64_t out_window = 0, slack = 0;
  bool due = false, finished = false;
  uint64_t launches = 0;
};
static uint64_t held(const Model &m) { return m.held_to - m.deliv; }

// one launch: from pos up to the first boundary at or behind out_limit (a boundary lies up to
// `slack` further), or to where the input ends; returns true when it left on the output limit
static bool launch(Model &m, uint64_t out_limit) {
  CHECK(held(m) == 0);
  const uint64_t start = m.pos;
  CHECK(out_limit > start && out_limit <= start + m.out_window);
  const uint64_t left = m.avail - m.decoded;
  uint64_t n = out_limit - start + below(m.slack + 1);
  bool need_output = true;
  if (n >= left) {
    n = left;
    need_output = false;
    if (m.avail == m.total) m.finished = true;
  }
  m.deliv = start;
  m.held_to = m.pos = start + n;
  m.decoded += n;
  m.launches++;
  return need_output;
}

// one call of the device path over one slot, as decoder_batch / decoder_batch_rounds run it;
// returns the status, *out the bytes given
static int call(Model &m, uint64_t more_input, uint64_t room0, uint64_t *out) {
  const uint64_t before = m.launches;
  m.avail = std::min(m.total, m.avail + more_input);
  bool run = m.due || (more_input && !m.finished);
  uint64_t room = room0, given = 0;
  while ((run || held(m)) && room > 0) {
    if (stream_plans_job(held(m), room, run)) {
      // (the history moves here, with nothing held: positions are rebased)
      const uint64_t delta = stream_compact_delta(m.pos, 10);
      m.pos -= delta;
      const uint64_t limit = stream_out_limit(m.pos, m.out_window, room);
      CHECK(limit <= m.pos + m.out_window);
      CHECK(limit - m.pos <= room);
      run = launch(m, limit);
    } else {
      CHECK(held(m) > 0);   // a round without a job delivers
    }
    const uint64_t n = deliver_len(held(m), room);
    CHECK(n <= room && n <= held(m));
    m.deliv += n;
    room -= n;
    given += n;
    m.given += n;
    CHECK(m.given + held(m) == m.decoded);   // delivered + held is conserved
  }
  m.due = run;
  if (room0 == 0) CHECK(m.launches == before && given == 0);   // room 0: no launch
  CHECK(given <= room0);
  *out = given;
  const bool more = stream_more_output(held(m), room, m.due);
  // MORE_OUTPUT exactly when the range is full and work remains
  CHECK(more == (given == room0 && (held(m) > 0 || m.due)));
  if (!more) CHECK(held(m) == 0 && !m.due);
  return more ? 1 : 0;
}

static void test_delivery(int rounds) {
  const uint64_t rooms[] = {0, 1, 2, 15, 16, 17, 4097, 65536, 1 << 20, kNoRoomLimit};
  for (int r = 0; r < rounds; r++) {
    Model m;
    m.total = below(3) == 0 ? below(50) : below(3 << 20);
    m.out_window = below(2) ? kStreamMinWindow : kStreamMinWindow + below(1 << 20);
    m.slack = below(3) == 0 ? 0 : below(2) ? below(300) : below(1 << 20);
    uint64_t fed = 0;
    int idle = 0;
    for (int step = 0; step < 100000 && !(m.finished && held(m) == 0 && !m.due); step++) {
      uint64_t in = 0;
      if (fed < m.total || m.total == 0) {
        in = below(4) == 0 ? 0 : 1 + below(m.total / 3 + 2);
        if (m.total == 0) in = 1;
      }
      uint64_t room = rooms[below(sizeof(rooms) / sizeof(rooms[0]))];
      if (idle > 3) room = 4097;   // (a run of empty ranges: let the session move)
      uint64_t got = 0;
      const uint64_t avail_before = m.avail;
      const int st = call(m, in, room, &got);
      fed = m.avail;
      if (st == 0) CHECK(m.given == m.avail);   // status 0: everything the input determines
      idle = (got == 0 && m.avail == avail_before) ? idle + 1 : 0;
      // drain with empty chunks, as a caller does
      if (below(2))
        for (int q = 0; q < 1 << 22; q++) {
          const uint64_t rm = 1 + below(70000);
          if (call(m, 0, rm, &got) == 0) break;
          CHECK(got == rm);
        }
    }
    CHECK(m.finished && m.given == m.total && m.decoded == m.total);
  }
  printf("delivery ok\n");
}

// the host call's slot: no limit, so every round's bytes are delivered whole and nothing is
// ever held or owed behind the call -- the planning reduces to what the host path always did
static void test_host_slot(int rounds) {
  for (int r = 0; r < rounds; r++) {
    const uint64_t start = below(1ull << 29), w = kStreamMinWindow + below(kStreamMaxWindow - kStreamMinWindow);
    CHECK(stream_out_limit(start, w, kNoRoomLimit) == start + w);
    const uint64_t h = below(1ull << 30);
    CHECK(deliver_len(h, kNoRoomLimit) == h);
    CHECK(!stream_more_output(h, kNoRoomLimit - h, true));
    CHECK(stream_plans_job(0, kNoRoomLimit, true) && !stream_plans_job(h + 1, kNoRoomLimit, true) &&
          !stream_plans_job(0, kNoRoomLimit, false) && !stream_plans_job(0, 0, true));
  }
  printf("host slot ok\n");
}

// the copy launches replayed on host memory: every (block, tile, thread) of every launch stores
// what copy_tile stores; each destination byte must be written exactly once, with its source
// byte, and nothing outside the destinations.  Destinations are packed with random gaps from 0,
// so neighbours share 16-byte granules.
static void test_copies(int rounds) {
  for (int r = 0; r < rounds; r++) {
    const size_t k = 1 + below(40);
    const size_t max_descs = 1 + below(r % 3 == 0 ? 3 : 50);
    std::vector<uint64_t> n(k), at(k), sat(k);
    uint64_t dtotal = below(16), stotal = below(16);
    for (size_t i = 0; i < k; i++) {
      const uint64_t pick = below(8);
      n[i] = pick == 0 ? 0 : pick == 1 ? 1 : pick < 5 ? below(70) : pick < 7 ? below(3 * kGatherTile) : kGatherTile * (1 + below(3)) + below(3) - 1;
      if (r % 50 == 7 && i == 0) n[i] = (kGatherSpread + 1) * kGatherTile + 17;   // more tiles than blocks
      at[i] = dtotal;
      dtotal += n[i] + (below(2) ? 0 : below(20));
      sat[i] = stotal;
      stotal += n[i] + below(20);
    }
    // 16-byte aligned bases, as device allocations are
    std::vector<uint8_t> dmem(dtotal + 48), smem(stotal + 48), cnt(dtotal + 48, 0);
    uint8_t *db = dmem.data() + ((16 - ((uintptr_t)dmem.data() & 15)) & 15);
    uint8_t *sb = smem.data() + ((16 - ((uintptr_t)smem.data() & 15)) & 15);
    for (size_t q = 0; q < smem.size(); q++) smem[q] = (uint8_t)rnd();
    memset(dmem.data(), 0xC5, dmem.size());
    std::vector<CopyDesc> d(k);
    for (size_t i = 0; i < k; i++) d[i] = CopyDesc{sb + sat[i], db + at[i], n[i]};
    std::vector<CopyLaunch> ls;
    plan_copies(d.data(), k, max_descs, ls);
    // the split covers every descriptor once, in order
    size_t next = 0;
    for (const CopyLaunch &l : ls) {
      CHECK(l.first == next && l.count >= 1 && l.count <= max_descs);
      CHECK(l.blocks >= 1 && l.blocks <= kGatherSpread);
      CHECK(l.blocks == copy_blocks(d.data() + l.first, l.count));
      next += l.count;
    }
    CHECK(next == k);
    for (const CopyLaunch &l : ls)
      for (size_t y = 0; y < l.count; y++) {
        const CopyDesc &c = d[l.first + y];
        const uint64_t mis = (uint64_t)(uintptr_t)c.dst & 15;
        const uint64_t tiles = tiles_of((uint64_t)(uintptr_t)c.dst, c.n, kGatherTile);
        CHECK(c.n == 0 ? tiles == 0 : tiles * kGatherTile >= c.n + mis);   // the tiles reach the last byte
        for (uint32_t b = 0; b < l.blocks; b++)
          for (uint64_t t = b; t < tiles; t += l.blocks)
            for (int tid = 0; tid < kGatherThreads; tid++) {
              const uint64_t g = t * kGatherThreads + (uint64_t)tid;
              const int64_t lo = (int64_t)(16 * g) - (int64_t)mis;
              const bool whole = lo >= 0 && (uint64_t)lo + 16 <= c.n;
              if (whole) CHECK(((uintptr_t)(c.dst + lo) & 15) == 0);   // the vector store is aligned
              for (int q = 0; q < 16; q++)
                if (lo + q >= 0 && (uint64_t)(lo + q) < c.n) {
                  c.dst[lo + q] = c.src[lo + q];
                  cnt[(size_t)(c.dst + lo + q - dmem.data())]++;
                }
            }
      }
    std::vector<uint8_t> want(dmem.size(), 0xC5), wcnt(dmem.size(), 0);
    for (size_t i = 0; i < k; i++)
      for (uint64_t q = 0; q < n[i]; q++) {
        want[(size_t)(db + at[i] + q - dmem.data())] = sb[sat[i] + q];
        wcnt[(size_t)(db + at[i] + q - dmem.data())] = 1;
      }
    CHECK(dmem == want);
    CHECK(cnt == wcnt);
  }
  printf("copies ok\n");
}

int main() {
  test_delivery(400);
  test_host_slot(2000);
  test_copies(150);
  return 0;
}
