// The rounds of the streaming decoder's calls, one session's or many (mib_decoder_update,
// mib_decoder_update_batch; DESIGN.md §4d "Rounds"): the descriptors the host and the move and
// copy kernels of decode_stream.hip share, and the planning of a round -- which sessions
// launch, where each session's output lies in the staging span, which block moves which tiles,
// how large the decode grid is, how much a slot delivers, what it goes on holding and when it
// launches (stream_rounds.h holds the loop over them).  Plain C++ (no HIP types):
// the planning is exercised by a stand-alone host program under sanitizers
// (tests/stream_batch_host_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mib {

// buf[0, n) <- buf[src, src + n), src > 0 (a session's history, or its pending input, moves to
// the front of its buffer); the ranges overlap when src < n
struct MoveDesc {
  uint8_t *buf;
  uint64_t src, n;
};
// One block of the move launch: tiles tile0, tile0 + step, ... of descriptor `desc`, ascending.
struct MoveUnit {
  uint32_t desc, tile0, step, reserved;
};
// dst[0, n) <- src[0, n), both of any alignment and pointers of their own: a slot's chunk goes
// to its session's pending input, a session's decoded bytes go to the caller's range or to the
// staging span
struct CopyDesc {
  const uint8_t *src;
  uint8_t *dst;
  uint64_t n;
};

constexpr int kMoveThreads = 1024;
constexpr uint64_t kMoveTile = (uint64_t)kMoveThreads * 16;
constexpr uint32_t kMoveSpread = 64;   // blocks a non-overlapping move is spread over at most
constexpr int kGatherThreads = 256;
constexpr uint64_t kGatherTile = (uint64_t)kGatherThreads * 16;
constexpr uint32_t kGatherSpread = 256;   // blocks per descriptor at most (each walks its tiles)
constexpr size_t kGatherMaxDescs = 65535;   // descriptors per launch (the grid's y extent)

// Tiles are laid over the destination's 16-byte granules: tile t holds the granules
// [t * kMoveThreads, (t + 1) * kMoveThreads), granule g the destination bytes
// [16 g - mis, 16 g - mis + 16) that lie in [0, n), where mis = the buffer address mod 16.
constexpr uint64_t tiles_of(uint64_t mis, uint64_t n, uint64_t tile) { return n ? (n + (mis & 15) + tile - 1) / tile : 0; }

// The move launch's blocks.  An overlapping move has ONE block, which owns every tile in
// ascending order (a tile is loaded whole before it is stored, so its stores, below its own
// sources, cannot reach what a later tile still reads); without overlap no store lands in the
// source range and the tiles are spread over up to kMoveSpread blocks.  Empty moves and
// src = 0 (nothing to do) get no block.
inline void plan_moves(const MoveDesc *d, size_t k, std::vector<MoveUnit> &units) {
  units.clear();
  for (size_t i = 0; i < k; i++) {
    if (d[i].n == 0 || d[i].src == 0) continue;
    const uint64_t tiles = tiles_of((uint64_t)(uintptr_t)d[i].buf, d[i].n, kMoveTile);
    const uint32_t nb = d[i].src < d[i].n ? 1u : (uint32_t)(tiles < kMoveSpread ? tiles : kMoveSpread);
    for (uint32_t b = 0; b < nb; b++) units.push_back(MoveUnit{(uint32_t)i, b, nb, 0});
  }
}

// Where each session's [start, out_pos) goes in the staging span: dense, in session order,
// each range starting on a 16-byte boundary (so the copy kernel stores whole 16-byte vectors up
// to a range's last granule).  Returns the span's size.
inline uint64_t plan_gather(const uint64_t *len, size_t k, uint64_t *dst) {
  uint64_t at = 0;
  for (size_t i = 0; i < k; i++) {
    dst[i] = at;
    at += (len[i] + 15) & ~15ull;
  }
  return at;
}

// A session launches in the first round of a call unless its last launch stopped in front of a
// raw or metadata block that is still not whole: that launch reported how many pending bytes
// the block needs (need_len), and until they are there -- or finish() says no more come -- a
// launch could only stop at the same place.  Later rounds take the sessions whose launch
// stopped on the output limit.
inline bool stream_enters_round(bool final, uint64_t in_len, uint64_t need_len) { return final || in_len >= need_len; }

// The decode launch's grid: a block per job up to cus x per_cu resident waves, and `cap`
// (mib_force_decoder_grid, 0: none) below that; the kernel's job loop takes the rest.
inline int stream_batch_grid(size_t jobs, int cus, int per_cu, int cap) {
  if (jobs == 0) return 0;
  if (cus < 1) cus = 1;
  if (per_cu < 1) per_cu = 1;
  uint64_t g = (uint64_t)cus * (uint64_t)per_cu;
  if (jobs < g) g = jobs;
  if (cap > 0 && (uint64_t)cap < g) g = (uint64_t)cap;
  return (int)g;
}

// ---------------------------------------------------------------- delivery
// (DESIGN.md §4d "Device-resident batches")
constexpr uint64_t kNoRoomLimit = ~0ull;   // a host call's slot: its results grow as needed

// A session between launches may hold decoded bytes the caller has not fetched, held = pos -
// deliv of its buffer, and may owe a launch (`due`: new input or finish() it has not launched
// for, or its last launch left on the output limit).  Delivery before launch: while it holds
// bytes it only delivers, so its history moves (stream_compact_delta) and its positions are
// rebased with nothing held, exactly as for a session that never holds anything.
constexpr uint64_t deliver_len(uint64_t held, uint64_t room) { return held < room ? held : room; }
// a session gets a job in a round only with nothing held and room left
constexpr bool stream_plans_job(uint64_t held, uint64_t room, bool due) { return due && held == 0 && room > 0; }
// ... and that job's output limit: no further than the range has room (kNoRoomLimit: the window)
constexpr uint64_t stream_out_limit(uint64_t start, uint64_t out_window, uint64_t room) {
  return start + (room < out_window ? room : out_window);
}
// a slot leaves its call on MIB_DEC_MORE_OUTPUT exactly when its range is full and work remains
constexpr bool stream_more_output(uint64_t held, uint64_t room, bool due) { return room == 0 && (held > 0 || due); }

// blocks per descriptor (the grid's x extent) of a copy launch: the most tiles any of its
// descriptors has over its destination's granules, kGatherSpread at most
inline uint32_t copy_blocks(const CopyDesc *d, size_t k) {
  uint64_t most = 1;
  for (size_t i = 0; i < k; i++) {
    const uint64_t t = tiles_of((uint64_t)(uintptr_t)d[i].dst, d[i].n, kGatherTile);
    if (t > most) most = t;
  }
  return (uint32_t)(most < kGatherSpread ? most : kGatherSpread);
}
// One copy launch: the descriptors [first, first + count), `blocks` blocks each.
struct CopyLaunch {
  size_t first, count;
  uint32_t blocks;
};
// k descriptors in launches of at most `max_descs` (kGatherMaxDescs: the grid's y extent)
inline void plan_copies(const CopyDesc *d, size_t k, size_t max_descs, std::vector<CopyLaunch> &launches) {
  launches.clear();
  for (size_t g0 = 0; g0 < k; g0 += max_descs) {
    const size_t n = k - g0 < max_descs ? k - g0 : max_descs;
    launches.push_back(CopyLaunch{g0, n, copy_blocks(d + g0, n)});
  }
}

// The round's read-back array: k jobs, then k checkpoint heads (the bytes of a StreamCkpt in
// front of its window), one device-to-host copy for both.
inline uint64_t stream_heads_offset(size_t k, size_t job_bytes) { return ((uint64_t)k * job_bytes + 15) & ~15ull; }

}  // namespace mib
