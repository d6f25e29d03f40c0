// The copy launches of stream_batch.h (plan_copies) replayed on host memory, for the stand-alone
// host programs: every (block, tile, thread) of every launch stores what copy_tile
// (decode_stream.hip) stores under stream_copy_batch_kernel's walk.  cnt[a - mem0] counts the
// stores to address a.  Include behind the program's CHECK.
#pragma once
#include <stdint.h>

#include <vector>

#include "stream_batch.h"

static void replay_copies(const mib::CopyDesc *d, const std::vector<mib::CopyLaunch> &ls, const uint8_t *mem0,
                          std::vector<uint8_t> &cnt) {
  using namespace mib;
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
                cnt[(size_t)(c.dst + lo + q - mem0)]++;
              }
          }
    }
}
