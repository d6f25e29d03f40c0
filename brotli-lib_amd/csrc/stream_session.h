// Streaming decoder session (mib_decoder_*): what the host and
// decode_resume_kernel share, and the session's position arithmetic.  Plain C++ (no HIP
// types), so the arithmetic is exercised by a stand-alone host program under sanitizers
// (tests/stream_session_host_main.cpp).
//
// A session decodes one stream in launches.  Between launches its whole state is a
// StreamCkpt: the decoder state at a command or metablock boundary in PartEntry layout
// (parts.h), plus the bit reader's exact state -- where its 4 KiB window stands in the input,
// the window's bytes, and (ho, bo, acc).  The reader is restored exactly, not re-seeked: which
// stale bytes a truncated stream's reader runs into, and with them the error it raises,
// depends on where the reference's reader last refilled its window (decode_core.inc, bit reader).
//
// Coordinates.  Input positions (bit, mb_bit, win_off) count from the first byte of the
// session's pending input, output positions (pos, mb_pos) from the first byte of the session
// buffer; the host rebases both when it drops consumed input or moves the history down.
#pragma once
#include <stdint.h>
#include <string.h>

#include "parts.h"

namespace mib {

constexpr uint32_t kStreamInputEnd = 4u;   // checkpoint flag (with kPartAtMb): the last metablock is decoded

constexpr int kStreamWin = 4096;           // the bit reader's window (decode_core.inc read_more_input)

struct StreamCkpt {
  PartEntry e;
  int64_t win_off;         // input offset of the reader window's first byte
  int32_t ho, bo;          // the reader's half-word offset and bit offset
  uint32_t acc;            // its accumulator (the half-words ho - 2, ho - 1)
  uint32_t reserved;
  uint8_t win[kStreamWin]; // the window as the reader last filled it; bytes the input now
                           // has are laid over it when a launch resumes
};
static_assert(sizeof(StreamCkpt) == 72 + 24 + kStreamWin, "stream checkpoint layout");
// the checkpoint without its window: what the host mirrors and a batch launch carries beside its jobs
constexpr size_t kStreamCkHead = sizeof(StreamCkpt) - kStreamWin;
static_assert(kStreamCkHead % 8 == 0, "checkpoint heads are copied in 8-byte words");

// what a launch reports (negative: the decoder's error code)
constexpr int kStreamNeedInput = 1;    // suspended: a command or header reaches past the input
constexpr int kStreamNeedOutput = 2;   // suspended: the output limit is reached
constexpr int kStreamFinished = 3;     // the last metablock is decoded; ckpt.e.bit = the stream's end

struct StreamJob {
  const uint8_t *in;       // pending input (device)
  uint64_t in_len;
  uint8_t *buf;            // session buffer (device): history, new output, slack
  uint64_t buf_cap;
  uint64_t out_limit;      // the launch leaves at the first boundary with pos >= out_limit
  const uint8_t *dict;     // compound dictionary (device) or null
  uint64_t dict_len;
  StreamCkpt *ck;          // in: where to resume; out: the last boundary the input covers
  int32_t lgwin;
  int32_t final;           // the end of `in` is the end of the stream (finish())
  int32_t status;          // out: kStream* or an error code
  int32_t dict_std;        // DecJob::dict_std: 1 -- `dict` is a prepared dictionary (mib_decoder_new_dictionary),
                           // a copy may lie anywhere inside it; 0 -- the reference's rule (customDictionary)
  int64_t out_pos;         // out: output is valid up to here (the checkpoint's pos; the end when finished)
  int64_t need_len;        // out, with kStreamNeedInput: no launch gets further before in_len reaches this (0: unknown)
  int64_t redone;          // out: output bytes decoded behind the checkpoint, which the next launch decodes again
};

// Slack behind the output limit.  A launch only starts a command at pos < out_limit, and a
// command that does not end in an error writes at most the rest of its metablock: an insert
// longer than that ends the metablock below zero (-10, its stores clamped by ring_cap), a
// copy longer than that is refused before it stores (-9), an uncompressed metablock is its
// length.  MLEN <= 2^24 (six nibbles).  A dictionary word may pass the metablock's end by its
// transform's affixes (< 64 bytes) before the -10.  A compound-dictionary copy is checked
// against the capacity before it stores (decode_core.inc, ST_COPY_FROM_COMPOUND); under either
// rule for its address (StreamJob::dict_std): a prepared dictionary's copy that passes its
// dictionary's end is refused earlier still (-9, use_dictionary), so that check only ever ends
// such a session in the metablock below zero (-10).
constexpr uint64_t kStreamMaxMlen = 1ull << 24;
constexpr uint64_t kStreamSlack = kStreamMaxMlen + 64 + 192;   // + the kernels' read slack
constexpr uint64_t kStreamMinWindow = 64ull << 10;
constexpr uint64_t kStreamMaxWindow = 512ull << 20;
constexpr uint64_t kStreamDefaultWindow = 16ull << 20;
static_assert((1ull << 24) + kStreamMaxWindow + kStreamSlack < (1ull << 30), "buffer positions stay below the ring mask 2^30 - 1");

inline uint64_t stream_clamp_window(uint64_t w) {
  if (w == 0) return kStreamDefaultWindow;
  return w < kStreamMinWindow ? kStreamMinWindow : w > kStreamMaxWindow ? kStreamMaxWindow : w;
}
inline uint64_t stream_buf_cap(int lgwin, uint64_t out_window) { return (1ull << lgwin) + out_window + kStreamSlack; }

// decodeWindowBits on a stream's first byte (RFC 7932 9.1): 10..24, or -1 for the reserved
// pattern the decoder refuses (-11)
inline int stream_window_bits(uint8_t b0) {
  if ((b0 & 1) == 0) return 16;
  int m = (b0 >> 1) & 7;
  if (m) return 17 + m;
  m = (b0 >> 4) & 7;
  if (m == 1) return -1;
  return m ? 8 + m : 17;
}

// The first checkpoint: at the first metablock header, behind the window bits, with the
// reader as the reference leaves it there (window at input offset 0, two half-words loaded).
inline void stream_initial_ckpt(StreamCkpt *c, int lgwin) {
  memset(c, 0, sizeof(*c));
  c->e.bit = (uint64_t)window_bits_len(lgwin);
  c->e.mb_bit = c->e.bit;
  c->e.ring[0] = 4; c->e.ring[1] = 11; c->e.ring[2] = 15; c->e.ring[3] = 16;
  c->e.flags = kPartValid | kPartAtMb;
  c->ho = 2;
  c->bo = (int32_t)c->e.bit;
}

// Input before this offset is no longer read: a resume re-reads the metablock header (mid-
// metablock checkpoints only) and refills the reader's window.  Even, as part_seek aligns.
inline uint64_t stream_keep_from(const StreamCkpt &c) {
  uint64_t k = c.e.bit >> 3;
  if (!(c.e.flags & kPartAtMb) && (c.e.mb_bit >> 3) < k) k = c.e.mb_bit >> 3;
  if (c.win_off >= 0 && (uint64_t)c.win_off < k) k = (uint64_t)c.win_off;
  if (c.win_off < 0) k = 0;
  return k & ~1ull;
}
// `drop` bytes (even, <= stream_keep_from) leave the front of the pending input
inline void stream_rebase_input(StreamCkpt *c, uint64_t drop) {
  c->e.bit -= 8 * drop;
  // (an at-header checkpoint does not use mb_bit: it may lie before the kept input)
  c->e.mb_bit = c->e.mb_bit >= 8 * drop ? c->e.mb_bit - 8 * drop : 0;
  c->win_off -= (int64_t)drop;
}

// History the next launch needs in front of pos: min(pos, 2^lgwin) bytes.  Positions move
// down by the returned amount (0: the buffer still has room for a window of output behind pos).
//
// max_dist = min(pos, max_back) comes out as the stream's under this rebasing: while fewer
// than 2^lgwin bytes are decoded nothing has moved and pos is the stream's own position; once
// a move has happened pos stays >= 2^lgwin > max_back = 2^lgwin - 16, as the stream's own
// position (never smaller than the buffer's) does, so both give max_back.
inline uint64_t stream_compact_delta(uint64_t pos, int lgwin) {
  const uint64_t h = 1ull << lgwin;
  return pos > h ? pos - h : 0;
}
inline void stream_rebase_output(StreamCkpt *c, uint64_t delta) {
  c->e.pos -= delta;
  c->e.mb_pos -= delta;   // (two's complement: a metablock may have started before the kept history)
}

}  // namespace mib
