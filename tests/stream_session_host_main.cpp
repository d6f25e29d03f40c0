// Stand-alone host program over brotli-lib_amd/csrc/stream_session.h (built with
// -fsanitize=address,undefined by tests/test_stream_session_host.py): the streaming decoder
// session's position arithmetic on a made-up stream.  A "launch" here just moves the
// checkpoint to a later boundary of a random walk; what is checked is what the host does
// between launches -- dropping consumed input, moving the history down, rebasing the
// checkpoint -- against the walk's absolute positions, with real byte arrays behind the
// pending input and the session buffer so that every index is a checked access.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "stream_session.h"

using namespace mib;

static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd() {
  rnd_state ^= rnd_state << 13;
  rnd_state ^= rnd_state >> 7;
  rnd_state ^= rnd_state << 17;
  return rnd_state;
}
#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static uint8_t in_byte(uint64_t off) { return (uint8_t)(off * 131 + (off >> 8) * 7 + 3); }
static uint8_t out_byte(uint64_t pos) { return (uint8_t)(pos * 29 + (pos >> 9) * 5 + 1); }

static void walk(int lgwin, uint64_t out_window, int steps) {
  const uint64_t cap = stream_buf_cap(lgwin, out_window);
  CHECK(cap < (1ull << 30));
  // (the slack is 16 MiB of address space only: the walk's commands are short, so the toy
  // buffer ends 4 KiB behind the window and the capacity rule is checked as arithmetic)
  const uint64_t toy_cap = (1ull << lgwin) + out_window + 4096;
  std::vector<uint8_t> buf(toy_cap), pend;
  uint64_t pend_base = 0, out_base = 0;   // absolute offsets of pend[0] / buf[0]
  uint64_t t_bit, t_pos = 0, t_mb_bit, t_mb_pos = 0, t_win = 0;   // the walk's absolute state
  bool at_mb = true;
  StreamCkpt ck;
  stream_initial_ckpt(&ck, lgwin);
  t_bit = t_mb_bit = ck.e.bit;
  CHECK(ck.e.flags == (kPartValid | kPartAtMb) && ck.ho == 2 && ck.bo == window_bits_len(lgwin) && ck.win_off == 0);
  CHECK(ck.e.ring[0] == 4 && ck.e.ring[1] == 11 && ck.e.ring[2] == 15 && ck.e.ring[3] == 16);
  for (int s = 0; s < steps; s++) {
    // an update: more input
    const uint64_t add = rnd() % 3 ? rnd() % 300 : rnd() % 70000;
    for (uint64_t k = 0; k < add; k++) pend.push_back(in_byte(pend_base + pend.size()));
    // launches: compaction, then the checkpoint moves on while the input covers it
    for (int pass = 0; pass < 4; pass++) {
      const uint64_t delta = stream_compact_delta(ck.e.pos, lgwin);
      if (delta) {
        const uint64_t n = ck.e.pos - delta;
        CHECK(n == (1ull << lgwin));
        for (uint64_t k = 0; k < n; k++) buf[k] = buf[delta + k];   // (ascending: what the move kernel's order gives)
        out_base += delta;
        stream_rebase_output(&ck, delta);
      }
      CHECK(ck.e.pos <= (1ull << lgwin));
      CHECK(ck.e.pos + out_window + kStreamSlack <= cap);   // room for a window of output and one command's overrun
      CHECK(ck.e.pos + out_base == t_pos);
      CHECK((uint64_t)((int64_t)ck.e.mb_pos + (int64_t)out_base) == t_mb_pos);
      // the history a copy may reach is in the buffer, byte for byte
      const uint64_t h = t_pos < (1ull << lgwin) ? t_pos : (1ull << lgwin);
      CHECK(ck.e.pos >= h);
      for (uint64_t k = 1; k <= h; k += 1 + rnd() % 997) CHECK(buf[ck.e.pos - k] == out_byte(t_pos - k));
      // the input a resume reads again is pending, byte for byte
      const uint64_t keep = stream_keep_from(ck);
      CHECK((keep & 1) == 0 && keep <= pend.size() && keep <= (ck.e.bit >> 3) && (int64_t)keep <= ck.win_off);
      if (!at_mb) CHECK(keep <= (ck.e.mb_bit >> 3));
      CHECK(ck.e.bit + 8 * pend_base == t_bit && (uint64_t)ck.win_off + pend_base == t_win);
      if (!at_mb) CHECK(ck.e.mb_bit + 8 * pend_base == t_mb_bit);
      for (uint64_t k = keep; k < pend.size(); k += 1 + rnd() % 499) CHECK(pend[k] == in_byte(pend_base + k));
      // the "launch": boundaries while bits and the output limit allow
      const uint64_t in_bits = 8 * (pend_base + pend.size());
      const uint64_t out_limit = t_pos + out_window;
      bool out_full = false;
      for (;;) {
        const uint64_t bits = 1 + rnd() % 6000, outn = rnd() % 3000;
        if (t_bit + bits > in_bits) break;
        if (t_pos >= out_limit) {
          out_full = true;
          break;
        }
        for (uint64_t k = 0; k < outn; k++) buf[(t_pos - out_base) + k] = out_byte(t_pos + k);
        t_bit += bits;
        t_pos += outn;
        if ((t_bit >> 3) > t_win + 4062) t_win = ((t_bit >> 3) - rnd() % 40) & ~1ull;   // a window refill
        if (t_win > (t_bit >> 3)) t_win = (t_bit >> 3) & ~1ull;
        if (rnd() % 50 == 0) {   // a new metablock
          at_mb = true;
          t_mb_bit = t_bit;
          t_mb_pos = t_pos;
        } else {
          at_mb = false;
        }
      }
      ck.e.bit = t_bit - 8 * pend_base;
      ck.e.pos = t_pos - out_base;
      ck.e.mb_bit = t_mb_bit - 8 * pend_base;
      ck.e.mb_pos = (uint64_t)((int64_t)t_mb_pos - (int64_t)out_base);
      ck.e.flags = kPartValid | (at_mb ? kPartAtMb : 0);
      ck.win_off = (int64_t)(t_win - pend_base);
      CHECK(ck.e.pos <= toy_cap);
      if (!out_full) break;
    }
    // consumed input leaves once it is worth a move (runtime.cpp's rule)
    const uint64_t keep = stream_keep_from(ck);
    if (keep >= (64u << 10) && 2 * keep >= pend.size()) {
      pend.erase(pend.begin(), pend.begin() + (long)keep);
      pend_base += keep;
      stream_rebase_input(&ck, keep);
      CHECK(ck.win_off >= 0);
    }
  }
  printf("lgwin %d window %llu: %llu bytes in, %llu out, input base %llu, output base %llu\n", lgwin,
         (unsigned long long)out_window, (unsigned long long)(t_bit >> 3), (unsigned long long)t_pos,
         (unsigned long long)pend_base, (unsigned long long)out_base);
  CHECK(out_base > 0 && pend_base > 0);
}

int main() {
  // option clamping and the window-bits byte
  CHECK(stream_clamp_window(0) == kStreamDefaultWindow && stream_clamp_window(1) == kStreamMinWindow);
  CHECK(stream_clamp_window(1ull << 40) == kStreamMaxWindow && stream_clamp_window(1 << 20) == (1 << 20));
  CHECK(stream_window_bits(0x00) == 16 && stream_window_bits(0x06) == 16 && stream_window_bits(0x01) == 17);
  CHECK(stream_window_bits(0x03) == 18 && stream_window_bits(0x0f) == 24 && stream_window_bits(0x21) == 10);
  CHECK(stream_window_bits(0x71) == 15 && stream_window_bits(0x11) == -1);
  for (int lg = 10; lg <= 24; lg++) {
    // the byte a stream of window lg starts with decodes back to lg
    const int code = lg == 16 ? 0 : lg >= 18 ? 1 | ((lg - 17) << 1) : lg == 17 ? 1 : 1 | ((lg - 8) << 4);
    CHECK(stream_window_bits((uint8_t)code) == lg);
  }
  walk(10, kStreamMinWindow, 400);
  walk(16, kStreamMinWindow, 400);
  walk(18, 1 << 20, 300);
  return 0;
}
