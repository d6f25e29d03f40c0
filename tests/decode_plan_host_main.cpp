// The host planning of a one-shot decode (brotli-lib_amd/csrc/decode_plan.h) as host code, built
// with AddressSanitizer and UBSan by tests/test_decode_plan_host.py.  Every stream handed to the
// readers lives in a heap block of exactly its length, so one byte read past it is the
// sanitizer's report.
//
//   decode_plan_host golden FILE   the part plan of FILE, printed for the Python side to compare
//   decode_plan_host chains        hand-built index chains: accepted, and one rejected per rule
//   decode_plan_host robust FILE   bit flips and truncations of FILE and of a hand-built chain
//   decode_plan_host window        all 65,536 two-byte prefixes: window bits, announced size
//   decode_plan_host layout FILE   a host batch's layout over a mixed list of spans (FILE: indexed)
// Prints "ok <checks>" last and returns 0, or a line saying what failed and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <vector>

#include "decode_plan.h"

using namespace mib;

static long g_checks = 0;
#define CHECK(c, ...)                \
  do {                               \
    g_checks++;                      \
    if (!(c)) {                      \
      printf("FAILED %s: ", #c);     \
      printf(__VA_ARGS__);           \
      printf("\n");                  \
      exit(1);                       \
    }                                \
  } while (0)

// an exact-size heap copy: ASan guards both ends
struct Block {
  uint8_t *p;
  size_t n;
  Block(const uint8_t *src, size_t len) : p((uint8_t *)malloc(len ? len : 1)), n(len) {
    if (n) memcpy(p, src, n);
  }
  explicit Block(const std::vector<uint8_t> &v) : Block(v.data(), v.size()) {}
  Block(const Block &) = delete;
  ~Block() { free(p); }
};

static std::vector<uint8_t> read_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    printf("FAILED: cannot open %s\n", path);
    exit(1);
  }
  std::vector<uint8_t> v;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + got);
  fclose(f);
  return v;
}

static bool plan_of(const Block &s, PartPlan &plan) {
  HostFetch f{s.p, s.n};
  return plan_parts(f, s.n, plan);
}

// ---------------------------------------------------------------- RFC 7932 section 9.1
// WBITS as the RFC lists them: the bit string (its rightmost bit is the stream's first) and the
// window's log2.  0010001 is the pattern the RFC reserves: the large-window escape.
struct Wbits {
  const char *bits;
  int lgwin;
};
static const Wbits kRfcWbits[] = {
    {"0100001", 10}, {"0110001", 11}, {"1000001", 12}, {"1010001", 13}, {"1100001", 14}, {"1110001", 15},
    {"0", 16},       {"0000001", 17}, {"0011", 18},    {"0101", 19},    {"0111", 20},    {"1001", 21},
    {"1011", 22},    {"1101", 23},    {"1111", 24},    {"0010001", kLargeWindow},
};
static const Wbits &rfc_wbits(uint32_t v) {   // the entry the stream's first bits spell
  for (const Wbits &w : kRfcWbits) {
    const int nb = (int)strlen(w.bits);
    if ((v & ((1u << nb) - 1)) == (uint32_t)strtoul(w.bits, nullptr, 2)) return w;
  }
  printf("FAILED: no WBITS pattern for %#x\n", v);
  exit(1);
}
static const Wbits &rfc_wbits_of(int lgwin) {
  for (const Wbits &w : kRfcWbits)
    if (w.lgwin == lgwin) return w;
  exit(1);
}

// zero-padded LSB-first bits of b[0, n), the test's own
static uint32_t bits_at(const uint8_t *b, size_t n, size_t &bit, int k) {
  uint32_t v = 0;
  for (int i = 0; i < k; i++, bit++)
    if ((bit >> 3) < n && ((b[bit >> 3] >> (bit & 7)) & 1)) v |= 1u << i;
  return v;
}
// brotliDecodedSize by RFC 7932 section 9.2: WBITS, ISLAST, ISLASTEMPTY, MNIBBLES, MLEN - 1; the
// first metablock's length when it is the last one, 0 for an empty stream, else -1.  (After the
// large-window escape: a bit that must be 0 and six bits of window size.)
static int64_t rfc_decoded_size(const uint8_t *b, size_t n) {
  size_t bit = 0;
  const Wbits &w = rfc_wbits(bits_at(b, n, bit, 7));
  bit = strlen(w.bits);
  if (w.lgwin == kLargeWindow) {
    if (bits_at(b, n, bit, 1)) return -1;
    bits_at(b, n, bit, 6);
  }
  const bool last = bits_at(b, n, bit, 1);
  if (last && bits_at(b, n, bit, 1)) return 0;
  const int nib = 4 + (int)bits_at(b, n, bit, 2);
  if (nib == 7) return -1;
  const int64_t mlen = (int64_t)bits_at(b, n, bit, 4 * nib) + 1;
  return last ? mlen : -1;
}

// ---------------------------------------------------------------- hand-built chains
struct BitWriter {
  std::vector<uint8_t> v;
  uint64_t bit = 0;
  void put(uint64_t x, int k) {
    for (int i = 0; i < k; i++, bit++) {
      if ((bit >> 3) >= v.size()) v.push_back(0);
      if ((x >> i) & 1) v[bit >> 3] |= (uint8_t)(1u << (bit & 7));
    }
  }
  void align() { bit = (bit + 7) & ~7ull; }
};

// A chain of one or two index blocks with two entries each, the bytes between and behind them
// 0xFE: no index block starts with them (the reserved bit is set), and as an entry they are not
// valid (flags bit 0 clear), so an entry count that runs past its block reads nothing worse.
// Offsets depend on the entry counts alone, so a mutation of heads and entries leaves the framing
// as parts.h computes it.
struct Chain {
  int wbits_lgwin;                  // what the window bits spell
  std::vector<PartHead> head;
  std::vector<std::vector<PartEntry>> ent;
  std::vector<uint64_t> at, end;    // each block's first byte and the byte after its payload
  uint64_t n = 0;                   // the stream's length
  bool lone_final = false;          // the last byte is the final empty metablock, 0x03
  static constexpr uint64_t kGap = 128;

  Chain(int lgwin, int nblocks, bool lone) : wbits_lgwin(lgwin), lone_final(lone) {
    uint64_t at_b = 0;
    for (int b = 0; b < nblocks; b++) {
      const uint64_t payload = sizeof(PartHead) + 2 * sizeof(PartEntry);
      at.push_back(at_b);
      end.push_back(at_b + part_index_bits(b == 0 ? window_bits_len(lgwin) : 0, payload) / 8);
      at_b = end.back() + kGap;
    }
    n = at_b + (lone ? 1 : 0);
    for (int b = 0; b < nblocks; b++) {
      PartHead h;
      memset(&h, 0, sizeof(h));
      h.magic = kPartMagic;
      h.version = 1;
      h.entry_bytes = sizeof(PartEntry);
      h.nentries = 2;
      h.lgwin = (uint32_t)lgwin;
      h.next_byte = b + 1 < nblocks ? at[b + 1] : lone ? n - 1 : 0;
      h.total = 4000 * (uint64_t)(b + 1);
      head.push_back(h);
      PartEntry e[2];
      memset(e, 0, sizeof(e));
      e[0].bit = e[0].mb_bit = e[1].mb_bit = 8 * end[b];
      e[0].pos = e[0].mb_pos = e[1].mb_pos = 4000 * (uint64_t)b;
      e[0].flags = kPartValid | kPartAtMb;
      e[1].bit = 8 * end[b] + 100;
      e[1].pos = 4000 * (uint64_t)b + 1000;
      e[1].flags = kPartValid;
      ent.push_back({e[0], e[1]});
    }
  }
  std::vector<uint8_t> bytes() const {
    BitWriter w;
    const Wbits &wb = rfc_wbits_of(wbits_lgwin);
    w.put(strtoul(wb.bits, nullptr, 2), (int)strlen(wb.bits));
    for (size_t b = 0; b < head.size(); b++) {
      const uint64_t payload = sizeof(PartHead) + ent[b].size() * sizeof(PartEntry);
      const int skip = part_skip_bytes(payload);
      w.put(0, 1);   // ISLAST
      w.put(3, 2);   // MNIBBLES 0: metadata
      w.put(0, 1);   // reserved
      w.put((uint64_t)skip, 2);
      w.put(payload - 1, 8 * skip);
      w.align();
      const uint8_t *hp = (const uint8_t *)&head[b];
      w.v.insert(w.v.end(), hp, hp + sizeof(PartHead));
      const uint8_t *ep = (const uint8_t *)ent[b].data();
      w.v.insert(w.v.end(), ep, ep + ent[b].size() * sizeof(PartEntry));
      w.bit = 8 * (uint64_t)w.v.size();
      CHECK(w.v.size() == end[b], "block %zu ends at %zu, parts.h says %llu", b, w.v.size(), (unsigned long long)end[b]);
      w.v.insert(w.v.end(), kGap, 0xFE);
      w.bit = 8 * (uint64_t)w.v.size();
    }
    if (lone_final) w.v.push_back(0x03);
    CHECK(w.v.size() == n, "the chain has %zu bytes, planned %llu", w.v.size(), (unsigned long long)n);
    return w.v;
  }
};

// what plan_parts and read_part_index promise of a plan they accept, on a stream of n bytes whose
// first index block ends at first_end
static void check_plan_rules(const PartPlan &p, uint64_t n, uint64_t first_end, const char *what) {
  CHECK(p.ent.size() >= 2, "%s: %zu entries", what, p.ent.size());
  CHECK(p.total > 0 && p.total <= (1ll << 30), "%s: total %lld", what, (long long)p.total);
  CHECK(p.lgwin >= 10 && p.lgwin <= 24, "%s: lgwin %d", what, p.lgwin);
  const PartEntry &e0 = p.ent[0];
  CHECK(e0.pos == 0 && (e0.flags & kPartAtMb), "%s: entry 0 at pos %llu flags %u", what, (unsigned long long)e0.pos, e0.flags);
  CHECK(e0.bit == 8 * first_end && e0.mb_bit == e0.bit && e0.mb_pos == 0, "%s: entry 0 at bit %llu, the first block ends at byte %llu",
        what, (unsigned long long)e0.bit, (unsigned long long)first_end);
  for (size_t i = 0; i < p.ent.size(); i++) {
    const PartEntry &x = p.ent[i];
    CHECK(x.flags & kPartValid, "%s: entry %zu is not valid", what, i);
    CHECK(x.bit < 8 * n && x.mb_bit <= x.bit && x.mb_pos <= x.pos && x.pos < (uint64_t)p.total, "%s: entry %zu out of range", what, i);
    CHECK(i == 0 || (x.pos > p.ent[i - 1].pos && x.bit > p.ent[i - 1].bit), "%s: entry %zu does not advance", what, i);
  }
}

// the byte after the first metadata block's payload, read with the test's own bits
static uint64_t first_block_end(const uint8_t *b, size_t n) {
  size_t bit = 0;
  bit = strlen(rfc_wbits(bits_at(b, n, bit, 7)).bits);
  bits_at(b, n, bit, 4);
  const int nb = (int)bits_at(b, n, bit, 2);
  const uint64_t len = (uint64_t)bits_at(b, n, bit, 8 * nb) + 1;
  return ((bit + 7) >> 3) + len;
}

static void expect_chain(const Chain &c, bool accept, const char *what) {
  const Block s(c.bytes());
  PartPlan plan;
  const bool got = plan_of(s, plan);
  CHECK(got == accept, "lgwin %d, %s: %s", c.wbits_lgwin, what, got ? "accepted" : "rejected");
  if (!accept) return;
  size_t ne = 0;
  for (auto &e : c.ent) ne += e.size();
  CHECK(plan.ent.size() == ne && plan.total == (int64_t)c.head.back().total && plan.lgwin == c.wbits_lgwin,
        "lgwin %d, %s: %zu entries, total %lld, lgwin %d", c.wbits_lgwin, what, plan.ent.size(), (long long)plan.total, plan.lgwin);
  size_t q = 0;
  for (auto &blk : c.ent)
    for (auto &e : blk) {
      CHECK(memcmp(&plan.ent[q], &e, sizeof(e)) == 0, "lgwin %d, %s: entry %zu differs", c.wbits_lgwin, what, q);
      q++;
    }
  check_plan_rules(plan, s.n, c.end[0], what);
  CHECK(looks_indexed(s.p, s.n), "lgwin %d, %s: does not look indexed", c.wbits_lgwin, what);
}

static int run_chains() {
  using Mut = std::function<void(Chain &)>;
  struct Case {
    const char *what;
    int nblocks;
    Mut mut;
  };
  const Case bad[] = {
      {"wrong magic", 1, [](Chain &c) { c.head[0].magic ^= 1; }},
      {"wrong magic in the second block", 2, [](Chain &c) { c.head[1].magic ^= 1; }},
      {"version 2", 1, [](Chain &c) { c.head[0].version = 2; }},
      {"entry_bytes 71", 1, [](Chain &c) { c.head[0].entry_bytes = 71; }},
      {"nentries 0", 1, [](Chain &c) { c.head[0].nentries = 0; }},
      {"nentries 0 in the second block", 2, [](Chain &c) { c.head[1].nentries = 0; }},
      {"nentries above 2^20", 1, [](Chain &c) { c.head[0].nentries = (1u << 20) + 1; }},
      {"nentries beyond the block", 1, [](Chain &c) { c.head[0].nentries = 3; }},
      {"head lgwin is not the window bits", 1, [](Chain &c) { c.head[0].lgwin += 1; }},
      {"next_byte is the current block", 2, [](Chain &c) { c.head[1].next_byte = c.at[1]; }},
      {"next_byte before the current block", 2, [](Chain &c) { c.head[1].next_byte = c.at[1] - 1; }},
      {"next_byte is n", 1, [](Chain &c) { c.head[0].next_byte = c.n; }},
      {"next_byte beyond n", 1, [](Chain &c) { c.head[0].next_byte = c.n + 5; }},
      {"the last block names a next that is no block", 2, [](Chain &c) { c.head[1].next_byte = c.end[1] + 8; }},
      {"the only block names a next that is no block", 1, [](Chain &c) { c.head[0].next_byte = c.end[0] + 8; }},
      {"one valid entry", 1, [](Chain &c) { c.ent[0][1].flags = 0; }},
      {"total 0", 1, [](Chain &c) { c.head[0].total = 0; }},
      {"total above 2^30", 1, [](Chain &c) { c.head[0].total = (1ull << 30) + 1; }},
      {"total negative as a signed number", 1, [](Chain &c) { c.head[0].total = 1ull << 63; }},
      {"entry 0 not at pos 0", 1, [](Chain &c) { c.ent[0][0].pos = 1; }},
      {"entry 0 not at a metablock header", 1, [](Chain &c) { c.ent[0][0].flags = kPartValid; }},
      {"entry 0 behind the first block's end", 1, [](Chain &c) { c.ent[0][0].bit += 8, c.ent[0][0].mb_bit += 8; }},
      {"entry 0 before the first block's end", 1, [](Chain &c) { c.ent[0][0].bit -= 8, c.ent[0][0].mb_bit -= 8; }},
      {"entry 0: mb_bit is not bit", 1, [](Chain &c) { c.ent[0][0].mb_bit -= 1; }},
      {"an entry's bit is 8n", 1, [](Chain &c) { c.ent[0][1].bit = 8 * c.n; }},
      {"an entry's mb_bit above its bit", 1, [](Chain &c) { c.ent[0][1].mb_bit = c.ent[0][1].bit + 1; }},
      {"an entry's mb_pos above its pos", 1, [](Chain &c) { c.ent[0][1].mb_pos = c.ent[0][1].pos + 1; }},
      {"an entry's pos is the total", 1, [](Chain &c) { c.ent[0][1].pos = c.head[0].total; }},
      {"pos does not increase", 1, [](Chain &c) { c.ent[0][1].pos = 0; }},
      {"pos decreases in the second block", 2, [](Chain &c) { c.ent[1][0].pos = c.ent[1][0].mb_pos = c.ent[1][1].mb_pos = 500; }},
      {"bit does not increase", 1, [](Chain &c) { c.ent[0][1].bit = c.ent[0][0].bit; }},
  };
  for (int lgwin : {16, 17, 22}) {   // window bits of 1, 7 and 4 bits
    CHECK(window_bits_len(lgwin) == (int)strlen(rfc_wbits_of(lgwin).bits), "window_bits_len(%d)", lgwin);
    expect_chain(Chain(lgwin, 1, false), true, "one block");
    expect_chain(Chain(lgwin, 2, false), true, "two blocks through next_byte");
    expect_chain(Chain(lgwin, 1, true), true, "one block and the lone final metablock");
    expect_chain(Chain(lgwin, 2, true), true, "two blocks and the lone final metablock");
    for (const Case &k : bad) {
      Chain c(lgwin, k.nblocks, false);
      k.mut(c);
      expect_chain(c, false, k.what);
    }
    {   // the byte a lone final metablock must be
      Chain c(lgwin, 1, true);
      std::vector<uint8_t> v = c.bytes();
      v.back() = 0x07;
      const Block s(v);
      PartPlan plan;
      CHECK(!plan_of(s, plan), "lgwin %d: a chain ending in 0x07 accepted", lgwin);
    }
    {   // wrong magic: not even a candidate
      Chain c(lgwin, 1, false);
      c.head[0].magic ^= 1;
      const Block s(c.bytes());
      CHECK(!looks_indexed(s.p, s.n), "lgwin %d: wrong magic looks indexed", lgwin);
    }
  }
  for (int own : {0, 1}) {   // the large-window escape in front of a sound block: rejected, and no candidate
    Chain c(17, 1, false);     // (own: the head's lgwin is whatever the reader makes of the escape)
    c.wbits_lgwin = kLargeWindow;
    if (own) c.head[0].lgwin = (uint32_t)kLargeWindow;
    const Block s(c.bytes());
    PartPlan plan;
    CHECK(!plan_of(s, plan) && !looks_indexed(s.p, s.n), "the large-window escape accepted");
  }
  return 0;
}

// ---------------------------------------------------------------- robustness
static long g_accepted = 0, g_tried = 0;
static void try_stream(const Block &s, const char *what) {
  PartPlan plan;
  g_tried++;
  if (plan_of(s, plan)) {
    g_accepted++;
    check_plan_rules(plan, s.n, first_block_end(s.p, s.n), what);
  }
  (void)looks_indexed(s.p, s.n);
  g_checks++;
}
static void run_robust_on(const std::vector<uint8_t> &v, const char *what) {
  {
    Block s(v);
    for (size_t bit = 0; bit < 8 * 2048 && bit < 8 * s.n; bit++) {
      s.p[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
      try_stream(s, what);
      s.p[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
    }
  }
  for (size_t cut = 0; cut <= 3000 && cut <= v.size(); cut++) {
    const Block s(v.data(), cut);
    try_stream(s, what);
  }
}
static int run_robust(const char *path) {
  run_robust_on(read_file(path), "the fixture, mutated");
  run_robust_on(Chain(22, 2, true).bytes(), "a hand-built chain, mutated");
  printf("accepted %ld of %ld\n", g_accepted, g_tried);
  return 0;
}

// ---------------------------------------------------------------- window bits, announced size
static int run_window() {
  static const uint8_t tails[][4] = {{0, 0, 0, 0}, {0xFF, 0xFF, 0xFF, 0xFF}, {0x5A, 0xC3, 0x17, 0x9E}, {0x01, 0x80, 0x00, 0x7F}};
  for (uint32_t v = 0; v < 65536; v++) {
    const uint8_t two[2] = {(uint8_t)v, (uint8_t)(v >> 8)};
    const Block s(two, 2);
    const Wbits &w = rfc_wbits(v);
    PadBits pad{s.p, s.n};
    const WindowBits a = read_window_bits(pad);
    HostFetch f{s.p, s.n};
    HdrBits<HostFetch> hdr{f, 0};
    const WindowBits b = read_window_bits(hdr);
    CHECK(a.lgwin == w.lgwin && a.nbits == (int)strlen(w.bits) && pad.bit == (size_t)a.nbits, "prefix %#x: lgwin %d in %d bits", v, a.lgwin, a.nbits);
    CHECK(b.lgwin == a.lgwin && b.nbits == a.nbits && hdr.ok && hdr.bit == (uint64_t)b.nbits, "prefix %#x: the two readers differ", v);
    // peek_window_bits: the window's log2, and 24 where the decoder will refuse the stream anyway
    CHECK(peek_window_bits(s.p, 2) == (w.lgwin == kLargeWindow ? 24 : w.lgwin), "prefix %#x: peek %d", v, peek_window_bits(s.p, 2));
    CHECK(decoded_size(s.p, 2) == rfc_decoded_size(s.p, 2), "prefix %#x alone: size %lld", v, (long long)decoded_size(s.p, 2));
    for (auto &t : tails) {
      const uint8_t six[6] = {two[0], two[1], t[0], t[1], t[2], t[3]};
      const Block l(six, 6);
      CHECK(decoded_size(l.p, 6) == rfc_decoded_size(l.p, 6), "prefix %#x tail %02x..: size %lld, by the RFC %lld", v, t[0],
            (long long)decoded_size(l.p, 6), (long long)rfc_decoded_size(l.p, 6));
    }
  }
  for (uint32_t v = 0; v < 256; v++) {   // one byte: every window pattern fits in it
    const uint8_t one = (uint8_t)v;
    const Block s(&one, 1);
    const int lg = rfc_wbits(v).lgwin;
    CHECK(peek_window_bits(s.p, 1) == (lg == kLargeWindow ? 24 : lg), "byte %#x: peek %d", v, peek_window_bits(s.p, 1));
    CHECK(decoded_size(s.p, 1) == rfc_decoded_size(s.p, 1), "byte %#x: size", v);
  }
  const Block none(nullptr, 0);   // no bytes read as zeros
  CHECK(peek_window_bits(none.p, 0) == 16 && decoded_size(none.p, 0) == -1, "the empty stream");
  return 0;
}

// ---------------------------------------------------------------- batch layout
// lgwin 16, then one metablock header announcing mlen (4 to 6 nibbles as needed)
static std::vector<uint8_t> header_stream(bool last, uint64_t mlen, size_t size) {
  BitWriter w;
  w.put(0, 1);
  w.put(last, 1);
  if (last) w.put(0, 1);   // ISLASTEMPTY
  const int nib = mlen - 1 < (1u << 16) ? 4 : mlen - 1 < (1u << 20) ? 5 : 6;
  w.put((uint64_t)(nib - 4), 2);
  w.put(mlen - 1, 4 * nib);
  w.v.resize(size, 0xA5);
  return w.v;
}

static int run_layout(const char *path) {
  const std::vector<uint8_t> indexed = read_file(path);
  struct Item {
    const char *what;
    std::vector<uint8_t> bytes;
    int64_t est;
  };
  const int64_t kLimit = 5000;
  // (an RFC 7932 header announces 2^24 bytes at most -- six nibbles of MLEN - 1 -- so no stream can
  // announce more than kBatchSlotMax, 64 MiB: the largest announcement stands for that case)
  const Item items[] = {
      {"empty input", {}, -1},
      {"header-sized: the empty stream", {0x06}, 0},
      {"no announced size, small", header_stream(false, 4661, 100), -1},
      {"no announced size, 100,000 bytes", header_stream(false, 4661, 100000), -1},
      {"announces 300 bytes", header_stream(true, 300, 40), 300},
      {"announces more than the limit", header_stream(true, 10000, 64), 10000},
      {"announces 16 MiB, the most a header can", header_stream(true, 1u << 24, 64), 1 << 24},
      {"the indexed fixture", indexed, -1},
      {"announces 65,536 bytes", header_stream(true, 65536, 300), 65536},
  };
  const size_t k = sizeof(items) / sizeof(items[0]);
  std::vector<Block *> blocks;
  std::vector<mib_span> spans;
  for (const Item &it : items) {
    blocks.push_back(new Block(it.bytes));
    spans.push_back(mib_span{blocks.back()->p, blocks.back()->n});
  }
  spans[0].data = nullptr;   // (an empty input may come without a pointer)
  CHECK(looks_indexed(spans[7].data, spans[7].size), "the fixture does not look indexed");
  CHECK(kBatchSlotMax == 64ll << 20 && items[6].est < kBatchSlotMax, "kBatchSlotMax");
  for (int alone = 0; alone < 2; alone++)
    for (int64_t max_out : {(int64_t)-1, kLimit}) {
      const BatchLayout l = plan_batch(spans.data(), k, max_out, alone != 0);
      CHECK(l.item.size() == k, "%zu items", l.item.size());
      uint64_t in_at = 0, out_at = 0;
      for (size_t i = 0; i < k; i++) {
        const BatchItem &t = l.item[i];
        const Item &it = items[i];
        CHECK(t.est == it.est, "%s: est %lld", it.what, (long long)t.est);
        const BatchHow want = max_out >= 0 && it.est > max_out ? kSettled : alone && i == 7 ? kAlone : kInLaunch;
        CHECK(t.how == want, "%s (alone rules %d, limit %lld): handled as %d, expected %d", it.what, alone, (long long)max_out, t.how, want);
        if (t.how != kInLaunch) continue;
        const uint64_t n = it.bytes.size();
        const uint64_t cap = it.est > 0 ? (uint64_t)it.est : (8 * n > 65536 ? 8 * n : 65536);
        CHECK(decode_cap(it.est, n) == cap, "%s: capacity %llu", it.what, (unsigned long long)decode_cap(it.est, n));
        CHECK(t.in_off == in_at && t.out_off == out_at, "%s: offsets %llu / %llu overlap or leave a hole", it.what,
              (unsigned long long)t.in_off, (unsigned long long)t.out_off);
        CHECK(t.in_off % 256 == 0 && t.out_off % 256 == 0 && t.out_slot % 256 == 0, "%s: not 256-aligned", it.what);
        CHECK(t.out_slot >= cap + MIB_IN_PLACE_SLACK + 64 && t.out_slot < cap + MIB_IN_PLACE_SLACK + 64 + 256 && t.out_slot == decode_slot(cap),
              "%s: slot %llu for capacity %llu", it.what, (unsigned long long)t.out_slot, (unsigned long long)cap);
        in_at += (n + 255) / 256 * 256;
        out_at += t.out_slot;
      }
      CHECK(l.in_bytes == in_at && l.out_bytes == out_at, "totals %llu / %llu", (unsigned long long)l.in_bytes, (unsigned long long)l.out_bytes);
    }
  for (Block *b : blocks) delete b;
  return 0;
}

static int run_golden(const char *path) {
  const Block s(read_file(path));
  PartPlan plan;
  CHECK(plan_of(s, plan), "the fixture's chain is rejected");
  check_plan_rules(plan, s.n, first_block_end(s.p, s.n), "the fixture");
  printf("plan %zu %lld %d %d\n", plan.ent.size(), (long long)plan.total, plan.lgwin, looks_indexed(s.p, s.n) ? 1 : 0);
  for (const PartEntry &e : plan.ent)
    printf("entry %llu %llu %llu %llu %u\n", (unsigned long long)e.bit, (unsigned long long)e.pos, (unsigned long long)e.mb_bit,
           (unsigned long long)e.mb_pos, e.flags);
  return 0;
}

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  int rc = 2;
  if (!strcmp(mode, "golden") && argc > 2) rc = run_golden(argv[2]);
  else if (!strcmp(mode, "chains")) rc = run_chains();
  else if (!strcmp(mode, "robust") && argc > 2) rc = run_robust(argv[2]);
  else if (!strcmp(mode, "window")) rc = run_window();
  else if (!strcmp(mode, "layout") && argc > 2) rc = run_layout(argv[2]);
  if (rc == 2) printf("usage: decode_plan_host golden FILE | chains | robust FILE | window | layout FILE\n");
  if (rc == 0) printf("ok %ld\n", g_checks);
  return rc;
}
