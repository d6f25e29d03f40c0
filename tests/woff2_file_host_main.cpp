// Stand-alone host build of the WOFF2 container parser and the serial sfnt assembly
// (brotli-lib_amd/csrc/woff2_file.h), meant to be built with -fsanitize=address,undefined
// (tests/test_woff2_file_host.py).
//
//   woff2_file_host assemble IN OUT   IN: pairs of records (file, decompressed stream); OUT gets
//                                     a pair per input: host_assemble's return code (4 bytes,
//                                     little-endian, two's complement) and the sfnt
//   woff2_file_host fuzz IN SEED N    IN as above.  Damaged copies of each file (byte flips,
//                                     truncations, length edits across header and directory, N
//                                     random double edits) with the file's own stream: each is
//                                     rejected, or its plan keeps the invariants below
// A record is a u32 little-endian length + bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "woff2_file.h"

using namespace mib::woff2file;
typedef std::vector<uint8_t> Bytes;

static std::vector<Bytes> read_records(const char *path) {
  std::vector<Bytes> r;
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t h[4];
  while (fread(h, 1, 4, f) == 4) {
    const uint32_t n = h[0] | (h[1] << 8) | (h[2] << 16) | ((uint32_t)h[3] << 24);
    Bytes b(n);
    if (n && fread(b.data(), 1, n, f) != n) {
      fprintf(stderr, "short record in %s\n", path);
      exit(2);
    }
    r.push_back(b);
  }
  fclose(f);
  return r;
}
static void write_record(FILE *f, const uint8_t *p, size_t n) {
  const uint8_t h[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
  fwrite(h, 1, 4, f);
  if (n) fwrite(p, 1, n, f);
}

static void fail(const char *what) {
  fprintf(stderr, "invariant broken: %s\n", what);
  exit(1);
}

// What a plan must keep whatever the file says: sources back to back inside the stream it
// announces; once laid out, destinations in ascending order behind the records, at 4-byte
// boundaries, apart, inside the announced size; the record order a permutation sorted by tag.
static void check_sources(const Plan &pl) {
  uint64_t at = 0;
  for (const Table &t : pl.t) {
    if (t.src_off != at) fail("source offsets are not back to back");
    at += t.src_len;
  }
  if (at != pl.stream_len || at > mib::woff2inv::kMaxInput) fail("sources leave the stream");
  if (pl.order.size() != pl.t.size()) fail("record order size");
  std::vector<char> seen(pl.t.size(), 0);
  for (size_t r = 0; r < pl.order.size(); r++) {
    if (pl.order[r] >= pl.t.size() || seen[pl.order[r]]++) fail("record order is no permutation");
    if (r && pl.t[pl.order[r - 1]].tag >= pl.t[pl.order[r]].tag) fail("records not sorted by tag");
  }
}
static void check_destinations(const Plan &pl, size_t out_size) {
  uint64_t at = 12 + 16 * (uint64_t)pl.t.size();
  for (const Table &t : pl.t) {
    if (t.dst_off != at || (t.dst_off & 3)) fail("destination not at the next 4-byte boundary");
    at = ((uint64_t)t.dst_off + t.dst_len + 3) & ~3ull;
    if (at > pl.sfnt_len) fail("destination leaves the announced size");
  }
  if (at != pl.sfnt_len || pl.sfnt_len != out_size) fail("announced size is not the output's");
}

// File and stream in heap blocks of exactly their sizes, so that a read past either is a
// sanitizer report.
static int run(const Bytes &file, const Bytes &stream, Bytes *sfnt) {
  uint8_t *f = (uint8_t *)malloc(file.size() ? file.size() : 1), *s = (uint8_t *)malloc(stream.size() ? stream.size() : 1);
  if (!file.empty()) memcpy(f, file.data(), file.size());
  if (!stream.empty()) memcpy(s, stream.data(), stream.size());
  Plan pl;
  if (parse(file.empty() ? nullptr : f, file.size(), &pl)) check_sources(pl);
  Plan laid;
  const int rc = host_assemble(file.empty() ? nullptr : f, file.size(), stream.empty() ? nullptr : s, stream.size(), sfnt, &laid);
  if (rc == 0) {
    check_sources(laid);
    check_destinations(laid, sfnt->size());
  } else if (!sfnt->empty() && rc != 0) {
    fail("a rejected file left output");
  }
  free(f);
  free(s);
  return rc;
}

static uint64_t g_rng;
static uint32_t rnd() {   // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 2685821657736338717ull) >> 32);
}

static uint32_t be32(const Bytes &b, size_t at) {
  return ((uint32_t)b[at] << 24) | ((uint32_t)b[at + 1] << 16) | ((uint32_t)b[at + 2] << 8) | b[at + 3];
}
static void set32(Bytes &b, size_t at, uint32_t v) {
  b[at] = (uint8_t)(v >> 24), b[at + 1] = (uint8_t)(v >> 16), b[at + 2] = (uint8_t)(v >> 8), b[at + 3] = (uint8_t)v;
}
static Bytes base128_of(uint32_t v) {
  Bytes out;
  for (int sh = 28; sh > 0; sh -= 7)
    if (v >> sh) out.push_back((uint8_t)(0x80 | ((v >> sh) & 0x7F)));
  out.push_back((uint8_t)(v & 0x7F));
  return out;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const std::string mode = argv[1];
  const std::vector<Bytes> rec = read_records(argv[2]);
  if (rec.size() % 2) return 2;
  if (mode == "assemble") {
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    for (size_t i = 0; i < rec.size(); i += 2) {
      Bytes sfnt;
      const int32_t rc = run(rec[i], rec[i + 1], &sfnt);
      const uint32_t u = (uint32_t)rc;
      const uint8_t c[4] = {(uint8_t)u, (uint8_t)(u >> 8), (uint8_t)(u >> 16), (uint8_t)(u >> 24)};
      write_record(out, c, 4);
      write_record(out, sfnt.data(), sfnt.size());
    }
    fclose(out);
    printf("assembled %zu\n", rec.size() / 2);
    return 0;
  }
  if (mode != "fuzz" || argc < 5) return 2;
  g_rng = strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
  const size_t doubles = strtoull(argv[4], nullptr, 10);
  size_t total = 0, accepted = 0;
  for (size_t i = 0; i < rec.size(); i += 2) {
    const Bytes &file = rec[i], &stream = rec[i + 1];
    auto one = [&](const Bytes &f) {
      Bytes sfnt;
      total++;
      if (run(f, stream, &sfnt) == 0) accepted++;
    };
    Bytes sfnt;
    Plan pl;
    if (run(file, stream, &sfnt) != 0 || !parse(file.data(), file.size(), &pl)) return 1;   // the undamaged file
    const size_t dir_end = pl.comp_off;
    // the bytes a reader has to act on: signature, length, numTables, totalCompressedSize, the
    // directory (flavor, the reserved field, totalSfntSize, versions, metadata and private
    // block fields are passed through or ignored: damage there is no damage)
    std::vector<size_t> live;
    for (size_t p = 0; p < dir_end; p++)
      if (p < 4 || (p >= 8 && p < 14) || (p >= 20 && p < 24) || p >= kHeaderBytes) live.push_back(p);
    // truncations: every length, with the header's length field as it was and made to agree
    for (size_t len = 0; len < file.size(); len++) {
      Bytes u(file.begin(), file.begin() + len);
      one(u);
      if (len >= 12) {
        set32(u, 8, (uint32_t)len);
        one(u);
      }
    }
    // every bit of the live bytes flipped
    for (size_t p : live)
      for (int b = 0; b < 8; b++) {
        Bytes u = file;
        u[p] ^= (uint8_t)(1u << b);
        one(u);
      }
    // length edits: the header's length and totalCompressedSize, then every UIntBase128 of the
    // directory rewritten (the file grows or shrinks with its encoding, the header's length
    // follows), to the value moved by +-1..32, halved, doubled, and to every power of two and
    // its predecessor
    auto values = [&](uint32_t v) {
      std::vector<uint32_t> out;
      for (uint32_t d = 1; d <= 32; d++) out.push_back(v + d), out.push_back(v - d);
      out.push_back(v / 2), out.push_back(v * 2), out.push_back(0), out.push_back(0xFFFFFFFFu);
      for (int s = 0; s < 32; s++) out.push_back(1u << s), out.push_back((1u << s) - 1);
      return out;
    };
    for (size_t at : {(size_t)8, (size_t)20})
      for (uint32_t v : values(be32(file, at))) {
        if (v == be32(file, at)) continue;
        Bytes u = file;
        set32(u, at, v);
        one(u);
      }
    {
      // the directory's fields again, by the rules of section 4.1 (the undamaged file parsed)
      size_t p = kHeaderBytes;
      for (size_t t = 0; t < pl.t.size(); t++) {
        const uint32_t flags = file[p];
        p += (flags & 63) == 63 ? 5 : 1;
        const int nlen = pl.t[t].kind == kCopy ? 1 : 2;
        for (int k = 0; k < nlen; k++) {
          size_t e = p;
          uint32_t v = 0;
          do v = (v << 7) | (file[e] & 0x7F);
          while (file[e++] & 0x80);
          // (a transformed table's origLength is a hint: whatever it says is accepted, so a
          // handful of values is all it gets)
          const bool hint = nlen == 2 && k == 0;
          std::vector<uint32_t> vals = values(v);
          if (hint) vals.resize(8);
          for (uint32_t nv : vals) {
            if (nv == v) continue;
            const Bytes enc = base128_of(nv);
            Bytes u(file.begin(), file.begin() + p);
            u.insert(u.end(), enc.begin(), enc.end());
            u.insert(u.end(), file.begin() + e, file.end());
            set32(u, 8, (uint32_t)u.size());
            one(u);
          }
          // malformed encodings: a leading 0x80, a continuation bit on the last byte
          Bytes u = file;
          u.insert(u.begin() + p, 0x80);
          set32(u, 8, (uint32_t)u.size());
          one(u);
          u = file;
          u[e - 1] |= 0x80;
          one(u);
          p = e;
        }
      }
      if (p != dir_end) fail("the fuzzer lost the directory");
    }
    // two live bytes at once: a random or an off-by-one / extreme value each
    for (size_t d = 0; d < doubles; d++) {
      Bytes u = file;
      for (int k = 0; k < 2; k++) {
        const size_t p = live[rnd() % live.size()];
        const uint32_t how = rnd() % 6;
        const uint8_t old = u[p];
        u[p] = how == 0 ? old + 1 : how == 1 ? old - 1 : how == 2 ? 0xFF : how == 3 ? 0 : how == 4 ? (old ^ (1u << (rnd() & 7))) : (uint8_t)rnd();
      }
      if (u != file) one(u);
    }
  }
  printf("damaged %zu accepted %zu rejected %zu\n", total, accepted, total - accepted);
  return 0;
}
