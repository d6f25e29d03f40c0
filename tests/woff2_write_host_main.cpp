// Stand-alone host build of the WOFF2 writer's plan (brotli-lib_amd/csrc/woff2_write.h), meant to
// be built with -fsanitize=address,undefined (tests/test_woff2_write_host.py).
//
//   woff2_write_host pack IN OUT    IN: groups of five records -- the sfnt, the transforms (one
//                                   byte), the transformed glyf table, the transformed hmtx table
//                                   (empty: none), the compressed size (4 bytes, little-endian).
//                                   OUT gets four records per group: parse()'s answer (4 bytes,
//                                   little-endian: 0, or the item of the rejection list, 9 for what
//                                   the glyf transform needs), the directory, the header, the
//                                   stream (empty where the font is rejected)
//   woff2_write_host fuzz IN        IN: sfnts, a record each.  Damaged copies of each (every
//                                   truncation up to the directory's end and a little beyond, every
//                                   bit of the offset table and the directory flipped, every
//                                   length and offset field set to a list of values): each is
//                                   rejected, or its plan keeps the invariants below and
//                                   host_pack runs over it
// A record is a u32 little-endian length + bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "woff2_write.h"

using namespace mib::woff2write;
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

// What a plan must keep whatever the sfnt says: every source range inside the input, tags
// ascending, no DSIG, glyf and loca together and in one state.
static void check_sources(const Plan &pl, size_t n) {
  if (pl.t.empty()) fail("no table kept");
  for (size_t i = 0; i < pl.t.size(); i++) {
    const Table &t = pl.t[i];
    if ((uint64_t)t.src_off + t.src_len > n) fail("a source range leaves the input");
    if (i && pl.t[i - 1].tag >= t.tag) fail("tags not ascending");
    if (t.tag == kDsigTag) fail("DSIG kept");
  }
  if ((pl.glyf == kNoTable) != (pl.loca == kNoTable)) fail("glyf without loca");
  if (pl.tr_glyf) {
    if (pl.glyf == kNoTable || pl.head == kNoTable || pl.maxp == kNoTable) fail("glyf transform without its tables");
    if (pl.t[pl.head].src_len < 54 || pl.t[pl.maxp].src_len < 6 || pl.num_glyphs == 0) fail("glyf transform's needs");
    if (((uint64_t)pl.num_glyphs + 1) * (pl.long_loca ? 4 : 2) > pl.t[pl.loca].src_len) fail("short loca accepted");
  }
  if (pl.hmtx_wanted) {
    if (!pl.tr_glyf || pl.hmtx == kNoTable || pl.hhea == kNoTable || pl.t[pl.hhea].src_len < 36) fail("hmtx transform without its tables");
    if (pl.num_hmetrics < 1 || pl.num_hmetrics > pl.num_glyphs) fail("numberOfHMetrics");
    if (pl.t[pl.hmtx].src_len != 4ull * pl.num_hmetrics + 2ull * (pl.num_glyphs - pl.num_hmetrics)) fail("hmtx size");
  }
}
// Once laid out: the pieces of the stream back to back from 0 (so apart), ending at stream_len.
static void check_stream(const Plan &pl) {
  uint64_t at = 0;
  for (const Table &t : pl.t) {
    if (t.at != at) fail("stream pieces are not back to back");
    at += t.len;
    if (at > pl.stream_len) fail("a stream piece leaves stream_len");
    if (t.state == kPlain && t.len != t.src_len) fail("a plain table's length changed");
  }
  if (at != pl.stream_len || at > mib::woff2inv::kMaxInput) fail("stream_len");
}

static int pack_mode(const char *in, const char *out) {
  const std::vector<Bytes> r = read_records(in);
  if (r.size() % 5) fail("pack wants groups of five records");
  FILE *f = fopen(out, "wb");
  if (!f) return 2;
  size_t done = 0;
  for (size_t i = 0; i < r.size(); i += 5) {
    const Bytes &sfnt = r[i], &tglyf = r[i + 2], &thmtx = r[i + 3];
    if (r[i + 1].size() != 1 || r[i + 4].size() != 4) fail("pack record sizes");
    const uint32_t comp = r[i + 4][0] | (r[i + 4][1] << 8) | (r[i + 4][2] << 16) | ((uint32_t)r[i + 4][3] << 24);
    Plan pl;
    // (an exact-size copy: a read past the end is a report)
    uint8_t *copy = (uint8_t *)malloc(sfnt.size() ? sfnt.size() : 1);
    if (sfnt.size()) memcpy(copy, sfnt.data(), sfnt.size());
    int rc = parse(sfnt.size() ? copy : nullptr, sfnt.size(), r[i + 1][0], &pl);
    Bytes stream;
    uint8_t hdr[mib::woff2file::kHeaderBytes] = {0};
    if (rc == kOk) {
      check_sources(pl, sfnt.size());
      if (!layout(&pl, tglyf.size(), thmtx.size()) || !finish(pl, copy, comp, hdr)) rc = -1;
      else {
        check_stream(pl);
        host_pack(pl, copy, tglyf.data(), thmtx.data(), &stream);
      }
    }
    free(copy);
    const uint8_t c[4] = {(uint8_t)rc, (uint8_t)(rc >> 8), (uint8_t)(rc >> 16), (uint8_t)(rc >> 24)};
    write_record(f, c, 4);
    write_record(f, pl.dir.data(), rc == kOk ? pl.dir.size() : 0);
    write_record(f, hdr, rc == kOk ? sizeof(hdr) : 0);
    write_record(f, stream.data(), stream.size());
    done++;
  }
  fclose(f);
  printf("packed %zu\n", done);
  return 0;
}

static size_t g_damaged = 0, g_accepted = 0;
static size_t g_why[10] = {0};

static void try_font(const uint8_t *p, size_t n) {
  uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(copy, p, n);
  g_damaged++;
  for (uint32_t transforms = 0; transforms < 4; transforms += 3) {
    Plan pl;
    const int rc = parse(copy, n, transforms, &pl);
    if (rc < 0 || rc > 9) fail("parse's answer");
    if (transforms == 3) g_why[rc]++;
    if (rc != kOk) continue;
    if (transforms == 3) g_accepted++;
    check_sources(pl, n);
    // transformed tables of made-up sizes: what matters is where the pieces go
    const Bytes tglyf(pl.tr_glyf ? 36 + 5 * (size_t)pl.num_glyphs : 0, 0x5A);
    const Bytes thmtx(pl.hmtx_wanted ? 1 + 2 * (size_t)pl.num_hmetrics : 0, 0xA5);
    for (int with_hmtx = 0; with_hmtx < 2; with_hmtx++) {
      if (!layout(&pl, tglyf.size(), with_hmtx ? thmtx.size() : 0)) continue;
      check_stream(pl);
      if (pl.tr_hmtx != (with_hmtx && pl.hmtx_wanted)) fail("hmtx state");
      Bytes stream;
      host_pack(pl, copy, tglyf.data(), thmtx.data(), &stream);
      if (stream.size() != pl.stream_len) fail("host_pack's size");
      uint8_t hdr[mib::woff2file::kHeaderBytes];
      if (!finish(pl, copy, stream.size(), hdr)) fail("finish");
      // the directory reads back as what was planned
      mib::woff2file::Reader r{pl.dir.data(), pl.dir.size(), 0, false};
      for (const Table &t : pl.t) {
        const uint32_t flags = r.u8();
        const uint32_t tag = (flags & 63) == 63 ? r.u32() : mib::woff2file::kKnownTags[flags & 63];
        if (tag != t.tag || r.base128() != t.src_len) fail("directory entry");
        if (t.state != kPlain && r.base128() != t.len) fail("directory transformLength");
      }
      if (r.bad || r.pos != pl.dir.size()) fail("directory size");
    }
  }
  free(copy);
}

static int fuzz_mode(const char *in) {
  static const uint32_t kValues[] = {0, 1, 2, 3, 4, 11, 12, 13, 16, 17, 18, 35, 36, 53, 54, 255, 256, 0x7FFF, 0x8000, 0xFFFF,
                                     0x10000, 0xFFFFFF, 0x10000000, 0x10000001, 0x7FFFFFFF, 0x80000000u, 0xFFFFFFFCu, 0xFFFFFFFFu};
  for (const Bytes &font : read_records(in)) {
    if (font.size() < 12) fail("fuzz wants sfnts");
    const size_t dir_end = 12 + 16 * (size_t)((font[4] << 8) | font[5]);
    if (dir_end > font.size()) fail("fuzz wants whole directories");
    const size_t accepted_before = g_accepted;
    try_font(font.data(), font.size());
    if (g_accepted != accepted_before + 1) fail("the undamaged font is rejected");
    for (size_t n = 0; n <= dir_end + 64 && n < font.size(); n++) try_font(font.data(), n);
    Bytes b = font;
    for (size_t at = 0; at < dir_end; at++)
      for (int bit = 0; bit < 8; bit++) {
        b[at] ^= (uint8_t)(1 << bit);
        try_font(b.data(), b.size());
        b[at] = font[at];
      }
    for (size_t rec = 12; rec < dir_end; rec += 16)
      for (size_t field = 8; field < 16; field += 4)
        for (uint32_t v : kValues) {
          for (int s = 0; s < 4; s++) b[rec + field + s] = (uint8_t)(v >> (24 - 8 * s));
          try_font(b.data(), b.size());
          // ... and the same value as a distance from the end of the input
          const uint32_t w = (uint32_t)font.size() - v;
          for (int s = 0; s < 4; s++) b[rec + field + s] = (uint8_t)(w >> (24 - 8 * s));
          try_font(b.data(), b.size());
          memcpy(&b[rec + field], &font[rec + field], 4);
        }
  }
  printf("damaged %zu accepted %zu rejected %zu why", g_damaged, g_accepted, g_damaged - g_accepted);
  for (int q = 1; q < 10; q++) printf(" %zu", g_why[q]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "pack")) return pack_mode(argv[2], argv[3]);
  if (argc == 3 && !strcmp(argv[1], "fuzz")) return fuzz_mode(argv[2]);
  fprintf(stderr, "usage: woff2_write_host pack IN OUT | fuzz IN\n");
  return 2;
}
