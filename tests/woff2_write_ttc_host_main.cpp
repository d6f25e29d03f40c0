// Stand-alone host build of the WOFF2 writer's collection plan (brotli-lib_amd/csrc/woff2_write_ttc.h),
// meant to be built with -fsanitize=address,undefined (tests/test_woff2_write_ttc_host.py).
//
//   woff2_write_ttc_host pack IN OUT   IN: groups of six records -- the TTC, the transforms (one
//                                      byte), the compare's answers (a byte per candidate, non-zero:
//                                      differs -- there is no device here), the transformed glyf
//                                      tables and the transformed hmtx tables (each a list of
//                                      directory index (4 bytes) + length (4 bytes) + bytes; an hmtx
//                                      unit without one stays as it is), the compressed size (4
//                                      bytes).  Integers are little-endian.  OUT gets five records
//                                      per group: the answer (4 bytes: 0, or the item of the
//                                      rejection list), directory + CollectionHeader, the header, the
//                                      stream, and the TTC that woff2_file.h's host_assemble makes of
//                                      the written container and that stream (the program exits
//                                      non-zero where the decoder's plan rejects what was written)
//   woff2_write_ttc_host fuzz IN       IN: TTCs, a record each.  Damaged copies of each (every
//                                      truncation up to the last directory's end and a little beyond,
//                                      every bit of the header and the directories flipped, every
//                                      offset and length field set to a list of values): each is
//                                      rejected, or its plan keeps the invariants below, with the
//                                      candidates compared here, and ttc_host_pack runs over it
// A record is a u32 little-endian length + bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "woff2_write_ttc.h"

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
static uint32_t le32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

static void fail(const char *what) {
  fprintf(stderr, "invariant broken: %s\n", what);
  exit(1);
}

// What a plan with its entries must keep whatever the TTC says.
static void check_entries(const TtcPlan &pl, size_t n, uint32_t transforms) {
  const size_t num = pl.t.size();
  if (num == 0 || num > 65535) fail("the number of entries");
  if (pl.fix.size() != num || pl.unit.size() != num) fail("per-entry vectors");
  for (size_t i = 0; i < num; i++) {
    const Table &t = pl.t[i];
    if ((uint64_t)t.src_off + t.src_len > n) fail("a source range leaves the input");
    if (t.tag == kDsigTag) fail("DSIG kept");
    if (t.tag == kGlyfTag && (i + 1 >= num || pl.t[i + 1].tag != kLocaTag)) fail("glyf without its loca behind it");
    if (t.tag == kLocaTag && (i == 0 || pl.t[i - 1].tag != kGlyfTag)) fail("loca without its glyf in front");
    if (t.tag == kGlyfTag && (t.state == kTrGlyf) != (pl.t[i + 1].state == kTrLoca)) fail("a pair in two states");
    if ((t.state == kTrGlyf) != (t.tag == kGlyfTag && pl.tr_glyf)) fail("glyf state");
    if (pl.fix[i] != kHeadNone && (t.tag != kHeadTag || t.src_len < 18)) fail("a head fix on another table");
    if (t.tag == kHeadTag && t.src_len >= 18 && pl.fix[i] == kHeadNone) fail("a head without its fix");
  }
  if (pl.tr_glyf != ((transforms & kTransformGlyf) != 0)) fail("tr_glyf");
  if (pl.fonts.size() != pl.num_fonts || pl.fonts.empty()) fail("members");
  std::vector<uint8_t> listed(num, 0);
  for (const TtcMember &m : pl.fonts) {
    if (m.idx.empty() || m.idx.size() != m.count) fail("a member's index count");
    for (size_t q = 0; q < m.idx.size(); q++) {
      if (m.idx[q] >= num) fail("a member's index at or past the entry count");
      if (q && m.idx[q - 1] >= m.idx[q]) fail("a member's indices not ascending");
      listed[m.idx[q]] = 1;
    }
    for (uint32_t i = m.first; i < m.first + m.count; i++) {
      const TtcRecord &r = pl.rec[i];
      if (r.entry >= num || pl.t[r.entry].tag != r.tag || pl.t[r.entry].src_len != r.len) fail("a record's entry");
    }
    if ((m.glyf == kNoTable) != (m.loca == kNoTable) || (m.glyf == kNoTable) != (m.pair == kNoTable)) fail("a member's pair");
    if (m.glyf != kNoTable && pl.rec[m.loca].entry != pl.rec[m.glyf].entry + 1) fail("a member lists another pair's loca");
  }
  for (size_t i = 0; i < num; i++)
    if (!listed[i]) fail("an entry that no member lists");
  for (size_t p = 0; p < pl.pairs.size(); p++) {
    const TtcPair &pr = pl.pairs[p];
    if (pr.glyf + 1 >= num || pl.unit[pr.glyf] != p || pl.unit[pr.glyf + 1] != p) fail("a pair's entries");
    if (pl.tr_glyf && (pr.num_glyphs == 0 || ((uint64_t)pr.num_glyphs + 1) * (pr.long_loca ? 4 : 2) > pl.t[pr.glyf + 1].src_len))
      fail("short loca accepted");
  }
  for (size_t u = 0; u < pl.hunits.size(); u++) {
    const TtcHmtx &h = pl.hunits[u];
    if (!pl.tr_glyf || !(transforms & kTransformHmtx)) fail("an hmtx unit without the transforms");
    if (h.hmtx >= num || pl.t[h.hmtx].tag != kHmtxTag || pl.unit[h.hmtx] != u || h.pair >= pl.pairs.size()) fail("an hmtx unit");
    const uint32_t ng = pl.pairs[h.pair].num_glyphs;
    if (h.nhm < 1 || h.nhm > ng || pl.t[h.hmtx].src_len != 4ull * h.nhm + 2ull * (ng - h.nhm)) fail("an hmtx unit's shape");
    if (u && pl.hunits[u - 1].hmtx >= h.hmtx) fail("hmtx units out of order");
    // every member that lists it lists the unit's pair and one hhea entry
    uint32_t hhea = kNoTable;
    for (const TtcMember &m : pl.fonts) {
      if (m.hmtx == kNoTable || pl.rec[m.hmtx].entry != h.hmtx) continue;
      if (m.pair != h.pair || m.hhea == kNoTable) fail("an hmtx unit's member");
      if (hhea == kNoTable) hhea = pl.rec[m.hhea].entry;
      if (hhea != pl.rec[m.hhea].entry || pl.t[hhea].src_len < 36) fail("an hmtx unit's hhea");
    }
  }
}
// Once laid out: the pieces of the stream back to back from 0 (so apart), ending at stream_len.
static void check_stream(const TtcPlan &pl) {
  uint64_t at = 0;
  for (const Table &t : pl.t) {
    if (t.at != at) fail("stream pieces are not back to back");
    at += t.len;
    if (at > pl.stream_len) fail("a stream piece leaves stream_len");
    if (t.state == kPlain && t.len != t.src_len) fail("a plain table's length changed");
    if (t.state == kTrLoca && t.len != 0) fail("a transformed loca with bytes");
  }
  if (at != pl.stream_len || at > mib::woff2inv::kMaxInput) fail("stream_len");
}

typedef std::map<uint32_t, Bytes> ByEntry;
static ByEntry read_list(const Bytes &b) {
  ByEntry out;
  size_t at = 0;
  while (at + 8 <= b.size()) {
    const uint32_t i = le32(&b[at]), n = le32(&b[at + 4]);
    if (at + 8 + n > b.size()) fail("a table list's record");
    out[i] = Bytes(b.begin() + at + 8, b.begin() + at + 8 + n);
    at += 8 + n;
  }
  if (at != b.size()) fail("a table list's size");
  return out;
}

static int pack_mode(const char *in, const char *out) {
  const std::vector<Bytes> r = read_records(in);
  if (r.size() % 6) fail("pack wants groups of six records");
  FILE *f = fopen(out, "wb");
  if (!f) return 2;
  size_t done = 0;
  for (size_t i = 0; i < r.size(); i += 6) {
    const Bytes &ttc = r[i], &differ = r[i + 2];
    if (r[i + 1].size() != 1 || r[i + 5].size() != 4) fail("pack record sizes");
    const uint32_t transforms = r[i + 1][0], comp = le32(r[i + 5].data());
    ByEntry tglyf = read_list(r[i + 3]), thmtx = read_list(r[i + 4]);
    TtcPlan pl;
    // (an exact-size copy: a read past the end is a report)
    uint8_t *copy = (uint8_t *)malloc(ttc.size() ? ttc.size() : 1);
    if (ttc.size()) memcpy(copy, ttc.data(), ttc.size());
    int rc = ttc_read(ttc.size() ? copy : nullptr, ttc.size(), transforms, &pl);
    Bytes stream, back;
    uint8_t hdr[mib::woff2file::kHeaderBytes] = {0};
    if (rc == kOk) {
      if (differ.size() != pl.cand.size()) fail("one answer per candidate");
      for (const TtcCandidate &c : pl.cand)
        if (pl.rec[c.rec].len != pl.rec[c.rep].len || pl.rec[c.rec].tag != pl.rec[c.rep].tag || c.rep >= c.rec)
          fail("a candidate's representative");
      // (the answer with every candidate equal comes first, as in the product: item 19's lower bound)
      rc = ttc_entries(&pl, copy, ttc.size(), transforms, nullptr);
      if (rc == kOk) rc = ttc_entries(&pl, copy, ttc.size(), transforms, differ.data());
    }
    if (rc == kOk) {
      check_entries(pl, ttc.size(), transforms);
      std::vector<uint64_t> glen(pl.pairs.size(), 0), hlen(pl.hunits.size(), 0);
      std::vector<const uint8_t *> gp(pl.pairs.size(), nullptr), hp(pl.hunits.size(), nullptr);
      for (size_t p = 0; p < pl.pairs.size() && pl.tr_glyf; p++) {
        if (!tglyf.count(pl.pairs[p].glyf)) fail("no transformed glyf for a pair");
        glen[p] = tglyf[pl.pairs[p].glyf].size();
        gp[p] = tglyf[pl.pairs[p].glyf].data();
      }
      for (size_t u = 0; u < pl.hunits.size(); u++)
        if (thmtx.count(pl.hunits[u].hmtx)) hlen[u] = thmtx[pl.hunits[u].hmtx].size(), hp[u] = thmtx[pl.hunits[u].hmtx].data();
      for (const auto &kv : thmtx)
        if (kv.first >= pl.t.size() || pl.unit[kv.first] == kNoTable || pl.t[kv.first].tag != kHmtxTag)
          fail("a transformed hmtx for an entry that is no unit");
      if (!ttc_layout(&pl, glen.data(), hlen.data()) || !ttc_finish(pl, copy, comp, hdr)) rc = -1;
      else {
        check_stream(pl);
        ttc_host_pack(pl, copy, gp.data(), hp.data(), &stream);
        // the decoder's view of what was written
        Bytes file(hdr, hdr + sizeof(hdr));
        file.insert(file.end(), pl.dir.begin(), pl.dir.end());
        file.resize((size_t)ttc_file_bytes(pl, comp), 0);
        if (mib::woff2file::host_assemble(file.data(), file.size(), stream.data(), stream.size(), &back) != 0)
          fail("the decoder's plan rejects the written container");
      }
    }
    free(copy);
    const uint8_t c[4] = {(uint8_t)rc, (uint8_t)(rc >> 8), (uint8_t)(rc >> 16), (uint8_t)(rc >> 24)};
    write_record(f, c, 4);
    write_record(f, pl.dir.data(), rc == kOk ? pl.dir.size() : 0);
    write_record(f, hdr, rc == kOk ? sizeof(hdr) : 0);
    write_record(f, stream.data(), stream.size());
    write_record(f, back.data(), back.size());
    done++;
  }
  fclose(f);
  printf("packed %zu\n", done);
  return 0;
}

static size_t g_damaged = 0, g_accepted = 0;
static size_t g_why[21] = {0};

static void try_ttc(const uint8_t *p, size_t n) {
  uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(copy, p, n);
  g_damaged++;
  for (uint32_t transforms = 0; transforms < 4; transforms += 3) {
    TtcPlan pl;
    int rc = ttc_read(copy, n, transforms, &pl);
    if (rc == kOk) rc = ttc_entries(&pl, copy, n, transforms, nullptr);
    if (rc < 0 || rc > 20) fail("the plan's answer");
    if (rc == kOk) {
      check_entries(pl, n, transforms);
      Bytes differ(pl.cand.size());
      for (size_t c = 0; c < pl.cand.size(); c++) {
        const TtcRecord &a = pl.rec[pl.cand[c].rec], &b = pl.rec[pl.cand[c].rep];
        if (a.len != b.len || (uint64_t)a.off + a.len > n || (uint64_t)b.off + b.len > n) fail("a candidate's ranges");
        differ[c] = a.len && memcmp(copy + a.off, copy + b.off, a.len) != 0;
      }
      rc = ttc_entries(&pl, copy, n, transforms, differ.data());
    }
    if (transforms == 3) g_why[rc]++;
    if (rc != kOk) continue;
    if (transforms == 3) g_accepted++;
    check_entries(pl, n, transforms);
    // transformed tables of made-up sizes: what matters is where the pieces go
    std::vector<Bytes> tg, th;
    std::vector<uint64_t> glen, hlen;
    std::vector<const uint8_t *> gp, hp;
    for (size_t q = 0; q < pl.pairs.size(); q++) tg.push_back(Bytes(pl.tr_glyf ? 36 + 5 * (size_t)pl.pairs[q].num_glyphs : 0, 0x5A));
    for (size_t u = 0; u < pl.hunits.size(); u++) th.push_back(Bytes(1 + 2 * (size_t)pl.hunits[u].nhm, 0xA5));
    for (const Bytes &b : tg) glen.push_back(b.size()), gp.push_back(b.data());
    for (int with_hmtx = 0; with_hmtx < 2; with_hmtx++) {
      hlen.clear();
      hp.clear();
      for (size_t u = 0; u < th.size(); u++) hlen.push_back(with_hmtx && u % 2 == 0 ? th[u].size() : 0), hp.push_back(th[u].data());
      if (!ttc_layout(&pl, glen.data(), hlen.data())) continue;
      check_stream(pl);
      Bytes stream;
      ttc_host_pack(pl, copy, gp.data(), hp.data(), &stream);
      if (stream.size() != pl.stream_len) fail("ttc_host_pack's size");
      uint8_t hdr[mib::woff2file::kHeaderBytes];
      if (!ttc_finish(pl, copy, stream.size(), hdr)) fail("ttc_finish");
      // directory and CollectionHeader read back as what was planned, and the decoder's parse takes them
      Bytes file(hdr, hdr + sizeof(hdr));
      file.insert(file.end(), pl.dir.begin(), pl.dir.end());
      file.resize((size_t)ttc_file_bytes(pl, stream.size()), 0);
      mib::woff2file::Plan rp;
      if (!mib::woff2file::parse(file.data(), file.size(), &rp)) fail("the decoder's parse rejects the container");
      if (rp.t.size() != pl.t.size() || rp.stream_len != pl.stream_len || rp.fonts.size() != pl.fonts.size()) fail("the container read back");
      for (size_t i = 0; i < pl.t.size(); i++)
        if (rp.t[i].tag != pl.t[i].tag || rp.t[i].src_off != pl.t[i].at || rp.t[i].src_len != pl.t[i].len) fail("an entry read back");
    }
  }
  free(copy);
}

static int fuzz_mode(const char *in) {
  static const uint32_t kValues[] = {0, 1, 2, 3, 4, 11, 12, 13, 16, 17, 18, 35, 36, 53, 54, 255, 256, 0x7FFF, 0x8000, 0xFFFF,
                                     0x10000, 0xFFFFFF, 0x10000000, 0x10000001, 0x7FFFFFFF, 0x80000000u, 0xFFFFFFFCu, 0xFFFFFFFFu};
  for (const Bytes &ttc : read_records(in)) {
    TtcPlan pl;
    if (ttc_read(ttc.data(), ttc.size(), 3, &pl) != kOk) fail("the undamaged collection is rejected");
    // the directories stand behind the header, back to back (tests/_woff2_collection_write.build_ttc,
    // and the TTCs that the decoder assembles)
    const size_t nf = pl.num_fonts, hdr_end = 12 + 4 * nf + (pl.version == mib::woff2file::kTtcVersion2 ? 12 : 0);
    size_t dir_end = hdr_end;
    std::vector<size_t> recs;   // where the records are
    for (size_t f = 0; f < nf; f++) {
      const size_t at = ((size_t)ttc[12 + 4 * f] << 24) | (ttc[13 + 4 * f] << 16) | (ttc[14 + 4 * f] << 8) | ttc[15 + 4 * f];
      const size_t nt = (ttc[at + 4] << 8) | ttc[at + 5];
      for (size_t q = 0; q < nt; q++) recs.push_back(at + 12 + 16 * q);
      dir_end = std::max(dir_end, at + 12 + 16 * nt);
    }
    const size_t accepted_before = g_accepted;
    try_ttc(ttc.data(), ttc.size());
    if (g_accepted != accepted_before + 1) fail("the undamaged collection is rejected");
    for (size_t n = 0; n <= dir_end + 64 && n < ttc.size(); n++) try_ttc(ttc.data(), n);
    Bytes b = ttc;
    for (size_t at = 0; at < dir_end; at++)
      for (int bit = 0; bit < 8; bit++) {
        b[at] ^= (uint8_t)(1 << bit);
        try_ttc(b.data(), b.size());
        b[at] = ttc[at];
      }
    std::vector<size_t> fields;
    for (size_t f = 0; f < nf; f++) fields.push_back(12 + 4 * f);   // the members' offsets
    for (size_t rec : recs) fields.push_back(rec + 8), fields.push_back(rec + 12);
    for (size_t field : fields)
      for (uint32_t v : kValues) {
        for (int s = 0; s < 4; s++) b[field + s] = (uint8_t)(v >> (24 - 8 * s));
        try_ttc(b.data(), b.size());
        // ... and the same value as a distance from the end of the input
        const uint32_t w = (uint32_t)ttc.size() - v;
        for (int s = 0; s < 4; s++) b[field + s] = (uint8_t)(w >> (24 - 8 * s));
        try_ttc(b.data(), b.size());
        memcpy(&b[field], &ttc[field], 4);
      }
  }
  printf("damaged %zu accepted %zu rejected %zu why", g_damaged, g_accepted, g_damaged - g_accepted);
  for (int q = 1; q <= 20; q++) printf(" %zu", g_why[q]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "pack")) return pack_mode(argv[2], argv[3]);
  if (argc == 3 && !strcmp(argv[1], "fuzz")) return fuzz_mode(argv[2]);
  fprintf(stderr, "usage: woff2_write_ttc_host pack IN OUT | fuzz IN\n");
  return 2;
}
