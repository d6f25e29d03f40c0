// Stand-alone host build of the WOFF2 collection plan (brotli-lib_amd/csrc/woff2_file.h and
// woff2_batch.h: flavor ttcf -> a TTC), meant to be built with -fsanitize=address,undefined
// (tests/test_woff2_collection_host.py).
//
//   woff2_collection_host assemble IN OUT  IN: pairs of records (file, decompressed stream); OUT
//                                          gets a pair per input: host_assemble's return code (4
//                                          bytes, little-endian, two's complement) and the TTC
//                                          (or the sfnt, of a single font)
//   woff2_collection_host batch IN         IN as above, single fonts and collections, all good.
//                                          The files in several orders (as given, reversed, every
//                                          rotation, doubled) through add_font and host_run, as the
//                                          device path runs them: every file's bytes equal
//                                          host_assemble's
//   woff2_collection_host fuzz IN SEED N   IN as above, collections.  Damaged copies of each file
//                                          with the file's own stream: every truncation, every bit
//                                          of the CollectionHeader, every 255UInt16 of it set to
//                                          each boundary value and written in its other forms, N
//                                          random double edits.  Each is rejected, or its plan and
//                                          its TTC keep the invariants below
//   woff2_collection_host layout           item 21 of the rejection list on hand-made plans
// A record is a u32 little-endian length + bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "woff2_batch.h"

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

static uint32_t be32(const Bytes &b, size_t at) {
  return ((uint32_t)b[at] << 24) | ((uint32_t)b[at + 1] << 16) | ((uint32_t)b[at + 2] << 8) | b[at + 3];
}
static void set32(Bytes &b, size_t at, uint32_t v) {
  b[at] = (uint8_t)(v >> 24), b[at + 1] = (uint8_t)(v >> 16), b[at + 2] = (uint8_t)(v >> 8), b[at + 3] = (uint8_t)v;
}

// a heap block of exactly n bytes: a read past it is a sanitizer report
static uint8_t *exact(const uint8_t *p, size_t n) {
  uint8_t *q = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(q, p, n);
  return q;
}

// What an accepted collection must keep whatever the file says.  The plan: sources back to
// back inside the stream it announces; the TTC header, the members' directories and the written
// tables' padded ranges in ascending order, apart, at 4-byte boundaries, inside the announced
// size; every member's records strictly sorted by tag and pointing at written tables; one
// member at most storing a head's adjustment.  The TTC: what its own header and directories say
// is what the plan says.
static void check_collection(const Plan &pl, const Bytes &ttc) {
  const size_t num = pl.t.size();
  uint64_t at = 0;
  for (const Table &t : pl.t) {
    if (t.src_off != at) fail("source offsets are not back to back");
    at += t.src_len;
  }
  if (at != pl.stream_len || at > mib::woff2inv::kMaxInput) fail("sources leave the stream");
  if (pl.ttc_version != kTtcVersion1 && pl.ttc_version != kTtcVersion2) fail("version");
  if (pl.fonts.empty() || pl.written.size() != num || pl.unit.size() != num) fail("plan sizes");
  if (pl.sfnt_len != ttc.size()) fail("announced size is not the output's");
  at = ttc_header_bytes(pl);
  if (at != 12 + 4 * pl.fonts.size() + (pl.ttc_version == kTtcVersion2 ? 12 : 0)) fail("header size");
  if (be32(ttc, 0) != kFlavorTtc || be32(ttc, 4) != pl.ttc_version || be32(ttc, 8) != pl.fonts.size()) fail("TTC header");
  std::vector<uint32_t> adjusters(num, 0);
  std::vector<char> listed(num, 0);
  uint64_t dirs = 0;
  for (size_t f = 0; f < pl.fonts.size(); f++) {
    const Member &m = pl.fonts[f];
    if (m.dir_off != at || (m.dir_off & 3)) fail("a directory is not behind the one before it");
    if (m.order.empty()) fail("a member without tables");
    at += 12 + 16 * (uint64_t)m.order.size();
    dirs += 12 + 16 * (uint64_t)m.order.size();
    if (at > pl.sfnt_len) fail("a directory leaves the announced size");
    if (be32(ttc, 12 + 4 * f) != m.dir_off) fail("the header's offset is not the directory's");
    if (be32(ttc, m.dir_off) != m.flavor || (be32(ttc, m.dir_off + 4) >> 16) != m.order.size()) fail("an offset table");
    uint32_t heads = 0;
    for (size_t r = 0; r < m.order.size(); r++) {
      const uint32_t i = m.order[r];
      if (i >= num || !pl.written[i]) fail("a record points at no written table");
      if (r && pl.t[m.order[r - 1]].tag >= pl.t[i].tag) fail("records not strictly sorted by tag");
      listed[i] = 1;
      const size_t rec = m.dir_off + 12 + 16 * r;
      if (be32(ttc, rec) != pl.t[i].tag || be32(ttc, rec + 8) != pl.t[i].dst_off || be32(ttc, rec + 12) != pl.t[i].dst_len)
        fail("a record is not its table's");
      if (pl.t[i].tag == kHeadTag) {
        heads++;
        if (m.head != i) fail("a member's head");
        adjusters[i] += m.adjusts;
      }
    }
    if ((heads == 0) != (m.head == kNoTable) || (m.head == kNoTable && m.adjusts)) fail("a member's head");
  }
  if (dirs > kMaxDirectoryBytes) fail("directories above their bound");
  if (pl.ttc_version == kTtcVersion2)
    for (size_t b = 12 + 4 * pl.fonts.size(); b < ttc_header_bytes(pl); b++)
      if (ttc[b]) fail("the DSIG fields are not zero");
  for (size_t i = 0; i < num; i++) {
    const Table &t = pl.t[i];
    if ((bool)pl.written[i] != (bool)listed[i]) fail("written is not listed");
    if (!pl.written[i]) continue;
    if (t.dst_off != at || (t.dst_off & 3)) fail("a table is not at the next 4-byte boundary");
    at = ((uint64_t)t.dst_off + t.dst_len + 3) & ~3ull;
    if (at > pl.sfnt_len) fail("a table leaves the announced size");
    if (t.tag == kHeadTag && adjusters[i] != 1) fail("not exactly one member stores a head's adjustment");
    if (t.kind != kCopy && pl.unit[i] >= (t.kind == kHmtx ? pl.hunits.size() : pl.pairs.size())) fail("a table's unit");
  }
  if (at != pl.sfnt_len) fail("the announced size is not the last table's end");
  for (const Pair &p : pl.pairs)
    if (p.loca != p.glyf + 1 || p.loca >= num || pl.t[p.glyf].kind != kGlyf || pl.t[p.loca].kind != kLoca) fail("a pair");
  for (const HmtxUnit &u : pl.hunits)
    if (u.hmtx >= num || u.hhea >= num || u.pair >= pl.pairs.size() || pl.t[u.hmtx].kind != kHmtx || pl.t[u.hhea].src_len < 36)
      fail("an hmtx unit");
}

// File and stream in heap blocks of exactly their sizes.
static int run(const Bytes &file, const Bytes &stream, Bytes *out, Plan *laid_out = nullptr) {
  uint8_t *f = exact(file.data(), file.size()), *s = exact(stream.data(), stream.size());
  Plan laid;
  const int rc = host_assemble(file.empty() ? nullptr : f, file.size(), stream.empty() ? nullptr : s, stream.size(), out, &laid);
  if (rc == 0) {
    if (laid.ttc_version) check_collection(laid, *out);
    else if (laid.sfnt_len != out->size()) fail("announced size is not the output's");
    if (laid_out) *laid_out = laid;
  } else if (!out->empty()) {
    fail("a rejected file left output");
  }
  free(f);
  free(s);
  return rc;
}

// ------------------------------------------------------------------ batch
static const uint8_t kFill = 0xA5;

struct Staged {   // a file's reconstructed tables as the per-file worker left them, a block each
  std::vector<uint8_t *> glyfs, locas, hmtxs;
};

static void batch_order(const std::vector<Bytes> &rec, const std::vector<Plan> &laid, const std::vector<Bytes> &solo,
                        const std::vector<size_t> &order) {
  Launch launch;
  std::vector<Staged> staged(order.size());
  std::vector<uint8_t *> streams(order.size());
  std::vector<uint64_t> base(order.size());
  for (size_t q = 0; q < order.size(); q++) {
    const size_t i = order[q];
    const Plan &pl = laid[i];
    const Bytes &stream = rec[2 * i + 1], &out = solo[i];
    streams[q] = exact(stream.data(), stream.size());
    Staged &s = staged[q];
    for (const Pair &p : pl.pairs) {
      s.glyfs.push_back(exact(out.data() + pl.t[p.glyf].dst_off, pl.t[p.glyf].dst_len));
      s.locas.push_back(exact(out.data() + pl.t[p.loca].dst_off, pl.t[p.loca].dst_len));
    }
    for (const HmtxUnit &u : pl.hunits) s.hmtxs.push_back(exact(out.data() + pl.t[u.hmtx].dst_off, pl.t[u.hmtx].dst_len));
    const size_t descs0 = launch.descs.size(), fonts0 = launch.fonts.size();
    const FontSrc src{streams[q], s.glyfs.empty() ? nullptr : s.glyfs[0], s.locas.empty() ? nullptr : s.locas[0],
                      s.hmtxs.empty() ? nullptr : s.hmtxs[0], s.glyfs.data(), s.locas.data(), s.hmtxs.data()};
    if (!add_font(&launch, pl, src)) fail("add_font refused a file");
    base[q] = launch.fonts.back().out_base;
    if (base[q] % kFontAlign || launch.out_bytes != base[q] + pl.sfnt_len) fail("a file's place in the output");
    size_t written = 0;
    for (size_t t = 0; t < pl.t.size(); t++) written += is_written(pl, t);
    if (launch.descs.size() - descs0 != written) fail("descriptor count");
    if (launch.fonts.size() - fonts0 != (pl.ttc_version ? pl.fonts.size() : 1)) fail("font count");
    for (size_t d = descs0; d < launch.descs.size(); d++) {
      const AsmDesc &a = launch.descs[d];
      const uint64_t padded = ((uint64_t)a.len + 3) & ~3ull;
      if (a.out_base != base[q] || a.sum != d || (a.dst_off & 3) || a.dst_off + padded > pl.sfnt_len) fail("a descriptor");
      if (a.zero_at != kNoZero && (a.zero_at != 8 || a.len < 12)) fail("zero_at");
    }
    for (size_t f = fonts0; f < launch.fonts.size(); f++) {
      const DirFont &df = launch.fonts[f];
      if (df.out_base != base[q] || df.first_sum != descs0 || (df.dir_off & 3)) fail("a font's base, sums or directory");
      if ((uint64_t)df.dir_off + 12 + 16 * (uint64_t)df.num > pl.sfnt_len) fail("a directory leaves its file");
      if ((uint64_t)df.first_rec + df.num > launch.recs.size()) fail("a font's records");
      for (uint32_t r = 0; r < df.num; r++)
        if (launch.recs[df.first_rec + r].table >= written) fail("a record's table leaves its file");
      if (df.adjust_at != kNoZero && (uint64_t)df.adjust_at + 4 > pl.sfnt_len) fail("adjust_at leaves its file");
      if (pl.ttc_version ? (df.ttc_index != f - fonts0 || df.ttc_fonts != pl.fonts.size() || df.ttc_version != pl.ttc_version)
                         : (df.ttc_index != kNoZero || df.dir_off != 0))
        fail("a font's collection fields");
    }
  }
  uint8_t *out = (uint8_t *)malloc(launch.out_bytes ? launch.out_bytes : 1);
  memset(out, kFill, launch.out_bytes);
  host_run(launch, out);
  uint64_t at = 0;
  for (size_t q = 0; q < order.size(); q++) {
    const Bytes &want = solo[order[q]];
    for (uint64_t b = at; b < base[q]; b++)
      if (out[b] != kFill) fail("a byte between two files was written");
    if (memcmp(out + base[q], want.data(), want.size()) != 0) fail("the batch's file is not the per-file worker's");
    at = base[q] + want.size();
    for (uint8_t *p : staged[q].glyfs) free(p);
    for (uint8_t *p : staged[q].locas) free(p);
    for (uint8_t *p : staged[q].hmtxs) free(p);
    free(streams[q]);
  }
  if (at != launch.out_bytes) fail("the output buffer is not the last file's end");
  free(out);
}

// ------------------------------------------------------------------ fuzz
static uint64_t g_rng;
static uint32_t rnd() {   // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 2685821657736338717ull) >> 32);
}

static Bytes u255_short(uint32_t v) {
  if (v < 253) return Bytes{(uint8_t)v};
  if (v < 506) return Bytes{255, (uint8_t)(v - 253)};
  if (v < 762) return Bytes{254, (uint8_t)(v - 506)};
  return Bytes{253, (uint8_t)(v >> 8), (uint8_t)v};
}

struct Field {   // a 255UInt16 of the CollectionHeader
  size_t at, len;
  uint32_t value;
  bool index;
};

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "layout") {
    // item 21: offsets that do not fit 32 bits, however the lengths come about
    Plan pl;
    pl.flavor = kFlavorTtc;
    pl.ttc_version = kTtcVersion1;
    pl.t = {Table{kGlyfTag, kGlyf, 0, 36, 0, 0}, Table{kLocaTag, kLoca, 36, 0, 0, 0}, Table{tag4('n', 'a', 'm', 'e'), kCopy, 36, 8, 0, 0}};
    pl.stream_len = 44;
    pl.fonts = {Member{0x00010000, {0, 1, 2}, kNoTable, false, 0}, Member{0x00010000, {0, 1}, kNoTable, false, 0}};
    if (!collection_members(&pl) || !collection_units(&pl) || pl.pairs.size() != 1) fail("the hand-made plan");
    const uint64_t none = 0;
    uint64_t glyf = 0xFFFFFE00ull, loca = 16;
    if (!layout_units(&pl, &glyf, &loca, &none) || pl.sfnt_len != 12 + 8 + 60 + 44 + 0xFFFFFE00ull + 16 + 8) fail("a TTC just inside 32 bits");
    loca = 0x200;
    if (layout_units(&pl, &glyf, &loca, &none)) fail("a TTC past 32 bits was laid out");
    glyf = 0x100000000ull;
    if (layout_units(&pl, &glyf, &loca, &none)) fail("a table past 32 bits was laid out");
    printf("layout ok\n");
    return 0;
  }
  if (argc < 3) return 2;
  const std::vector<Bytes> rec = read_records(argv[2]);
  if (rec.size() % 2) return 2;
  if (mode == "assemble") {
    if (argc < 4) return 2;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    for (size_t i = 0; i < rec.size(); i += 2) {
      Bytes ttc;
      const uint32_t u = (uint32_t)run(rec[i], rec[i + 1], &ttc);
      const uint8_t c[4] = {(uint8_t)u, (uint8_t)(u >> 8), (uint8_t)(u >> 16), (uint8_t)(u >> 24)};
      write_record(out, c, 4);
      write_record(out, ttc.data(), ttc.size());
    }
    fclose(out);
    printf("assembled %zu\n", rec.size() / 2);
    return 0;
  }
  if (mode == "batch") {
    const size_t k = rec.size() / 2;
    std::vector<Plan> laid(k);
    std::vector<Bytes> solo(k);
    size_t collections = 0;
    for (size_t i = 0; i < k; i++) {
      if (run(rec[2 * i], rec[2 * i + 1], &solo[i], &laid[i]) != 0) fail("a file of the batch is rejected");
      collections += laid[i].ttc_version != 0;
    }
    if (collections == 0 || collections == k) fail("the batch does not mix single fonts and collections");
    std::vector<std::vector<size_t>> orders;
    std::vector<size_t> o(k);
    for (size_t i = 0; i < k; i++) o[i] = i;
    for (size_t r = 0; r < k; r++) {   // every rotation
      std::vector<size_t> p(k);
      for (size_t i = 0; i < k; i++) p[i] = o[(i + r) % k];
      orders.push_back(p);
    }
    orders.push_back(std::vector<size_t>(o.rbegin(), o.rend()));
    std::vector<size_t> twice = o;
    twice.insert(twice.end(), o.rbegin(), o.rend());   // (the same file in two slots)
    orders.push_back(twice);
    for (size_t i = 0; i < k; i++) orders.push_back(std::vector<size_t>{i});
    for (const std::vector<size_t> &p : orders) batch_order(rec, laid, solo, p);
    printf("batch files %zu collections %zu orders %zu\n", k, collections, orders.size());
    return 0;
  }
  if (mode != "fuzz" || argc < 5) return 2;
  g_rng = strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
  const size_t doubles = strtoull(argv[4], nullptr, 10);
  size_t total = 0, accepted = 0, same = 0;
  for (size_t i = 0; i < rec.size(); i += 2) {
    const Bytes &file = rec[i], &stream = rec[i + 1];
    Bytes good;
    Plan pl;
    if (run(file, stream, &good, &pl) != 0 || !pl.ttc_version) return 1;   // the undamaged file: a collection
    auto one = [&](const Bytes &f, bool same_result = false) {
      Bytes ttc;
      total++;
      const int rc = run(f, stream, &ttc);
      if (rc == 0) accepted++;
      if (same_result) {
        if (rc != 0 || ttc != good) fail("another encoding of the same value gave another result");
        same++;
      }
    };
    // the CollectionHeader: behind the directory, in front of the stream.  The directory's end
    // and the header's 255UInt16 fields by the rules of sections 4.1 and 4.2 (the undamaged file
    // parsed)
    const size_t ch_end = pl.comp_off;
    size_t ch0 = kHeaderBytes;
    for (const Table &t : pl.t) {
      ch0 += (file[ch0] & 63) == 63 ? 5 : 1;
      for (int k = t.kind == kCopy ? 1 : 2; k > 0; k--)
        while (file[ch0++] & 0x80) {
        }
    }
    std::vector<Field> fields;
    {
      size_t p = ch0 + 4;
      auto take = [&](bool index) {
        const uint32_t b = file[p];
        const size_t len = b < 253 ? 1 : b == 253 ? 3 : 2;
        const uint32_t v = b < 253 ? b : b == 253 ? ((uint32_t)file[p + 1] << 8) | file[p + 2] : (b == 254 ? 506u : 253u) + file[p + 1];
        fields.push_back(Field{p, len, v, index});
        p += len;
        return v;
      };
      if (be32(file, ch0) != pl.ttc_version || take(false) != pl.fonts.size()) fail("the fuzzer lost the CollectionHeader");
      for (const Member &m : pl.fonts) {
        if (take(false) != m.order.size() || be32(file, p) != m.flavor) fail("the fuzzer lost a font");
        p += 4;
        for (size_t t = 0; t < m.order.size(); t++) take(true);
      }
      if (p != ch_end) fail("the fuzzer lost the CollectionHeader's end");
    }
    const uint32_t num = (uint32_t)pl.t.size();
    // truncations: every length, with the header's length field as it was and made to agree
    for (size_t len = 0; len < file.size(); len++) {
      Bytes u(file.begin(), file.begin() + len);
      one(u);
      if (len >= 12) {
        set32(u, 8, (uint32_t)len);
        one(u);
      }
    }
    // every bit of the CollectionHeader, and of numTables and totalCompressedSize in front of it
    std::vector<size_t> live;
    for (size_t p = 12; p < 14; p++) live.push_back(p);
    for (size_t p = 20; p < 24; p++) live.push_back(p);
    for (size_t p = ch0; p < ch_end; p++) live.push_back(p);
    for (size_t p : live)
      for (int b = 0; b < 8; b++) {
        Bytes u = file;
        u[p] ^= (uint8_t)(1u << b);
        one(u);
      }
    // every field rewritten (the file grows or shrinks with the encoding, the header's length
    // follows): to each boundary value; in its other forms, which give the same TTC; as a lone
    // first byte of a longer form, which swallows what follows
    auto splice = [&](const Field &fd, const Bytes &enc) {
      Bytes u(file.begin(), file.begin() + fd.at);
      u.insert(u.end(), enc.begin(), enc.end());
      u.insert(u.end(), file.begin() + fd.at + fd.len, file.end());
      set32(u, 8, (uint32_t)u.size());
      return u;
    };
    const uint32_t bounds[] = {0, 1, num - 1, num, num + 1, 252, 253, 254, 255, 256, 505, 506, 507, 761, 762, 763, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF};
    for (const Field &fd : fields) {
      for (uint32_t v : bounds) {
        if (v == fd.value || (!fd.index && v > 64)) continue;   // (a count of thousands only runs past the file)
        one(splice(fd, u255_short(v)));
      }
      if (!fd.index) one(splice(fd, u255_short(0xFFFF)));
      const uint32_t v = fd.value;
      if (fd.len != 3) one(splice(fd, Bytes{253, (uint8_t)(v >> 8), (uint8_t)v}), true);
      if (v >= 253 && v < 253 + 256 && file[fd.at] != 255) one(splice(fd, Bytes{255, (uint8_t)(v - 253)}), true);
      if (v >= 506 && v < 506 + 256 && file[fd.at] != 254) one(splice(fd, Bytes{254, (uint8_t)(v - 506)}), true);
      for (uint8_t lead : {253, 254, 255}) one(splice(fd, Bytes{lead}));
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
  printf("damaged %zu accepted %zu rejected %zu same %zu\n", total, accepted, total - accepted, same);
  return 0;
}
