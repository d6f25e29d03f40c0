// The WOFF2 container, write direction, of an OpenType collection (TTC): the plan of the .woff2 file
// of flavor ttcf (W3C WOFF2 section 4.2; DESIGN.md 4c "Writing a collection").  Plain C++ beside
// woff2_write.h, whose Table states, put_base128 and put_entry it shares: woff2_write.hip runs the
// plan on the device, ttc_host_pack below states the stream serially (the CPU tests' path under
// sanitizers, tests/woff2_write_ttc_host_main.cpp).  The TTC is untrusted: every byte of it is read
// through woff2file::Reader.
//
// The plan is made in steps, because which tables are one depends on their bytes:
//   ttc_read     header, offset tables and records -> the members' kept records (DSIG dropped;
//                ascending tag, loca directly behind glyf) and the candidates: records that may be
//                one table by content.  Records of one tag, offset and length are one table here.
//                The others are grouped by (tag, length, the record's checkSum field -- a hint, never
//                trusted); a group's first record is its representative, every other record of
//                another offset a candidate (record, representative) whose bytes are compared
//                exactly (on the device: w2enc_same_kernel).  A candidate that differs keeps a table
//                of its own and is not compared with further candidates.
//   ttc_entries  the answers (differ[c] per candidate) -> the directory: walking the members in the
//                collection's order and each member's records in theirs, an entry is appended the
//                first time a member lists its table.  glyf and loca are shared as a pair, keyed by
//                (glyf table, loca table, and where glyf is transformed the member's numGlyphs and
//                indexToLocFormat): the pair's loca entry follows its glyf entry.  A member's index
//                list is ascending.
//   ttc_layout   the transformed sizes per pair and per hmtx unit -> the places in the stream, the
//                directory and the CollectionHeader.
//   ttc_finish   the 48-byte header.
// Transforms: every pair where MIB_WOFF2_GLYF is set; an hmtx entry where MIB_WOFF2_HMTX is set,
// every member that lists it lists the same transformed pair and the same hhea entry, the
// single-font conditions hold (hhea of 36 bytes, 1 <= numberOfHMetrics <= numGlyphs, the exact
// length) and a side-bearing array equals the glyphs' xMin (thmtx_len != 0); otherwise it is stored
// as it is.  Every head entry of at least 18 bytes goes into the stream with bytes 8..11 zero, and
// with flags bit 11 set when a member that lists it has a transformed pair.
// Fixed bytes: header wOF2, ttcf, length, numTables = the directory's entries, totalSfntSize = 12 +
// 4 numFonts (+ 12 for version 2.0) + per member 12 + 16 its kept tables + per entry origLength
// padded to 4, totalCompressedSize, the version from bytes 4..7 of the head of the first member
// that lists a head of at least 8 bytes (else 0), the rest 0; the file zero-padded to 4 bytes.
// CollectionHeader: the input's version, numFonts, per member numTables, its flavor (the first four
// bytes of its offset table) and its indices, every 255UInt16 in its shortest form.
//
// Rejected (MIB_E_INVALID_ARG), continuing woff2_write.h's list, before any device work:
//   10 the header, an offset table or a directory runs past the input (a version 2.0 header's three
//      DSIG words included; they are otherwise ignored)
//   11 a version other than 0x00010000 or 0x00020000
//   12 numFonts 0 or above 65,535, or a member's numTables 0
//   13 a record whose offset + length runs past the input
//   14 a tag twice in one member
//   15 the members' directories (12 + 16 numTables each) above 16 MiB in sum
//   16 the lengths, summed once per distinct (offset, length), above 256 MiB
//   17 a member with exactly one of glyf and loca
//   18 a member with nothing left after dropping DSIG
//   19 more than 65,535 directory entries (decided with every candidate taken as equal where the
//      compare has not run yet: the fewest entries the collection can have)
//   20 where glyf is to be transformed, a member that fails what the single-font plan asks (9)
// Checksums, search fields, alignment and overlap are not checked, as in the single-font plan.
#ifndef MIB_WOFF2_WRITE_TTC_H_
#define MIB_WOFF2_WRITE_TTC_H_
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "woff2_write.h"

namespace mib {
namespace woff2write {

enum TtcReject : int {
  kTtcPast = 10, kTtcVersion = 11, kTtcCount = 12, kTtcRecord = 13, kTtcTwice = 14, kTtcDirs = 15, kTtcSum = 16,
  kTtcGlyfLoca = 17, kTtcEmpty = 18, kTtcEntries = 19, kTtcGlyfNeeds = 20
};

struct TtcRecord {   // a kept record of a member
  uint32_t tag, check, off, len;
  uint32_t cls;      // the first record (index into TtcPlan::rec) of the same tag, offset and length
  uint32_t entry;    // its directory entry, after ttc_entries()
};
struct TtcMember {
  uint32_t flavor;
  uint32_t first, count;   // its kept records in TtcPlan::rec
  uint32_t glyf, loca, hmtx, hhea, head, maxp;   // record indices, kNoTable for none
  uint32_t num_glyphs, long_loca;                // where its glyf is transformed
  uint32_t pair;                                 // in TtcPlan::pairs, after ttc_entries()
  std::vector<uint32_t> idx;                     // its directory indices, ascending, after ttc_entries()
};
struct TtcCandidate {
  uint32_t rec, rep;   // record indices: both of `len` bytes
};
struct TtcPair {
  uint32_t glyf;       // the glyf entry; its loca is the next
  uint32_t num_glyphs, long_loca;
};
struct TtcHmtx {       // an hmtx entry that is transformed if the device finds an array equal to xMin
  uint32_t hmtx, pair, nhm;
};

struct TtcPlan {
  uint32_t version = 0, num_fonts = 0;
  std::vector<TtcRecord> rec;        // the members' kept records, member after member
  std::vector<TtcMember> fonts;
  std::vector<TtcCandidate> cand;    // ascending in rec
  bool tr_glyf = false;              // pairs are transformed
  // after ttc_entries()
  std::vector<Table> t;              // the directory
  std::vector<uint32_t> fix;         // per entry: HeadFix
  std::vector<uint32_t> unit;        // per entry: its place in pairs (glyf, loca) or hunits, else kNoTable
  std::vector<TtcPair> pairs;        // in directory order
  std::vector<TtcHmtx> hunits;       // in directory order
  uint32_t version_at = kNoTable;    // where the header's version bytes lie in the input
  uint64_t total_sfnt = 0;
  // after ttc_layout()
  uint64_t stream_len = 0;
  std::vector<uint8_t> dir;          // the directory and the CollectionHeader
};

inline int ttc_read(const uint8_t *ttc, size_t n, uint32_t transforms, TtcPlan *pl) {
  *pl = TtcPlan();
  if (!ttc) return kTtcPast;
  woff2file::Reader r{ttc, n, 0, false};
  const uint32_t sig = r.u32();
  pl->version = r.u32();
  const uint32_t nf = r.u32();
  if (r.bad) return kTtcPast;
  if (sig != woff2file::kFlavorTtc) return kFlavor;
  if (pl->version != woff2file::kTtcVersion1 && pl->version != woff2file::kTtcVersion2) return kTtcVersion;
  if (nf == 0 || nf > 65535) return kTtcCount;
  if (12 + 4 * (uint64_t)nf + (pl->version == woff2file::kTtcVersion2 ? 12 : 0) > n) return kTtcPast;
  pl->num_fonts = nf;
  pl->tr_glyf = (transforms & kTransformGlyf) != 0;
  uint64_t dirs = 0;
  std::vector<std::pair<uint32_t, uint32_t>> ranges;   // every record's (offset, length)
  std::vector<uint32_t> tags;
  for (uint32_t f = 0; f < nf; f++) {
    const uint32_t at = r.u32();   // (inside the input: the header's size was checked)
    woff2file::Reader d{ttc, n, (size_t)at, false};
    const uint32_t flavor = d.u32(), nt = d.u16();
    if (d.bad || (uint64_t)at + 12 > n) return kTtcPast;
    if (nt == 0) return kTtcCount;
    dirs += 12 + 16 * (uint64_t)nt;
    if (dirs > woff2file::kMaxDirectoryBytes) return kTtcDirs;   // (before anything grows with it)
    if ((uint64_t)at + 12 + 16 * (uint64_t)nt > n) return kTtcPast;
    d.pos = (size_t)at + 12;
    TtcMember m{flavor, (uint32_t)pl->rec.size(), 0, kNoTable, kNoTable, kNoTable, kNoTable, kNoTable, kNoTable, 0, 0, kNoTable, {}};
    tags.clear();
    for (uint32_t i = 0; i < nt; i++) {
      const uint32_t tag = d.u32(), check = d.u32(), off = d.u32(), len = d.u32();
      if (d.bad) return kTtcPast;
      if ((uint64_t)off + len > n) return kTtcRecord;
      ranges.push_back({off, len});
      tags.push_back(tag);
      if (tag != kDsigTag) pl->rec.push_back(TtcRecord{tag, check, off, len, 0, kNoTable});
    }
    std::sort(tags.begin(), tags.end());
    for (uint32_t i = 1; i < nt; i++)
      if (tags[i] == tags[i - 1]) return kTtcTwice;
    m.count = (uint32_t)pl->rec.size() - m.first;
    // ascending tag, loca directly behind glyf
    auto rank = [](uint32_t tag) { return tag == kLocaTag ? ((uint64_t)kGlyfTag << 1) | 1 : (uint64_t)tag << 1; };
    std::sort(pl->rec.begin() + m.first, pl->rec.end(),
              [&](const TtcRecord &a, const TtcRecord &b) { return rank(a.tag) < rank(b.tag); });
    for (uint32_t i = m.first; i < m.first + m.count; i++) {
      const uint32_t tag = pl->rec[i].tag;
      uint32_t *slot = tag == kGlyfTag ? &m.glyf : tag == kLocaTag ? &m.loca : tag == kHmtxTag ? &m.hmtx
                       : tag == kHheaTag ? &m.hhea : tag == kHeadTag ? &m.head : tag == kMaxpTag ? &m.maxp : nullptr;
      if (slot) *slot = i;
    }
    pl->fonts.push_back(m);
  }
  std::sort(ranges.begin(), ranges.end());
  uint64_t sum = 0;
  for (size_t i = 0; i < ranges.size(); i++)
    if (i == 0 || ranges[i] != ranges[i - 1]) sum += ranges[i].second;
  if (sum > woff2inv::kMaxInput) return kTtcSum;
  for (const TtcMember &m : pl->fonts)
    if ((m.glyf == kNoTable) != (m.loca == kNoTable)) return kTtcGlyfLoca;
  for (const TtcMember &m : pl->fonts)
    if (m.count == 0) return kTtcEmpty;
  if (pl->tr_glyf)
    for (TtcMember &m : pl->fonts) {
      if (m.glyf == kNoTable) continue;
      if (m.head == kNoTable || pl->rec[m.head].len < 54 || m.maxp == kNoTable || pl->rec[m.maxp].len < 6) return kTtcGlyfNeeds;
      woff2file::Reader h{ttc, n, (size_t)pl->rec[m.head].off + 50, false};
      m.long_loca = (int16_t)h.u16() != 0 ? 1 : 0;
      woff2file::Reader g{ttc, n, (size_t)pl->rec[m.maxp].off + 4, false};
      m.num_glyphs = g.u16();
      if (h.bad || g.bad || m.num_glyphs == 0 || ((uint64_t)m.num_glyphs + 1) * (m.long_loca ? 4 : 2) > pl->rec[m.loca].len)
        return kTtcGlyfNeeds;
    }
  // one table by tag, offset and length; the others' candidates
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> first, rep;
  for (uint32_t i = 0; i < pl->rec.size(); i++) {
    TtcRecord &q = pl->rec[i];
    const auto at = first.emplace(std::make_tuple(q.tag, q.off, q.len), i);
    q.cls = at.first->second;
    if (!at.second) continue;
    const auto group = rep.emplace(std::make_tuple(q.tag, q.len, q.check), i);
    // (at another offset than its representative: tag and length are the group's, and the three together are new)
    if (!group.second) pl->cand.push_back(TtcCandidate{i, group.first->second});
  }
  return kOk;
}

// differ[c] != 0: candidate c's bytes are not its representative's (null: every candidate is
// equal).  kOk or kTtcEntries.
inline int ttc_entries(TtcPlan *pl, const uint8_t *ttc, size_t n, uint32_t transforms, const uint8_t *differ) {
  const size_t nr = pl->rec.size();
  std::vector<uint32_t> table(nr);   // per record: the record that stands for its table
  for (size_t i = 0; i < nr; i++) table[i] = pl->rec[i].cls;
  std::vector<uint32_t> merged(nr, kNoTable);
  for (size_t c = 0; c < pl->cand.size(); c++)
    if (!differ || !differ[c]) merged[pl->cand[c].rec] = pl->cand[c].rep;
  for (size_t i = 0; i < nr; i++)
    if (merged[table[i]] != kNoTable) table[i] = merged[table[i]];   // (a representative is no candidate: no chains)
  pl->t.clear();
  pl->pairs.clear();
  pl->hunits.clear();
  pl->unit.clear();
  pl->version_at = kNoTable;
  std::map<uint32_t, uint32_t> entry_of;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, uint32_t> pair_of;
  for (TtcMember &m : pl->fonts) {
    m.idx.clear();
    m.pair = kNoTable;
    for (uint32_t i = m.first; i < m.first + m.count; i++) {
      TtcRecord &q = pl->rec[i];
      if (q.tag == kLocaTag) continue;   // (entered with its glyf, which stands directly in front)
      if (q.tag == kGlyfTag) {
        const TtcRecord &l = pl->rec[m.loca];
        const auto at = pair_of.emplace(std::make_tuple(table[i], table[m.loca], m.num_glyphs, m.long_loca),
                                        (uint32_t)pl->pairs.size());
        if (at.second) {
          pl->pairs.push_back(TtcPair{(uint32_t)pl->t.size(), m.num_glyphs, m.long_loca});
          pl->t.push_back(Table{kGlyfTag, (uint8_t)(pl->tr_glyf ? kTrGlyf : kPlain), q.off, q.len, 0, 0});
          pl->t.push_back(Table{kLocaTag, (uint8_t)(pl->tr_glyf ? kTrLoca : kPlain), l.off, l.len, 0, 0});
        }
        m.pair = at.first->second;
        q.entry = pl->pairs[m.pair].glyf;
        pl->rec[m.loca].entry = q.entry + 1;
        m.idx.push_back(q.entry);
        m.idx.push_back(q.entry + 1);
        continue;
      }
      const auto at = entry_of.emplace(table[i], (uint32_t)pl->t.size());
      if (at.second) pl->t.push_back(Table{q.tag, kPlain, q.off, q.len, 0, 0});
      q.entry = at.first->second;
      m.idx.push_back(q.entry);
    }
    std::sort(m.idx.begin(), m.idx.end());
    if (pl->version_at == kNoTable && m.head != kNoTable && pl->rec[m.head].len >= 8) pl->version_at = pl->rec[m.head].off + 4;
  }
  const size_t num = pl->t.size();
  if (num > 65535) return kTtcEntries;
  pl->unit.assign(num, kNoTable);
  pl->fix.assign(num, kHeadNone);
  for (size_t p = 0; p < pl->pairs.size(); p++) pl->unit[pl->pairs[p].glyf] = pl->unit[pl->pairs[p].glyf + 1] = (uint32_t)p;
  // head: cleared; flagged where a member that lists it has a transformed pair
  for (const TtcMember &m : pl->fonts) {
    if (m.head == kNoTable || pl->rec[m.head].len < 18) continue;
    uint32_t &fix = pl->fix[pl->rec[m.head].entry];
    if (fix == kHeadNone) fix = kHeadZero;
    if (pl->tr_glyf && m.pair != kNoTable) fix = kHeadZeroFlag;
  }
  // hmtx: one pair and one hhea entry for every member that lists the entry
  if (pl->tr_glyf && (transforms & kTransformHmtx)) {
    std::vector<uint32_t> pair_of_hmtx(num, kNoTable), hhea_of(num, kNoTable);
    std::vector<uint8_t> no(num, 0);
    for (const TtcMember &m : pl->fonts) {
      if (m.hmtx == kNoTable) continue;
      const uint32_t e = pl->rec[m.hmtx].entry;
      if (m.pair == kNoTable || m.hhea == kNoTable) {
        no[e] = 1;
        continue;
      }
      const uint32_t hh = pl->rec[m.hhea].entry;
      if (pair_of_hmtx[e] == kNoTable) pair_of_hmtx[e] = m.pair, hhea_of[e] = hh;
      if (pair_of_hmtx[e] != m.pair || hhea_of[e] != hh) no[e] = 1;
    }
    for (size_t e = 0; e < num; e++) {
      if (pair_of_hmtx[e] == kNoTable || no[e]) continue;
      const Table &hh = pl->t[hhea_of[e]];
      if (hh.src_len < 36) continue;
      woff2file::Reader q{ttc, n, (size_t)hh.src_off + 34, false};
      const uint32_t nhm = q.u16(), ng = pl->pairs[pair_of_hmtx[e]].num_glyphs;
      // (a longer hmtx stays as it is: the transform would lose its trailing bytes)
      if (q.bad || nhm < 1 || nhm > ng || (uint64_t)pl->t[e].src_len != 4ull * nhm + 2ull * (ng - nhm)) continue;
      pl->unit[e] = (uint32_t)pl->hunits.size();
      pl->hunits.push_back(TtcHmtx{(uint32_t)e, pair_of_hmtx[e], nhm});
    }
  }
  pl->total_sfnt = 12 + 4 * (uint64_t)pl->num_fonts + (pl->version == woff2file::kTtcVersion2 ? 12 : 0);
  for (const TtcMember &m : pl->fonts) pl->total_sfnt += 12 + 16 * (uint64_t)m.count;
  for (const Table &t : pl->t) pl->total_sfnt += ((uint64_t)t.src_len + 3) & ~3ull;
  return kOk;
}

inline void put_255(std::vector<uint8_t> *o, uint32_t v) {   // 255UInt16, the shortest form
  if (v < 253) {
    o->push_back((uint8_t)v);
  } else if (v < 506) {
    o->push_back(255);
    o->push_back((uint8_t)(v - 253));
  } else if (v < 762) {
    o->push_back(254);
    o->push_back((uint8_t)(v - 506));
  } else {
    o->push_back(253);
    o->push_back((uint8_t)(v >> 8));
    o->push_back((uint8_t)v);
  }
}

// The places in the stream, the directory and the CollectionHeader.  tglyf_len: per pair (unused
// unless tr_glyf); thmtx_len: per hmtx unit, 0 where the entry stays as it is.  False for a stream
// that woff2_file.h's parse would refuse.
inline bool ttc_layout(TtcPlan *pl, const uint64_t *tglyf_len, const uint64_t *thmtx_len) {
  for (size_t u = 0; u < pl->hunits.size(); u++) pl->t[pl->hunits[u].hmtx].state = thmtx_len[u] ? kTrHmtx : kPlain;
  uint64_t at = 0;
  pl->dir.clear();
  for (size_t i = 0; i < pl->t.size(); i++) {
    Table &t = pl->t[i];
    const uint64_t len = t.state == kTrGlyf ? tglyf_len[pl->unit[i]] : t.state == kTrLoca ? 0
                         : t.state == kTrHmtx ? thmtx_len[pl->unit[i]] : t.src_len;
    if (len > 0xFFFFFFFFull) return false;
    t.at = at;
    t.len = (uint32_t)len;
    at += len;
    if (at > woff2inv::kMaxInput) return false;
    put_entry(&pl->dir, t);
  }
  pl->stream_len = at;
  for (int s = 24; s >= 0; s -= 8) pl->dir.push_back((uint8_t)(pl->version >> s));
  put_255(&pl->dir, pl->num_fonts);
  for (const TtcMember &m : pl->fonts) {
    put_255(&pl->dir, (uint32_t)m.idx.size());
    for (int s = 24; s >= 0; s -= 8) pl->dir.push_back((uint8_t)(m.flavor >> s));
    for (uint32_t i : m.idx) put_255(&pl->dir, i);
  }
  return true;
}

inline uint64_t ttc_file_bytes(const TtcPlan &pl, uint64_t compressed) {
  return (woff2file::kHeaderBytes + (uint64_t)pl.dir.size() + compressed + 3) & ~3ull;
}

inline bool ttc_finish(const TtcPlan &pl, const uint8_t *ttc, uint64_t compressed, uint8_t hdr[woff2file::kHeaderBytes]) {
  const uint64_t length = ttc_file_bytes(pl, compressed);
  if (length > 0xFFFFFFFFull || pl.total_sfnt > 0xFFFFFFFFull) return false;
  for (size_t i = 0; i < woff2file::kHeaderBytes; i++) hdr[i] = 0;
  woff2file::put32(hdr, woff2file::kSigWoff2);
  woff2file::put32(hdr + 4, woff2file::kFlavorTtc);
  woff2file::put32(hdr + 8, (uint32_t)length);
  woff2inv::put16(hdr + 12, (uint32_t)pl.t.size());
  woff2file::put32(hdr + 16, (uint32_t)pl.total_sfnt);
  woff2file::put32(hdr + 20, (uint32_t)compressed);
  if (pl.version_at != kNoTable)
    for (int b = 0; b < 4; b++) hdr[24 + b] = ttc[(size_t)pl.version_at + b];
  return true;
}

// The stream, serially, from a laid-out plan: tglyf[p] / thmtx[u] are the transformed tables whose
// sizes ttc_layout() was given (thmtx[u] unused where the entry stays as it is).
inline void ttc_host_pack(const TtcPlan &pl, const uint8_t *ttc, const uint8_t *const *tglyf, const uint8_t *const *thmtx,
                          std::vector<uint8_t> *stream) {
  stream->assign((size_t)pl.stream_len, 0);
  uint8_t *o = stream->data();
  for (size_t i = 0; i < pl.t.size(); i++) {
    const Table &t = pl.t[i];
    const uint8_t *src = t.state == kTrGlyf ? tglyf[pl.unit[i]] : t.state == kTrHmtx ? thmtx[pl.unit[i]] : ttc + t.src_off;
    for (uint32_t b = 0; b < t.len; b++) o[t.at + b] = src[b];
    if (pl.fix[i] != kHeadNone) {
      for (int b = 8; b < 12; b++) o[t.at + b] = 0;
      if (pl.fix[i] == kHeadZeroFlag) o[t.at + 16] |= 0x08;
    }
  }
}

}  // namespace woff2write
}  // namespace mib
#endif
