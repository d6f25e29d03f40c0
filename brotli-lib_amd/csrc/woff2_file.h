// The WOFF2 container (W3C WOFF2 sections 3 - 5), read direction: the 48-byte header and the
// table directory of a single-font .woff2 file become a plan -- where each table's bytes lie in
// the decompressed stream, how each is transformed, where each goes in the sfnt -- and the sfnt
// is assembled from it.  Plain C++ in the manner of woff2_inv.h: woff2_file.hip runs the plan
// on the device, host_assemble below runs it serially (the CPU tests' path under sanitizers,
// tests/woff2_file_host_main.cpp, and the device path's restatement).  The file is untrusted:
// every byte of it is read through Reader, which refuses to pass the end.
//
// The sfnt's layout is fixed so that results compare byte for byte:
//   offset table (12 bytes) | table records sorted by tag (16 each) | the tables in the order
//   of the WOFF2 directory, each at a 4-byte boundary and zero-padded to the next.
//   A table's checksum is the wrapping sum of its padded big-endian words, head's with its
//   bytes 8..11 as zero; head's bytes 8..11 become 0xB1B0AFBA - the whole file's sum.
// A font collection (flavor ttcf: the CollectionHeader behind the directory, section 4.2)
// becomes a TTC (DESIGN.md 4c "A font collection"):
//   'ttcf', version, numFonts, the members' offset-table offsets (version 2.0: three zero
//   words more) | the members' directories back to back, records sorted by tag, offsets
//   file-relative | every directory entry that a member lists, once, in the directory's order.
//   A table has one checksum whoever lists it; a head's bytes 8..11 become 0xB1B0AFBA - the sum
//   of the last member that lists it (its directory and its tables' checksums).
#ifndef MIB_WOFF2_FILE_H_
#define MIB_WOFF2_FILE_H_
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "woff2_inv.h"

namespace mib {
namespace woff2file {

constexpr size_t kHeaderBytes = 48;
constexpr uint32_t kSigWoff2 = 0x774F4632;   // 'wOF2'
constexpr uint32_t kFlavorTtc = 0x74746366;  // 'ttcf'
constexpr uint32_t kHeadMagic = 0xB1B0AFBA;

constexpr uint32_t tag4(char a, char b, char c, char d) {
  return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint8_t)d;
}
constexpr uint32_t kGlyfTag = tag4('g', 'l', 'y', 'f'), kLocaTag = tag4('l', 'o', 'c', 'a'),
                   kHmtxTag = tag4('h', 'm', 't', 'x'), kHheaTag = tag4('h', 'h', 'e', 'a'),
                   kHeadTag = tag4('h', 'e', 'a', 'd');
// the known tags of the directory's flag byte (WOFF2 section 4.1); 63: a tag follows
constexpr uint32_t kKnownTags[63] = {
    tag4('c', 'm', 'a', 'p'), tag4('h', 'e', 'a', 'd'), tag4('h', 'h', 'e', 'a'), tag4('h', 'm', 't', 'x'),
    tag4('m', 'a', 'x', 'p'), tag4('n', 'a', 'm', 'e'), tag4('O', 'S', '/', '2'), tag4('p', 'o', 's', 't'),
    tag4('c', 'v', 't', ' '), tag4('f', 'p', 'g', 'm'), tag4('g', 'l', 'y', 'f'), tag4('l', 'o', 'c', 'a'),
    tag4('p', 'r', 'e', 'p'), tag4('C', 'F', 'F', ' '), tag4('V', 'O', 'R', 'G'), tag4('E', 'B', 'D', 'T'),
    tag4('E', 'B', 'L', 'C'), tag4('g', 'a', 's', 'p'), tag4('h', 'd', 'm', 'x'), tag4('k', 'e', 'r', 'n'),
    tag4('L', 'T', 'S', 'H'), tag4('P', 'C', 'L', 'T'), tag4('V', 'D', 'M', 'X'), tag4('v', 'h', 'e', 'a'),
    tag4('v', 'm', 't', 'x'), tag4('B', 'A', 'S', 'E'), tag4('G', 'D', 'E', 'F'), tag4('G', 'P', 'O', 'S'),
    tag4('G', 'S', 'U', 'B'), tag4('E', 'B', 'S', 'C'), tag4('J', 'S', 'T', 'F'), tag4('M', 'A', 'T', 'H'),
    tag4('C', 'B', 'D', 'T'), tag4('C', 'B', 'L', 'C'), tag4('C', 'O', 'L', 'R'), tag4('C', 'P', 'A', 'L'),
    tag4('S', 'V', 'G', ' '), tag4('s', 'b', 'i', 'x'), tag4('a', 'c', 'n', 't'), tag4('a', 'v', 'a', 'r'),
    tag4('b', 'd', 'a', 't'), tag4('b', 'l', 'o', 'c'), tag4('b', 's', 'l', 'n'), tag4('c', 'v', 'a', 'r'),
    tag4('f', 'd', 's', 'c'), tag4('f', 'e', 'a', 't'), tag4('f', 'm', 't', 'x'), tag4('f', 'v', 'a', 'r'),
    tag4('g', 'v', 'a', 'r'), tag4('h', 's', 't', 'y'), tag4('j', 'u', 's', 't'), tag4('l', 'c', 'a', 'r'),
    tag4('m', 'o', 'r', 't'), tag4('m', 'o', 'r', 'x'), tag4('o', 'p', 'b', 'd'), tag4('p', 'r', 'o', 'p'),
    tag4('t', 'r', 'a', 'k'), tag4('Z', 'a', 'p', 'f'), tag4('S', 'i', 'l', 'f'), tag4('G', 'l', 'a', 't'),
    tag4('G', 'l', 'o', 'c'), tag4('F', 'e', 'a', 't'), tag4('S', 'i', 'l', 'l')};

// The one way the file's bytes are read: past the end, `bad` is raised and zeros come back.
struct Reader {
  const uint8_t *p;
  size_t n, pos;
  bool bad;
  uint32_t u8() {
    if (pos >= n) {
      bad = true;
      return 0;
    }
    return p[pos++];
  }
  uint32_t u16() {
    const uint32_t hi = u8();
    return (hi << 8) | u8();
  }
  uint32_t u32() {
    const uint32_t hi = u16();
    return (hi << 16) | u16();
  }
  // UIntBase128 (section 4.1): at most 5 bytes, no leading zeros, below 2^32
  uint32_t base128() {
    uint32_t v = 0;
    for (int i = 0; i < 5; i++) {
      const uint32_t b = u8();
      if (bad) return 0;
      if ((i == 0 && b == 0x80) || (v & 0xFE000000u)) {
        bad = true;
        return 0;
      }
      v = (v << 7) | (b & 0x7F);
      if (!(b & 0x80)) return v;
    }
    bad = true;   // a sixth byte would follow
    return 0;
  }
  // 255UInt16 (section 6.1.1): every encoding of a value is accepted, the non-canonical ones too
  uint32_t u255() {
    const uint32_t b = u8();
    if (b < 253) return b;
    if (b == 253) return u16();
    return (b == 254 ? 506u : 253u) + u8();
  }
};

enum Kind : uint8_t { kCopy, kGlyf, kLoca, kHmtx };   // kCopy: the stream's bytes; else reconstructed
constexpr uint32_t kNoTable = 0xFFFFFFFFu;

struct Table {
  uint32_t tag;
  uint8_t kind;
  uint32_t src_off, src_len;   // in the decompressed stream
  uint32_t dst_off, dst_len;   // in the sfnt; of a reconstructed table known after layout()
};

// A font collection (flavor ttcf; DESIGN.md 4c "A font collection"): the directory holds every
// table of every member font once, and a member lists its tables by their indices in it.
struct Member {
  uint32_t flavor;
  std::vector<uint32_t> order;   // its tables (indices into Plan::t) sorted by tag: its records
  uint32_t head;                 // the head it lists, or kNoTable
  bool adjusts;                  // no later member lists that head: this one stores its checkSumAdjustment
  uint32_t dir_off;              // its offset table in the TTC, after layout_units()
};
struct Pair {
  uint32_t glyf, loca;           // a transformed glyf entry and its loca: reconstructed together
};
struct HmtxUnit {
  uint32_t hmtx, pair, hhea;     // a transformed hmtx entry, its glyf's pair (in Plan::pairs), its hhea
};
constexpr uint32_t kTtcVersion1 = 0x00010000, kTtcVersion2 = 0x00020000;
constexpr uint64_t kMaxDirectoryBytes = (uint64_t)16 << 20;   // of a collection's members together

struct Plan {
  uint32_t flavor;
  std::vector<Table> t;          // in the directory's order (the order of the table data)
  std::vector<uint32_t> order;   // table indices sorted by tag (the order of the records); a single font's
  uint64_t stream_len;           // what the Brotli stream must decode to, exactly
  size_t comp_off, comp_len;     // the compressed stream in the file
  uint32_t glyf, loca, hmtx, hhea, head;   // table indices, kNoTable for none (and in a collection)
  uint64_t sfnt_len;             // after layout()
  // what is reconstructed, of a single font and of a collection alike (filled by parse())
  std::vector<Pair> pairs;         // the transformed glyf / loca pairs that are written, in directory order
  std::vector<HmtxUnit> hunits;    // the transformed hmtx entries that are written, in directory order
  std::vector<uint32_t> unit;      // per table: its place in pairs (kGlyf, kLoca) or hunits (kHmtx)
  // the collection
  uint32_t ttc_version = 0;        // 0: a single font
  std::vector<Member> fonts;       // in the collection's order
  std::vector<uint8_t> written;    // per table: some member lists it (a single font's tables all are)
};

inline bool is_written(const Plan &pl, size_t i) { return !pl.ttc_version || pl.written[i]; }

// The members' records and what follows from who lists what: records sorted by tag, no tag twice
// in one font (item 16), `written`, each member's head and whether it stores the adjustment.
inline bool collection_members(Plan *pl) {
  const size_t num = pl->t.size();
  pl->written.assign(num, 0);
  std::vector<uint32_t> last(num, kNoTable);   // per head entry: the last member that lists it
  for (size_t f = 0; f < pl->fonts.size(); f++) {
    Member &m = pl->fonts[f];
    std::sort(m.order.begin(), m.order.end(), [&](uint32_t a, uint32_t b) { return pl->t[a].tag < pl->t[b].tag; });
    m.head = kNoTable;
    m.adjusts = false;
    m.dir_off = 0;
    for (size_t r = 0; r < m.order.size(); r++) {
      const uint32_t i = m.order[r];
      if (r && pl->t[m.order[r - 1]].tag == pl->t[i].tag) return false;
      pl->written[i] = 1;
      if (pl->t[i].tag == kHeadTag) m.head = i, last[i] = (uint32_t)f;
    }
  }
  for (size_t f = 0; f < pl->fonts.size(); f++) {
    Member &m = pl->fonts[f];
    m.adjusts = m.head != kNoTable && last[m.head] == f;
  }
  return true;
}

// Items 18 and 19 of the rejection list, and with them the collection's pairs and hmtx units.
inline bool collection_units(Plan *pl) {
  const size_t num = pl->t.size();
  pl->pairs.clear();
  pl->hunits.clear();
  pl->unit.assign(num, kNoTable);
  for (size_t i = 0; i < num; i++) {
    const Table &t = pl->t[i];
    if (t.tag == kGlyfTag &&
        (i + 1 >= num || pl->t[i + 1].tag != kLocaTag || (t.kind == kGlyf) != (pl->t[i + 1].kind == kLoca)))
      return false;
    if (t.tag == kLocaTag && (i == 0 || pl->t[i - 1].tag != kGlyfTag)) return false;
  }
  // (a member lists a tag once at most: one glyf, one loca, one hmtx, one hhea)
  auto listed = [&](const Member &m, uint32_t tag) {
    for (uint32_t i : m.order)
      if (pl->t[i].tag == tag) return i;
    return kNoTable;
  };
  for (const Member &m : pl->fonts) {
    const uint32_t g = listed(m, kGlyfTag), l = listed(m, kLocaTag);
    if ((g == kNoTable) != (l == kNoTable) || (g != kNoTable && l != g + 1)) return false;
  }
  for (size_t i = 0; i < num; i++)
    if (pl->t[i].kind == kGlyf && pl->written[i]) {   // (its loca is written with it: the loop above)
      pl->unit[i] = pl->unit[i + 1] = (uint32_t)pl->pairs.size();
      pl->pairs.push_back(Pair{(uint32_t)i, (uint32_t)i + 1});
    }
  std::vector<uint32_t> glyf_of(num, kNoTable), hhea_of(num, kNoTable);   // per transformed hmtx entry
  for (const Member &m : pl->fonts) {
    const uint32_t h = listed(m, kHmtxTag);
    if (h == kNoTable || pl->t[h].kind != kHmtx) continue;
    const uint32_t g = listed(m, kGlyfTag), hh = listed(m, kHheaTag);
    if (g == kNoTable || pl->t[g].kind != kGlyf || hh == kNoTable || pl->t[hh].src_len < 36) return false;
    if (glyf_of[h] == kNoTable) glyf_of[h] = g, hhea_of[h] = hh;
    if (glyf_of[h] != g || hhea_of[h] != hh) return false;   // the entry would reconstruct to two tables
  }
  for (size_t i = 0; i < num; i++)
    if (glyf_of[i] != kNoTable) {
      pl->unit[i] = (uint32_t)pl->hunits.size();
      pl->hunits.push_back(HmtxUnit{(uint32_t)i, pl->unit[glyf_of[i]], hhea_of[i]});
    }
  return true;
}

// The CollectionHeader behind the directory (section 4.2): items 14 - 17 and 20.
inline bool parse_collection(Reader *r, uint32_t num, Plan *pl) {
  pl->ttc_version = r->u32();
  const uint32_t nf = r->u255();
  if (r->bad || (pl->ttc_version != kTtcVersion1 && pl->ttc_version != kTtcVersion2) || nf == 0) return false;
  uint64_t dirs = 0;
  for (uint32_t f = 0; f < nf; f++) {
    const uint32_t nt = r->u255(), flavor = r->u32();
    if (r->bad || nt == 0) return false;
    dirs += 12 + 16 * (uint64_t)nt;
    // (before anything grows with it; and an index takes a byte of the file at least)
    if (dirs > kMaxDirectoryBytes || nt > r->n - r->pos) return false;
    pl->fonts.push_back(Member{flavor, {}, kNoTable, false, 0});
    std::vector<uint32_t> &order = pl->fonts.back().order;
    order.reserve(nt);
    for (uint32_t i = 0; i < nt; i++) {
      const uint32_t idx = r->u255();
      if (r->bad || idx >= num) return false;
      order.push_back(idx);
    }
  }
  return true;
}

// Header and directory -> plan (everything but the destinations).  False: MIB_E_INVALID_ARG.
inline bool parse(const uint8_t *file, size_t n, Plan *pl) {
  if (!file || n < kHeaderBytes) return false;
  Reader r{file, n, 0, false};
  const uint32_t sig = r.u32();
  pl->flavor = r.u32();
  const uint32_t length = r.u32(), num = r.u16();
  r.u16();   // reserved
  r.u32();   // totalSfntSize: a hint
  const uint32_t comp = r.u32();
  r.pos = kHeaderBytes;   // versions, metadata and private blocks: ignored
  if (sig != kSigWoff2 || (size_t)length != n || num == 0) return false;
  const bool ttc = pl->flavor == kFlavorTtc;
  pl->t.clear();
  pl->glyf = pl->loca = pl->hmtx = pl->hhea = pl->head = kNoTable;
  pl->pairs.clear();
  pl->hunits.clear();
  pl->unit.clear();
  pl->ttc_version = 0;
  pl->fonts.clear();
  pl->written.clear();
  pl->order.clear();
  pl->sfnt_len = 0;
  uint64_t at = 0;
  bool glyf_tr = false, loca_tr = false;
  for (uint32_t i = 0; i < num; i++) {
    const uint32_t flags = r.u8();
    const uint32_t tag = (flags & 63) == 63 ? r.u32() : kKnownTags[flags & 63], ver = flags >> 6;
    const uint32_t orig = r.base128();
    if (r.bad) return false;
    Table t{tag, kCopy, 0, orig, 0, 0};
    bool transformed = false;
    if (tag == kGlyfTag || tag == kLocaTag) {
      if (ver != 0 && ver != 3) return false;
      transformed = ver == 0;
      if (transformed) t.kind = tag == kGlyfTag ? kGlyf : kLoca;
      (tag == kGlyfTag ? glyf_tr : loca_tr) = transformed;
    } else if (tag == kHmtxTag) {
      if (ver > 1) return false;
      transformed = ver == 1;
      if (transformed) t.kind = kHmtx;
    } else if (ver != 0) {
      return false;
    }
    if (transformed) {   // origLength is only a hint then
      t.src_len = r.base128();
      if (r.bad) return false;
      if (t.kind == kLoca && t.src_len != 0) return false;
    }
    uint32_t *slot = tag == kGlyfTag ? &pl->glyf : tag == kLocaTag ? &pl->loca : tag == kHmtxTag ? &pl->hmtx
                     : tag == kHheaTag ? &pl->hhea : tag == kHeadTag ? &pl->head : nullptr;
    if (slot && !ttc) {   // (across a collection's directory repeated tags are normal)
      if (*slot != kNoTable) return false;   // (the other tags' duplicates: found in the sorted order)
      *slot = i;
    }
    at += t.src_len;
    if (at > woff2inv::kMaxInput) return false;
    t.src_off = (uint32_t)(at - t.src_len);
    pl->t.push_back(t);
  }
  pl->stream_len = at;
  if (ttc && !parse_collection(&r, num, pl)) return false;
  pl->comp_off = r.pos;
  pl->comp_len = comp;
  if ((uint64_t)comp > (uint64_t)(n - r.pos)) return false;
  if (ttc) return collection_members(pl) && collection_units(pl);
  pl->order.resize(num);
  for (uint32_t i = 0; i < num; i++) pl->order[i] = i;
  std::sort(pl->order.begin(), pl->order.end(), [&](uint32_t a, uint32_t b) { return pl->t[a].tag < pl->t[b].tag; });
  for (uint32_t i = 1; i < num; i++)
    if (pl->t[pl->order[i]].tag == pl->t[pl->order[i - 1]].tag) return false;
  // glyf and loca come together and in the same state
  if ((pl->glyf == kNoTable) != (pl->loca == kNoTable) || glyf_tr != loca_tr) return false;
  if (pl->hmtx != kNoTable && pl->t[pl->hmtx].kind == kHmtx) {
    if (!glyf_tr || pl->hhea == kNoTable || pl->t[pl->hhea].src_len < 36) return false;
  }
  pl->unit.assign(num, kNoTable);
  if (glyf_tr) {
    pl->pairs.push_back(Pair{pl->glyf, pl->loca});
    pl->unit[pl->glyf] = pl->unit[pl->loca] = 0;
  }
  if (pl->hmtx != kNoTable && pl->t[pl->hmtx].kind == kHmtx) {
    pl->hunits.push_back(HmtxUnit{pl->hmtx, 0, pl->hhea});
    pl->unit[pl->hmtx] = 0;
  }
  return true;
}

inline bool glyf_transformed(const Plan &pl) { return pl.glyf != kNoTable && pl.t[pl.glyf].kind == kGlyf; }
inline bool hmtx_transformed(const Plan &pl) { return pl.hmtx != kNoTable && pl.t[pl.hmtx].kind == kHmtx; }
// head's bytes 8..11 are the file's checkSumAdjustment only where the table has them
inline bool head_adjusted(const Plan &pl) { return pl.head != kNoTable && pl.t[pl.head].dst_len >= 12; }

// The destinations, once the reconstructed tables' sizes are known.  False for an sfnt whose
// offsets would not fit 32 bits.
inline bool layout(Plan *pl, uint64_t glyf_len, uint64_t loca_len, uint64_t hmtx_len) {
  uint64_t at = 12 + 16 * (uint64_t)pl->t.size();
  for (Table &t : pl->t) {
    const uint64_t len = t.kind == kGlyf ? glyf_len : t.kind == kLoca ? loca_len : t.kind == kHmtx ? hmtx_len : t.src_len;
    if (len > 0xFFFFFFFFull || at + len > 0xFFFFFFFCull) return false;
    t.dst_off = (uint32_t)at;
    t.dst_len = (uint32_t)len;
    at = (at + len + 3) & ~3ull;
  }
  pl->sfnt_len = at;
  return true;
}

inline uint64_t ttc_header_bytes(const Plan &pl) {
  return 12 + 4 * (uint64_t)pl.fonts.size() + (pl.ttc_version == kTtcVersion2 ? 12 : 0);
}

// The destinations over any number of reconstructed lengths: glyf_len / loca_len per pair,
// hmtx_len per hmtx unit (null where there is none).  A collection: TTC header, the members'
// directories back to back, then the written tables in the directory's order; sfnt_len is the
// TTC's size.  (The directories are 16 MiB at most: parse_collection.)
inline bool layout_units(Plan *pl, const uint64_t *glyf_len, const uint64_t *loca_len, const uint64_t *hmtx_len) {
  if (!pl->ttc_version)
    return layout(pl, pl->pairs.empty() ? 0 : glyf_len[0], pl->pairs.empty() ? 0 : loca_len[0],
                  pl->hunits.empty() ? 0 : hmtx_len[0]);
  uint64_t at = ttc_header_bytes(*pl);
  for (Member &m : pl->fonts) {
    m.dir_off = (uint32_t)at;
    at += 12 + 16 * (uint64_t)m.order.size();
  }
  for (size_t i = 0; i < pl->t.size(); i++) {
    Table &t = pl->t[i];
    t.dst_off = t.dst_len = 0;
    if (!pl->written[i]) continue;
    const uint64_t len = t.kind == kGlyf ? glyf_len[pl->unit[i]] : t.kind == kLoca ? loca_len[pl->unit[i]]
                         : t.kind == kHmtx ? hmtx_len[pl->unit[i]] : t.src_len;
    if (len > 0xFFFFFFFFull || at + len > 0xFFFFFFFCull) return false;
    t.dst_off = (uint32_t)at;
    t.dst_len = (uint32_t)len;
    at = (at + len + 3) & ~3ull;
  }
  pl->sfnt_len = at;
  return true;
}
// a member's head carries a checkSumAdjustment (and this member stores it) only where it has the bytes
inline bool head_zeroed(const Plan &pl, size_t i) {
  return pl.ttc_version ? pl.t[i].tag == kHeadTag && pl.written[i] && pl.t[i].dst_len >= 12
                        : i == pl.head && pl.t[i].dst_len >= 12;
}
inline bool member_adjusts(const Plan &pl, const Member &m) { return m.adjusts && pl.t[m.head].dst_len >= 12; }

// searchRange, entrySelector, rangeShift of the offset table (their low 16 bits, which is all
// the fields hold: OpenType leaves more than 4095 tables undefined)
inline void search_fields(uint32_t num, uint32_t *range, uint32_t *selector, uint32_t *shift) {
  uint32_t sel = 0;
  while ((2u << sel) <= num) sel++;
  *range = ((1u << sel) * 16) & 0xFFFF;
  *selector = sel;
  *shift = (num * 16 - (1u << sel) * 16) & 0xFFFF;
}

inline void put32(uint8_t *o, uint32_t v) {
  o[0] = (uint8_t)(v >> 24);
  o[1] = (uint8_t)(v >> 16);
  o[2] = (uint8_t)(v >> 8);
  o[3] = (uint8_t)v;
}
inline uint32_t sum_words(const uint8_t *p, size_t n) {   // n a multiple of 4
  uint32_t s = 0;
  for (size_t i = 0; i < n; i += 4)
    s += ((uint32_t)p[i] << 24) | ((uint32_t)p[i + 1] << 16) | ((uint32_t)p[i + 2] << 8) | p[i + 3];
  return s;
}

// An offset table and its records at o: `order` lists the tables in tag order.  The sum of what
// was written and of the listed tables' checksums: what a font's checkSumAdjustment is taken from.
inline uint32_t put_directory(uint8_t *o, uint32_t flavor, const std::vector<Table> &t, const std::vector<uint32_t> &order,
                              const std::vector<uint32_t> &sums) {
  const uint32_t num = (uint32_t)order.size();
  uint32_t range, selector, shift;
  search_fields(num, &range, &selector, &shift);
  put32(o, flavor);
  woff2inv::put16(o + 4, num);
  woff2inv::put16(o + 6, range);
  woff2inv::put16(o + 8, selector);
  woff2inv::put16(o + 10, shift);
  uint32_t total = 0;
  for (uint32_t r = 0; r < num; r++) {
    const uint32_t i = order[r];
    uint8_t *rec = o + 12 + 16 * (size_t)r;
    put32(rec, t[i].tag);
    put32(rec + 4, sums[i]);
    put32(rec + 8, t[i].dst_off);
    put32(rec + 12, t[i].dst_len);
    total += sums[i];
  }
  return total + sum_words(o, 12 + 16 * (size_t)num);
}

// host_assemble's collection: the parsed plan and its stream -> the TTC.
inline int host_assemble_collection(Plan *pl, const uint8_t *stream, std::vector<uint8_t> *ttc) {
  const size_t np = pl->pairs.size(), nh = pl->hunits.size(), num = pl->t.size();
  std::vector<std::vector<uint8_t>> glyf(np), loca(np), hmtx(nh);
  std::vector<uint64_t> glyf_len(np), loca_len(np), hmtx_len(nh);
  for (size_t p = 0; p < np; p++) {
    const Table &g = pl->t[pl->pairs[p].glyf];
    if (woff2inv::host_reconstruct(stream + g.src_off, g.src_len, &glyf[p], &loca[p]) != 0) return -1;
    glyf_len[p] = glyf[p].size();
    loca_len[p] = loca[p].size();
  }
  for (size_t u = 0; u < nh; u++) {
    const HmtxUnit &hu = pl->hunits[u];
    const Table &h = pl->t[hu.hmtx];
    const uint8_t *hhea = stream + pl->t[hu.hhea].src_off, *gh = stream + pl->t[pl->pairs[hu.pair].glyf].src_off;
    const uint32_t ng = ((uint32_t)gh[4] << 8) | gh[5], nhm = ((uint32_t)hhea[34] << 8) | hhea[35];
    if (woff2inv::host_reconstruct_hmtx(h.src_len ? stream + h.src_off : nullptr, h.src_len, glyf[hu.pair].data(),
                                        glyf[hu.pair].size(), loca[hu.pair].data(), loca[hu.pair].size(), ng, nhm,
                                        &hmtx[u]) != 0)
      return -1;
    hmtx_len[u] = hmtx[u].size();
  }
  if (!layout_units(pl, glyf_len.data(), loca_len.data(), hmtx_len.data())) return -1;
  ttc->assign((size_t)pl->sfnt_len, 0);
  uint8_t *o = ttc->data();
  std::vector<uint32_t> sums(num, 0);
  for (size_t i = 0; i < num; i++) {
    const Table &t = pl->t[i];
    if (!pl->written[i]) continue;
    const uint8_t *src = t.kind == kGlyf ? glyf[pl->unit[i]].data() : t.kind == kLoca ? loca[pl->unit[i]].data()
                         : t.kind == kHmtx ? hmtx[pl->unit[i]].data() : stream + t.src_off;
    for (uint32_t b = 0; b < t.dst_len; b++) o[t.dst_off + b] = src[b];
    if (head_zeroed(*pl, i))
      for (int b = 8; b < 12; b++) o[t.dst_off + b] = 0;
    sums[i] = sum_words(o + t.dst_off, ((size_t)t.dst_len + 3) & ~(size_t)3);
  }
  put32(o, kFlavorTtc);
  put32(o + 4, pl->ttc_version);
  put32(o + 8, (uint32_t)pl->fonts.size());
  for (size_t f = 0; f < pl->fonts.size(); f++) {
    const Member &m = pl->fonts[f];
    put32(o + 12 + 4 * f, m.dir_off);
    const uint32_t total = put_directory(o + m.dir_off, m.flavor, pl->t, m.order, sums);
    if (member_adjusts(*pl, m)) put32(o + pl->t[m.head].dst_off + 8, kHeadMagic - total);
  }
  return 0;
}

// The serial assembly.  0, or -1 for a file (or a stream) that is rejected.  `stream` is what
// the file's Brotli stream decoded to.  *plan_out: the plan as laid out (the tests check it).
// A collection gives its TTC.
inline int host_assemble(const uint8_t *file, size_t n, const uint8_t *stream, size_t stream_n, std::vector<uint8_t> *sfnt,
                         Plan *plan_out = nullptr) {
  Plan pl;
  sfnt->clear();
  if (!parse(file, n, &pl) || pl.stream_len != stream_n || (!stream && stream_n)) return -1;
  if (pl.ttc_version) {
    if (host_assemble_collection(&pl, stream, sfnt) != 0) return -1;
    if (plan_out) *plan_out = pl;
    return 0;
  }
  std::vector<uint8_t> glyf, loca, hmtx;
  if (glyf_transformed(pl)) {
    const Table &g = pl.t[pl.glyf];
    if (woff2inv::host_reconstruct(stream + g.src_off, g.src_len, &glyf, &loca) != 0) return -1;
    if (hmtx_transformed(pl)) {
      const Table &h = pl.t[pl.hmtx];
      const uint8_t *hhea = stream + pl.t[pl.hhea].src_off, *gh = stream + g.src_off;
      const uint32_t ng = ((uint32_t)gh[4] << 8) | gh[5], nhm = ((uint32_t)hhea[34] << 8) | hhea[35];
      if (woff2inv::host_reconstruct_hmtx(h.src_len ? stream + h.src_off : nullptr, h.src_len, glyf.data(), glyf.size(),
                                          loca.data(), loca.size(), ng, nhm, &hmtx) != 0)
        return -1;
    }
  }
  if (!layout(&pl, glyf.size(), loca.size(), hmtx.size())) return -1;
  sfnt->assign((size_t)pl.sfnt_len, 0);
  uint8_t *o = sfnt->data();
  const uint32_t num = (uint32_t)pl.t.size();
  std::vector<uint32_t> sums(num);
  for (uint32_t i = 0; i < num; i++) {
    const Table &t = pl.t[i];
    const uint8_t *src = t.kind == kGlyf ? glyf.data() : t.kind == kLoca ? loca.data() : t.kind == kHmtx ? hmtx.data()
                                                                                                        : stream + t.src_off;
    for (uint32_t b = 0; b < t.dst_len; b++) o[t.dst_off + b] = src[b];
    if (i == pl.head && head_adjusted(pl))
      for (int b = 8; b < 12; b++) o[t.dst_off + b] = 0;
    sums[i] = sum_words(o + t.dst_off, ((size_t)t.dst_len + 3) & ~(size_t)3);
  }
  uint32_t range, selector, shift;
  search_fields(num, &range, &selector, &shift);
  put32(o, pl.flavor);
  woff2inv::put16(o + 4, num);
  woff2inv::put16(o + 6, range);
  woff2inv::put16(o + 8, selector);
  woff2inv::put16(o + 10, shift);
  uint32_t total = 0;
  for (uint32_t r = 0; r < num; r++) {
    const uint32_t i = pl.order[r];
    uint8_t *rec = o + 12 + 16 * (size_t)r;
    put32(rec, pl.t[i].tag);
    put32(rec + 4, sums[i]);
    put32(rec + 8, pl.t[i].dst_off);
    put32(rec + 12, pl.t[i].dst_len);
    total += sums[i];
  }
  total += sum_words(o, 12 + 16 * (size_t)num);
  if (head_adjusted(pl)) put32(o + pl.t[pl.head].dst_off + 8, kHeadMagic - total);
  if (plan_out) *plan_out = pl;
  return 0;
}

}  // namespace woff2file
}  // namespace mib
#endif
