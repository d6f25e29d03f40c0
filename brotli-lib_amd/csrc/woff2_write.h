// The WOFF2 container (W3C WOFF2 sections 3 - 5), write direction: an sfnt becomes a plan -- which
// tables the file keeps and in what order, where each table's bytes lie in the sfnt, which are
// transformed, where each goes in the stream that is handed to the Brotli encoder -- and from the
// plan come the directory and the 48-byte header.  Plain C++ in the manner of woff2_file.h:
// woff2_write.hip runs the plan on the device, host_pack below states the stream serially (the
// CPU tests' path under sanitizers, tests/woff2_write_host_main.cpp).  The sfnt is untrusted:
// every byte of it is read through woff2file::Reader, which refuses to pass the end.
//
// Every byte of the file but the Brotli stream is fixed (DESIGN.md 4c "Writing a file"):
//   header     wOF2, the sfnt's flavor, length, numTables, 0, totalSfntSize = 12 + 16 numTables +
//              the sum of the tables' origLength padded to 4, totalCompressedSize, the version
//              (head's fontRevision, bytes 4..7, where head has them; else 0.0), metadata and
//              private fields 0.  Zero bytes pad the compressed stream to a 4-byte boundary and
//              count in `length`; nothing else follows it.  (Version and padding are what
//              fontTools writes: the golden files of tests/golden/woff2 are the reference.)
//   directory  the tables in ascending bytewise tag order, DSIG dropped; flag byte = known-tag
//              index (63: the tag follows) | version << 6 (glyf / loca: 0 transformed, 3 not;
//              hmtx: 1 transformed, 0 not; others 0); origLength; transformLength for transformed
//              tables only (loca: 0); UIntBase128 values minimal.
//   stream     the tables back to back in directory order: the transformed glyf, an empty loca,
//              the transformed hmtx, head (of at least 18 bytes) with bytes 8..11 zero and flags
//              bit 11 (byte 16 |= 0x08) set when glyf / loca are transformed, every other table as
//              it is in the sfnt.
// origLength is the table's length in the input font, for glyf and loca too.  The specification
// makes it a hint for transformed tables (woff2_file.h sizes nothing from it): for a font that is
// not already normalised -- glyphs not padded to 4 bytes, a loca format the glyf table does not
// need -- the tables that mib_woff2_decode reconstructs have other lengths, and totalSfntSize
// then differs from the decoded font's size.
//
// Rejected (MIB_E_INVALID_ARG), all here, before any device work:
//   1 fewer than 12 bytes                       5 a tag twice
//   2 first four bytes ttcf, wOF2 or wOFF       6 table lengths above 256 MiB in sum
//   3 numTables 0, or a directory past the end  7 exactly one of glyf and loca
//   4 a record whose offset + length runs past  8 nothing left after dropping DSIG
// and, where glyf / loca are to be transformed, what the transform needs: a head of 54 bytes, a
// maxp of 6, numGlyphs above 0, a loca of numGlyphs + 1 entries.  (A malformed glyph is found on
// the device.)  Checksums, the searchRange fields, record order, table alignment and table
// overlap are not checked: each table is read through its own record.
// (parse() answers 2 for ttcf because a collection is not a single font: its plan is
// woff2_write_ttc.h's, which continues this list, and encode_batch sends it there.)
#ifndef MIB_WOFF2_WRITE_H_
#define MIB_WOFF2_WRITE_H_
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "woff2_file.h"

namespace mib {
namespace woff2write {

using woff2file::kGlyfTag;
using woff2file::kHeadTag;
using woff2file::kHheaTag;
using woff2file::kHmtxTag;
using woff2file::kLocaTag;
using woff2file::kNoTable;
using woff2file::tag4;

constexpr uint32_t kTransformGlyf = 1u, kTransformHmtx = 2u;   // MIB_WOFF2_GLYF, MIB_WOFF2_HMTX
constexpr uint32_t kMaxpTag = tag4('m', 'a', 'x', 'p'), kDsigTag = tag4('D', 'S', 'I', 'G');
constexpr uint32_t kSigWoff = 0x774F4646;   // 'wOFF'

enum Reject : int {   // why parse() said no: the numbers of the list above; 9: the transform's needs
  kOk = 0, kShort = 1, kFlavor = 2, kDirectory = 3, kRecord = 4, kTwice = 5, kSum = 6, kGlyfLoca = 7, kEmpty = 8,
  kGlyfNeeds = 9
};

enum State : uint8_t { kPlain, kTrGlyf, kTrLoca, kTrHmtx };
enum HeadFix : uint32_t { kHeadNone = 0, kHeadZero = 1, kHeadZeroFlag = 2 };   // what the copy does to head

struct Table {
  uint32_t tag;
  uint8_t state;
  uint32_t src_off, src_len;   // in the sfnt (src_off + src_len <= its size)
  uint64_t at;                 // in the stream, after layout()
  uint32_t len;                // in the stream, after layout()
};

struct Plan {
  uint32_t flavor;
  std::vector<Table> t;   // the kept tables in directory order (ascending tag)
  uint32_t glyf, loca, hmtx, hhea, head, maxp;   // table indices, kNoTable for none
  bool tr_glyf;         // glyf and loca are transformed
  bool hmtx_wanted;     // hmtx is transformed if a side-bearing array equals the glyphs' xMin
  bool tr_hmtx;         // after layout()
  uint32_t num_glyphs, num_hmetrics, long_loca;   // where tr_glyf (num_hmetrics: where hmtx_wanted)
  uint64_t total_sfnt;    // the header's totalSfntSize
  uint64_t stream_len;    // after layout()
  std::vector<uint8_t> dir;   // after layout()
};

inline uint32_t head_fix(const Plan &pl) {
  if (pl.head == kNoTable || pl.t[pl.head].src_len < 18) return kHeadNone;
  return pl.tr_glyf ? kHeadZeroFlag : kHeadZero;
}

// sfnt -> plan (everything but the places in the stream).  kOk, or the reason.
inline int parse(const uint8_t *sfnt, size_t n, uint32_t transforms, Plan *pl) {
  if (!sfnt || n < 12) return kShort;
  woff2file::Reader r{sfnt, n, 0, false};
  pl->flavor = r.u32();
  if (pl->flavor == woff2file::kFlavorTtc || pl->flavor == woff2file::kSigWoff2 || pl->flavor == kSigWoff) return kFlavor;
  const uint32_t num = r.u16();
  if (num == 0 || 12 + 16 * (uint64_t)num > n) return kDirectory;
  r.pos = 12;
  pl->t.clear();
  pl->dir.clear();
  pl->glyf = pl->loca = pl->hmtx = pl->hhea = pl->head = pl->maxp = kNoTable;
  pl->tr_glyf = pl->hmtx_wanted = pl->tr_hmtx = false;
  pl->num_glyphs = pl->num_hmetrics = pl->long_loca = 0;
  pl->total_sfnt = pl->stream_len = 0;
  uint64_t sum = 0;
  std::vector<uint32_t> tags;
  for (uint32_t i = 0; i < num; i++) {
    const uint32_t tag = r.u32();
    r.u32();   // checkSum
    const uint32_t off = r.u32(), len = r.u32();
    if (r.bad) return kDirectory;
    if ((uint64_t)off + len > n) return kRecord;
    sum += len;
    tags.push_back(tag);
    if (tag != kDsigTag) pl->t.push_back(Table{tag, kPlain, off, len, 0, 0});
  }
  std::sort(tags.begin(), tags.end());
  for (uint32_t i = 1; i < num; i++)
    if (tags[i] == tags[i - 1]) return kTwice;
  if (sum > woff2inv::kMaxInput) return kSum;
  std::sort(pl->t.begin(), pl->t.end(), [](const Table &a, const Table &b) { return a.tag < b.tag; });
  for (uint32_t i = 0; i < pl->t.size(); i++) {
    const uint32_t tag = pl->t[i].tag;
    uint32_t *slot = tag == kGlyfTag ? &pl->glyf : tag == kLocaTag ? &pl->loca : tag == kHmtxTag ? &pl->hmtx
                     : tag == kHheaTag ? &pl->hhea : tag == kHeadTag ? &pl->head : tag == kMaxpTag ? &pl->maxp : nullptr;
    if (slot) *slot = i;
  }
  if ((pl->glyf == kNoTable) != (pl->loca == kNoTable)) return kGlyfLoca;
  if (pl->t.empty()) return kEmpty;
  pl->total_sfnt = 12 + 16 * (uint64_t)pl->t.size();
  for (const Table &t : pl->t) pl->total_sfnt += ((uint64_t)t.src_len + 3) & ~3ull;
  if ((transforms & kTransformGlyf) && pl->glyf != kNoTable) {
    // what mib_woff2_transform_glyf asks of the font; no falling back to the null transform
    if (pl->head == kNoTable || pl->t[pl->head].src_len < 54 || pl->maxp == kNoTable || pl->t[pl->maxp].src_len < 6)
      return kGlyfNeeds;
    woff2file::Reader h{sfnt, n, (size_t)pl->t[pl->head].src_off + 50, false};
    pl->long_loca = (int16_t)h.u16() != 0 ? 1 : 0;
    woff2file::Reader m{sfnt, n, (size_t)pl->t[pl->maxp].src_off + 4, false};
    pl->num_glyphs = m.u16();
    if (h.bad || m.bad || pl->num_glyphs == 0 ||
        ((uint64_t)pl->num_glyphs + 1) * (pl->long_loca ? 4 : 2) > pl->t[pl->loca].src_len)
      return kGlyfNeeds;
    pl->tr_glyf = true;
    pl->t[pl->glyf].state = kTrGlyf;
    pl->t[pl->loca].state = kTrLoca;
    if ((transforms & kTransformHmtx) && pl->hmtx != kNoTable && pl->hhea != kNoTable && pl->t[pl->hhea].src_len >= 36) {
      woff2file::Reader e{sfnt, n, (size_t)pl->t[pl->hhea].src_off + 34, false};
      const uint32_t nhm = e.u16(), ng = pl->num_glyphs;
      // (a longer hmtx stays as it is: the transform would lose its trailing bytes)
      if (!e.bad && nhm >= 1 && nhm <= ng && (uint64_t)pl->t[pl->hmtx].src_len == 4ull * nhm + 2ull * (ng - nhm)) {
        pl->hmtx_wanted = true;
        pl->num_hmetrics = nhm;
      }
    }
  }
  return kOk;
}

inline void put_base128(std::vector<uint8_t> *o, uint32_t v) {   // minimal: no leading zero groups
  int groups = 1;
  for (uint32_t w = v >> 7; w; w >>= 7) groups++;
  for (int g = groups - 1; g >= 0; g--) o->push_back((uint8_t)(((v >> (7 * g)) & 0x7F) | (g ? 0x80 : 0)));
}

// One directory entry of a laid-out table (a collection's entries are written the same way)
inline void put_entry(std::vector<uint8_t> *dir, const Table &t) {
  uint32_t known = 63;
  for (uint32_t q = 0; q < 63; q++)
    if (woff2file::kKnownTags[q] == t.tag) known = q;
  const bool gl = t.tag == kGlyfTag || t.tag == kLocaTag;
  const uint32_t ver = gl ? (t.state == kPlain ? 3 : 0) : t.state == kTrHmtx ? 1 : 0;
  dir->push_back((uint8_t)(known | (ver << 6)));
  if (known == 63)
    for (int s = 24; s >= 0; s -= 8) dir->push_back((uint8_t)(t.tag >> s));
  put_base128(dir, t.src_len);
  if (t.state != kPlain) put_base128(dir, t.len);
}

// The places in the stream and the directory, once the transformed sizes are known.  tglyf_len:
// the transformed glyf table's (ignored unless tr_glyf); thmtx_len: the transformed hmtx table's,
// 0 where hmtx stays as it is (both side-bearing arrays differ, or it was never wanted).  False
// for a stream that woff2_file.h's parse would refuse (above 256 MiB, a length above 32 bits).
inline bool layout(Plan *pl, uint64_t tglyf_len, uint64_t thmtx_len) {
  pl->tr_hmtx = pl->hmtx_wanted && thmtx_len != 0;
  if (pl->hmtx != kNoTable) pl->t[pl->hmtx].state = pl->tr_hmtx ? kTrHmtx : kPlain;
  uint64_t at = 0;
  pl->dir.clear();
  for (Table &t : pl->t) {
    const uint64_t len = t.state == kTrGlyf ? tglyf_len : t.state == kTrLoca ? 0 : t.state == kTrHmtx ? thmtx_len : t.src_len;
    if (len > 0xFFFFFFFFull) return false;
    t.at = at;
    t.len = (uint32_t)len;
    at += len;
    if (at > woff2inv::kMaxInput) return false;
    put_entry(&pl->dir, t);
  }
  pl->stream_len = at;
  return true;
}

// header + directory + compressed stream, padded to a 4-byte boundary
inline uint64_t file_bytes(const Plan &pl, uint64_t compressed) {
  return (woff2file::kHeaderBytes + (uint64_t)pl.dir.size() + compressed + 3) & ~3ull;
}

// The header of the laid-out plan's file, whose Brotli stream has `compressed` bytes; `sfnt`: the
// font parse() was given.  False where the file's length would not fit the header's 32 bits.
inline bool finish(const Plan &pl, const uint8_t *sfnt, uint64_t compressed, uint8_t hdr[woff2file::kHeaderBytes]) {
  const uint64_t length = file_bytes(pl, compressed);
  if (length > 0xFFFFFFFFull || pl.total_sfnt > 0xFFFFFFFFull) return false;
  for (size_t i = 0; i < woff2file::kHeaderBytes; i++) hdr[i] = 0;
  woff2file::put32(hdr, woff2file::kSigWoff2);
  woff2file::put32(hdr + 4, pl.flavor);
  woff2file::put32(hdr + 8, (uint32_t)length);
  woff2inv::put16(hdr + 12, (uint32_t)pl.t.size());
  woff2file::put32(hdr + 16, (uint32_t)pl.total_sfnt);
  woff2file::put32(hdr + 20, (uint32_t)compressed);
  if (pl.head != kNoTable && pl.t[pl.head].src_len >= 8)   // majorVersion, minorVersion
    for (int b = 0; b < 4; b++) hdr[24 + b] = sfnt[pl.t[pl.head].src_off + 4 + b];
  return true;
}

// The stream, serially, from a laid-out plan: tglyf / thmtx are the transformed tables whose
// sizes layout() was given (thmtx unused where the plan keeps hmtx as it is).
inline void host_pack(const Plan &pl, const uint8_t *sfnt, const uint8_t *tglyf, const uint8_t *thmtx,
                      std::vector<uint8_t> *stream) {
  stream->assign((size_t)pl.stream_len, 0);
  uint8_t *o = stream->data();
  const uint32_t fix = head_fix(pl);
  for (uint32_t i = 0; i < pl.t.size(); i++) {
    const Table &t = pl.t[i];
    const uint8_t *src = t.state == kTrGlyf ? tglyf : t.state == kTrHmtx ? thmtx : sfnt + t.src_off;
    for (uint32_t b = 0; b < t.len; b++) o[t.at + b] = src[b];
    if (i == pl.head && fix != kHeadNone) {
      for (int b = 8; b < 12; b++) o[t.at + b] = 0;
      if (fix == kHeadZeroFlag) o[t.at + 16] |= 0x08;
    }
  }
}

}  // namespace woff2write
}  // namespace mib
#endif
