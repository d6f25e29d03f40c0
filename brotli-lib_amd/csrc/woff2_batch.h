// A batch of .woff2 files (DESIGN.md 4c "A batch of files"): everything that decides where bytes
// go when k files are worked in shared launches, in plain C++ in the manner of woff2_file.h, so
// that a stand-alone program can hold it under sanitizers (tests/woff2_batch_host_main.cpp).
// woff2_file.hip runs it on the device.
//
//   groups     the parsed files of a call, in order, cut so that a group's decompressed streams
//              sum to at most a budget; a file above the budget is a group alone
//   StreamPack a group's compressed streams back to back in one upload buffer (the decoder takes
//              each stream's exact length from the offsets' differences) and its decompressed
//              streams in slots that begin at 256-byte boundaries, each with a capacity of exactly
//              its plan's stream_len
//   Launch     the descriptor arrays of the two assembly kernels over every font of the group
//              that got as far as a layout: the tables of all fonts flattened, each with its
//              font's output base and its own sum slot; the directory records font after font; a
//              descriptor per font.  Every sfnt begins at a 16-byte boundary of the one output
//              buffer: the assembly lays 16-byte granules over the output, and two fonts must
//              not share one.  A font's base is 64 bits and the offsets inside a font stay the 32
//              bits they are in the sfnt, so a group's output may pass 4 GiB.  A collection is
//              one output file (its TTC) with a DirFont per member: the members share the
//              file's base and sums, and each has its directory's place in the file (dir_off).
#ifndef MIB_WOFF2_BATCH_H_
#define MIB_WOFF2_BATCH_H_
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "woff2_file.h"

namespace mib {
namespace woff2file {

constexpr uint64_t kGroupBytes = (uint64_t)512 << 20;   // the default budget of a group
constexpr uint64_t kSlotAlign = 256, kFontAlign = 16;
constexpr uint32_t kAsmThreads = 256;
constexpr uint64_t kAsmTile = (uint64_t)kAsmThreads * 16;   // bytes of output a block covers at a time
constexpr uint32_t kNoZero = 0xFFFFFFFFu;

struct Group {
  size_t first, count;   // a run of the parsed files' list
};

// stream_len[i]: what parsed file i's stream decodes to.  budget 0: the default.
inline std::vector<Group> make_groups(const std::vector<uint64_t> &stream_len, uint64_t budget) {
  if (!budget) budget = kGroupBytes;
  std::vector<Group> g;
  uint64_t sum = 0;
  bool alone = false;   // the open group is one file above the budget
  for (size_t i = 0; i < stream_len.size(); i++) {
    const bool big = stream_len[i] > budget;
    // (sum <= budget, and the room left is compared before anything is added: no wrap)
    if (g.empty() || alone || big || stream_len[i] > budget - sum) {
      g.push_back(Group{i, 0});
      sum = 0;
    }
    g.back().count++;
    sum += big ? 0 : stream_len[i];
    alone = big;
  }
  return g;
}

struct StreamPack {
  std::vector<uint64_t> in_off;     // n + 1: font i's compressed bytes in the upload buffer
  std::vector<uint64_t> slot_off;   // n: font i's decompressed stream, at a 256-byte boundary
  std::vector<uint64_t> cap;        // n: exactly stream_len
  uint64_t stream_bytes;            // the slots' buffer
};

inline StreamPack pack_streams(const Plan *const *plans, size_t n) {
  StreamPack p;
  p.in_off.assign(n + 1, 0);
  p.slot_off.assign(n, 0);
  p.cap.assign(n, 0);
  uint64_t at = 0;
  for (size_t i = 0; i < n; i++) {
    p.in_off[i + 1] = p.in_off[i] + plans[i]->comp_len;
    p.slot_off[i] = at;
    p.cap[i] = plans[i]->stream_len;
    at = (at + plans[i]->stream_len + kSlotAlign - 1) & ~(kSlotAlign - 1);
  }
  p.stream_bytes = at;
  return p;
}

// One table of the assembly launch.  dst_off is a multiple of 4 and out_base one of 16; src has
// any alignment and 16 readable bytes of slack behind its allocation's last byte (load16.h).
struct AsmDesc {
  const uint8_t *src;
  uint64_t out_base;   // its font's place in the output buffer
  uint32_t dst_off, len;
  uint32_t zero_at;    // head with its checkSumAdjustment: 8 (bytes 8..11 are stored as zero); else kNoZero
  uint32_t sum;        // its slot of the launch's sums
};
// One record of a font's directory, in tag order.  `table` counts from the font's first sum:
// the file's written tables in the directory's order (a table that several members of a
// collection list has one sum, and every record that lists it reaches it).
struct DirRec {
  uint32_t tag, table, dst_off, len;
};
// One font of the directory launch: a single font, or a member of a collection -- the members of
// one collection share out_base (the TTC's place), first_sum, and nothing else.
struct DirFont {
  uint64_t out_base;
  uint32_t flavor, num, range, selector, shift;
  uint32_t first_rec, first_sum;   // in the launch's records and sums
  uint32_t adjust_at;              // head's checkSumAdjustment in the file, or kNoZero (a member: unless
                                   // it is the last that lists its head)
  uint32_t dir_off = 0;            // the offset table's place in the file (0: a single font)
  uint32_t ttc_index = kNoZero;    // a member's place in its collection: it stores its word of the TTC
                                   // header, member 0 the words before them (and behind, version 2.0)
  uint32_t ttc_version = 0, ttc_fonts = 0;
};

// Where a font's tables lie once its stream is decoded and its tables are reconstructed.  A
// collection's (and any plan's, by its pairs and hmtx units): glyfs / locas per pair, hmtxs per unit.
struct FontSrc {
  const uint8_t *stream, *glyf, *loca, *hmtx;
  const uint8_t *const *glyfs = nullptr, *const *locas = nullptr, *const *hmtxs = nullptr;
};

struct Launch {
  std::vector<AsmDesc> descs;
  std::vector<DirRec> recs;
  std::vector<DirFont> fonts;
  uint64_t out_bytes = 0;   // the output buffer so far
  uint64_t most_tiles = 1;  // of any one table (the tile spread of the launch)
};

// Append a laid-out collection: one output file, a descriptor per written table, a DirFont per
// member.  False (nothing appended) as add_font.
inline bool add_collection(Launch *l, const Plan &pl, const FontSrc &src) {
  const uint64_t num = pl.t.size();
  uint64_t written = 0, records = 0;
  for (uint64_t i = 0; i < num; i++) written += pl.written[i];
  for (const Member &m : pl.fonts) records += m.order.size();
  if ((uint64_t)l->descs.size() + written > 0x7FFFFFFFull || (uint64_t)l->recs.size() + records > 0x7FFFFFFFull ||
      (uint64_t)l->fonts.size() + pl.fonts.size() > 0x7FFFFFFFull)
    return false;
  const uint64_t base = (l->out_bytes + kFontAlign - 1) & ~(kFontAlign - 1);
  const uint32_t first = (uint32_t)l->descs.size();
  std::vector<uint32_t> slot(num, 0);   // a written table's place among the file's sums
  for (uint32_t i = 0; i < num; i++) {
    if (!pl.written[i]) continue;
    const Table &t = pl.t[i];
    const uint8_t *s = t.kind == kGlyf ? src.glyfs[pl.unit[i]] : t.kind == kLoca ? src.locas[pl.unit[i]]
                       : t.kind == kHmtx ? src.hmtxs[pl.unit[i]] : src.stream + t.src_off;
    slot[i] = (uint32_t)l->descs.size() - first;
    l->descs.push_back(AsmDesc{s, base, t.dst_off, t.dst_len, head_zeroed(pl, i) ? 8u : kNoZero, first + slot[i]});
    const uint64_t tiles = ((uint64_t)t.dst_len + 3 + (t.dst_off & 15) + kAsmTile - 1) / kAsmTile;
    l->most_tiles = tiles > l->most_tiles ? tiles : l->most_tiles;
  }
  for (size_t m = 0; m < pl.fonts.size(); m++) {
    const Member &mem = pl.fonts[m];
    DirFont f;
    f.out_base = base;
    f.flavor = mem.flavor;
    f.num = (uint32_t)mem.order.size();
    search_fields(f.num, &f.range, &f.selector, &f.shift);
    f.selector &= 0xFFFF;
    f.first_rec = (uint32_t)l->recs.size();
    f.first_sum = first;
    f.adjust_at = member_adjusts(pl, mem) ? pl.t[mem.head].dst_off + 8 : kNoZero;
    f.dir_off = mem.dir_off;
    f.ttc_index = (uint32_t)m;
    f.ttc_version = pl.ttc_version;
    f.ttc_fonts = (uint32_t)pl.fonts.size();
    for (uint32_t i : mem.order) l->recs.push_back(DirRec{pl.t[i].tag, slot[i], pl.t[i].dst_off, pl.t[i].dst_len});
    l->fonts.push_back(f);
  }
  l->out_bytes = base + pl.sfnt_len;
  return true;
}

// Append a laid-out font (a collection: add_collection).  False (nothing appended) where the
// launch's table count would leave what one grid dimension holds.
inline bool add_font(Launch *l, const Plan &pl, const FontSrc &src) {
  if (pl.ttc_version) return add_collection(l, pl, src);
  const uint64_t num = pl.t.size();
  if ((uint64_t)l->descs.size() + num > 0x7FFFFFFFull || (uint64_t)l->recs.size() + num > 0x7FFFFFFFull) return false;
  const uint64_t base = (l->out_bytes + kFontAlign - 1) & ~(kFontAlign - 1);
  // (the records run ahead of the tables only behind a collection whose members share tables)
  const uint32_t first = (uint32_t)l->descs.size(), first_rec = (uint32_t)l->recs.size();
  for (uint32_t i = 0; i < num; i++) {
    const Table &t = pl.t[i];
    const uint8_t *s = t.kind == kGlyf ? src.glyf : t.kind == kLoca ? src.loca : t.kind == kHmtx ? src.hmtx
                                                                                                : src.stream + t.src_off;
    l->descs.push_back(AsmDesc{s, base, t.dst_off, t.dst_len, i == pl.head && head_adjusted(pl) ? 8u : kNoZero, first + i});
    const uint64_t tiles = ((uint64_t)t.dst_len + 3 + (t.dst_off & 15) + kAsmTile - 1) / kAsmTile;
    l->most_tiles = tiles > l->most_tiles ? tiles : l->most_tiles;
  }
  for (uint32_t r = 0; r < num; r++) {
    const Table &t = pl.t[pl.order[r]];
    l->recs.push_back(DirRec{t.tag, pl.order[r], t.dst_off, t.dst_len});
  }
  DirFont f;
  f.out_base = base;
  f.flavor = pl.flavor;
  f.num = (uint32_t)num;
  search_fields(f.num, &f.range, &f.selector, &f.shift);
  f.selector &= 0xFFFF;
  f.first_rec = first_rec;
  f.first_sum = first;
  f.adjust_at = head_adjusted(pl) ? pl.t[pl.head].dst_off + 8 : kNoZero;
  l->fonts.push_back(f);
  l->out_bytes = base + pl.sfnt_len;
  return true;
}

// The two kernels' work stated serially over a launch: `out` has l.out_bytes bytes.  The bytes
// between two fonts are left as they are.
inline void host_run(const Launch &l, uint8_t *out) {
  std::vector<uint32_t> sums(l.descs.size(), 0);
  for (const AsmDesc &d : l.descs) {
    uint8_t *dst = out + d.out_base + d.dst_off;
    const uint32_t padded = (d.len + 3) & ~3u;
    for (uint32_t b = 0; b < padded; b++) {
      uint8_t v = b < d.len ? d.src[b] : 0;
      if (d.zero_at != kNoZero && b - d.zero_at < 4) v = 0;
      dst[b] = v;
    }
    sums[d.sum] = sum_words(dst, padded);
  }
  for (const DirFont &f : l.fonts) {
    uint8_t *o = out + f.out_base + f.dir_off;
    if (f.ttc_index != kNoZero) {
      uint8_t *h = out + f.out_base;
      put32(h + 12 + 4 * (size_t)f.ttc_index, f.dir_off);
      if (f.ttc_index == 0) {
        put32(h, kFlavorTtc);
        put32(h + 4, f.ttc_version);
        put32(h + 8, f.ttc_fonts);
        if (f.ttc_version == kTtcVersion2)
          for (int w = 0; w < 3; w++) put32(h + 12 + 4 * ((size_t)f.ttc_fonts + w), 0);
      }
    }
    put32(o, f.flavor);
    woff2inv::put16(o + 4, f.num);
    woff2inv::put16(o + 6, f.range);
    woff2inv::put16(o + 8, f.selector);
    woff2inv::put16(o + 10, f.shift);
    uint32_t total = 0;
    for (uint32_t r = 0; r < f.num; r++) {
      const DirRec &rec = l.recs[f.first_rec + r];
      uint8_t *p = o + 12 + 16 * (size_t)r;
      put32(p, rec.tag);
      put32(p + 4, sums[f.first_sum + rec.table]);
      put32(p + 8, rec.dst_off);
      put32(p + 12, rec.len);
      total += sums[f.first_sum + rec.table];
    }
    total += sum_words(o, 12 + 16 * (size_t)f.num);
    if (f.adjust_at != kNoZero) put32(out + f.out_base + f.adjust_at, kHeadMagic - total);
  }
}

}  // namespace woff2file
}  // namespace mib
#endif
