// Inverse of the WOFF2 'glyf' transform (W3C WOFF2 sections 5.1 - 5.3): the parsing half that
// woff2_inv.hip runs on the GPU, written so that it also compiles as plain C++.  The bytes
// come from a .woff2 file, so nothing here trusts them: every stream read goes through rd8,
// which clamps at the stream's end and raises `bad`; nothing is written except through the
// walker's `out`, whose size the same walker announced in its sizing pass.
//
//   * View / parse_header: the seven streams and two bitmaps of a transformed table (host).
//   * rd255, trip_len, comp_walk: the pieces the offset-resolution kernels share with the
//     walker (255UInt16 values, the triplet byte count of a flag, a composite's length).
//   * walk_glyph: one glyph from its cursors in the six variable streams to its TrueType
//     record, laid out as fontTools 4.62 compiles it (Glyph.compile, compileDeltasGreedy,
//     GlyphComponent.compile, 4-byte padding).  out == nullptr: only sizes it.  It also
//     returns the cursors it stopped at, i.e. the next glyph's.
//   * host_reconstruct: the serial driver -- walk_glyph glyph by glyph, each glyph's end
//     cursors the next one's start.  The CPU tests run it under sanitizers
//     (tests/woff2_inv_host_main.cpp); the GPU finds the same cursors with scans and
//     speculation and checks them against the walker's.
#ifndef MIB_WOFF2_INV_H_
#define MIB_WOFF2_INV_H_
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define MIB_HD __host__ __device__
#else
#define MIB_HD
#endif

namespace mib {
namespace woff2inv {

enum { kNContour, kNPoints, kFlags, kGlyph, kComposite, kBBox, kInstr, kStreams };
constexpr int kHeaderBytes = 36;
constexpr size_t kMaxInput = (size_t)1 << 28;   // keeps every offset and the output size in 32 bits

struct View {
  const uint8_t *s[kStreams];   // s[kBBox]: the explicit boxes, past the bitmap
  uint32_t n[kStreams];
  const uint8_t *bbox_bm;       // ((num_glyphs + 31) >> 5) << 2 bytes
  const uint8_t *ovl_bm;        // (num_glyphs + 7) >> 3 bytes, or nullptr
  uint32_t num_glyphs;
  uint32_t long_loca;
};

// Header checks before anything else looks at the table.  `base` is where the table's bytes
// will be read from (the host copy, or its device copy); `t` is the host copy.
inline bool parse_header(const uint8_t *t, size_t n, const uint8_t *base, View *v) {
  if (!t || n < (size_t)kHeaderBytes || n > kMaxInput) return false;
  auto b16 = [&](int at) { return ((uint32_t)t[at] << 8) | t[at + 1]; };
  auto b32 = [&](int at) { return (b16(at) << 16) | b16(at + 2); };
  const uint32_t opt = b16(2), ng = b16(4), fmt = b16(6);
  if ((opt & ~1u) || ng == 0 || fmt > 1) return false;
  uint64_t pos = kHeaderBytes;
  for (int i = 0; i < kStreams; i++) {
    const uint32_t sz = b32(8 + 4 * i);
    if (sz > n) return false;
    v->s[i] = base + pos;
    v->n[i] = sz;
    pos += sz;
  }
  const uint32_t ovl = (opt & 1) ? (ng + 7) >> 3 : 0;
  if (pos + ovl != n) return false;
  if (v->n[kNContour] != 2 * ng) return false;
  const uint32_t bbm = ((ng + 31) >> 5) << 2;
  if (v->n[kBBox] < bbm) return false;
  v->bbox_bm = v->s[kBBox];
  v->s[kBBox] += bbm;
  v->n[kBBox] -= bbm;
  v->ovl_bm = ovl ? base + pos : nullptr;
  v->num_glyphs = ng;
  v->long_loca = fmt;
  return true;
}

MIB_HD inline uint32_t rd8(const View &v, int st, uint32_t pos, int &bad) {
  if (pos >= v.n[st]) {
    bad = 1;
    return 0;
  }
  return v.s[st][pos];
}
MIB_HD inline uint32_t rd16(const View &v, int st, uint32_t pos, int &bad) {
  const uint32_t hi = rd8(v, st, pos, bad);
  return (hi << 8) | rd8(v, st, pos + 1, bad);
}
MIB_HD inline int32_t rds16(const View &v, int st, uint32_t pos, int &bad) { return (int16_t)rd16(v, st, pos, bad); }

MIB_HD inline int32_t ncontours(const View &v, uint32_t g) {
  return (int16_t)(((uint32_t)v.s[kNContour][2 * g] << 8) | v.s[kNContour][2 * g + 1]);
}
MIB_HD inline bool bit_of(const uint8_t *bm, uint32_t g) { return (bm[g >> 3] & (0x80u >> (g & 7))) != 0; }

// bytes a 255UInt16 takes, from its first byte
MIB_HD inline int len255_code(uint32_t b) { return b == 253 ? 3 : b >= 254 ? 2 : 1; }
// fontTools unpack255UShort; moves pos past the value
MIB_HD inline uint32_t rd255(const View &v, int st, uint32_t &pos, int &bad) {
  const uint32_t b = rd8(v, st, pos, bad);
  uint32_t val = b;
  if (b == 253) val = rd16(v, st, pos + 1, bad);
  else if (b == 254) val = 506 + rd8(v, st, pos + 1, bad);
  else if (b == 255) val = 253 + rd8(v, st, pos + 1, bad);
  const uint32_t next = pos + (uint32_t)len255_code(b);
  pos = next > v.n[st] ? v.n[st] : next;
  return val;
}
// glyph-stream bytes of one point, from its flag byte (section 5.2; `triplet()` backwards)
MIB_HD inline int trip_len(uint32_t flag) {
  flag &= 0x7F;
  return flag < 84 ? 1 : flag < 120 ? 2 : flag < 124 ? 3 : 4;
}

// component flags (glyf table)
constexpr uint32_t kArgWords = 0x0001, kXYValues = 0x0002, kHaveScale = 0x0008, kMore = 0x0020, kXYScale = 0x0040,
                   kTwoByTwo = 0x0080, kHaveInstr = 0x0100;
constexpr uint32_t kKeptFlags = 0x0004 | 0x0010 | 0x0200 | 0x0400 | 0x0800 | 0x1000;
// glyph flags
constexpr uint32_t kOnCurve = 0x01, kXShort = 0x02, kYShort = 0x04, kRepeat = 0x08, kXSame = 0x10, kYSame = 0x20,
                   kOverlapSimple = 0x40;

MIB_HD inline uint32_t comp_len(uint32_t fl) {
  uint32_t len = 4 + ((fl & kArgWords) ? 4 : 2);
  if (fl & kHaveScale) len += 2;
  else if (fl & kXYScale) len += 4;
  else if (fl & kTwoByTwo) len += 8;
  return len;
}
// One composite glyph's bytes in the composite stream: moves pos past its last component.
MIB_HD inline void comp_walk(const View &v, uint32_t &pos, bool &have_instr, int &bad) {
  have_instr = false;
  for (;;) {
    const uint32_t fl = rd16(v, kComposite, pos, bad);
    const uint32_t next = pos + comp_len(fl);
    if (bad || next > v.n[kComposite]) {
      bad = 1;
      pos = v.n[kComposite];
      return;
    }
    pos = next;
    have_instr = have_instr || (fl & kHaveInstr);
    if (!(fl & kMore)) return;
  }
}

struct Cursors {
  uint32_t c[kStreams];   // byte positions in the streams ([kNContour] unused)
};

MIB_HD inline void put16(uint8_t *o, uint32_t v) {
  o[0] = (uint8_t)(v >> 8);
  o[1] = (uint8_t)v;
}

// One point's delta from its flag and triplet bytes (fontTools _decodeTriplets).
MIB_HD inline void triplet_delta(const View &v, uint32_t flag, uint32_t &gpos, int &dx, int &dy, int &bad) {
  const uint32_t f = flag & 0x7F;
  const int nb = trip_len(f);
  uint32_t t[4] = {0, 0, 0, 0};
  for (int i = 0; i < nb; i++) t[i] = rd8(v, kGlyph, gpos + i, bad);
  gpos += nb;
  int ax, ay;
  const bool xpos = f & 1, ypos = (f >> 1) & 1;
  if (f < 10) {
    ax = 0;
    ay = (int)(((f & 14) << 7) + t[0]);
    dx = 0;
    dy = xpos ? ay : -ay;   // (a one-coordinate form carries its sign in bit 0)
    return;
  }
  if (f < 20) {
    ax = (int)((((f - 10) & 14) << 7) + t[0]);
    dx = xpos ? ax : -ax;
    dy = 0;
    return;
  }
  if (f < 84) {
    const uint32_t b0 = f - 20;
    ax = (int)(1 + (b0 & 0x30) + (t[0] >> 4));
    ay = (int)(1 + ((b0 & 0x0C) << 2) + (t[0] & 0x0F));
  } else if (f < 120) {
    const uint32_t b0 = f - 84;
    ax = (int)(1 + ((b0 / 12) << 8) + t[0]);
    ay = (int)(1 + (((b0 % 12) >> 2) << 8) + t[1]);
  } else if (f < 124) {
    ax = (int)((t[0] << 4) + (t[1] >> 4));
    ay = (int)(((t[1] & 0x0F) << 8) + t[2]);
  } else {
    ax = (int)((t[0] << 8) + t[1]);
    ay = (int)((t[2] << 8) + t[3]);
  }
  dx = xpos ? ax : -ax;
  dy = ypos ? ay : -ay;
}

// Glyph g from the cursors `cur`: its padded TrueType record into out (nullptr: none), the
// record's size into *size, the cursors after it into *end.  False (and size 0) for a glyph
// that fontTools could not reconstruct or compile, or whose bytes run past a stream.
MIB_HD inline bool walk_glyph(const View &v, uint32_t g, const Cursors &cur, uint8_t *out, uint32_t *size,
                              Cursors *end) {
  *end = cur;
  *size = 0;
  int bad = 0;
  const int32_t nc = ncontours(v, g);
  if (nc == 0) return true;   // empty glyph: no bytes anywhere else
  if (nc < -1) return false;
  const bool have_bbox = bit_of(v.bbox_bm, g);
  uint8_t box[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (have_bbox) {
    for (int i = 0; i < 8; i++) box[i] = (uint8_t)rd8(v, kBBox, cur.c[kBBox] + i, bad);
    if (bad) return false;
    end->c[kBBox] = cur.c[kBBox] + 8;
  }
  uint32_t n = 0;   // bytes of the record
  if (nc > 0) {
    // contours: one 255UInt16 each, at least one point, the last end point within uint16
    uint32_t np = cur.c[kNPoints], npts = 0;
    for (int32_t c = 0; c < nc; c++) {
      const uint32_t k = rd255(v, kNPoints, np, bad);
      if (bad || k == 0 || npts + k > 65536) return false;
      npts += k;
      if (out) put16(out + 10 + 2 * c, npts - 1);
    }
    end->c[kNPoints] = np;
    const uint32_t f0 = cur.c[kFlags];
    if (f0 > v.n[kFlags] || npts > v.n[kFlags] - f0) return false;
    end->c[kFlags] = f0 + npts;
    // the instruction length follows the triplets: measure them first
    uint32_t gp = cur.c[kGlyph];
    for (uint32_t i = 0; i < npts; i++) gp += (uint32_t)trip_len(v.s[kFlags][f0 + i]);
    if (gp > v.n[kGlyph]) return false;
    const uint32_t ilen = rd255(v, kGlyph, gp, bad);
    if (bad || ilen > 32767) return false;
    end->c[kGlyph] = gp;
    const uint32_t i0 = cur.c[kInstr];
    if (i0 > v.n[kInstr] || ilen > v.n[kInstr] - i0) return false;
    end->c[kInstr] = i0 + ilen;
    n = 10 + 2 * (uint32_t)nc + 2 + ilen;
    if (out) {
      put16(out + 10 + 2 * nc, ilen);
      for (uint32_t i = 0; i < ilen; i++) out[12 + 2 * nc + i] = v.s[kInstr][i0 + i];
    }
    const bool overlap = v.ovl_bm && bit_of(v.ovl_bm, g);
    // pass 0 counts the flag / x / y bytes and the bounds; pass 1 (writing) places them
    uint32_t nfl = 0, nx = 0, ny = 0;
    long long xmin = 0, xmax = 0, ymin = 0, ymax = 0;
    for (int pass = 0; pass < (out ? 2 : 1); pass++) {
      uint8_t *of = out ? out + n : nullptr, *ox = out ? of + nfl : nullptr, *oy = out ? ox + nx : nullptr;
      const bool w = pass == 1;
      uint32_t kf = 0, kx = 0, ky = 0, tp = cur.c[kGlyph];
      int last = -1, repeat = 0;
      long long x = 0, y = 0;
      for (uint32_t i = 0; i < npts; i++) {
        const uint32_t tf = v.s[kFlags][f0 + i];
        int dx, dy;
        triplet_delta(v, tf, tp, dx, dy, bad);
        if (bad || dx > 32767 || dy > 32767 || dx < -32768 || dy < -32768) return false;
        x += dx;
        y += dy;
        if (i == 0 || x < xmin) xmin = x;
        if (i == 0 || x > xmax) xmax = x;
        if (i == 0 || y < ymin) ymin = y;
        if (i == 0 || y > ymax) ymax = y;
        uint32_t fl = (tf & 0x80) ? 0 : kOnCurve;
        if (i == 0 && overlap) fl |= kOverlapSimple;
        if (dx == 0) {
          fl |= kXSame;
        } else if (dx >= -255 && dx <= 255) {
          fl |= kXShort | (dx > 0 ? kXSame : 0);
          if (w) ox[kx] = (uint8_t)(dx > 0 ? dx : -dx);
          kx += 1;
        } else {
          if (w) put16(ox + kx, (uint32_t)dx);
          kx += 2;
        }
        if (dy == 0) {
          fl |= kYSame;
        } else if (dy >= -255 && dy <= 255) {
          fl |= kYShort | (dy > 0 ? kYSame : 0);
          if (w) oy[ky] = (uint8_t)(dy > 0 ? dy : -dy);
          ky += 1;
        } else {
          if (w) put16(oy + ky, (uint32_t)dy);
          ky += 2;
        }
        // a repeated flag: written twice, then folded into flag | REPEAT and a count up to 255
        if ((int)fl == last && repeat != 255) {
          repeat++;
          if (repeat == 1) {
            if (w) of[kf] = (uint8_t)fl;
            kf++;
          } else if (w) {
            of[kf - 2] = (uint8_t)(fl | kRepeat);
            of[kf - 1] = (uint8_t)repeat;
          }
        } else {
          repeat = 0;
          if (w) of[kf] = (uint8_t)fl;
          kf++;
        }
        last = (int)fl;
      }
      nfl = kf;
      nx = kx;
      ny = ky;
    }
    if (!have_bbox) {
      if (xmin < -32768 || ymin < -32768 || xmax > 32767 || ymax > 32767) return false;
      put16(box, (uint32_t)xmin);
      put16(box + 2, (uint32_t)ymin);
      put16(box + 4, (uint32_t)xmax);
      put16(box + 6, (uint32_t)ymax);
    }
    n += nfl + nx + ny;
  } else {
    if (!have_bbox) return false;   // a composite's box is never implied
    uint32_t cp = cur.c[kComposite];
    bool more = true, have_instr = false;
    n = 10;
    while (more) {
      const uint32_t fl = rd16(v, kComposite, cp, bad), gid = rd16(v, kComposite, cp + 2, bad);
      const uint32_t len = comp_len(fl);
      if (bad || cp + len > v.n[kComposite]) return false;
      uint32_t a = cp + 4;
      int v0, v1;
      if (fl & kArgWords) {
        v0 = (fl & kXYValues) ? rds16(v, kComposite, a, bad) : (int)rd16(v, kComposite, a, bad);
        v1 = (fl & kXYValues) ? rds16(v, kComposite, a + 2, bad) : (int)rd16(v, kComposite, a + 2, bad);
        a += 4;
      } else {
        v0 = (fl & kXYValues) ? (int)(int8_t)rd8(v, kComposite, a, bad) : (int)rd8(v, kComposite, a, bad);
        v1 = (fl & kXYValues) ? (int)(int8_t)rd8(v, kComposite, a + 1, bad) : (int)rd8(v, kComposite, a + 1, bad);
        a += 2;
      }
      int t00 = 0x4000, t01 = 0, t10 = 0, t11 = 0x4000;
      const bool has_t = (fl & (kHaveScale | kXYScale | kTwoByTwo)) != 0;
      if (fl & kHaveScale) {
        t00 = t11 = rds16(v, kComposite, a, bad);
      } else if (fl & kXYScale) {
        t00 = rds16(v, kComposite, a, bad);
        t11 = rds16(v, kComposite, a + 2, bad);
      } else if (fl & kTwoByTwo) {
        t00 = rds16(v, kComposite, a, bad);
        t01 = rds16(v, kComposite, a + 2, bad);
        t10 = rds16(v, kComposite, a + 4, bad);
        t11 = rds16(v, kComposite, a + 6, bad);
      }
      cp += len;
      more = (fl & kMore) != 0;
      have_instr = have_instr || (fl & kHaveInstr);
      // GlyphComponent.compile: kept flags, argument and scale forms by value
      uint32_t of = (fl & kKeptFlags) | (more ? kMore : 0) | (!more && have_instr ? kHaveInstr : 0);
      bool words;
      if (fl & kXYValues) {
        of |= kXYValues;
        words = !(v0 >= -128 && v0 <= 127 && v1 >= -128 && v1 <= 127);
      } else {
        words = !(v0 >= 0 && v0 <= 255 && v1 >= 0 && v1 <= 255);
      }
      if (words) of |= kArgWords;
      int tkind = 0;   // 1 scale, 2 x and y, 3 two by two
      if (has_t) tkind = (t01 || t10) ? 3 : (t00 != t11) ? 2 : 1;
      of |= tkind == 3 ? kTwoByTwo : tkind == 2 ? kXYScale : tkind == 1 ? kHaveScale : 0;
      if (out) {
        uint8_t *o = out + n;
        put16(o, of);
        put16(o + 2, gid);
        o += 4;
        if (words) {
          put16(o, (uint32_t)v0);
          put16(o + 2, (uint32_t)v1);
          o += 4;
        } else {
          o[0] = (uint8_t)v0;
          o[1] = (uint8_t)v1;
          o += 2;
        }
        if (tkind == 1) {
          put16(o, (uint32_t)t00);
        } else if (tkind == 2) {
          put16(o, (uint32_t)t00);
          put16(o + 2, (uint32_t)t11);
        } else if (tkind == 3) {
          put16(o, (uint32_t)t00);
          put16(o + 2, (uint32_t)t01);
          put16(o + 4, (uint32_t)t10);
          put16(o + 6, (uint32_t)t11);
        }
      }
      n += 4 + (words ? 4 : 2) + (tkind == 3 ? 8 : tkind == 2 ? 4 : tkind == 1 ? 2 : 0);
    }
    end->c[kComposite] = cp;
    if (have_instr) {
      uint32_t gp = cur.c[kGlyph];
      const uint32_t ilen = rd255(v, kGlyph, gp, bad);
      if (bad || ilen > 32767) return false;
      end->c[kGlyph] = gp;
      const uint32_t i0 = cur.c[kInstr];
      if (i0 > v.n[kInstr] || ilen > v.n[kInstr] - i0) return false;
      end->c[kInstr] = i0 + ilen;
      if (out) {
        put16(out + n, ilen);
        for (uint32_t i = 0; i < ilen; i++) out[n + 2 + i] = v.s[kInstr][i0 + i];
      }
      n += 2 + ilen;
    }
  }
  const uint32_t padded = (n + 3) & ~3u;
  if (out) {
    put16(out, (uint32_t)nc);
    for (int i = 0; i < 8; i++) out[2 + i] = box[i];
    for (uint32_t i = n; i < padded; i++) out[i] = 0;
  }
  *size = padded;
  return true;
}

// loca entry i for glyph offset `off`
MIB_HD inline void put_loca(uint8_t *loca, uint32_t long_loca, uint32_t i, uint32_t off) {
  if (long_loca) {
    put16(loca + 4 * (size_t)i, off >> 16);
    put16(loca + 4 * (size_t)i + 2, off & 0xFFFF);
  } else {
    put16(loca + 2 * (size_t)i, off >> 1);
  }
}
// what the caller checks once every glyph is sized: all streams used up, loca can hold it
inline bool totals_ok(const View &v, const Cursors &end, uint64_t total) {
  for (int s = kNPoints; s < kStreams; s++)
    if (end.c[s] != v.n[s]) return false;
  return v.long_loca ? total <= 0xFFFFFFFFull : total < 0x20000;
}

// The serial driver.  0, or -1 for a table that is rejected.  *announced: the glyf size the
// sizing pass gave (the write pass stays within it by construction; the tests check that).
inline int host_reconstruct(const uint8_t *t, size_t n, std::vector<uint8_t> *glyf, std::vector<uint8_t> *loca,
                            uint64_t *announced = nullptr) {
  View v;
  if (!parse_header(t, n, t, &v)) return -1;
  std::vector<uint32_t> off((size_t)v.num_glyphs + 1);
  std::vector<Cursors> cur((size_t)v.num_glyphs + 1);
  for (int s = 0; s < kStreams; s++) cur[0].c[s] = 0;
  uint64_t total = 0;
  for (uint32_t g = 0; g < v.num_glyphs; g++) {
    uint32_t sz;
    if (!walk_glyph(v, g, cur[g], nullptr, &sz, &cur[g + 1])) return -1;
    off[g] = (uint32_t)total;
    total += sz;
  }
  off[v.num_glyphs] = (uint32_t)total;
  if (!totals_ok(v, cur[v.num_glyphs], total)) return -1;
  if (announced) *announced = total;
  glyf->assign(total ? (size_t)total : 1, 0);   // every glyph empty: one zero byte
  loca->assign(((size_t)v.num_glyphs + 1) * (v.long_loca ? 4 : 2), 0);
  for (uint32_t g = 0; g < v.num_glyphs; g++) {
    uint32_t sz;
    Cursors e;
    if (off[g + 1] != off[g] && !walk_glyph(v, g, cur[g], glyf->data() + off[g], &sz, &e)) return -1;
  }
  for (uint32_t i = 0; i <= v.num_glyphs; i++) put_loca(loca->data(), v.long_loca, i, off[i]);
  return 0;
}

// ---- hmtx (section 5.4)
// a glyph's xMin from glyf / loca (0 for an empty glyph); false for a loca entry that does
// not fit the glyf table
MIB_HD inline bool glyph_xmin(const uint8_t *glyf, uint32_t glyf_n, const uint8_t *loca, uint32_t long_loca,
                              uint32_t g, int32_t *xmin) {
  uint32_t o0, o1;
  if (long_loca) {
    const uint8_t *p = loca + 4 * (size_t)g;
    o0 = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    o1 = ((uint32_t)p[4] << 24) | ((uint32_t)p[5] << 16) | ((uint32_t)p[6] << 8) | p[7];
  } else {
    const uint8_t *p = loca + 2 * (size_t)g;
    o0 = 2 * (((uint32_t)p[0] << 8) | p[1]);
    o1 = 2 * (((uint32_t)p[2] << 8) | p[3]);
  }
  *xmin = 0;
  if (o1 == o0) return true;
  if (o1 < o0 || o1 > glyf_n || o1 - o0 < 10) return false;
  *xmin = (int16_t)(((uint32_t)glyf[o0 + 2] << 8) | glyf[o0 + 3]);
  return true;
}
// hmtx bytes of glyph g: its longHorMetric (g < nhm) or its lsb
MIB_HD inline bool hmtx_glyph(const uint8_t *t, const uint8_t *glyf, uint32_t glyf_n, const uint8_t *loca,
                              uint32_t long_loca, uint32_t ng, uint32_t nhm, uint32_t g, uint8_t *out) {
  const uint32_t flags = t[0];
  const bool prop = g < nhm;
  const bool stored = prop ? !(flags & 1) : !(flags & 2);
  uint8_t *o = prop ? out + 4 * (size_t)g : out + 4 * (size_t)nhm + 2 * (size_t)(g - nhm);
  if (prop) {
    o[0] = t[1 + 2 * (size_t)g];
    o[1] = t[2 + 2 * (size_t)g];
    o += 2;
  }
  if (stored) {
    // the kept array follows the advance widths (only one of the two can be there)
    const uint8_t *l = t + 1 + 2 * (size_t)nhm + 2 * (size_t)(prop ? g : g - nhm);
    o[0] = l[0];
    o[1] = l[1];
    return true;
  }
  int32_t xmin;
  if (!glyph_xmin(glyf, glyf_n, loca, long_loca, g, &xmin)) return false;
  put16(o, (uint32_t)xmin);
  return true;
}
// argument checks of mib_woff2_reconstruct_hmtx; *long_loca from the loca table's size
// in two halves: what the table's first byte decides (reserved bits, a flag set, the size the
// flags imply -- the device checks this where the table never visits the host), and the rest
MIB_HD inline bool hmtx_flags_ok(uint32_t flags, uint64_t n, uint32_t ng, uint32_t nhm) {
  if ((flags & 0xFC) || !(flags & 3)) return false;
  const uint64_t want = 1 + 2ull * nhm + ((flags & 1) ? 0 : 2ull * nhm) + ((flags & 2) ? 0 : 2ull * (ng - nhm));
  return n == want;
}
inline bool hmtx_shape_ok(size_t n, size_t glyf_n, size_t loca_n, uint32_t ng, uint32_t nhm, uint32_t *long_loca) {
  if (n < 1 || ng == 0 || ng > 65535 || nhm == 0 || nhm > ng || glyf_n > 0xFFFFFFFFull) return false;
  if (loca_n == 4 * ((size_t)ng + 1)) *long_loca = 1;
  else if (loca_n == 2 * ((size_t)ng + 1)) *long_loca = 0;
  else return false;
  return true;
}
inline bool hmtx_args_ok(const uint8_t *t, size_t n, size_t glyf_n, size_t loca_n, uint32_t ng, uint32_t nhm,
                         uint32_t *long_loca) {
  return t && hmtx_shape_ok(n, glyf_n, loca_n, ng, nhm, long_loca) && hmtx_flags_ok(t[0], n, ng, nhm);
}
inline int host_reconstruct_hmtx(const uint8_t *t, size_t n, const uint8_t *glyf, size_t glyf_n, const uint8_t *loca,
                                 size_t loca_n, uint32_t ng, uint32_t nhm, std::vector<uint8_t> *out) {
  uint32_t long_loca;
  if (!hmtx_args_ok(t, n, glyf_n, loca_n, ng, nhm, &long_loca)) return -1;
  out->assign(4 * (size_t)nhm + 2 * (size_t)(ng - nhm), 0);
  for (uint32_t g = 0; g < ng; g++)
    if (!hmtx_glyph(t, glyf, (uint32_t)glyf_n, loca, long_loca, ng, nhm, g, out->data())) return -1;
  return 0;
}

}  // namespace woff2inv
}  // namespace mib
#endif
