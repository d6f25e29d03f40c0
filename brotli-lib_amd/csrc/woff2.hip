// WOFF2 'glyf' transform (the FONT-mode caller of the encoder, reference
// README.md:63) on the GPU: a TrueType glyf + loca table pair becomes the seven streams of
// the W3C WOFF2 specification section 5.1 -- nContour, nPoints (255UInt16), flags,
// glyph (triplet-coded coordinate deltas + instruction lengths), composite, bbox (bitmap +
// explicit boxes) and instructions -- plus the overlap-simple bitmap.
//
// One thread per glyph, two passes: `glyf_sizes_kernel` parses each glyph (flags with
// repeats, x / y deltas, contours, components) and counts its bytes in every stream; the
// per-stream counts are scanned; `glyf_write_kernel` parses again and writes each glyph's
// bytes at its offsets.  The byte choices follow fontTools 4.62 (`WOFF2GlyfTable`), the
// implementation the tests compare against (tests/test_gpu_woff2.py).
//
// Each transform is a core over device pointers (woff2_dev.h: a sizing step and a write step
// that writes the whole table, header included, at any device address) and a host wrapper
// around it, mib_woff2_transform_glyf / _hmtx; the file writer (woff2_write.hip) runs the cores
// on the font it has uploaded and lets them write into its stream buffer.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "woff2_dev.h"

namespace mib {
namespace woff2 {

enum { kNContour, kNPoints, kFlags, kGlyph, kComposite, kBBox, kInstr, kStreams };
constexpr int kHeaderBytes = 36;   // version, optionFlags, numGlyphs, indexFormat, 7 stream sizes

struct Font {                      // device view of one font's glyf / loca
  const uint8_t *glyf;
  uint32_t glyf_len;
  const uint8_t *loca;
  uint32_t num_glyphs;
  int32_t long_loca;
};

__device__ __forceinline__ uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
__device__ __forceinline__ int32_t sbe16(const uint8_t *p) { return (int16_t)be16(p); }
__device__ __forceinline__ uint32_t be32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
__device__ __forceinline__ int len255(uint32_t v) { return v < 253 ? 1 : v < 762 ? 2 : 3; }
__device__ __forceinline__ int put255(uint8_t *o, uint32_t v) {   // fontTools pack255UShort
  if (v < 253) {
    o[0] = (uint8_t)v;
    return 1;
  }
  if (v < 506) {
    o[0] = 255;
    o[1] = (uint8_t)(v - 253);
    return 2;
  }
  if (v < 762) {
    o[0] = 254;
    o[1] = (uint8_t)(v - 506);
    return 2;
  }
  o[0] = 253;
  o[1] = (uint8_t)(v >> 8);
  o[2] = (uint8_t)v;
  return 3;
}
// triplet encoding of one (dx, dy) (WOFF2 section 5.2): the flag byte and the data bytes
__device__ __forceinline__ int triplet(int x, int y, bool on, uint8_t *flag, uint8_t *t) {
  const int ax = x < 0 ? -x : x, ay = y < 0 ? -y : y;
  const int onb = on ? 0 : 128, xs = x < 0 ? 0 : 1, ys = y < 0 ? 0 : 1, xy = xs + 2 * ys;
  if (x == 0 && ay < 1280) {
    *flag = (uint8_t)(onb + ((ay & 0xF00) >> 7) + ys);
    t[0] = (uint8_t)ay;
    return 1;
  }
  if (y == 0 && ax < 1280) {
    *flag = (uint8_t)(onb + 10 + ((ax & 0xF00) >> 7) + xs);
    t[0] = (uint8_t)ax;
    return 1;
  }
  if (ax < 65 && ay < 65) {
    *flag = (uint8_t)(onb + 20 + ((ax - 1) & 0x30) + (((ay - 1) & 0x30) >> 2) + xy);
    t[0] = (uint8_t)((((ax - 1) & 0xF) << 4) | ((ay - 1) & 0xF));
    return 1;
  }
  if (ax < 769 && ay < 769) {
    *flag = (uint8_t)(onb + 84 + 12 * (((ax - 1) & 0x300) >> 8) + (((ay - 1) & 0x300) >> 6) + xy);
    t[0] = (uint8_t)(ax - 1);
    t[1] = (uint8_t)(ay - 1);
    return 2;
  }
  if (ax < 4096 && ay < 4096) {
    *flag = (uint8_t)(onb + 120 + xy);
    t[0] = (uint8_t)(ax >> 4);
    t[1] = (uint8_t)(((ax & 0xF) << 4) | (ay >> 8));
    t[2] = (uint8_t)ay;
    return 3;
  }
  *flag = (uint8_t)(onb + 124 + xy);
  t[0] = (uint8_t)(ax >> 8);
  t[1] = (uint8_t)ax;
  t[2] = (uint8_t)(ay >> 8);
  t[3] = (uint8_t)ay;
  return 4;
}

// TrueType glyph flags (glyf table) and component flags
constexpr int kOnCurve = 0x01, kXShort = 0x02, kYShort = 0x04, kRepeat = 0x08, kXSame = 0x10, kYSame = 0x20,
              kOverlapSimple = 0x40;
constexpr int kArgWords = 0x0001, kXYValues = 0x0002, kHaveScale = 0x0008, kMore = 0x0020, kXYScale = 0x0040,
              kTwoByTwo = 0x0080, kHaveInstr = 0x0100;
// flags a component keeps (ROUND_XY_TO_GRID, NON_OVERLAPPING, USE_MY_METRICS, OVERLAP_COMPOUND,
// SCALED / UNSCALED_COMPONENT_OFFSET); the others are recomputed
constexpr int kKeptFlags = 0x0004 | 0x0010 | 0x0200 | 0x0400 | 0x0800 | 0x1000;

// Walks one glyph; with out == nullptr only counts.  Returns false on a malformed glyph.
struct Sink {
  uint8_t *s[kStreams];   // stream cursors (write pass) or nullptr
  uint32_t n[kStreams];   // bytes per stream
  bool overlap, bbox;
};
__device__ bool walk_glyph(const Font &f, uint32_t g, Sink &k) {
  for (int i = 0; i < kStreams; i++) k.n[i] = 0;
  k.overlap = k.bbox = false;
  const uint32_t o0 = f.long_loca ? be32(f.loca + 4 * g) : 2 * be16(f.loca + 2 * g);
  const uint32_t o1 = f.long_loca ? be32(f.loca + 4 * g + 4) : 2 * be16(f.loca + 2 * g + 2);
  const bool w = k.s[0] != nullptr;
  auto emit = [&](int st, uint8_t b) {
    if (w) k.s[st][k.n[st]] = b;
    k.n[st]++;
  };
  if (o1 < o0 || o1 > f.glyf_len) return false;
  if (o1 == o0) {   // empty glyph: numberOfContours 0 and nothing else
    emit(kNContour, 0);
    emit(kNContour, 0);
    return true;
  }
  const uint8_t *p = f.glyf + o0, *end = f.glyf + o1;
  if (o1 - o0 < 10) return false;
  const int nc = sbe16(p);
  emit(kNContour, p[0]);
  emit(kNContour, p[1]);
  if (nc == 0) return true;
  const uint8_t *hdr = p;
  p += 10;
  if (nc > 0) {   // simple glyph
    if (p + 2 * nc + 2 > end) return false;
    int last = -1;
    for (int c = 0; c < nc; c++) {
      const int e = (int)be16(p + 2 * c);
      if (e <= last) return false;
      uint8_t tmp[3];
      const int m = put255(tmp, (uint32_t)(e - last));
      for (int q = 0; q < m; q++) emit(kNPoints, tmp[q]);
      last = e;
    }
    const int npts = last + 1;
    p += 2 * nc;
    const uint32_t ilen = be16(p);
    p += 2;
    const uint8_t *instr = p;
    p += ilen;
    if (p > end) return false;
    // flags (with repeats), then the x and y delta arrays they describe
    const uint8_t *fl = p;
    int nf = 0;
    const uint8_t *q = fl;
    uint32_t xbytes = 0;
    bool first = true;
    while (nf < npts) {
      if (q >= end) return false;
      const int fb = *q++;
      int rep = 1;
      if (fb & kRepeat) {
        if (q >= end) return false;
        rep += *q++;
      }
      if (first) {
        k.overlap = (fb & kOverlapSimple) != 0;
        first = false;
      }
      nf += rep;
      xbytes += (uint32_t)rep * ((fb & kXShort) ? 1u : (fb & kXSame) ? 0u : 2u);
    }
    if (nf != npts) return false;
    const uint8_t *xs = q, *ys = q + xbytes;
    // decode the points, emit flags + triplets, track the bounds
    const uint8_t *fq = fl;
    int fb = 0, rep = 0;
    int x = 0, y = 0, xmin = 0, xmax = 0, ymin = 0, ymax = 0;
    const uint8_t *xp = xs, *yp = ys;
    for (int i = 0; i < npts; i++) {
      if (rep == 0) {
        fb = *fq++;
        rep = 1;
        if (fb & kRepeat) rep += *fq++;
      }
      rep--;
      int dx, dy;
      if (fb & kXShort) {
        if (xp >= end) return false;
        dx = (fb & kXSame) ? *xp : -(int)*xp;
        xp++;
      } else if (fb & kXSame) {
        dx = 0;
      } else {
        if (xp + 2 > end) return false;
        dx = sbe16(xp);
        xp += 2;
      }
      if (fb & kYShort) {
        if (yp >= end) return false;
        dy = (fb & kYSame) ? *yp : -(int)*yp;
        yp++;
      } else if (fb & kYSame) {
        dy = 0;
      } else {
        if (yp + 2 > end) return false;
        dy = sbe16(yp);
        yp += 2;
      }
      x += dx;
      y += dy;
      if (i == 0 || x < xmin) xmin = x;
      if (i == 0 || x > xmax) xmax = x;
      if (i == 0 || y < ymin) ymin = y;
      if (i == 0 || y > ymax) ymax = y;
      uint8_t flag, t[4];
      const int m = triplet(dx, dy, (fb & kOnCurve) != 0, &flag, t);
      emit(kFlags, flag);
      for (int j = 0; j < m; j++) emit(kGlyph, t[j]);
    }
    uint8_t tmp[3];
    const int m = put255(tmp, ilen);
    for (int j = 0; j < m; j++) emit(kGlyph, tmp[j]);
    for (uint32_t j = 0; j < ilen; j++) emit(kInstr, instr[j]);
    // the explicit box only when the header's differs from the points' bounds
    const bool same = npts > 0 && sbe16(hdr + 2) == xmin && sbe16(hdr + 4) == ymin && sbe16(hdr + 6) == xmax &&
                      sbe16(hdr + 8) == ymax;
    k.bbox = !same;
  } else {   // composite glyph: the component records (re-encoded the way fontTools'
             // GlyphComponent.compile does: kept flags, minimal argument and scale forms,
             // MORE / WE_HAVE_INSTRUCTIONS recomputed), then its instructions
    bool more = true, have_instr = false;
    while (more) {
      if (p + 4 > end) return false;
      const uint32_t fl = be16(p), gid = be16(p + 2);
      const uint8_t *a = p + 4;
      int len = 4 + ((fl & kArgWords) ? 4 : 2);
      if (fl & kHaveScale) len += 2;
      else if (fl & kXYScale) len += 4;
      else if (fl & kTwoByTwo) len += 8;
      if (p + len > end) return false;
      more = (fl & kMore) != 0;
      have_instr = have_instr || (fl & kHaveInstr) != 0;
      int v0, v1;
      if (fl & kArgWords) {
        v0 = (fl & kXYValues) ? sbe16(a) : (int)be16(a);
        v1 = (fl & kXYValues) ? sbe16(a + 2) : (int)be16(a + 2);
        a += 4;
      } else {
        v0 = (fl & kXYValues) ? (int)(int8_t)a[0] : (int)a[0];
        v1 = (fl & kXYValues) ? (int)(int8_t)a[1] : (int)a[1];
        a += 2;
      }
      int t00 = 0x4000, t01 = 0, t10 = 0, t11 = 0x4000;
      const bool has_t = (fl & (kHaveScale | kXYScale | kTwoByTwo)) != 0;
      if (fl & kHaveScale) {
        t00 = t11 = sbe16(a);
      } else if (fl & kXYScale) {
        t00 = sbe16(a);
        t11 = sbe16(a + 2);
      } else if (fl & kTwoByTwo) {
        t00 = sbe16(a);
        t01 = sbe16(a + 2);
        t10 = sbe16(a + 4);
        t11 = sbe16(a + 6);
      }
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
      emit(kComposite, (uint8_t)(of >> 8));
      emit(kComposite, (uint8_t)of);
      emit(kComposite, (uint8_t)(gid >> 8));
      emit(kComposite, (uint8_t)gid);
      if (words) {
        emit(kComposite, (uint8_t)(v0 >> 8));
        emit(kComposite, (uint8_t)v0);
        emit(kComposite, (uint8_t)(v1 >> 8));
        emit(kComposite, (uint8_t)v1);
      } else {
        emit(kComposite, (uint8_t)v0);
        emit(kComposite, (uint8_t)v1);
      }
      const int tv[4] = {t00, t01, t10, t11};
      const int nt = tkind == 3 ? 4 : tkind == 2 ? 2 : tkind == 1 ? 1 : 0;
      for (int q = 0; q < nt; q++) {
        const int v = tkind == 2 ? (q == 0 ? t00 : t11) : tv[q];
        emit(kComposite, (uint8_t)(v >> 8));
        emit(kComposite, (uint8_t)v);
      }
      p += len;
    }
    if (have_instr) {
      if (p + 2 > end) return false;
      const uint32_t ilen = be16(p);
      p += 2;
      if (p + ilen > end) return false;
      uint8_t tmp[3];
      const int m = put255(tmp, ilen);
      for (int j = 0; j < m; j++) emit(kGlyph, tmp[j]);
      for (uint32_t j = 0; j < ilen; j++) emit(kInstr, p[j]);
    }
    k.bbox = true;
  }
  if (k.bbox)
    for (int j = 0; j < 8; j++) emit(kBBox, hdr[2 + j]);
  return true;
}

__global__ void glyf_sizes_kernel(Font f, uint32_t *sizes /* [kStreams][n] */, uint8_t *bits /* per glyph */,
                                  int *bad) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= f.num_glyphs) return;
  Sink k;
  for (int i = 0; i < kStreams; i++) k.s[i] = nullptr;
  if (!walk_glyph(f, g, k)) {
    atomicOr(bad, 1);
    for (int i = 0; i < kStreams; i++) k.n[i] = 0;
  }
  for (int i = 0; i < kStreams; i++) sizes[(size_t)i * f.num_glyphs + g] = k.n[i];
  bits[g] = (uint8_t)((k.overlap ? 1 : 0) | (k.bbox ? 2 : 0));
}

// offs: exclusive scans of sizes; base.v[s] = the stream's offset in the output
struct StreamBase {
  uint32_t v[kStreams];
};
__global__ void glyf_write_kernel(Font f, const uint32_t *offs, StreamBase base, uint8_t *out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= f.num_glyphs) return;
  Sink k;
  for (int i = 0; i < kStreams; i++) {
    const uint32_t extra = i == kBBox ? ((f.num_glyphs + 31) >> 5) << 2 : 0;   // the bbox bitmap comes first
    k.s[i] = out + (uint32_t)(base.v[i] + extra + offs[(size_t)i * f.num_glyphs + g]);
  }
  walk_glyph(f, g, k);
}

// the bbox and overlap-simple bitmaps (bit 7 first), one thread per byte
__global__ void glyf_bitmaps_kernel(uint32_t n, const uint8_t *bits, uint8_t *bbox_bm, uint8_t *ovl_bm, int with_ovl) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nb_bbox = ((n + 31) >> 5) << 2;
  if (b < nb_bbox) {
    uint8_t v = 0;
    for (int j = 0; j < 8; j++) {
      const uint32_t g = 8 * b + j;
      if (g < n && (bits[g] & 2)) v |= (uint8_t)(0x80 >> j);
    }
    bbox_bm[b] = v;
  }
  if (with_ovl && b < ((n + 7) >> 3)) {
    uint8_t v = 0;
    for (int j = 0; j < 8; j++) {
      const uint32_t g = 8 * b + j;
      if (g < n && (bits[g] & 1)) v |= (uint8_t)(0x80 >> j);
    }
    ovl_bm[b] = v;
  }
}

// the transformed table's 36-byte header, stated by the host once the streams' sizes are known;
// byte stores: the table may lie at any address
struct GlyfHeader {
  uint8_t b[kHeaderBytes];
};
__global__ void glyf_header_kernel(GlyfHeader h, uint8_t *out) {
  if (threadIdx.x < kHeaderBytes) out[threadIdx.x] = h.b[threadIdx.x];
}

// ---------------------------------------------------------------- hmtx (WOFF2 section 5.4)
// fontTools WOFF2HmtxTable.transform: the proportional (i < numberOfHMetrics) and monospaced
// glyphs' left side bearings are dropped when every one equals its glyph's xMin (0 for an
// empty glyph).  Thread per glyph: a mismatch sets bit 0 (proportional) or 1 (monospaced).
__global__ void hmtx_check_kernel(Font f, const uint8_t *hmtx, uint32_t nhm, uint32_t *mismatch) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= f.num_glyphs) return;
  const uint32_t o0 = f.long_loca ? be32(f.loca + 4 * g) : 2 * be16(f.loca + 2 * g);
  const uint32_t o1 = f.long_loca ? be32(f.loca + 4 * g + 4) : 2 * be16(f.loca + 2 * g + 2);
  const int32_t xmin = (o1 > o0 && o0 + 10 <= f.glyf_len) ? sbe16(f.glyf + o0 + 2) : 0;
  const int32_t lsb = g < nhm ? sbe16(hmtx + 4 * g + 2) : sbe16(hmtx + 4 * nhm + 2 * (g - nhm));
  if (lsb != xmin) atomicOr(mismatch, g < nhm ? 1u : 2u);
}
// the transformed table: flags, advance widths, then the lsb array that is kept (if any)
__global__ void hmtx_write_kernel(uint32_t ng, const uint8_t *hmtx, uint32_t nhm, uint32_t keep, uint8_t *out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ng) return;
  if (g == 0) out[0] = (uint8_t)((keep == 1 ? 0 : 1) | (keep == 2 ? 0 : 2));   // set: that array is absent
  if (g < nhm) {
    out[1 + 2 * g] = hmtx[4 * g];
    out[2 + 2 * g] = hmtx[4 * g + 1];
  }
  const uint32_t lsb_at = 1 + 2 * nhm;
  if (keep == 1 && g < nhm) {          // proportional glyphs' lsbs
    out[lsb_at + 2 * g] = hmtx[4 * g + 2];
    out[lsb_at + 2 * g + 1] = hmtx[4 * g + 3];
  } else if (keep == 2 && g >= nhm) {  // monospaced glyphs' lsbs
    out[lsb_at + 2 * (g - nhm)] = hmtx[4 * nhm + 2 * (g - nhm)];
    out[lsb_at + 2 * (g - nhm) + 1] = hmtx[4 * nhm + 2 * (g - nhm) + 1];
  }
}

}  // namespace woff2

// ---------------------------------------------------------------- the cores (woff2_dev.h)
namespace woff2dev {

using namespace mib::woff2;

namespace {
void put16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}
void put32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}
Font font_of(const GlyfIn &in) { return Font{in.d_glyf, in.glyf_len, in.d_loca, in.num_glyphs, (int32_t)in.long_loca}; }
}  // namespace

int transform_glyf_size(hipStream_t st, Timer &tm, DevMem &m, const GlyfIn &in, GlyfSized *z) {
  const uint32_t ng = in.num_glyphs;
  const size_t nsz = (size_t)kStreams * ng;
  uint32_t *d_sizes = m.take<uint32_t>(nsz), *d_offs = m.take<uint32_t>(nsz);
  uint8_t *d_bits = m.take<uint8_t>(ng);
  int *d_bad = m.take<int>(1);
  if (!d_sizes || !d_offs || !d_bits || !d_bad) return MIB_E_OUT_OF_MEMORY;
  hipMemsetAsync(d_bad, 0, 4, st);
  const Font f = font_of(in);
  const dim3 grid((ng + 255) / 256), block(256);
  tm.start("w2enc_glyf_sizes");
  hipLaunchKernelGGL(glyf_sizes_kernel, grid, block, 0, st, f, d_sizes, d_bits, d_bad);
  tm.stop();
  // exclusive scan of every stream's per-glyph sizes (one flat scan: each stream's run
  // starts at its own total, subtracted below)
  size_t tmp_b = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_b, d_sizes, d_offs, (int)nsz, st);
  uint8_t *d_tmp = m.take<uint8_t>(tmp_b);
  if (!d_tmp) return MIB_E_OUT_OF_MEMORY;
  tm.start("w2enc_glyf_scan");
  hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_b, d_sizes, d_offs, (int)nsz, st);
  tm.stop();
  uint32_t starts[kStreams + 1], tot[kStreams];
  int bad = 0;
  uint32_t last_off = 0, last_size = 0;
  std::vector<uint8_t> bits(ng);   // the overlap bitmap only when some simple glyph has the flag
  for (int s = 0; s < kStreams; s++) hipMemcpyAsync(&starts[s], d_offs + (size_t)s * ng, 4, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(&last_off, d_offs + nsz - 1, 4, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(&last_size, d_sizes + nsz - 1, 4, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(bits.data(), d_bits, ng, hipMemcpyDeviceToHost, st);
  if (hipStreamSynchronize(st) != hipSuccess) return MIB_E_NO_DEVICE;
  if (bad) return MIB_E_INVALID_ARG;   // a malformed glyph
  starts[kStreams] = last_off + last_size;
  for (int s = 0; s < kStreams; s++) tot[s] = starts[s + 1] - starts[s];
  const uint32_t bbm = ((ng + 31) >> 5) << 2;
  tot[kBBox] += bbm;
  // output layout: header, the streams, (overlap bitmap); each stream's glyph offsets are
  // the flat scan minus the stream's start
  uint64_t pos = kHeaderBytes;
  for (int s = 0; s < kStreams; s++) {
    z->base[s] = (uint32_t)(pos - starts[s]);
    pos += tot[s];
  }
  bool ovl = false;
  for (uint32_t g = 0; g < ng; g++) ovl = ovl || (bits[g] & 1);
  z->in = in;
  z->d_offs = d_offs;
  z->d_bits = d_bits;
  z->bbox_at = z->base[kBBox] + starts[kBBox];
  z->streams_end = pos;
  z->overlap = ovl;
  z->total = pos + (ovl ? ((ng + 7) >> 3) : 0);
  put16(&z->header[0], 0);
  put16(&z->header[2], ovl ? 1 : 0);
  put16(&z->header[4], ng);
  put16(&z->header[6], in.long_loca ? 1 : 0);
  for (int s = 0; s < kStreams; s++) put32(&z->header[8 + 4 * s], tot[s]);
  return 0;
}

void transform_glyf_write(hipStream_t st, Timer &tm, const GlyfSized &z, uint8_t *d_out) {
  const uint32_t ng = z.in.num_glyphs, bbm = ((ng + 31) >> 5) << 2;
  const Font f = font_of(z.in);
  StreamBase base;
  for (int s = 0; s < kStreams; s++) base.v[s] = z.base[s];
  GlyfHeader h;
  memcpy(h.b, z.header, kHeaderBytes);
  tm.start("w2enc_glyf_write");
  hipLaunchKernelGGL(glyf_header_kernel, dim3(1), dim3(64), 0, st, h, d_out);
  hipLaunchKernelGGL(glyf_write_kernel, dim3((ng + 255) / 256), dim3(256), 0, st, f, z.d_offs, base, d_out);
  hipLaunchKernelGGL(glyf_bitmaps_kernel, dim3((bbm + 255) / 256), dim3(256), 0, st, ng, z.d_bits, d_out + z.bbox_at,
                     d_out + z.streams_end, z.overlap ? 1 : 0);
  tm.stop();
}

int transform_hmtx_size(hipStream_t st, Timer &tm, DevMem &m, const GlyfIn &in, const uint8_t *d_hmtx, uint32_t nhm,
                        HmtxSized *z) {
  uint32_t *d_mis = m.take<uint32_t>(1);
  if (!d_mis) return MIB_E_OUT_OF_MEMORY;
  hipMemsetAsync(d_mis, 0, 4, st);
  const uint32_t ng = in.num_glyphs;
  tm.start("w2enc_hmtx_check");
  hipLaunchKernelGGL(hmtx_check_kernel, dim3((ng + 255) / 256), dim3(256), 0, st, font_of(in), d_hmtx, nhm, d_mis);
  tm.stop();
  uint32_t mis = 0;
  hipMemcpyAsync(&mis, d_mis, 4, hipMemcpyDeviceToHost, st);
  if (hipStreamSynchronize(st) != hipSuccess) return MIB_E_NO_DEVICE;
  z->num_glyphs = ng;
  z->d_hmtx = d_hmtx;
  z->nhm = nhm;
  z->keep = mis;   // 0: none, 1: proportional lsbs, 2: monospaced lsbs, 3: both needed -- no transform
  z->total = mis == 3 ? 0 : 1 + 2ull * nhm + (mis == 1 ? 2ull * nhm : mis == 2 ? 2ull * (ng - nhm) : 0);
  return 0;
}

void transform_hmtx_write(hipStream_t st, Timer &tm, const HmtxSized &z, uint8_t *d_out) {
  tm.start("w2enc_hmtx_write");
  hipLaunchKernelGGL(hmtx_write_kernel, dim3((z.num_glyphs + 255) / 256), dim3(256), 0, st, z.num_glyphs, z.d_hmtx, z.nhm,
                     z.keep, d_out);
  tm.stop();
}

}  // namespace woff2dev
}  // namespace mib

using mib::woff2dev::Call;
using mib::woff2dev::GlyfIn;
using mib::woff2dev::GlyfSized;
using mib::woff2dev::HmtxSized;

namespace {
uint32_t hbe16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
uint32_t hbe32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// The tables the transforms read, in the order the wrappers index them: glyf needs the first
// four, hmtx all six.
enum { kGlyf, kLoca, kHead, kMaxp, kHhea, kHmtx, kTags };
const char *const kTag[kTags] = {"glyf", "loca", "head", "maxp", "hhea", "hmtx"};
struct DirEntry {
  uint64_t off = 0, len = 0;
  bool have = false;
};

// One walk over the sfnt's table records (host: a few dozen bytes).  False for fewer than 12
// bytes, a directory that runs past the input, or any record whose offset + length does;
// otherwise out[t] is the record of kTag[t], t < count (of the last one, where a tag comes twice).
bool scan_directory(const uint8_t *ttf, size_t n, int count, DirEntry *out) {
  if (n < 12) return false;
  const uint32_t ntab = hbe16(ttf + 4);
  if (12 + 16ull * ntab > n) return false;
  for (uint32_t i = 0; i < ntab; i++) {
    const uint8_t *r = ttf + 12 + 16 * i;
    const uint32_t off = hbe32(r + 8), len = hbe32(r + 12);
    if ((uint64_t)off + len > n) return false;
    for (int t = 0; t < count; t++)
      if (!memcmp(r, kTag[t], 4)) out[t] = DirEntry{off, len, true};
  }
  return true;
}
}  // namespace

extern "C" int mib_woff2_transform_glyf(const uint8_t *ttf, size_t n, mib_buf *out) {
  if (!out || (!ttf && n)) return MIB_E_INVALID_ARG;
  out->data = nullptr;
  out->size = 0;
  DirEntry t[kMaxp + 1];
  if (!scan_directory(ttf, n, kMaxp + 1, t)) return MIB_E_INVALID_ARG;
  for (const DirEntry &e : t)
    if (!e.have) return MIB_E_INVALID_ARG;
  if (t[kHead].off + 54 > n || t[kMaxp].off + 6 > n) return MIB_E_INVALID_ARG;
  const uint64_t glyf_len = t[kGlyf].len, loca_len = t[kLoca].len;
  const int long_loca = (int16_t)hbe16(ttf + t[kHead].off + 50) != 0 ? 1 : 0;
  const uint32_t ng = hbe16(ttf + t[kMaxp].off + 4);
  if ((uint64_t)(ng + 1) * (long_loca ? 4 : 2) > loca_len || ng == 0) return MIB_E_INVALID_ARG;
  Call use(false);   // (the transform wrappers report no kernel times)
  if (!use.c) return MIB_E_NO_DEVICE;
  uint8_t *d_font = use.m.take<uint8_t>(glyf_len + loca_len);
  if (!d_font) return use.rc = MIB_E_OUT_OF_MEMORY;
  hipMemcpyAsync(d_font, ttf + t[kGlyf].off, glyf_len, hipMemcpyHostToDevice, use.st);
  hipMemcpyAsync(d_font + glyf_len, ttf + t[kLoca].off, loca_len, hipMemcpyHostToDevice, use.st);
  GlyfSized z;
  const GlyfIn in{d_font, (uint32_t)glyf_len, d_font + glyf_len, ng, (uint32_t)long_loca};
  if ((use.rc = mib::woff2dev::transform_glyf_size(use.st, use.tm, use.m, in, &z))) return use.rc;
  uint8_t *d_out = use.m.take<uint8_t>((size_t)z.total);
  if (!d_out) return use.rc = MIB_E_OUT_OF_MEMORY;
  mib::woff2dev::transform_glyf_write(use.st, use.tm, z, d_out);
  return use.rc = use.fetch(d_out, (size_t)z.total, out);
}

// WOFF2 hmtx transform (fontTools WOFF2HmtxTable.transform).  Returns 0 with out->size = 0
// when no transform applies (both side-bearing arrays must be kept: the table stays as is).
extern "C" int mib_woff2_transform_hmtx(const uint8_t *ttf, size_t n, mib_buf *out) {
  if (!out || (!ttf && n)) return MIB_E_INVALID_ARG;
  out->data = nullptr;
  out->size = 0;
  DirEntry t[kTags];
  if (!scan_directory(ttf, n, kTags, t)) return MIB_E_INVALID_ARG;
  for (const DirEntry &e : t)
    if (!e.have) return MIB_E_INVALID_ARG;
  if (t[kHead].len < 54 || t[kMaxp].len < 6 || t[kHhea].len < 36) return MIB_E_INVALID_ARG;
  const int long_loca = (int16_t)hbe16(ttf + t[kHead].off + 50) != 0 ? 1 : 0;
  const uint32_t ng = hbe16(ttf + t[kMaxp].off + 4), nhm = hbe16(ttf + t[kHhea].off + 34);
  const uint64_t gl = t[kGlyf].len, ll = t[kLoca].len, hl = t[kHmtx].len;
  if (ng == 0 || nhm == 0 || nhm > ng || (uint64_t)(ng + 1) * (long_loca ? 4 : 2) > ll || 4ull * nhm + 2ull * (ng - nhm) > hl)
    return MIB_E_INVALID_ARG;
  Call use(false);   // (the transform wrappers report no kernel times)
  if (!use.c) return MIB_E_NO_DEVICE;
  uint8_t *d_font = use.m.take<uint8_t>(gl + ll + hl);
  if (!d_font) return use.rc = MIB_E_OUT_OF_MEMORY;
  hipMemcpyAsync(d_font, ttf + t[kGlyf].off, gl, hipMemcpyHostToDevice, use.st);
  hipMemcpyAsync(d_font + gl, ttf + t[kLoca].off, ll, hipMemcpyHostToDevice, use.st);
  hipMemcpyAsync(d_font + gl + ll, ttf + t[kHmtx].off, hl, hipMemcpyHostToDevice, use.st);
  HmtxSized z;
  const GlyfIn in{d_font, (uint32_t)gl, d_font + gl, ng, (uint32_t)long_loca};
  if ((use.rc = mib::woff2dev::transform_hmtx_size(use.st, use.tm, use.m, in, d_font + gl + ll, nhm, &z))) return use.rc;
  if (!z.total) return 0;   // both arrays needed: no transform
  uint8_t *d_out = use.m.take<uint8_t>((size_t)z.total);
  if (!d_out) return use.rc = MIB_E_OUT_OF_MEMORY;
  mib::woff2dev::transform_hmtx_write(use.st, use.tm, z, d_out);
  return use.rc = use.fetch(d_out, (size_t)z.total, out);
}

